"""Python binding of libsdrg.so (include/sdrg.h) — host-side mirror of the reference's SDRBridge surface.

The reference exposes the hot path to Kotlin through JNI (java/fr/intuite/sdr/bridge/SDRBridge.kt:23-154):
`SDRConfig`, `applyConfig(...)`, `read(12 callbacks)` and per-field setters.  This module mirrors that
surface over the engine's C ABI with the same names and argument meaning:

    cfg = SDRConfig(centerFrequency=100_000_000, sampleRate=2_000_000, samplesPerReading=16384)
    eng = Engine(cfg, n_streams=4096)          # one reference "process" per stream
    eng.applyConfig(cfg); eng.setFrequency(...); eng.setFrequencyFocusRange(...); eng.setSoundMode(...)
    eng.read(fftCallback=..., meanSnrCallback=..., pcmCallback=...)   # register callbacks (JNI read)
    spectra, records, pcm = eng.process(iq_frames, fmt=CS8)           # one frame per stream

Everything runs in the HIP kernels of libsdrg.so; there is no CPU fallback.  If the library is missing
or no gfx950 device is present, the calls raise.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
LIB_PATH = os.environ.get("SDRG_LIB_PATH") or os.path.join(PKG, "lib", "libsdrg.so")  # override: diagnostic builds

# include/sdrg.h
CF32, CS8, CU8, CS16, CS12 = 0, 1, 2, 3, 4
STAGE_SPECTRUM, STAGE_STATS, STAGE_SSB, STAGE_HOT_PATH = 1, 2, 4, 7
STAGE_SPECTRAL_PULSE, STAGE_AUDIO_PULSE, STAGE_ALL = 8, 16, 31
PIPELINE_OFF, PIPELINE_ON, PIPELINE_INPUTS_READY = 0, 1, 2  # sdrg_engine_set_pipelining modes
PIPELINE_STATS_ASYNC = 4  # OR'ed with ON / INPUTS_READY: statistics on a stream of their own
PULSE_SPECTRAL, PULSE_AUDIO = 0, 1
DISPLAY_SPAN_FULL, DISPLAY_SPAN_FOCUS, DISPLAY_SPAN_BINS = 0, 1, 2  # sdrg_display_config.span
DISPLAY_MAX, DISPLAY_MEAN = 0, 1                                    # .reduce
DISPLAY_DB_F32, DISPLAY_U8 = 0, 1                                   # .format
INTEGRATE_MEAN, INTEGRATE_MAX, INTEGRATE_EMA = 0, 1, 2              # sdrg_integrate_config.mode
INTEGRATE_MAX_PERIOD = 64
PEAKS_MAX, PEAKS_MAX_SEPARATION = 64, 4096                          # SDRG_PEAKS_MAX, SDRG_PEAKS_MAX_SEPARATION
DDC_MAX_TAPS, DDC_MAX_DECIMATION = 511, 512                         # SDRG_DDC_MAX_TAPS, SDRG_DDC_MAX_DECIMATION
BANK_MAX_CHANNELS = 4096                                            # SDRG_BANK_MAX_CHANNELS
DEMOD_AM, DEMOD_FM = 0, 1                                           # SDRG_DEMOD_AM, SDRG_DEMOD_FM
DEMOD_OUT_S16, DEMOD_OUT_F32 = 0, 1                                 # SDRG_DEMOD_OUT_*
DEMOD_MAX_TAPS, DEMOD_MAX_DECIMATION, DEMOD_MAX_IN = 255, 64, 1 << 20  # SDRG_DEMOD_MAX_*
CHANNELIZER_MAX_CHANNELS, CHANNELIZER_MAX_TAPS_PER_CHANNEL, CHANNELIZER_MAX_TAPS = 256, 32, 4096  # SDRG_CHANNELIZER_*
DEMOD_OUT_DTYPE = {DEMOD_OUT_S16: np.int16, DEMOD_OUT_F32: np.float32}
RESAMPLE_OUT_S16, RESAMPLE_OUT_F32 = 0, 1                           # SDRG_RESAMPLE_OUT_*
RESAMPLE_MAX_FACTOR, RESAMPLE_MAX_TAPS_PER_PHASE, RESAMPLE_MAX_TAPS, RESAMPLE_MAX_IN = 512, 64, 8192, 1 << 20
RESAMPLE_OUT_DTYPE = {RESAMPLE_OUT_S16: np.int16, RESAMPLE_OUT_F32: np.float32}
SIDEBAND_UPPER, SIDEBAND_LOWER, SIDEBAND_BOTH = 0, 1, 2             # SDRG_SIDEBAND_UPPER / _LOWER / _BOTH
SIDEBAND_OUT_S16, SIDEBAND_OUT_F32 = 0, 1                           # SDRG_SIDEBAND_OUT_*
SIDEBAND_MAX_TAPS, SIDEBAND_MAX_DECIMATION, SIDEBAND_MAX_IN = 511, 64, 1 << 20  # SDRG_SIDEBAND_MAX_*
SIDEBAND_OUT_DTYPE = {SIDEBAND_OUT_S16: np.int16, SIDEBAND_OUT_F32: np.float32}
STATUS = {0: "SDRG_OK", -1: "SDRG_E_INVALID", -2: "SDRG_E_UNSUPPORTED", -3: "SDRG_E_NOMEM", -4: "SDRG_E_HIP",
          -5: "SDRG_E_NODEVICE"}
BYTES_PER_SAMPLE = {CF32: 8, CS8: 2, CU8: 2, CS16: 4}
NUMPY_DTYPE = {CF32: np.float32, CS8: np.int8, CU8: np.uint8, CS16: np.int16}

RECORD_DTYPE = np.dtype(
    [
        ("tracking_frequency", "<i8"),
        ("mean_snr_db", "<f4"),
        ("mean_snr_sigma", "<f4"),
        ("peak_above_noise_mean_db", "<f4"),
        ("max_bin_snr_db", "<f4"),
        ("max_bin_snr_sigma", "<f4"),
        ("best1khz_snr_db", "<f4"),
        ("best1khz_snr_sigma", "<f4"),
        ("best1khz_center_freq_hz", "<f4"),
        ("per_bin_mean", "<f4"),
        ("detection_flag", "<i4"),
        ("peak_bin", "<i4"),
        ("abs_peak_db", "<f4"),
        ("signal_power_db", "<f4"),
        ("valid", "<i4"),
        ("n_ref_windows", "<i4"),
    ],
    align=True,
)

PULSE_OUTPUT_DTYPE = np.dtype(
    [
        ("strength", "<f4"),
        ("live_etat", "<i4"),
        ("level", "<i4"),
        ("locked", "<i4"),
        ("period_s", "<f4"),
        ("est_freq_hz", "<f4"),
        ("est_freq_hz_rounded", "<i8"),
        ("input", "<f4"),
        ("n_energy", "<i4"),
        ("n_rois", "<i4"),
        ("overflow", "<i4"),
    ],
    align=True,
)

PEAK_DTYPE = np.dtype([("bin", "<i4"), ("power", "<f4"), ("db", "<f4"), ("snr_db", "<f4")])  # sdrg_peak
PEAKS_SUMMARY_DTYPE = np.dtype([("count", "<i4"), ("n_above", "<i4"), ("floor_power", "<f4"), ("floor_db", "<f4")])

# Every entry point include/sdrg.h declares (checked by tests/test_abi.py).
EXPORTS = [
    "sdrg_abi_version", "sdrg_last_error", "sdrg_ssb_pcm_len", "sdrg_ssb_layout", "sdrg_focus_window", "sdrg_host_alloc", "sdrg_host_free", "sdrg_ssb_design", "sdrg_engine_create", "sdrg_engine_destroy",
    "sdrg_engine_apply_config", "sdrg_engine_set_frequency", "sdrg_engine_set_frequency_focus_range",
    "sdrg_engine_set_sound_mode", "sdrg_engine_set_sample_rate", "sdrg_engine_set_samples_per_reading",
    "sdrg_engine_input_released", "sdrg_engine_wait_input_released", "sdrg_engine_wait_outputs", "sdrg_engine_set_upper_sideband", "sdrg_engine_get_config", "sdrg_engine_n_streams", "sdrg_engine_pcm_len",
    "sdrg_engine_reset_state", "sdrg_engine_process_device", "sdrg_engine_synchronize", "sdrg_engine_set_stream",
    "sdrg_engine_set_pipelining", "sdrg_engine_set_ssb_variant", "sdrg_engine_get_ssb_variant",
    "sdrg_engine_process_host", "sdrg_engine_signal_strength_device", "sdrg_engine_signal_strength_host",
    "sdrg_engine_set_callbacks", "sdrg_engine_set_profiling", "sdrg_engine_get_timings",
    "sdrg_engine_get_timing_stats", "sdrg_engine_reset_timing_stats",
    "sdrg_engine_set_spectral_pulse_config", "sdrg_engine_set_audio_pulse_config", "sdrg_engine_pulse_outputs",
    "sdrg_engine_get_pulse_outputs",
    "sdrg_pulse_config_default", "sdrg_pulse_bank_create", "sdrg_pulse_bank_destroy", "sdrg_pulse_bank_configure",
    "sdrg_pulse_bank_get_config", "sdrg_pulse_bank_reset", "sdrg_pulse_bank_process_spectral_device",
    "sdrg_pulse_bank_process_audio_device", "sdrg_pulse_bank_process_spectral_host",
    "sdrg_pulse_bank_process_audio_host", "sdrg_pulse_bank_synchronize", "sdrg_pulse_bank_set_stream",
    "sdrg_ingest_create", "sdrg_ingest_destroy", "sdrg_ingest_output_format", "sdrg_ingest_push", "sdrg_ingest_status",
    "sdrg_ingest_pop_batch", "sdrg_ingest_pop", "sdrg_ingest_set_samples_per_reading",
    "sdrg_ssb_processor_create", "sdrg_ssb_processor_destroy", "sdrg_ssb_processor_start", "sdrg_ssb_processor_stop",
    "sdrg_ssb_processor_enqueue", "sdrg_ssb_processor_set_sound_mode", "sdrg_ssb_processor_set_pulse_config",
    "sdrg_ssb_processor_get_ambient_energy", "sdrg_ssb_processor_get_current_ratio", "sdrg_ssb_processor_drain",
    "sdrg_ssb_processor_counters",
    "sdrg_dist_unique_id", "sdrg_dist_create", "sdrg_dist_destroy", "sdrg_dist_info", "sdrg_dist_set_one_rank_rccl",
    "sdrg_engine_gather",
    "sdrg_engine_gather_records", "sdrg_engine_gather_focus", "sdrg_engine_gather_spectra", "sdrg_engine_gather_pcm",
    "sdrg_device_alloc", "sdrg_device_free", "sdrg_memcpy", "sdrg_measure_hbm_copy",
    "sdrg_display_column_range", "sdrg_display_code", "sdrg_engine_set_display", "sdrg_engine_get_display",
    "sdrg_engine_display_geometry", "sdrg_engine_display_device", "sdrg_engine_display_host",
    "sdrg_engine_set_integration", "sdrg_engine_get_integration", "sdrg_engine_integrate_reset",
    "sdrg_engine_integrate_device", "sdrg_engine_integrate_host", "sdrg_engine_display_integrated_host",
    "sdrg_bin_offset_hz", "sdrg_engine_set_peaks", "sdrg_engine_get_peaks", "sdrg_engine_peaks_device",
    "sdrg_engine_peaks_host", "sdrg_engine_peaks_integrated_host",
    "sdrg_ddc_design", "sdrg_nco_tables", "sdrg_ddc_tile_outputs", "sdrg_engine_set_ddc", "sdrg_engine_get_ddc",
    "sdrg_engine_ddc_reset", "sdrg_engine_ddc_max_out", "sdrg_engine_ddc_device", "sdrg_engine_ddc_host",
    "sdrg_bank_geometry", "sdrg_engine_set_bank", "sdrg_engine_bank_retune", "sdrg_engine_get_bank",
    "sdrg_engine_bank_offsets", "sdrg_engine_bank_reset", "sdrg_engine_bank_max_out", "sdrg_engine_bank_device",
    "sdrg_engine_bank_host",
    "sdrg_demod_design", "sdrg_demod_geometry", "sdrg_engine_set_demod", "sdrg_engine_get_demod",
    "sdrg_engine_demod_reset", "sdrg_engine_demod_max_out", "sdrg_engine_demod_device", "sdrg_engine_demod_host",
    "sdrg_engine_ddc_demod_host",
    "sdrg_channelizer_design", "sdrg_channelizer_tile_outputs", "sdrg_engine_set_channelizer",
    "sdrg_engine_get_channelizer", "sdrg_engine_channelizer_reset", "sdrg_engine_channelizer_max_out",
    "sdrg_engine_channelizer_device", "sdrg_engine_channelizer_host",
    "sdrg_resample_design", "sdrg_resample_tile_outputs", "sdrg_resample_ratio", "sdrg_engine_set_resample",
    "sdrg_engine_get_resample", "sdrg_engine_resample_reset", "sdrg_engine_resample_max_out",
    "sdrg_engine_resample_device", "sdrg_engine_resample_host", "sdrg_engine_ddc_demod_resample_host",
    "sdrg_squelch_design", "sdrg_squelch_geometry", "sdrg_engine_set_squelch", "sdrg_engine_get_squelch",
    "sdrg_engine_squelch_reset", "sdrg_engine_squelch_device", "sdrg_engine_squelch_host",
    "sdrg_engine_ddc_squelch_demod_host", "sdrg_engine_ddc_squelch_demod_resample_host",
    "sdrg_agc_design", "sdrg_agc_geometry", "sdrg_engine_set_agc", "sdrg_engine_get_agc", "sdrg_engine_agc_reset",
    "sdrg_engine_agc_device", "sdrg_engine_agc_host", "sdrg_engine_listen_host",
    "sdrg_sideband_design", "sdrg_sideband_geometry", "sdrg_engine_set_sideband", "sdrg_engine_get_sideband",
    "sdrg_engine_sideband_reset", "sdrg_engine_sideband_max_out", "sdrg_engine_sideband_device",
    "sdrg_engine_sideband_host", "sdrg_engine_listen_sideband_host",
    "sdrg_iqcorr_design", "sdrg_iqcorr_geometry", "sdrg_engine_set_iqcorr", "sdrg_engine_get_iqcorr",
    "sdrg_engine_iqcorr_reset", "sdrg_engine_iqcorr_device", "sdrg_engine_iqcorr_host",
    "sdrg_engine_iqcorr_process_host",
    "sdrg_blanker_design", "sdrg_blanker_geometry", "sdrg_engine_set_blanker", "sdrg_engine_get_blanker",
    "sdrg_engine_blanker_reset", "sdrg_engine_blanker_device", "sdrg_engine_blanker_host",
    "sdrg_engine_clean_process_host",
    "sdrg_tones_design", "sdrg_tones_geometry", "sdrg_engine_set_tones", "sdrg_engine_get_tones",
    "sdrg_engine_tones_reset", "sdrg_engine_tones_max_blocks", "sdrg_engine_tones_device", "sdrg_engine_tones_host",
    "sdrg_engine_listen_tones_host",
    "sdrg_afc_design", "sdrg_afc_geometry", "sdrg_afc_offset_hz", "sdrg_engine_set_afc", "sdrg_engine_get_afc",
    "sdrg_engine_afc_reset", "sdrg_engine_afc_device", "sdrg_engine_afc_host", "sdrg_engine_listen_afc_host",
    "sdrg_symbols_design", "sdrg_symbols_geometry", "sdrg_symbols_count", "sdrg_engine_set_symbols",
    "sdrg_engine_get_symbols", "sdrg_engine_symbols_reset", "sdrg_engine_symbols_max_out", "sdrg_engine_symbols_device",
    "sdrg_engine_symbols_host", "sdrg_engine_listen_symbols_host",
]
DIST_ID_BYTES = 128  # SDRG_DIST_ID_BYTES (ncclUniqueId)


class SdrgError(RuntimeError):
    pass


class _Config(ctypes.Structure):
    _fields_ = [
        ("center_frequency", ctypes.c_int64),
        ("sample_rate", ctypes.c_int64),
        ("samples_per_reading", ctypes.c_int32),
        ("freq_focus_range_khz", ctypes.c_int32),
        ("gain", ctypes.c_int32),
        ("sound_mode", ctypes.c_int32),
        ("refresh_fft_ms", ctypes.c_int64),
        ("refresh_peak_ms", ctypes.c_int64),
        ("refresh_signal_strength_ms", ctypes.c_int64),
    ]


class PulseConfig(ctypes.Structure):
    """sdrg_pulse_config: SpectralPulseDetector::Config / AudioPulseDetector::Config (include/sdrg.h)."""
    _fields_ = [(k, ctypes.c_float) for k in ("fs_energy", "z_default_s", "t_target_init", "dt_tol_s", "snr_min",
                                              "snr_rhythm", "snr_strong", "dispersion_max")] + [
        ("sum_n_max", ctypes.c_int32), ("live_window_t", ctypes.c_float), ("live_divisor", ctypes.c_float),
        ("sample_rate", ctypes.c_float), ("f_min", ctypes.c_float), ("f_max", ctypes.c_float),
        ("smooth_cutoff", ctypes.c_float), ("noise_ref_far", ctypes.c_int32), ("noise_ref_near", ctypes.c_int32)]

    @classmethod
    def default(cls, kind: int, **overrides) -> "PulseConfig":
        c = cls()
        _check(load().sdrg_pulse_config_default(kind, ctypes.byref(c)), "sdrg_pulse_config_default")
        for k, v in overrides.items():
            setattr(c, k, v)
        return c


class DisplayConfig(ctypes.Structure):
    """sdrg_display_config: the display stage's span, width, reduction and output format (include/sdrg.h)."""
    _fields_ = [("span", ctypes.c_int32), ("first_bin", ctypes.c_int32), ("n_bins", ctypes.c_int32),
                ("width", ctypes.c_int32), ("reduce", ctypes.c_int32), ("format", ctypes.c_int32),
                ("db_min", ctypes.c_float), ("db_max", ctypes.c_float)]


class IntegrateConfig(ctypes.Structure):
    """sdrg_integrate_config: the integration stage's mode, period (MEAN, MAX) and alpha (EMA) (include/sdrg.h)."""
    _fields_ = [("mode", ctypes.c_int32), ("period", ctypes.c_int32), ("alpha", ctypes.c_float)]


class PeaksConfig(ctypes.Structure):
    """sdrg_peaks_config: the peak table stage's span, table size, spacing and threshold (include/sdrg.h)."""
    _fields_ = [("span", ctypes.c_int32), ("first_bin", ctypes.c_int32), ("n_bins", ctypes.c_int32),
                ("max_peaks", ctypes.c_int32), ("min_separation", ctypes.c_int32), ("threshold_db", ctypes.c_float)]


class SsbLayout(ctypes.Structure):
    """sdrg_ssb_layout_info: what the SSB launcher does with (sample_rate, n, fir_taps) (include/sdrg.h)."""
    _fields_ = [(k, ctypes.c_int32) for k in ("decimation", "taps", "pcm_len", "pipeline", "slots", "chunk",
                                              "chunk_outputs", "max_chunk_outputs")]


class DdcConfig(ctypes.Structure):
    """sdrg_ddc_config: the DDC stage's channel offset, low-pass cutoff, decimation and tap count (include/sdrg.h)."""
    _fields_ = [("offset_hz", ctypes.c_double), ("cutoff_hz", ctypes.c_double), ("decimation", ctypes.c_int32),
                ("taps", ctypes.c_int32)]


class BankConfig(ctypes.Structure):
    """sdrg_bank_config: the DDC bank's shared low-pass cutoff, decimation and tap count, and its channels per stream
    (include/sdrg.h)."""
    _fields_ = [("cutoff_hz", ctypes.c_double), ("decimation", ctypes.c_int32), ("taps", ctypes.c_int32),
                ("channels", ctypes.c_int32)]


class DemodConfig(ctypes.Structure):
    """sdrg_demod_config: the demodulator stage's mode, rates, filters, gain, output format and row length
    (include/sdrg.h)."""
    _fields_ = [("channel_rate_hz", ctypes.c_double), ("deviation_hz", ctypes.c_double),
                ("dc_cutoff_hz", ctypes.c_double), ("deemphasis_us", ctypes.c_double),
                ("audio_cutoff_hz", ctypes.c_double), ("mode", ctypes.c_int32), ("audio_decimation", ctypes.c_int32),
                ("audio_taps", ctypes.c_int32), ("out_format", ctypes.c_int32), ("max_in", ctypes.c_int32),
                ("gain", ctypes.c_float)]


class ChannelizerConfig(ctypes.Structure):
    """sdrg_channelizer_config: the channelizer stage's prototype cutoff, channel count, taps per channel, oversampling
    and the span of rows written (include/sdrg.h)."""
    _fields_ = [("cutoff_rel", ctypes.c_double), ("channels", ctypes.c_int32), ("taps_per_channel", ctypes.c_int32),
                ("oversample", ctypes.c_int32), ("first_channel", ctypes.c_int32), ("n_channels", ctypes.c_int32)]


class ResampleConfig(ctypes.Structure):
    """sdrg_resample_config: the resampler stage's prototype cutoff, ratio interp / decim, taps per phase, row type,
    output format, row length and gain (include/sdrg.h)."""
    _fields_ = [("cutoff_rel", ctypes.c_double), ("interp", ctypes.c_int32), ("decim", ctypes.c_int32),
                ("taps_per_phase", ctypes.c_int32), ("components", ctypes.c_int32), ("out_format", ctypes.c_int32),
                ("max_in", ctypes.c_int32), ("gain", ctypes.c_float)]


class SquelchConfig(ctypes.Structure):
    """sdrg_squelch_config: the squelch stage's thresholds, smoothing, block length, hang time and row length
    (include/sdrg.h)."""
    _fields_ = [("open_db", ctypes.c_double), ("close_db", ctypes.c_double), ("tau_blocks", ctypes.c_double),
                ("block", ctypes.c_int32), ("hang_blocks", ctypes.c_int32), ("max_in", ctypes.c_int32)]


# sdrg_squelch_record
SquelchRecord = np.dtype([("level", "<f4"), ("level_db", "<f4"), ("open", "<i4"), ("open_blocks", "<i4")])


class IqcorrConfig(ctypes.Structure):
    """sdrg_iqcorr_config: the IQ correction stage's two time constants, floor, mode, block length and row length
    (include/sdrg.h)."""
    _fields_ = [("dc_tau_blocks", ctypes.c_double), ("balance_tau_blocks", ctypes.c_double),
                ("floor_db", ctypes.c_double), ("mode", ctypes.c_int32), ("block", ctypes.c_int32),
                ("max_in", ctypes.c_int32)]


# sdrg_iqcorr_record
IqcorrRecord = np.dtype([("dc_re", "<f4"), ("dc_im", "<f4"), ("w_re", "<f4"), ("w_im", "<f4"), ("power", "<f4"),
                         ("image_db", "<f4"), ("held_blocks", "<i4"), ("seeded", "<i4")])
IQCORR_DC, IQCORR_BALANCE = 1, 2


class AfcConfig(ctypes.Structure):
    """sdrg_afc_config: the AFC stage's channel rate, clamp, time constant, floor, lock threshold, mode, block length and
    row length (include/sdrg.h)."""
    _fields_ = [("channel_rate", ctypes.c_double), ("max_offset_hz", ctypes.c_double), ("tau_blocks", ctypes.c_double),
                ("floor_db", ctypes.c_double), ("lock_threshold", ctypes.c_double), ("mode", ctypes.c_int32),
                ("block", ctypes.c_int32), ("max_in", ctypes.c_int32)]


class AfcDesign(ctypes.Structure):
    """sdrg_afc_design_values: the seven values of the AFC stage's design."""
    _fields_ = [(k, ctypes.c_float) for k in ("beta", "floor_thr", "lock_thr", "max_s", "K", "hz_per_inc",
                                              "rad_per_inc")]


# sdrg_afc_record
AfcRecord = np.dtype([("offset_hz", "<f4"), ("step", "<f4"), ("inc", "<i4"), ("coherence", "<f4"), ("level", "<f4"),
                      ("level_db", "<f4"), ("held_blocks", "<i4"), ("flags", "<i4")])
AFC_TRACK, AFC_MEASURE = 1, 2
AFC_LOCKED, AFC_SEEDED = 1, 2  # sdrg_afc_record.flags


class SymbolsConfig(ctypes.Structure):
    """sdrg_symbols_config: the symbol stage's rates, time constants, floor, lock threshold, trim, levels, block length,
    format and row length (include/sdrg.h)."""
    _fields_ = [(k, ctypes.c_double) for k in ("sample_rate", "symbol_rate", "tau_blocks", "tau_level_blocks", "floor_db",
                                               "lock_threshold", "phase_trim", "level_scale", "fixed_centre",
                                               "fixed_threshold")] + \
               [(k, ctypes.c_int32) for k in ("levels", "block", "level_mode", "format", "max_in")]


class SymbolsDesign(ctypes.Structure):
    """sdrg_symbols_design_values: the symbol stage's design but for the table."""
    _fields_ = [("trim", ctypes.c_int64), ("inc", ctypes.c_uint32)] + \
               [(k, ctypes.c_float) for k in ("rinc", "beta", "beta_level", "floor_thr", "lock_thr", "K", "rs",
                                              "scale", "centre", "threshold")]


# sdrg_symbols_record
SymbolsRecord = np.dtype([("tau_frac", "<f4"), ("tau", "<u4"), ("coherence", "<f4"), ("centre", "<f4"),
                          ("threshold", "<f4"), ("slips", "<i4"), ("held_blocks", "<i4"), ("flags", "<i4")])
SYM_LEVEL_TRACK, SYM_LEVEL_FIXED = 1, 2
SYM_HARD, SYM_SOFT = 1, 2
SYM_LOCKED, SYM_SEEDED = 1, 2  # sdrg_symbols_record.flags
SYM_UNLOCKED = 0x80            # a SYM_HARD byte sampled while unlocked
SYM_HISTORY, SYM_TABLE = 66, 1024


class BlankerConfig(ctypes.Structure):
    """sdrg_blanker_config: the noise blanker stage's time constant, threshold, floor, block length, window and row
    length (include/sdrg.h)."""
    _fields_ = [("tau_blocks", ctypes.c_double), ("threshold_db", ctypes.c_double), ("floor_db", ctypes.c_double),
                ("block", ctypes.c_int32), ("lead", ctypes.c_int32), ("tail", ctypes.c_int32),
                ("max_in", ctypes.c_int32)]


# sdrg_blanker_record
BlankerRecord = np.dtype([("level", "<f4"), ("level_db", "<f4"), ("hits", "<i4"), ("blanked", "<i4")])
CLEAN_IQCORR = 1  # SDRG_CLEAN_IQCORR
BLANKER_MAX_LEAD, BLANKER_MAX_TAIL = 16, 64


TONES_MAX_TONES, TONES_MAX_SUB_BLOCKS, TONES_MAX_IN = 64, 256, 65536
TONES_RECT, TONES_HANN = 0, 1


class TonesConfig(ctypes.Structure):
    """sdrg_tones_config: the tone detector stage's rate, frequencies, decision thresholds, components, tone count,
    block length in sub-blocks of 64, window, latch counts and row length (include/sdrg.h)."""
    _fields_ = [("rate_hz", ctypes.c_double), ("freq_hz", ctypes.c_double * TONES_MAX_TONES),
                ("min_db", ctypes.c_double), ("dominance_db", ctypes.c_double), ("share", ctypes.c_double),
                ("components", ctypes.c_int32), ("n_tones", ctypes.c_int32), ("sub_blocks", ctypes.c_int32),
                ("window", ctypes.c_int32), ("confirm_blocks", ctypes.c_int32), ("release_blocks", ctypes.c_int32),
                ("max_in", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class TonesScalars(ctypes.Structure):
    """sdrg_tones_scalars: the five scalars of the tone detector's design."""
    _fields_ = [("pnorm", ctypes.c_float), ("enorm", ctypes.c_float), ("min_power", ctypes.c_float),
                ("dom", ctypes.c_float), ("share_thr", ctypes.c_float)]


# sdrg_tones_record
TonesRecord = np.dtype([("tone", "<i4"), ("candidate", "<i4"), ("power", "<f4"), ("power_db", "<f4"), ("share", "<f4"),
                        ("tone_blocks", "<i4"), ("changes", "<i4"), ("run", "<i4")])


def _tones_filled(fields: dict) -> TonesConfig:
    """A TonesConfig of `fields`; freq_hz is a sequence of at most 64 frequencies, and n_tones defaults to its length."""
    fields = dict(fields)
    freq = [float(f) for f in fields.pop("freq_hz", ())]
    if len(freq) > TONES_MAX_TONES:
        raise TypeError(f"freq_hz has {len(freq)} entries, more than {TONES_MAX_TONES}")
    fields.setdefault("n_tones", len(freq))
    c = _filled(TonesConfig, "tones", fields)
    for k, f in enumerate(freq):
        c.freq_hz[k] = f
    return c


def _tones_dict(c: TonesConfig) -> dict:
    d = _as_dict(c)
    d["freq_hz"] = [c.freq_hz[k] for k in range(max(0, min(c.n_tones, TONES_MAX_TONES)))]
    del d["reserved"]
    return d


class AgcConfig(ctypes.Structure):
    """sdrg_agc_config: the AGC stage's target, gain limits, floor, attack and decay times, detector, block length,
    hang time and row length (include/sdrg.h)."""
    _fields_ = [("target", ctypes.c_double), ("max_gain_db", ctypes.c_double), ("initial_gain_db", ctypes.c_double),
                ("floor_db", ctypes.c_double), ("attack_blocks", ctypes.c_double), ("decay_blocks", ctypes.c_double),
                ("detector", ctypes.c_int32), ("block", ctypes.c_int32), ("hang_blocks", ctypes.c_int32),
                ("max_in", ctypes.c_int32)]


# sdrg_agc_record
AGC_RECORD_DTYPE = np.dtype([("gain", "<f4"), ("gain_db", "<f4"), ("level_db", "<f4"), ("attacks", "<i4")])
AGC_DET_MEAN, AGC_DET_PEAK = 0, 1
AGC_DESIGN_FIELDS = ("max_gain", "init_gain", "floor_thr", "alpha_a", "alpha_d")


class SidebandConfig(ctypes.Structure):
    """sdrg_sideband_config: the sideband stage's channel rate, band, mode, decimation, tap count, output format, row
    length and gain (include/sdrg.h)."""
    _fields_ = [("channel_rate_hz", ctypes.c_double), ("low_hz", ctypes.c_double), ("high_hz", ctypes.c_double),
                ("mode", ctypes.c_int32), ("audio_decimation", ctypes.c_int32), ("taps", ctypes.c_int32),
                ("out_format", ctypes.c_int32), ("max_in", ctypes.c_int32), ("gain", ctypes.c_float)]


# the steps of Engine.listen and Engine.listen_sideband (SDRG_LISTEN_*)
LISTEN_SQUELCH, LISTEN_AGC, LISTEN_RESAMPLE = 1, 2, 4


def _filled(cls, what: str, fields: dict):
    """A cls() (one of the configuration structures above) with `fields` set and the rest 0; `what` names the stage."""
    c = cls()
    for k, v in fields.items():
        if k not in dict(cls._fields_):
            raise TypeError(f"unknown {what} field {k!r}")
        setattr(c, k, v)
    return c


def _as_dict(c: ctypes.Structure) -> dict:
    return {k: getattr(c, k) for k, _ in c._fields_}


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class _Timings(ctypes.Structure):
    _fields_ = [("spectrum_ms", ctypes.c_float), ("stats_ms", ctypes.c_float), ("ssb_ms", ctypes.c_float),
                ("total_ms", ctypes.c_float)]


_V = ctypes.c_void_p
_I32, _I64, _F = ctypes.c_int32, ctypes.c_int64, ctypes.c_float
CB_FFT = ctypes.CFUNCTYPE(None, _V, _I32, ctypes.POINTER(ctypes.c_float), _I32)
CB_I = ctypes.CFUNCTYPE(None, _V, _I32, _I32)
CB_F = ctypes.CFUNCTYPE(None, _V, _I32, _F)
CB_J = ctypes.CFUNCTYPE(None, _V, _I32, _I64)
CB_PCM = ctypes.CFUNCTYPE(None, _V, _I32, ctypes.POINTER(ctypes.c_int16), _I32)
CB_FF = ctypes.CFUNCTYPE(None, _V, _I32, _F, _F)
CB_FIJ = ctypes.CFUNCTYPE(None, _V, _I32, _F, _I32, _I64)
CB_FI = ctypes.CFUNCTYPE(None, _V, _I32, _F, _I32)


class _Callbacks(ctypes.Structure):
    _fields_ = [
        ("user", _V),
        ("fft", CB_FFT),
        ("detection_flag", CB_I),
        ("mean_snr", CB_F),
        ("mean_snr_sigma", CB_F),
        ("peak_frequency", CB_J),
        ("pcm", CB_PCM),
        ("peak_above_noise_mean", CB_F),
        ("max_bin", CB_FF),
        ("best1khz", CB_FF),
        ("noise_level", CB_F),
        ("spectral_pulse", CB_FIJ),
        ("audio_pulse", CB_FI),
    ]


CB_SSB_PCM = ctypes.CFUNCTYPE(None, _V, ctypes.POINTER(ctypes.c_int16), _I32)
CB_SSB_PULSE = ctypes.CFUNCTYPE(None, _V, _F, _I32)


class _SsbCallbacks(ctypes.Structure):
    _fields_ = [("user", _V), ("pcm", CB_SSB_PCM), ("pulse", CB_SSB_PULSE)]


class _GatherBuffers(ctypes.Structure):
    _fields_ = [(k, _V) for k in ("records", "records_out", "focus_spectra", "focus_out", "spectra", "spectra_out",
                                  "pcm", "pcm_out")]


_lib = None


def lib_path() -> str:
    return LIB_PATH


def load() -> ctypes.CDLL:
    """Load libsdrg.so; raise if it has not been built (no CPU fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SdrgError(f"{LIB_PATH} not built: run `make -C sdr-for-android-lib_amd` "
                        "(or __graft_entry__.build())")
    L = ctypes.CDLL(LIB_PATH)
    P = ctypes.c_void_p
    sig = {
        "sdrg_abi_version": (_I32, []),
        "sdrg_last_error": (ctypes.c_char_p, []),
        "sdrg_ssb_pcm_len": (_I32, [_I32, _I64]),
        "sdrg_ssb_layout": (_I32, [_I64, _I32, _I32, ctypes.POINTER(SsbLayout)]),
        "sdrg_ssb_design": (_I32, [_I32, _I64, _I32, P, P, P, P, ctypes.POINTER(_I32)]),
        "sdrg_engine_create": (_I32, [ctypes.POINTER(_Config), _I32, _I32, ctypes.POINTER(P)]),
        "sdrg_engine_destroy": (_I32, [P]),
        "sdrg_engine_apply_config": (_I32, [P, ctypes.POINTER(_Config)]),
        "sdrg_engine_set_frequency": (_I32, [P, _I64]),
        "sdrg_engine_set_frequency_focus_range": (_I32, [P, _I32]),
        "sdrg_engine_set_sound_mode": (_I32, [P, _I32]),
        "sdrg_engine_set_sample_rate": (_I32, [P, _I64]),
        "sdrg_engine_set_samples_per_reading": (_I32, [P, _I32]),
        "sdrg_engine_input_released": (_I32, [P, ctypes.POINTER(_I32)]),
        "sdrg_engine_wait_input_released": (_I32, [P, P]),
        "sdrg_engine_set_upper_sideband": (_I32, [P, _I32]),
        "sdrg_engine_get_config": (_I32, [P, ctypes.POINTER(_Config)]),
        "sdrg_engine_n_streams": (_I32, [P]),
        "sdrg_engine_pcm_len": (_I32, [P]),
        "sdrg_engine_reset_state": (_I32, [P]),
        "sdrg_engine_process_device": (_I32, [P, P, _I32, _I32, P, P, P, _I64]),
        "sdrg_engine_synchronize": (_I32, [P]),
        "sdrg_engine_wait_outputs": (_I32, [P, P]),
        "sdrg_engine_set_stream": (_I32, [P, P]),
        "sdrg_engine_set_pipelining": (_I32, [P, _I32]),
        "sdrg_engine_set_ssb_variant": (_I32, [P, ctypes.c_double, _I32]),
        "sdrg_focus_window": (_I32, [_I64, _I32, _I32, P, P]),
        "sdrg_host_alloc": (_I32, [ctypes.c_size_t, P]),
        "sdrg_host_free": (_I32, [P]),
        "sdrg_engine_get_ssb_variant": (_I32, [P, P, P, P, P]),
        "sdrg_engine_process_host": (_I32, [P, P, _I32, _I32, P, P, P, _I64]),
        "sdrg_engine_signal_strength_device": (_I32, [P, P, P, _I64]),
        "sdrg_engine_signal_strength_host": (_I32, [P, P, P, _I64]),
        "sdrg_engine_set_callbacks": (_I32, [P, ctypes.POINTER(_Callbacks)]),
        "sdrg_engine_set_profiling": (_I32, [P, _I32]),
        "sdrg_engine_get_timings": (_I32, [P, ctypes.POINTER(_Timings)]),
        "sdrg_engine_get_timing_stats": (_I32, [P, ctypes.POINTER(_Timings), ctypes.POINTER(_I32)]),
        "sdrg_engine_reset_timing_stats": (_I32, [P]),
        "sdrg_engine_set_spectral_pulse_config": (_I32, [P, ctypes.POINTER(PulseConfig)]),
        "sdrg_engine_set_audio_pulse_config": (_I32, [P, ctypes.POINTER(PulseConfig)]),
        "sdrg_engine_pulse_outputs": (_I32, [P, ctypes.POINTER(P), ctypes.POINTER(P)]),
        "sdrg_engine_get_pulse_outputs": (_I32, [P, P, P]),
        "sdrg_pulse_config_default": (_I32, [_I32, ctypes.POINTER(PulseConfig)]),
        "sdrg_pulse_bank_create": (_I32, [_I32, ctypes.POINTER(PulseConfig), _I32, _I32, ctypes.POINTER(P)]),
        "sdrg_pulse_bank_destroy": (_I32, [P]),
        "sdrg_pulse_bank_configure": (_I32, [P, ctypes.POINTER(PulseConfig)]),
        "sdrg_pulse_bank_get_config": (_I32, [P, ctypes.POINTER(PulseConfig)]),
        "sdrg_pulse_bank_reset": (_I32, [P]),
        "sdrg_pulse_bank_process_spectral_device": (_I32, [P, P, P, _I32, P]),
        "sdrg_pulse_bank_process_audio_device": (_I32, [P, P, _I32, _I32, _I32, P]),
        "sdrg_pulse_bank_process_spectral_host": (_I32, [P, P, P, P]),
        "sdrg_pulse_bank_process_audio_host": (_I32, [P, P, _I32, _I32, P]),
        "sdrg_pulse_bank_synchronize": (_I32, [P]),
        "sdrg_pulse_bank_set_stream": (_I32, [P, P]),
        "sdrg_ingest_create": (_I32, [_I32, _I32, _I32, _I32, ctypes.POINTER(P)]),
        "sdrg_ingest_destroy": (_I32, [P]),
        "sdrg_ingest_output_format": (_I32, [P]),
        "sdrg_ingest_push": (_I32, [P, _I32, P, _I64]),
        "sdrg_ingest_status": (_I32, [P, _I32, ctypes.POINTER(_I32), ctypes.POINTER(_I32), ctypes.POINTER(_I64)]),
        "sdrg_ingest_pop_batch": (_I32, [P, P, ctypes.POINTER(_I32)]),
        "sdrg_ingest_pop": (_I32, [P, _I32, P, ctypes.POINTER(_I32)]),
        "sdrg_ingest_set_samples_per_reading": (_I32, [P, _I32]),
        "sdrg_ssb_processor_create": (_I32, [_I32, _I32, ctypes.POINTER(P)]),
        "sdrg_ssb_processor_destroy": (_I32, [P]),
        "sdrg_ssb_processor_start": (_I32, [P, ctypes.POINTER(_SsbCallbacks)]),
        "sdrg_ssb_processor_stop": (_I32, [P]),
        "sdrg_ssb_processor_enqueue": (_I32, [P, P, _I32, _I32, _I64]),
        "sdrg_ssb_processor_set_sound_mode": (_I32, [P, _I32]),
        "sdrg_ssb_processor_set_pulse_config": (_I32, [P, ctypes.POINTER(PulseConfig)]),
        "sdrg_ssb_processor_get_ambient_energy": (_F, [P]),
        "sdrg_ssb_processor_get_current_ratio": (_F, [P]),
        "sdrg_ssb_processor_drain": (_I32, [P]),
        "sdrg_ssb_processor_counters": (_I32, [P, ctypes.POINTER(_I64), ctypes.POINTER(_I64), ctypes.POINTER(_I64),
                                              ctypes.POINTER(_I32)]),
        "sdrg_dist_unique_id": (_I32, [P, _I32]),
        "sdrg_dist_create": (_I32, [P, _I32, _I32, _I32, ctypes.POINTER(P)]),
        "sdrg_dist_destroy": (_I32, [P]),
        "sdrg_dist_info": (_I32, [P, ctypes.POINTER(_I32), ctypes.POINTER(_I32), ctypes.POINTER(_I32),
                                  ctypes.POINTER(_I32)]),
        "sdrg_dist_set_one_rank_rccl": (_I32, [P, _I32]),
        "sdrg_engine_gather": (_I32, [P, P, _I32, ctypes.POINTER(_GatherBuffers)]),
        "sdrg_engine_gather_records": (_I32, [P, P, _I32, P, P]),
        "sdrg_engine_gather_focus": (_I32, [P, P, _I32, P, P]),
        "sdrg_engine_gather_spectra": (_I32, [P, P, _I32, P, P]),
        "sdrg_engine_gather_pcm": (_I32, [P, P, _I32, P, P]),
        "sdrg_device_alloc": (_I32, [_I32, ctypes.c_size_t, ctypes.POINTER(P)]),
        "sdrg_device_free": (_I32, [_I32, P]),
        "sdrg_memcpy": (_I32, [_I32, P, P, ctypes.c_size_t]),
        "sdrg_measure_hbm_copy": (_I32, [_I32, ctypes.c_size_t, _I32, ctypes.POINTER(ctypes.c_double)]),
        "sdrg_display_column_range": (_I32, [_I32, _I32, _I32, ctypes.POINTER(_I32), ctypes.POINTER(_I32)]),
        "sdrg_display_code": (_I32, [_F, _F, _F, ctypes.POINTER(ctypes.c_uint8)]),
        "sdrg_engine_set_display": (_I32, [P, ctypes.POINTER(DisplayConfig)]),
        "sdrg_engine_get_display": (_I32, [P, ctypes.POINTER(DisplayConfig)]),
        "sdrg_engine_display_geometry": (_I32, [P, ctypes.POINTER(_I32), ctypes.POINTER(_I32), ctypes.POINTER(_I32)]),
        "sdrg_engine_display_device": (_I32, [P, P, P]),
        "sdrg_engine_display_host": (_I32, [P, P, P]),
        "sdrg_engine_set_integration": (_I32, [P, ctypes.POINTER(IntegrateConfig)]),
        "sdrg_engine_get_integration": (_I32, [P, ctypes.POINTER(IntegrateConfig), ctypes.POINTER(_I32)]),
        "sdrg_engine_integrate_reset": (_I32, [P]),
        "sdrg_engine_integrate_device": (_I32, [P, P, P]),
        "sdrg_engine_integrate_host": (_I32, [P, P, P]),
        "sdrg_engine_display_integrated_host": (_I32, [P, P]),
        "sdrg_bin_offset_hz": (_I32, [_I32, _I64, _I32, ctypes.POINTER(ctypes.c_double)]),
        "sdrg_engine_set_peaks": (_I32, [P, ctypes.POINTER(PeaksConfig)]),
        "sdrg_engine_get_peaks": (_I32, [P, ctypes.POINTER(PeaksConfig)]),
        "sdrg_engine_peaks_device": (_I32, [P, P, P, P]),
        "sdrg_engine_peaks_host": (_I32, [P, P, P, P]),
        "sdrg_engine_peaks_integrated_host": (_I32, [P, P, P]),
        "sdrg_ddc_design": (_I32, [_I64, ctypes.POINTER(DdcConfig), P]),
        "sdrg_nco_tables": (_I32, [P]),
        "sdrg_ddc_tile_outputs": (_I32, [_I32, _I32, ctypes.POINTER(_I32)]),
        "sdrg_engine_set_ddc": (_I32, [P, ctypes.POINTER(DdcConfig)]),
        "sdrg_engine_get_ddc": (_I32, [P, ctypes.POINTER(DdcConfig), ctypes.POINTER(ctypes.c_uint32),
                                       ctypes.POINTER(ctypes.c_uint64)]),
        "sdrg_engine_ddc_reset": (_I32, [P]),
        "sdrg_engine_ddc_max_out": (_I32, [P, ctypes.POINTER(_I32)]),
        "sdrg_engine_ddc_device": (_I32, [P, P, _I32, P, ctypes.POINTER(_I32)]),
        "sdrg_engine_ddc_host": (_I32, [P, P, _I32, P, ctypes.POINTER(_I32)]),
        "sdrg_bank_geometry": (_I32, [_I32, _I32, _I32, _I32, ctypes.POINTER(_I32), ctypes.POINTER(_I32)]),
        "sdrg_engine_set_bank": (_I32, [P, ctypes.POINTER(BankConfig), P]),
        "sdrg_engine_bank_retune": (_I32, [P, P]),
        "sdrg_engine_get_bank": (_I32, [P, ctypes.POINTER(BankConfig), ctypes.POINTER(ctypes.c_uint64)]),
        "sdrg_engine_bank_offsets": (_I32, [P, P, P]),
        "sdrg_engine_bank_reset": (_I32, [P]),
        "sdrg_engine_bank_max_out": (_I32, [P, ctypes.POINTER(_I32)]),
        "sdrg_engine_bank_device": (_I32, [P, P, _I32, P, ctypes.POINTER(_I32)]),
        "sdrg_engine_bank_host": (_I32, [P, P, _I32, P, ctypes.POINTER(_I32)]),
        "sdrg_demod_design": (_I32, [ctypes.POINTER(DemodConfig), ctypes.POINTER(_F), ctypes.POINTER(_F),
                                     ctypes.POINTER(_F), P]),
        "sdrg_demod_geometry": (_I32, [_I32, _I32, ctypes.POINTER(_I32), ctypes.POINTER(_I32)]),
        "sdrg_engine_set_demod": (_I32, [P, ctypes.POINTER(DemodConfig)]),
        "sdrg_engine_get_demod": (_I32, [P, ctypes.POINTER(DemodConfig), ctypes.POINTER(_F), ctypes.POINTER(_F),
                                         ctypes.POINTER(_F), P, ctypes.POINTER(ctypes.c_uint64)]),
        "sdrg_engine_demod_reset": (_I32, [P]),
        "sdrg_engine_demod_max_out": (_I32, [P, ctypes.POINTER(_I32)]),
        "sdrg_engine_demod_device": (_I32, [P, P, _I32, P, ctypes.POINTER(_I32)]),
        "sdrg_engine_demod_host": (_I32, [P, P, _I32, P, ctypes.POINTER(_I32)]),
        "sdrg_engine_ddc_demod_host": (_I32, [P, P, _I32, P, ctypes.POINTER(_I32)]),
        "sdrg_channelizer_design": (_I32, [ctypes.POINTER(ChannelizerConfig), P]),
        "sdrg_channelizer_tile_outputs": (_I32, [ctypes.POINTER(ChannelizerConfig), ctypes.POINTER(_I32)]),
        "sdrg_engine_set_channelizer": (_I32, [P, ctypes.POINTER(ChannelizerConfig)]),
        "sdrg_engine_get_channelizer": (_I32, [P, ctypes.POINTER(ChannelizerConfig), ctypes.POINTER(ctypes.c_uint64)]),
        "sdrg_engine_channelizer_reset": (_I32, [P]),
        "sdrg_engine_channelizer_max_out": (_I32, [P, ctypes.POINTER(_I32)]),
        "sdrg_engine_channelizer_device": (_I32, [P, P, _I32, P, ctypes.POINTER(_I32)]),
        "sdrg_engine_channelizer_host": (_I32, [P, P, _I32, P, ctypes.POINTER(_I32)]),
        "sdrg_resample_design": (_I32, [ctypes.POINTER(ResampleConfig), P]),
        "sdrg_resample_tile_outputs": (_I32, [ctypes.POINTER(ResampleConfig), ctypes.POINTER(_I32)]),
        "sdrg_resample_ratio": (_I32, [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(_I32),
                                       ctypes.POINTER(_I32)]),
        "sdrg_engine_set_resample": (_I32, [P, ctypes.POINTER(ResampleConfig)]),
        "sdrg_engine_get_resample": (_I32, [P, ctypes.POINTER(ResampleConfig), P, ctypes.POINTER(ctypes.c_uint64)]),
        "sdrg_engine_resample_reset": (_I32, [P]),
        "sdrg_engine_resample_max_out": (_I32, [P, ctypes.POINTER(_I32)]),
        "sdrg_engine_resample_device": (_I32, [P, P, _I32, _I32, P, ctypes.POINTER(_I32)]),
        "sdrg_engine_resample_host": (_I32, [P, P, _I32, _I32, P, ctypes.POINTER(_I32)]),
        "sdrg_engine_ddc_demod_resample_host": (_I32, [P, P, _I32, P, ctypes.POINTER(_I32)]),
        "sdrg_squelch_design": (_I32, [ctypes.POINTER(SquelchConfig), ctypes.POINTER(_F), ctypes.POINTER(_F),
                                       ctypes.POINTER(_F)]),
        "sdrg_squelch_geometry": (_I32, [_I32, ctypes.POINTER(_I32)]),
        "sdrg_iqcorr_design": (_I32, [ctypes.POINTER(IqcorrConfig), ctypes.POINTER(_F), ctypes.POINTER(_F),
                                      ctypes.POINTER(_F)]),
        "sdrg_iqcorr_geometry": (_I32, [_I32, ctypes.POINTER(_I32)]),
        "sdrg_engine_set_iqcorr": (_I32, [P, ctypes.POINTER(IqcorrConfig)]),
        "sdrg_engine_get_iqcorr": (_I32, [P, ctypes.POINTER(IqcorrConfig), ctypes.POINTER(_F), ctypes.POINTER(_F),
                                          ctypes.POINTER(_F), ctypes.POINTER(ctypes.c_uint64)]),
        "sdrg_engine_iqcorr_reset": (_I32, [P]),
        "sdrg_engine_iqcorr_device": (_I32, [P, P, _I32, _I32, _I32, P, P, ctypes.POINTER(_I32)]),
        "sdrg_engine_iqcorr_host": (_I32, [P, P, _I32, _I32, _I32, P, P, ctypes.POINTER(_I32)]),
        "sdrg_engine_iqcorr_process_host": (_I32, [P, P, _I32, _I32, P, P, P, _I64, P]),
        "sdrg_blanker_design": (_I32, [ctypes.POINTER(BlankerConfig), ctypes.POINTER(_F), ctypes.POINTER(_F),
                                       ctypes.POINTER(_F)]),
        "sdrg_blanker_geometry": (_I32, [_I32, ctypes.POINTER(_I32), ctypes.POINTER(_I32)]),
        "sdrg_engine_set_blanker": (_I32, [P, ctypes.POINTER(BlankerConfig)]),
        "sdrg_engine_get_blanker": (_I32, [P, ctypes.POINTER(BlankerConfig), ctypes.POINTER(_F), ctypes.POINTER(_F),
                                           ctypes.POINTER(_F), ctypes.POINTER(ctypes.c_uint64)]),
        "sdrg_engine_blanker_reset": (_I32, [P]),
        "sdrg_engine_blanker_device": (_I32, [P, P, _I32, _I32, _I32, P, P, ctypes.POINTER(_I32)]),
        "sdrg_engine_blanker_host": (_I32, [P, P, _I32, _I32, _I32, P, P, ctypes.POINTER(_I32)]),
        "sdrg_engine_clean_process_host": (_I32, [P, P, _I32, _I32, _I32, P, P, P, _I64, P, P]),
        "sdrg_tones_design": (_I32, [ctypes.POINTER(TonesConfig), P, P, ctypes.POINTER(TonesScalars)]),
        "sdrg_tones_geometry": (_I32, [ctypes.POINTER(_I32)]),
        "sdrg_engine_set_tones": (_I32, [P, ctypes.POINTER(TonesConfig)]),
        "sdrg_engine_get_tones": (_I32, [P, ctypes.POINTER(TonesConfig), ctypes.POINTER(TonesScalars),
                                         ctypes.POINTER(ctypes.c_uint64)]),
        "sdrg_engine_tones_reset": (_I32, [P]),
        "sdrg_engine_tones_max_blocks": (_I32, [P, ctypes.POINTER(_I32)]),
        "sdrg_engine_tones_device": (_I32, [P, P, _I32, _I32, P, P, ctypes.POINTER(_I32)]),
        "sdrg_engine_tones_host": (_I32, [P, P, _I32, _I32, P, P, ctypes.POINTER(_I32)]),
        "sdrg_engine_listen_tones_host": (_I32, [P, _I32, P, _I32, P, ctypes.POINTER(_I32), P, P, P, P,
                                                 ctypes.POINTER(_I32)]),
        "sdrg_afc_design": (_I32, [ctypes.POINTER(AfcConfig), ctypes.POINTER(AfcDesign)]),
        "sdrg_afc_geometry": (_I32, [_I32, ctypes.POINTER(_I32)]),
        "sdrg_afc_offset_hz": (ctypes.c_double, [_I32, ctypes.c_double]),
        "sdrg_engine_set_afc": (_I32, [P, ctypes.POINTER(AfcConfig)]),
        "sdrg_engine_get_afc": (_I32, [P, ctypes.POINTER(AfcConfig), ctypes.POINTER(AfcDesign),
                                       ctypes.POINTER(ctypes.c_uint64)]),
        "sdrg_engine_afc_reset": (_I32, [P]),
        "sdrg_engine_afc_device": (_I32, [P, P, _I32, _I32, P, P, ctypes.POINTER(_I32)]),
        "sdrg_engine_afc_host": (_I32, [P, P, _I32, _I32, P, P, ctypes.POINTER(_I32)]),
        "sdrg_engine_listen_afc_host": (_I32, [P, _I32, P, _I32, P, ctypes.POINTER(_I32), P, P, P]),
        "sdrg_symbols_design": (_I32, [ctypes.POINTER(SymbolsConfig), ctypes.POINTER(SymbolsDesign), P]),
        "sdrg_symbols_geometry": (_I32, [_I32, ctypes.POINTER(_I32), ctypes.POINTER(_I32)]),
        "sdrg_symbols_count": (_I64, [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64]),
        "sdrg_engine_set_symbols": (_I32, [P, ctypes.POINTER(SymbolsConfig)]),
        "sdrg_engine_get_symbols": (_I32, [P, ctypes.POINTER(SymbolsConfig), ctypes.POINTER(SymbolsDesign),
                                            ctypes.POINTER(ctypes.c_uint64)]),
        "sdrg_engine_symbols_reset": (_I32, [P]),
        "sdrg_engine_symbols_max_out": (_I32, [P, ctypes.POINTER(_I32)]),
        "sdrg_engine_symbols_device": (_I32, [P, P, _I32, _I32, P, P, ctypes.POINTER(_I32)]),
        "sdrg_engine_symbols_host": (_I32, [P, P, _I32, _I32, P, P, ctypes.POINTER(_I32)]),
        "sdrg_engine_listen_symbols_host": (_I32, [P, _I32, P, _I32, P, ctypes.POINTER(_I32), P, P, P, P,
                                                    ctypes.POINTER(_I32)]),
        "sdrg_engine_set_squelch": (_I32, [P, ctypes.POINTER(SquelchConfig)]),
        "sdrg_engine_get_squelch": (_I32, [P, ctypes.POINTER(SquelchConfig), ctypes.POINTER(_F), ctypes.POINTER(_F),
                                           ctypes.POINTER(_F), ctypes.POINTER(ctypes.c_uint64)]),
        "sdrg_engine_squelch_reset": (_I32, [P]),
        "sdrg_engine_squelch_device": (_I32, [P, P, _I32, _I32, P, P, ctypes.POINTER(_I32)]),
        "sdrg_engine_squelch_host": (_I32, [P, P, _I32, _I32, P, P, ctypes.POINTER(_I32)]),
        "sdrg_engine_ddc_squelch_demod_host": (_I32, [P, P, _I32, P, ctypes.POINTER(_I32), P]),
        "sdrg_engine_ddc_squelch_demod_resample_host": (_I32, [P, P, _I32, P, ctypes.POINTER(_I32), P]),
        "sdrg_agc_design": (_I32, [ctypes.POINTER(AgcConfig)] + [ctypes.POINTER(_F)] * 5),
        "sdrg_agc_geometry": (_I32, [_I32, ctypes.POINTER(_I32)]),
        "sdrg_engine_set_agc": (_I32, [P, ctypes.POINTER(AgcConfig)]),
        "sdrg_engine_get_agc": (_I32, [P, ctypes.POINTER(AgcConfig)] + [ctypes.POINTER(_F)] * 5 +
                                [ctypes.POINTER(ctypes.c_uint64)]),
        "sdrg_engine_agc_reset": (_I32, [P]),
        "sdrg_engine_agc_device": (_I32, [P, P, _I32, _I32, P, P, ctypes.POINTER(_I32)]),
        "sdrg_engine_agc_host": (_I32, [P, P, _I32, _I32, P, P, ctypes.POINTER(_I32)]),
        "sdrg_engine_listen_host": (_I32, [P, _I32, P, _I32, P, ctypes.POINTER(_I32), P, P]),
        "sdrg_sideband_design": (_I32, [ctypes.POINTER(SidebandConfig), P, P]),
        "sdrg_sideband_geometry": (_I32, [_I32, _I32, ctypes.POINTER(_I32)]),
        "sdrg_engine_set_sideband": (_I32, [P, ctypes.POINTER(SidebandConfig)]),
        "sdrg_engine_get_sideband": (_I32, [P, ctypes.POINTER(SidebandConfig), P, P, ctypes.POINTER(ctypes.c_uint64)]),
        "sdrg_engine_sideband_reset": (_I32, [P]),
        "sdrg_engine_sideband_max_out": (_I32, [P, ctypes.POINTER(_I32)]),
        "sdrg_engine_sideband_device": (_I32, [P, P, _I32, P, ctypes.POINTER(_I32)]),
        "sdrg_engine_sideband_host": (_I32, [P, P, _I32, P, ctypes.POINTER(_I32)]),
        "sdrg_engine_listen_sideband_host": (_I32, [P, _I32, P, _I32, P, ctypes.POINTER(_I32), P, P]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def _check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().sdrg_last_error()
        raise SdrgError(f"{what}: {STATUS.get(rc, rc)}: {msg.decode() if msg else ''}")


def ssb_pcm_len(n: int, sample_rate: int) -> int:
    return int(load().sdrg_ssb_pcm_len(n, sample_rate))


def ssb_layout(sample_rate: int, n: int, fir_taps: int = 0) -> dict:
    """The SSB launcher's layout for a frame of n samples at sample_rate with fir_taps (0: 255), host-side, no device:
    decimation, taps, pcm_len, pipeline (False: the lane-per-stream kernels), slots (4, 8, 16 or 32; 0 without the
    pipeline), chunk, chunk_outputs and max_chunk_outputs."""
    o = SsbLayout()
    _check(load().sdrg_ssb_layout(sample_rate, n, fir_taps, ctypes.byref(o)), "ssb_layout")
    d = {k: int(getattr(o, k)) for k, _ in SsbLayout._fields_}
    d["pipeline"] = bool(d["pipeline"])
    return d


class HostBuffer:
    """Page-locked host memory (sdrg_host_alloc) viewed as a numpy array, for Engine.process outputs and inputs
    at the full PCIe rate.  Freed by close() or when garbage-collected."""

    def __init__(self, shape, dtype):
        self.dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape)) * self.dtype.itemsize
        p = ctypes.c_void_p()
        _check(load().sdrg_host_alloc(max(nbytes, 1), ctypes.byref(p)), "sdrg_host_alloc")
        self._p = p
        buf = (ctypes.c_char * max(nbytes, 1)).from_address(p.value)
        self.array = np.frombuffer(buf, dtype=self.dtype, count=int(np.prod(shape))).reshape(shape)

    def close(self) -> None:
        if getattr(self, "_p", None) is not None and self._p.value:
            self.array = None
            load().sdrg_host_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceBuffer:
    """Device memory through the C ABI (sdrg_device_alloc): a torch-free host can feed the engine and the gathers.
    upload / download are synchronous copies (not ordered with the engine's streams: synchronize the engine first)."""

    def __init__(self, nbytes: int, device: int = 0):
        self.device, self.nbytes = device, int(nbytes)
        p = ctypes.c_void_p()
        _check(load().sdrg_device_alloc(device, max(self.nbytes, 1), ctypes.byref(p)), "sdrg_device_alloc")
        self._p = p

    @property
    def ptr(self) -> int:
        return self._p.value

    def upload(self, a: np.ndarray) -> None:
        a = np.ascontiguousarray(a)
        if a.nbytes > self.nbytes:
            raise ValueError(f"{a.nbytes} bytes into a {self.nbytes}-byte device buffer")
        _check(load().sdrg_memcpy(self.device, self._p, a.ctypes.data_as(ctypes.c_void_p), a.nbytes), "sdrg_memcpy")

    def download(self, shape, dtype) -> np.ndarray:
        out = np.empty(shape, dtype)
        if out.nbytes > self.nbytes:
            raise ValueError(f"{out.nbytes} bytes from a {self.nbytes}-byte device buffer")
        _check(load().sdrg_memcpy(self.device, out.ctypes.data_as(ctypes.c_void_p), self._p, out.nbytes), "sdrg_memcpy")
        return out

    def close(self) -> None:
        if getattr(self, "_p", None) is not None and self._p.value:
            load().sdrg_device_free(self.device, self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def measure_hbm_copy(device: int = 0, nbytes: int = 1 << 30, reps: int = 10) -> float:
    """Read + write GB/s of the library's float4 streaming copy of nbytes (sdrg_measure_hbm_copy): the achievable
    HBM rate behind bench.py's roofline basis."""
    g = ctypes.c_double(0.0)
    _check(load().sdrg_measure_hbm_copy(device, nbytes, reps, ctypes.byref(g)), "sdrg_measure_hbm_copy")
    return g.value


def dist_unique_id() -> bytes:
    """ncclGetUniqueId (sdrg_dist_unique_id) on one rank; hand the bytes to every rank of the job."""
    buf = ctypes.create_string_buffer(DIST_ID_BYTES)
    _check(load().sdrg_dist_unique_id(buf, DIST_ID_BYTES), "sdrg_dist_unique_id")
    return buf.raw


class Dist:
    """An RCCL communicator over the job's ranks (sdrg_dist_create: one process per GPU).  Engine.gather moves the
    per-frame outputs of every rank's engine to a root rank with it."""

    def __init__(self, unique_id: bytes, world_size: int, rank: int, device: int = 0):
        if len(unique_id) != DIST_ID_BYTES:
            raise ValueError(f"unique id must be {DIST_ID_BYTES} bytes")
        h = ctypes.c_void_p()
        _check(load().sdrg_dist_create(ctypes.c_char_p(unique_id), world_size, rank, device, ctypes.byref(h)),
               "sdrg_dist_create")
        self._h, self.world_size, self.rank, self.device = h, world_size, rank, device

    def set_one_rank_rccl(self, on: bool) -> None:
        """One rank: gathers through ncclGather (True) or as device copies (False, the default)."""
        _check(load().sdrg_dist_set_one_rank_rccl(self._h, 1 if on else 0), "sdrg_dist_set_one_rank_rccl")

    def info(self) -> dict:
        r, w, v, x = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        _check(load().sdrg_dist_info(self._h, ctypes.byref(r), ctypes.byref(w), ctypes.byref(v), ctypes.byref(x)),
               "sdrg_dist_info")
        return {"rank": r.value, "world_size": w.value, "rccl_version": v.value, "rccl_data": bool(x.value)}

    def close(self) -> None:
        if getattr(self, "_h", None):
            load().sdrg_dist_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def focus_window(sample_rate: int, n: int, focus_khz: int) -> tuple[int, int]:
    """(first_bin, n_bins) of evaluateSignalStrength's focus window in the fftshifted spectrum (host-side)."""
    lo, nb = ctypes.c_int32(), ctypes.c_int32()
    _check(load().sdrg_focus_window(sample_rate, n, focus_khz, ctypes.byref(lo), ctypes.byref(nb)), "focus_window")
    return lo.value, nb.value


def display_column_range(n_bins: int, width: int, column: int) -> tuple[int, int]:
    """(first, count): the span-relative bins column `column` of `width` covers in a span of n_bins (host-side)."""
    first, count = ctypes.c_int32(), ctypes.c_int32()
    _check(load().sdrg_display_column_range(n_bins, width, column, ctypes.byref(first), ctypes.byref(count)),
           "display_column_range")
    return first.value, count.value


def display_code(db: float, db_min: float, db_max: float) -> int:
    """The display stage's 8-bit code of a dB value (host-side)."""
    code = ctypes.c_uint8()
    _check(load().sdrg_display_code(db, db_min, db_max, ctypes.byref(code)), "display_code")
    return code.value


def bin_offset_hz(n: int, sample_rate: int, bin: int) -> float:
    """The offset of bin `bin` of an fftshifted spectrum of n bins from the centre frequency, Hz (host-side)."""
    out = ctypes.c_double()
    _check(load().sdrg_bin_offset_hz(n, sample_rate, bin, ctypes.byref(out)), "bin_offset_hz")
    return out.value


def ddc_design(sample_rate: int, offset_hz: float = 0.0, cutoff_hz: float = 0.0, decimation: int = 1,
               taps: int = 1) -> np.ndarray:
    """The DDC stage's taps for a configuration at sample_rate (host-side, no device): float32 [taps]."""
    c = DdcConfig(offset_hz, cutoff_hz, decimation, taps)
    h = np.zeros(max(int(taps), 1) if 0 < int(taps) <= DDC_MAX_TAPS else 1, np.float32)
    _check(load().sdrg_ddc_design(sample_rate, ctypes.byref(c), h.ctypes.data_as(ctypes.c_void_p)), "ddc_design")
    return h


def nco_tables() -> np.ndarray:
    """The NCO's phasor tables (host-side): float32 [2][1024][2], hi then lo, {re, im}."""
    tab = np.zeros((2, 1024, 2), np.float32)
    _check(load().sdrg_nco_tables(tab.ctypes.data_as(ctypes.c_void_p)), "nco_tables")
    return tab


def ddc_tile_outputs(decimation: int, taps: int) -> int:
    """Consecutive outputs per workgroup of the DDC kernel for (decimation, taps)."""
    t = _I32()
    _check(load().sdrg_ddc_tile_outputs(decimation, taps, ctypes.byref(t)), "ddc_tile_outputs")
    return t.value


def bank_geometry(decimation: int, taps: int, channels: int, n_streams: int) -> tuple[int, int]:
    """(tile_outputs, channels_per_group) of the DDC bank's kernel: consecutive outputs, and consecutive channels of a
    stream, per workgroup (host-side)."""
    t, g = _I32(), _I32()
    _check(load().sdrg_bank_geometry(decimation, taps, channels, n_streams, ctypes.byref(t), ctypes.byref(g)),
           "bank_geometry")
    return t.value, g.value


def demod_design(**fields) -> dict:
    """The demodulator stage's design for a configuration (host-side, no device): kf, alpha, a as np.float32 and
    taps float32 [audio_taps].  The fields are sdrg_demod_config's (fields left out are 0)."""
    c = _filled(DemodConfig, "demod", fields)
    kf, alpha, a = _F(), _F(), _F()
    h = np.zeros(c.audio_taps if 0 < c.audio_taps <= DEMOD_MAX_TAPS else 1, np.float32)
    _check(load().sdrg_demod_design(ctypes.byref(c), ctypes.byref(kf), ctypes.byref(alpha), ctypes.byref(a),
                                    h.ctypes.data_as(ctypes.c_void_p)), "demod_design")
    return {"kf": np.float32(kf.value), "alpha": np.float32(alpha.value), "a": np.float32(a.value), "taps": h}


def demod_geometry(audio_decimation: int, audio_taps: int) -> tuple:
    """(tile, chunk): FIR outputs per workgroup for (R, T2), and samples per step of the recurrence kernel."""
    tile, chunk = _I32(), _I32()
    _check(load().sdrg_demod_geometry(audio_decimation, audio_taps, ctypes.byref(tile), ctypes.byref(chunk)),
           "demod_geometry")
    return tile.value, chunk.value


def channelizer_design(**fields) -> np.ndarray:
    """The channelizer stage's prototype for a configuration (host-side, no device): float32 [channels *
    taps_per_channel].  The fields are sdrg_channelizer_config's (fields left out are 0)."""
    c = _filled(ChannelizerConfig, "channelizer", fields)
    L = c.channels * c.taps_per_channel
    h = np.zeros(L if 0 < L <= CHANNELIZER_MAX_TAPS else 1, np.float32)
    _check(load().sdrg_channelizer_design(ctypes.byref(c), h.ctypes.data_as(ctypes.c_void_p)), "channelizer_design")
    return h


def channelizer_tile_outputs(**fields) -> int:
    """Consecutive output times per workgroup of the channelizer kernel for a configuration."""
    c, t = _filled(ChannelizerConfig, "channelizer", fields), _I32()
    _check(load().sdrg_channelizer_tile_outputs(ctypes.byref(c), ctypes.byref(t)), "channelizer_tile_outputs")
    return t.value


def resample_design(**fields) -> np.ndarray:
    """The resampler stage's prototype for a configuration (host-side, no device): float32 [interp * taps_per_phase].
    The fields are sdrg_resample_config's (fields left out are 0)."""
    c = _filled(ResampleConfig, "resample", fields)
    n = c.interp * c.taps_per_phase
    h = np.zeros(n if 0 < n <= RESAMPLE_MAX_TAPS else 1, np.float32)
    _check(load().sdrg_resample_design(ctypes.byref(c), h.ctypes.data_as(ctypes.c_void_p)), "resample_design")
    return h


def resample_tile_outputs(**fields) -> int:
    """Consecutive outputs per workgroup of the resampler kernel for a configuration."""
    c, t = _filled(ResampleConfig, "resample", fields), _I32()
    _check(load().sdrg_resample_tile_outputs(ctypes.byref(c), ctypes.byref(t)), "resample_tile_outputs")
    return t.value


def resample_ratio(in_num: int, in_den: int, out_hz: int) -> tuple[int, int]:
    """(interp, decim): out_hz * in_den / in_num in lowest terms, the ratio that takes in_num / in_den Hz to out_hz Hz;
    SdrgError if it is outside the resampler's limits.  (2_000_000, 41, 48_000) -> (123, 125)."""
    for v in (in_num, in_den, out_hz):
        if not 0 <= int(v) < 1 << 64:
            raise SdrgError(f"resample_ratio: {v} is not an unsigned 64-bit integer")
    L, M = _I32(), _I32()
    _check(load().sdrg_resample_ratio(int(in_num), int(in_den), int(out_hz), ctypes.byref(L), ctypes.byref(M)),
           "resample_ratio")
    return L.value, M.value


def squelch_design(**fields) -> dict:
    """The squelch stage's design for a configuration (host-side, no device): open_thr, close_thr and beta as
    np.float32.  The fields are sdrg_squelch_config's (fields left out are 0)."""
    c = _filled(SquelchConfig, "squelch", fields)
    o, cl, beta = _F(), _F(), _F()
    _check(load().sdrg_squelch_design(ctypes.byref(c), ctypes.byref(o), ctypes.byref(cl), ctypes.byref(beta)),
           "squelch_design")
    return {"open_thr": np.float32(o.value), "close_thr": np.float32(cl.value), "beta": np.float32(beta.value)}


def squelch_geometry(block: int) -> int:
    """tile: consecutive samples per workgroup of the squelch's power kernel (by global index) and of its gate kernel
    (by the call's index) for a block length."""
    t = _I32()
    _check(load().sdrg_squelch_geometry(block, ctypes.byref(t)), "squelch_geometry")
    return t.value


def iqcorr_design(**fields) -> dict:
    """The IQ correction stage's design for a configuration (host-side, no device): beta_dc, beta_bal and floor_thr as
    np.float32.  The fields are sdrg_iqcorr_config's (fields left out are 0)."""
    c = _filled(IqcorrConfig, "iqcorr", fields)
    bd, bb, fl = _F(), _F(), _F()
    _check(load().sdrg_iqcorr_design(ctypes.byref(c), ctypes.byref(bd), ctypes.byref(bb), ctypes.byref(fl)),
           "iqcorr_design")
    return {"beta_dc": np.float32(bd.value), "beta_bal": np.float32(bb.value), "floor_thr": np.float32(fl.value)}


def iqcorr_geometry(block: int) -> int:
    """tile: consecutive samples per workgroup of the IQ correction's moments kernel (by global index) and of its pass
    kernel (by the call's index) for a block length."""
    t = _I32()
    _check(load().sdrg_iqcorr_geometry(block, ctypes.byref(t)), "iqcorr_geometry")
    return t.value


def _afc_design_dict(d: AfcDesign) -> dict:
    return {k: np.float32(getattr(d, k)) for k, _ in AfcDesign._fields_}


def afc_design(**fields) -> dict:
    """The AFC stage's design for a configuration (host-side, no device): beta, floor_thr, lock_thr, max_s, K,
    hz_per_inc and rad_per_inc as np.float32.  The fields are sdrg_afc_config's (fields left out are 0)."""
    c, d = _filled(AfcConfig, "afc", fields), AfcDesign()
    _check(load().sdrg_afc_design(ctypes.byref(c), ctypes.byref(d)), "afc_design")
    return _afc_design_dict(d)


def _symbols_design_dict(d: SymbolsDesign) -> dict:
    return {k: (int(getattr(d, k)) if k in ("trim", "inc") else np.float32(getattr(d, k))) for k, _ in SymbolsDesign._fields_}


def symbols_design(**fields) -> dict:
    """The symbol stage's design for a configuration (host-side, no device): trim and inc as int, rinc, beta,
    beta_level, floor_thr, lock_thr, K, rs, scale, centre and threshold as np.float32, and `table`,
    float32 [SYM_TABLE][2] (cos, sin).  The fields are sdrg_symbols_config's (fields left out are 0)."""
    c, d = _filled(SymbolsConfig, "symbols", fields), SymbolsDesign()
    table = np.empty((SYM_TABLE, 2), np.float32)
    _check(load().sdrg_symbols_design(ctypes.byref(c), ctypes.byref(d), _ptr(table)), "symbols_design")
    return dict(_symbols_design_dict(d), table=table)


def symbols_geometry(block: int) -> tuple:
    """(tile, pass_tile): the consecutive values a workgroup of the symbol stage's moments kernel takes (by position in
    the run of blocks), and the consecutive symbols of a row a workgroup of its pass kernel writes."""
    t, q = _I32(), _I32()
    _check(load().sdrg_symbols_geometry(block, ctypes.byref(t), ctypes.byref(q)), "symbols_geometry")
    return t.value, q.value


def symbols_count(inc: int, g: int, n: int) -> int:
    """sdrg_symbols_count: the symbols a call of n values writes at stream position g."""
    r = int(load().sdrg_symbols_count(int(inc), int(g), int(n)))
    if r < 0:
        raise SdrgError("symbols_count: inc outside [2^26, 2^31]")
    return r


def afc_geometry(block: int) -> int:
    """tile: consecutive samples a workgroup of the AFC's moments kernel takes (by position in the run of blocks); a
    workgroup of its pass kernel takes four such tiles of the call's indices one after the other."""
    t = _I32()
    _check(load().sdrg_afc_geometry(block, ctypes.byref(t)), "afc_geometry")
    return t.value


def afc_offset_hz(inc: int, channel_rate: float) -> float:
    """A record's inc in Hz, in double: inc * channel_rate / 2^32 (NaN unless channel_rate is finite and positive)."""
    return float(load().sdrg_afc_offset_hz(int(inc), float(channel_rate)))


def blanker_design(**fields) -> dict:
    """The noise blanker stage's design for a configuration (host-side, no device): beta, ratio and floor_thr as
    np.float32.  The fields are sdrg_blanker_config's (fields left out are 0)."""
    c = _filled(BlankerConfig, "blanker", fields)
    beta, ratio, fl = _F(), _F(), _F()
    _check(load().sdrg_blanker_design(ctypes.byref(c), ctypes.byref(beta), ctypes.byref(ratio), ctypes.byref(fl)),
           "blanker_design")
    return {"beta": np.float32(beta.value), "ratio": np.float32(ratio.value), "floor_thr": np.float32(fl.value)}


def blanker_geometry(block: int) -> tuple[int, int]:
    """(floor_tile, pass_tile): consecutive positions per workgroup of the blanker's floor kernel (counted from the
    start of the block in progress) and consecutive outputs of the call per workgroup of its pass kernel."""
    f, t = _I32(), _I32()
    _check(load().sdrg_blanker_geometry(block, ctypes.byref(f), ctypes.byref(t)), "blanker_geometry")
    return f.value, t.value


def _scalars_dict(sc: TonesScalars) -> dict:
    return {k: np.float32(getattr(sc, k)) for k, _ in sc._fields_}


def tones_design(**fields) -> dict:
    """The tone detector stage's design for a configuration (host-side, no device): table float32 [K][S][2] (c, s), wf
    float32 [S] and pnorm, enorm, min_power, dom and share_thr as np.float32.  The fields are sdrg_tones_config's
    (fields left out are 0; freq_hz a sequence, n_tones its length unless given)."""
    c = _tones_filled(fields)
    _check(load().sdrg_tones_design(ctypes.byref(c), None, None, None), "tones_design")
    S, K, sc = 64 * c.sub_blocks, c.n_tones, TonesScalars()
    table, wf = np.empty((K, S, 2), np.float32), np.empty(S, np.float32)
    _check(load().sdrg_tones_design(ctypes.byref(c), _ptr(table), _ptr(wf), ctypes.byref(sc)), "tones_design")
    return dict(_scalars_dict(sc), table=table, wf=wf)


def tones_geometry() -> int:
    """Consecutive sub-blocks of 64 values per workgroup of the tone detector's correlate kernel, counted from the
    start of the sub-block in progress."""
    t = _I32()
    _check(load().sdrg_tones_geometry(ctypes.byref(t)), "tones_geometry")
    return t.value


def agc_design(**fields) -> dict:
    """The AGC stage's design for a configuration (host-side, no device): max_gain, init_gain, floor_thr, alpha_a and
    alpha_d as np.float32.  The fields are sdrg_agc_config's (fields left out are 0)."""
    c = _filled(AgcConfig, "agc", fields)
    v = [_F() for _ in AGC_DESIGN_FIELDS]
    _check(load().sdrg_agc_design(ctypes.byref(c), *[ctypes.byref(x) for x in v]), "agc_design")
    return {k: np.float32(x.value) for k, x in zip(AGC_DESIGN_FIELDS, v)}


def agc_geometry(block: int) -> int:
    """tile: consecutive samples per workgroup of the AGC's power kernel (counted from the start of the block in
    progress) and of its apply kernel (by the call's index) for a block length."""
    t = _I32()
    _check(load().sdrg_agc_geometry(block, ctypes.byref(t)), "agc_geometry")
    return t.value


def sideband_design(**fields) -> dict:
    """The sideband stage's band-pass for a configuration (host-side, no device): cr and ci, float32 [taps] each.  The
    fields are sdrg_sideband_config's (fields left out are 0)."""
    c = _filled(SidebandConfig, "sideband", fields)
    T = c.taps if 0 < c.taps <= SIDEBAND_MAX_TAPS else 1
    cr, ci = np.zeros(T, np.float32), np.zeros(T, np.float32)
    _check(load().sdrg_sideband_design(ctypes.byref(c), _ptr(cr), _ptr(ci)), "sideband_design")
    return dict(cr=cr, ci=ci)


def sideband_geometry(audio_decimation: int, taps: int) -> int:
    """How many consecutive outputs one workgroup of the sideband kernel computes for (R, T)."""
    tile = _I32()
    _check(load().sdrg_sideband_geometry(audio_decimation, taps, ctypes.byref(tile)), "sideband_geometry")
    return tile.value


def ssb_design(samp_count: int, sample_rate: int, sound_mode: int = 1) -> dict:
    """The engine's SSB filter design for a configuration (host-side, no device)."""
    lpf, hp, bp = (np.zeros(5, np.float32) for _ in range(3))
    taps = np.zeros(256, np.float32)
    nt = ctypes.c_int32()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    _check(load().sdrg_ssb_design(samp_count, sample_rate, sound_mode, p(lpf), p(hp), p(bp), p(taps),
                                  ctypes.byref(nt)), "ssb_design")
    return {"lpf": lpf, "hp": hp, "bp": bp, "taps": taps[: nt.value].copy()}


@dataclass
class SDRConfig:
    """Kotlin SDRConfig (SDRBridge.kt:23-37): same field names and defaults."""
    centerFrequency: int = 430_000_000
    samplesPerReading: int = 16384
    sampleRate: int = 2_500_000
    gain: int = 10
    freqFocusRangeKhz: int = 5
    refreshFFTMs: int = 50
    refreshPeakMs: int = 200
    refreshSignalStrengthMs: int = 30
    soundMode: int = 1

    def _c(self) -> _Config:
        return _Config(self.centerFrequency, self.sampleRate, self.samplesPerReading, self.freqFocusRangeKhz,
                       self.gain, self.soundMode, self.refreshFFTMs, self.refreshPeakMs, self.refreshSignalStrengthMs)


class Engine:
    """n_streams independent receivers on one GPU; each process call consumes one frame per stream."""

    def __init__(self, cfg: SDRConfig, n_streams: int, device: int = 0):
        L = load()
        h = ctypes.c_void_p()
        c = cfg._c()
        _check(L.sdrg_engine_create(ctypes.byref(c), n_streams, device, ctypes.byref(h)), "sdrg_engine_create")
        self._h = h
        self.n_streams = n_streams
        self.cfg = cfg
        self._cbs = None

    # ---- SDRBridge surface -------------------------------------------------------------------------
    def applyConfig(self, cfg: SDRConfig) -> bool:
        c = cfg._c()
        _check(load().sdrg_engine_apply_config(self._h, ctypes.byref(c)), "applyConfig")
        self.cfg = cfg
        return True

    def setFrequency(self, frequency: int) -> None:
        _check(load().sdrg_engine_set_frequency(self._h, frequency), "setFrequency")
        self.cfg.centerFrequency = frequency

    def setFrequencyFocusRange(self, khz: int) -> None:
        _check(load().sdrg_engine_set_frequency_focus_range(self._h, khz), "setFrequencyFocusRange")
        self.cfg.freqFocusRangeKhz = khz

    def setSoundMode(self, mode: int) -> None:
        _check(load().sdrg_engine_set_sound_mode(self._h, mode), "setSoundMode")
        self.cfg.soundMode = mode

    def setSampleRate(self, sample_rate: int) -> None:
        """JNI setSampleRate: BridgeConfig only (the SSB sees it next frame; the statistics at the next configure)."""
        _check(load().sdrg_engine_set_sample_rate(self._h, sample_rate), "setSampleRate")
        self.cfg.sampleRate = sample_rate

    def setSamplesPerReading(self, n: int) -> None:
        """JNI setSamplesPerReading: BridgeConfig only; the frame size of the next calls."""
        _check(load().sdrg_engine_set_samples_per_reading(self._h, n), "setSamplesPerReading")
        self.cfg.samplesPerReading = n

    def input_released(self) -> bool:
        """True once every kernel of the last call that reads its iq buffer has finished (non-blocking)."""
        r = ctypes.c_int32()
        _check(load().sdrg_engine_input_released(self._h, ctypes.byref(r)), "input_released")
        return bool(r.value)

    def wait_input_released(self, hip_stream: int | None = None) -> None:
        """Make hip_stream (None: the engine's main stream) wait until the last call has released its iq buffer."""
        _check(load().sdrg_engine_wait_input_released(self._h, hip_stream), "wait_input_released")

    def setUpperSideband(self, upper: bool) -> None:
        _check(load().sdrg_engine_set_upper_sideband(self._h, int(upper)), "setUpperSideband")

    def read(self, fftCallback=None, detectionFlagCallback=None, meanSnrCallback=None, meanSnrSigmaCallback=None,
             peakFrequencyCallback=None, pcmCallback=None, peakAboveNoiseMeanCallback=None, maxBinCallback=None,
             best1kHzCallback=None, noiseLevelCallback=None, spectralPulseCallback=None,
             audioPulseCallback=None) -> None:
        """Register per-frame callbacks (JNI read(), SDRBridge.kt:141-154).  Each receives the stream index
        first, then the reference callback's arguments; arrays arrive as numpy copies."""
        def wrap(fn, ctype, conv):
            if fn is None:
                return ctype()
            return ctype(lambda _u, s, *a: fn(s, *conv(*a)))

        n_of = lambda p, n: (np.ctypeslib.as_array(p, shape=(n,)).copy(),)  # noqa: E731
        ident = lambda *a: a  # noqa: E731
        self._cbs = _Callbacks(
            None,
            wrap(fftCallback, CB_FFT, n_of),
            wrap(detectionFlagCallback, CB_I, ident),
            wrap(meanSnrCallback, CB_F, ident),
            wrap(meanSnrSigmaCallback, CB_F, ident),
            wrap(peakFrequencyCallback, CB_J, ident),
            wrap(pcmCallback, CB_PCM, n_of),
            wrap(peakAboveNoiseMeanCallback, CB_F, ident),
            wrap(maxBinCallback, CB_FF, ident),
            wrap(best1kHzCallback, CB_FF, ident),
            wrap(noiseLevelCallback, CB_F, ident),
            wrap(spectralPulseCallback, CB_FIJ, ident),
            wrap(audioPulseCallback, CB_FI, ident),
        )
        _check(load().sdrg_engine_set_callbacks(self._h, ctypes.byref(self._cbs)), "read")

    def stopReading(self) -> None:
        _check(load().sdrg_engine_set_callbacks(self._h, None), "stopReading")
        self._cbs = None

    # ---- engine ------------------------------------------------------------------------------------
    @property
    def pcm_len(self) -> int:
        return int(load().sdrg_engine_pcm_len(self._h))

    def reset_state(self) -> None:
        _check(load().sdrg_engine_reset_state(self._h), "reset_state")

    def set_spectral_pulse_config(self, cfg: PulseConfig) -> None:
        """SpectralPulseDetector::configure for every stream (state kept)."""
        _check(load().sdrg_engine_set_spectral_pulse_config(self._h, ctypes.byref(cfg)), "set_spectral_pulse_config")

    def setPulseConfig(self, cfg: PulseConfig) -> None:
        """SSBProcessor::setPulseConfig: fresh AudioPulseDetectors with cfg from the next frame."""
        _check(load().sdrg_engine_set_audio_pulse_config(self._h, ctypes.byref(cfg)), "setPulseConfig")

    def pulse_outputs(self, spectral: bool = True, audio: bool = True):
        """Host copies of the last call's pulse-detector outputs (PULSE_OUTPUT_DTYPE arrays, or None)."""
        sp = np.zeros(self.n_streams, PULSE_OUTPUT_DTYPE) if spectral else None
        au = np.zeros(self.n_streams, PULSE_OUTPUT_DTYPE) if audio else None
        ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        _check(load().sdrg_engine_get_pulse_outputs(self._h, ptr(sp), ptr(au)), "get_pulse_outputs")
        return sp, au

    def pulse_output_ptrs(self):
        """Device pointers of the last call's pulse outputs (valid until the next call)."""
        a, b = ctypes.c_void_p(), ctypes.c_void_p()
        _check(load().sdrg_engine_pulse_outputs(self._h, ctypes.byref(a), ctypes.byref(b)), "pulse_outputs")
        return a.value, b.value

    def process(self, iq: np.ndarray, fmt: int = CS8, stages: int = STAGE_ALL, now_ms: int = 0, out=None):
        """Host path: iq is [n_streams][samplesPerReading * 2] raw samples. Returns (spectra, records, pcm).

        out: optional (spectra, records, pcm) arrays to write into (e.g. HostBuffer arrays, page-locked, for the
        full PCIe rate); entries for stages not run may be None.  By default fresh arrays are allocated."""
        n = self.cfg.samplesPerReading
        iq = self._iq(iq, fmt)
        plen = self.pcm_len
        if out is not None:
            spec, recs, pcm = out
            for a, shape, dt in ((spec, (self.n_streams, n), np.float32), (recs, (self.n_streams,), RECORD_DTYPE),
                                 (pcm, (self.n_streams, max(plen, 0)), np.int16)):
                if a is not None and (a.shape != shape or a.dtype != dt or not a.flags.c_contiguous):
                    raise SdrgError(f"out array {a.shape} {a.dtype}: expected contiguous {shape} {np.dtype(dt)}")
            if (stages & STAGE_SPECTRUM and spec is None) or (stages & STAGE_STATS and recs is None) or \
                    (stages & STAGE_SSB and pcm is None):
                raise SdrgError("out lacks an array for a requested stage")
        else:
            spec = np.empty((self.n_streams, n), np.float32) if stages & STAGE_SPECTRUM else None
            recs = np.zeros(self.n_streams, RECORD_DTYPE) if stages & STAGE_STATS else None
            pcm = np.empty((self.n_streams, max(plen, 0)), np.int16) if stages & STAGE_SSB else None
        _check(load().sdrg_engine_process_host(self._h, _ptr(iq), fmt, stages, _ptr(spec), _ptr(recs),
                                               _ptr(pcm) if plen > 0 else None, now_ms), "process_host")
        return spec, recs, pcm

    def _iq(self, iq: np.ndarray, fmt: int) -> np.ndarray:
        """A frame per stream, [n_streams][samplesPerReading * 2] raw samples: contiguous, in the type of fmt."""
        n = self.cfg.samplesPerReading
        iq = np.ascontiguousarray(iq, dtype=NUMPY_DTYPE[fmt])
        if iq.size != self.n_streams * n * 2:
            raise SdrgError(f"iq has {iq.size} values, expected {self.n_streams}x{n}x2")
        return iq

    def _spectra(self, spectra: np.ndarray | None):
        """(array, its pointer) of caller spectra as contiguous float32 [n_streams][samplesPerReading], the array to be
        kept alive over the call; (None, None) for None."""
        if spectra is None:
            return None, None
        n = self.cfg.samplesPerReading
        spectra = np.ascontiguousarray(spectra, dtype=np.float32)
        if spectra.shape != (self.n_streams, n):
            raise SdrgError(f"spectra {spectra.shape}: expected ({self.n_streams}, {n})")
        return spectra, _ptr(spectra)

    def _set_stage(self, cls, what: str, fields: dict) -> None:
        """sdrg_engine_set_<what> with a cls of `fields`, or for off=True with a null configuration: the stage off."""
        off = fields.pop("off", False)
        if off and fields:
            raise TypeError("off=True takes no other field")
        c = None if off else ctypes.byref(_filled(cls, what, fields))
        _check(getattr(load(), "sdrg_engine_set_" + what)(self._h, c), "set_" + what)

    def _i32_call(self, fn, what: str, *args) -> int:
        """fn(h, *args, &value) of the library: the int32 it writes, a stage's max_out or a call's n_out."""
        value = _I32()
        _check(fn(self._h, *args, ctypes.byref(value)), what)
        return value.value

    def _iq_call(self, fn, what: str, iq: np.ndarray, fmt: int, make_out) -> np.ndarray:
        """A host call fn of the library on a frame per stream: the rows make_out() allocates, cut to its n_out."""
        iq = self._iq(iq, fmt)
        out = make_out()
        return out[..., :self._i32_call(fn, what, _ptr(iq), fmt, _ptr(out))]

    def signal_strength(self, spectra: np.ndarray, now_ms: int = 0) -> np.ndarray:
        """evaluateSignalStrength alone on caller spectra ([n_streams][samplesPerReading] fftshifted linear power,
        fft_process.cpp:122-379): returns the records; each stream's statistics state advances as in process()."""
        spectra, ptr = self._spectra(np.asarray(spectra))  # no spectra are no source here: a wrong shape
        recs = np.zeros(self.n_streams, RECORD_DTYPE)
        _check(load().sdrg_engine_signal_strength_host(self._h, ptr, _ptr(recs), now_ms), "signal_strength_host")
        return recs

    # ---- display stage ----------------------------------------------------------------------------
    def set_display(self, **fields) -> None:
        """sdrg_engine_set_display: span, first_bin, n_bins, width, reduce, format, db_min, db_max (fields left out
        are 0: the full span, MAX, float dB).  A rejected configuration leaves the previous one in force."""
        c = _filled(DisplayConfig, "display", fields)
        _check(load().sdrg_engine_set_display(self._h, ctypes.byref(c)), "set_display")

    def display_config(self) -> dict:
        c = DisplayConfig()
        _check(load().sdrg_engine_get_display(self._h, ctypes.byref(c)), "get_display")
        return _as_dict(c)

    def _display_rows(self) -> np.ndarray:
        cfg = self.display_config()
        return np.empty((self.n_streams, cfg["width"]), np.uint8 if cfg["format"] == DISPLAY_U8 else np.float32)

    def display_geometry(self) -> tuple[int, int, int]:
        """(first_bin, n_bins, row_bytes) the next display call would use."""
        lo, nb, rb = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        _check(load().sdrg_engine_display_geometry(self._h, ctypes.byref(lo), ctypes.byref(nb), ctypes.byref(rb)),
               "display_geometry")
        return lo.value, nb.value, rb.value

    def display_device(self, spectra_ptr: int, out_ptr: int) -> None:
        """Device path: spectra [n_streams][N] float32 in, display rows [n_streams][row_bytes] out; asynchronous on the
        main stream (right after process_device it reads that call's spectra)."""
        _check(load().sdrg_engine_display_device(self._h, spectra_ptr, out_ptr), "display_device")

    def display(self, spectra: np.ndarray | None = None) -> np.ndarray:
        """Host path: the display rows [n_streams][width], float32 dB or uint8 codes, of caller spectra
        ([n_streams][samplesPerReading] float32) or, with None, of the spectra the last process() call with
        STAGE_SPECTRUM left on the device."""
        out = self._display_rows()
        spectra, ptr = self._spectra(spectra)
        _check(load().sdrg_engine_display_host(self._h, ptr, _ptr(out)), "display_host")
        return out

    # ---- integration stage ------------------------------------------------------------------------
    def set_integration(self, mode: int = INTEGRATE_MEAN, period: int = 0, alpha: float = 0.0) -> None:
        """sdrg_engine_set_integration: MEAN / MAX over the last `period` frames (1 .. 64) or EMA with `alpha` in
        (0, 1].  Resets the history; a rejected configuration leaves the previous one and its history in force."""
        c = IntegrateConfig(mode, period, alpha)
        _check(load().sdrg_engine_set_integration(self._h, ctypes.byref(c)), "set_integration")

    def integration(self) -> dict:
        """The configuration in force and `depth`, the number of frames the last output integrates (0 after a
        reset)."""
        c, depth = IntegrateConfig(), ctypes.c_int32()
        _check(load().sdrg_engine_get_integration(self._h, ctypes.byref(c), ctypes.byref(depth)), "get_integration")
        return dict(mode=c.mode, period=c.period, alpha=c.alpha, depth=depth.value)

    def integration_depth(self) -> int:
        depth = ctypes.c_int32()
        _check(load().sdrg_engine_get_integration(self._h, None, ctypes.byref(depth)), "get_integration")
        return depth.value

    def integrate_reset(self) -> None:
        _check(load().sdrg_engine_integrate_reset(self._h), "integrate_reset")

    def integrate_device(self, spectra_ptr: int, out_ptr: int) -> None:
        """Device path: spectra [n_streams][N] float32 in, integrated rows of the same shape out (out_ptr may be
        spectra_ptr); asynchronous on the main stream (right after process_device it reads that call's spectra)."""
        _check(load().sdrg_engine_integrate_device(self._h, spectra_ptr, out_ptr), "integrate_device")

    def integrate(self, spectra: np.ndarray | None = None, want_output: bool = True) -> np.ndarray | None:
        """Host path: feeds caller spectra ([n_streams][samplesPerReading] float32) or, with None, the spectra the
        last process() call with STAGE_SPECTRUM left on the device, and returns the integrated rows; with
        want_output=False they stay on the device (display_integrated() shows them) and None is returned."""
        spectra, ptr = self._spectra(spectra)
        out = np.empty((self.n_streams, self.cfg.samplesPerReading), np.float32) if want_output else None
        _check(load().sdrg_engine_integrate_host(self._h, ptr, _ptr(out)), "integrate_host")
        return out

    def display_integrated(self) -> np.ndarray:
        """The display rows [n_streams][width] (current display configuration) of the rows the last integrate() call
        left on the device."""
        out = self._display_rows()
        _check(load().sdrg_engine_display_integrated_host(self._h, _ptr(out)), "display_integrated_host")
        return out

    # ---- peak table stage ------------------------------------------------------------------------
    def set_peaks(self, **fields) -> None:
        """sdrg_engine_set_peaks: span, first_bin, n_bins, max_peaks, min_separation, threshold_db (fields left out
        are 0)."""
        c = _filled(PeaksConfig, "peaks", fields)
        _check(load().sdrg_engine_set_peaks(self._h, ctypes.byref(c)), "set_peaks")

    def peaks_config(self) -> dict:
        c = PeaksConfig()
        _check(load().sdrg_engine_get_peaks(self._h, ctypes.byref(c)), "get_peaks")
        return _as_dict(c)

    def peaks_device(self, spectra_ptr: int, peaks_ptr: int, summary_ptr: int) -> None:
        """Device path: spectra [n_streams][N] float32 in, peaks [n_streams][max_peaks] PEAK_DTYPE and summary
        [n_streams] PEAKS_SUMMARY_DTYPE out; asynchronous on the main stream."""
        _check(load().sdrg_engine_peaks_device(self._h, spectra_ptr, peaks_ptr, summary_ptr), "peaks_device")

    def _peaks_out(self):
        k = self.peaks_config()["max_peaks"]
        return np.empty((self.n_streams, k), PEAK_DTYPE), np.empty(self.n_streams, PEAKS_SUMMARY_DTYPE)

    def peaks(self, spectra: np.ndarray | None = None):
        """Host path: (peaks [n_streams][max_peaks], summary [n_streams]) of caller spectra [n_streams][N], or, with
        spectra=None, of the spectra the last process() call with STAGE_SPECTRUM left on the device."""
        pk, sm = self._peaks_out()
        spectra, ptr = self._spectra(spectra)
        _check(load().sdrg_engine_peaks_host(self._h, ptr, _ptr(pk), _ptr(sm)), "peaks_host")
        return pk, sm

    def peaks_integrated(self):
        """(peaks, summary) of the rows the last integrate() call left on the device."""
        pk, sm = self._peaks_out()
        _check(load().sdrg_engine_peaks_integrated_host(self._h, _ptr(pk), _ptr(sm)), "peaks_integrated_host")
        return pk, sm

    # ---- DDC stage -------------------------------------------------------------------------------
    def set_ddc(self, **fields) -> None:
        """sdrg_engine_set_ddc: offset_hz, cutoff_hz, decimation, taps (fields left out are 0); set_ddc(off=True)
        switches the stage off."""
        self._set_stage(DdcConfig, "ddc", fields)

    def ddc_config(self) -> dict:
        """The configuration in force, plus nco_increment (at the current sample rate) and samples_consumed."""
        c, inc, g0 = DdcConfig(), ctypes.c_uint32(), ctypes.c_uint64()
        _check(load().sdrg_engine_get_ddc(self._h, ctypes.byref(c), ctypes.byref(inc), ctypes.byref(g0)), "get_ddc")
        return dict(_as_dict(c), nco_increment=inc.value, samples_consumed=g0.value)

    def ddc_reset(self) -> None:
        _check(load().sdrg_engine_ddc_reset(self._h), "ddc_reset")

    def ddc_max_out(self) -> int:
        """ceil(samplesPerReading / decimation): the row length of a ddc call's output, in complex samples."""
        return self._i32_call(load().sdrg_engine_ddc_max_out, "ddc_max_out")

    def ddc_device(self, iq_ptr: int, fmt: int, out_ptr: int) -> int:
        """Device path: iq [n_streams][N] raw samples in, out [n_streams][ddc_max_out()] complex64 out; asynchronous
        on the main stream.  Returns n_out, the outputs this call produced per stream (the rest of a row is zero)."""
        return self._i32_call(load().sdrg_engine_ddc_device, "ddc_device", iq_ptr, fmt, out_ptr)

    def ddc(self, iq: np.ndarray, fmt: int = CS8) -> np.ndarray:
        """Host path: iq is [n_streams][samplesPerReading * 2] raw samples; returns complex64 [n_streams][n_out]."""
        return self._iq_call(load().sdrg_engine_ddc_host, "ddc_host", iq, fmt,
                             lambda: np.empty((self.n_streams, self.ddc_max_out()), np.complex64))

    # ---- DDC bank stage --------------------------------------------------------------------------
    def _bank_offsets(self, offsets_hz, channels: int) -> np.ndarray:
        """offsets_hz as contiguous float64 [n_streams][channels]."""
        o = np.ascontiguousarray(offsets_hz, dtype=np.float64)
        if o.shape != (self.n_streams, channels):
            raise SdrgError(f"offsets_hz {o.shape}: expected ({self.n_streams}, {channels})")
        return o

    def set_bank(self, offsets_hz=None, **fields) -> None:
        """sdrg_engine_set_bank: offsets_hz [n_streams][C] and cutoff_hz, decimation, taps (fields left out are 0);
        channels is offsets_hz's C unless given.  set_bank(off=True) switches the stage off."""
        if fields.pop("off", False):
            if fields or offsets_hz is not None:
                raise TypeError("off=True takes no other field")
            _check(load().sdrg_engine_set_bank(self._h, None, None), "set_bank")
            return
        if offsets_hz is None:
            raise TypeError("set_bank needs offsets_hz")
        o = np.ascontiguousarray(offsets_hz, dtype=np.float64)
        fields.setdefault("channels", o.shape[-1] if o.ndim == 2 else 0)
        c = _filled(BankConfig, "bank", fields)
        o = self._bank_offsets(o, c.channels)  # the library reads n_streams * channels values
        _check(load().sdrg_engine_set_bank(self._h, ctypes.byref(c), _ptr(o)), "set_bank")

    def bank_retune(self, offsets_hz) -> None:
        """sdrg_engine_bank_retune: replace all offsets [n_streams][C]; restarts nothing (see include/sdrg.h)."""
        o = self._bank_offsets(offsets_hz, self.bank_config()["channels"])
        _check(load().sdrg_engine_bank_retune(self._h, _ptr(o)), "bank_retune")

    def bank_config(self) -> dict:
        """The configuration in force, plus samples_consumed."""
        c, g0 = BankConfig(), ctypes.c_uint64()
        _check(load().sdrg_engine_get_bank(self._h, ctypes.byref(c), ctypes.byref(g0)), "get_bank")
        return dict(_as_dict(c), samples_consumed=g0.value)

    def bank_offsets(self) -> tuple[np.ndarray, np.ndarray]:
        """(offsets_hz float64, increments uint32 at the current sample rate), each [n_streams][C]."""
        C = self.bank_config()["channels"]
        o, inc = np.zeros((self.n_streams, C), np.float64), np.zeros((self.n_streams, C), np.uint32)
        _check(load().sdrg_engine_bank_offsets(self._h, _ptr(o), _ptr(inc)), "bank_offsets")
        return o, inc

    def bank_reset(self) -> None:
        _check(load().sdrg_engine_bank_reset(self._h), "bank_reset")

    def bank_max_out(self) -> int:
        """ceil(samplesPerReading / decimation): the row length of a bank call's output, in complex samples."""
        return self._i32_call(load().sdrg_engine_bank_max_out, "bank_max_out")

    def bank_device(self, iq_ptr: int, fmt: int, out_ptr: int) -> int:
        """Device path: iq [n_streams][N] raw samples in, out [n_streams][C][bank_max_out()] complex64 out;
        asynchronous on the main stream.  Returns n_out, the outputs this call produced per row (the rest is zero)."""
        return self._i32_call(load().sdrg_engine_bank_device, "bank_device", iq_ptr, fmt, out_ptr)

    def bank(self, iq: np.ndarray, fmt: int = CS8) -> np.ndarray:
        """Host path: iq is [n_streams][samplesPerReading * 2] raw samples; returns complex64 [n_streams][C][n_out]."""
        C = self.bank_config()["channels"]
        return self._iq_call(load().sdrg_engine_bank_host, "bank_host", iq, fmt,
                             lambda: np.empty((self.n_streams, C, self.bank_max_out()), np.complex64))

    # ---- demodulator stage -----------------------------------------------------------------------
    def set_demod(self, **fields) -> None:
        """sdrg_engine_set_demod: the fields of sdrg_demod_config (fields left out are 0); set_demod(off=True) switches
        the stage off."""
        self._set_stage(DemodConfig, "demod", fields)

    def demod_config(self) -> dict:
        """The configuration in force, plus its design (kf, alpha, a as np.float32, taps) and samples_consumed."""
        c, kf, alpha, a, g = DemodConfig(), _F(), _F(), _F(), ctypes.c_uint64()
        h = np.zeros(DEMOD_MAX_TAPS, np.float32)
        _check(load().sdrg_engine_get_demod(self._h, ctypes.byref(c), ctypes.byref(kf), ctypes.byref(alpha),
                                            ctypes.byref(a), h.ctypes.data_as(ctypes.c_void_p), ctypes.byref(g)),
               "get_demod")
        return dict(_as_dict(c), kf=np.float32(kf.value), alpha=np.float32(alpha.value), a=np.float32(a.value),
                    taps=h[:c.audio_taps].copy(), samples_consumed=g.value)

    def demod_reset(self) -> None:
        _check(load().sdrg_engine_demod_reset(self._h), "demod_reset")

    def demod_max_out(self) -> int:
        """ceil(max_in / audio_decimation): the row length of a demod call's output."""
        return self._i32_call(load().sdrg_engine_demod_max_out, "demod_max_out")

    def demod_device(self, chan_ptr: int, n: int, out_ptr: int) -> int:
        """Device path: chan [n_streams][max_in] complex64 in (the first n of every row are the call's), out
        [n_streams][demod_max_out()] int16 or float32 out; asynchronous on the main stream.  Returns n_out."""
        return self._i32_call(load().sdrg_engine_demod_device, "demod_device", chan_ptr, n, out_ptr)

    def _demod_out(self) -> np.ndarray:
        fmt = self.demod_config()["out_format"]
        return np.empty((self.n_streams, self.demod_max_out()), DEMOD_OUT_DTYPE[fmt])

    def demod(self, chan: np.ndarray) -> np.ndarray:
        """Host path: chan is complex64 [n_streams][n], n <= max_in; returns int16 or float32 [n_streams][n_out]."""
        chan = np.asarray(chan, np.complex64).reshape(self.n_streams, -1)
        n, max_in = chan.shape[1], self.demod_config()["max_in"]
        if n > max_in:
            raise SdrgError(f"chan has {n} samples per stream, max_in is {max_in}")
        rows = np.zeros((self.n_streams, max_in), np.complex64)
        rows[:, :n] = chan
        out = self._demod_out()
        n_out = _I32()
        _check(load().sdrg_engine_demod_host(self._h, rows.ctypes.data_as(ctypes.c_void_p), n,
                                             out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n_out)), "demod_host")
        return out[:, :n_out.value]

    def ddc_demod(self, iq: np.ndarray, fmt: int = CS8) -> np.ndarray:
        """Tune and listen: iq [n_streams][samplesPerReading * 2] raw samples through the DDC and the demodulator, the
        channel left on the device; returns the audio, int16 or float32 [n_streams][n_out]."""
        return self._iq_call(load().sdrg_engine_ddc_demod_host, "ddc_demod_host", iq, fmt, self._demod_out)

    # ---- channelizer stage ------------------------------------------------------------------------
    def set_channelizer(self, **fields) -> None:
        """sdrg_engine_set_channelizer: cutoff_rel, channels, taps_per_channel, oversample, first_channel, n_channels
        (fields left out are 0); set_channelizer(off=True) switches the stage off."""
        self._set_stage(ChannelizerConfig, "channelizer", fields)

    def channelizer_config(self) -> dict:
        """The configuration in force, plus samples_consumed."""
        c, g0 = ChannelizerConfig(), ctypes.c_uint64()
        _check(load().sdrg_engine_get_channelizer(self._h, ctypes.byref(c), ctypes.byref(g0)), "get_channelizer")
        return dict(_as_dict(c), samples_consumed=g0.value)

    def channelizer_reset(self) -> None:
        _check(load().sdrg_engine_channelizer_reset(self._h), "channelizer_reset")

    def channelizer_max_out(self) -> int:
        """ceil(samplesPerReading / (channels / oversample)): the row length of a channelizer call's output."""
        return self._i32_call(load().sdrg_engine_channelizer_max_out, "channelizer_max_out")

    def channelizer_device(self, iq_ptr: int, fmt: int, out_ptr: int) -> int:
        """Device path: iq [n_streams][N] raw samples in, out [n_streams][n_channels][channelizer_max_out()] complex64
        out; asynchronous on the main stream.  Returns n_out, the outputs this call produced per row (the rest of a row
        is zero)."""
        return self._i32_call(load().sdrg_engine_channelizer_device, "channelizer_device", iq_ptr, fmt, out_ptr)

    def channelizer(self, iq: np.ndarray, fmt: int = CS8) -> np.ndarray:
        """Host path: iq is [n_streams][samplesPerReading * 2] raw samples; returns complex64
        [n_streams][n_channels][n_out]."""
        def rows():
            n_rows = self.channelizer_config()["n_channels"]
            return np.empty((self.n_streams, n_rows, self.channelizer_max_out()), np.complex64)
        return self._iq_call(load().sdrg_engine_channelizer_host, "channelizer_host", iq, fmt, rows)

    # ---- resampler stage --------------------------------------------------------------------------
    def set_resample(self, **fields) -> None:
        """sdrg_engine_set_resample: the fields of sdrg_resample_config (fields left out are 0); set_resample(off=True)
        switches the stage off."""
        self._set_stage(ResampleConfig, "resample", fields)

    def resample_config(self) -> dict:
        """The configuration in force, plus its prototype (taps) and samples_consumed."""
        c, g = ResampleConfig(), ctypes.c_uint64()
        h = np.zeros(RESAMPLE_MAX_TAPS, np.float32)
        _check(load().sdrg_engine_get_resample(self._h, ctypes.byref(c), h.ctypes.data_as(ctypes.c_void_p),
                                               ctypes.byref(g)), "get_resample")
        return dict(_as_dict(c), taps=h[:c.interp * c.taps_per_phase].copy(), samples_consumed=g.value)

    def resample_reset(self) -> None:
        _check(load().sdrg_engine_resample_reset(self._h), "resample_reset")

    def resample_max_out(self) -> int:
        """ceil(max_in * interp / decim): the row length of a resample call's output."""
        return self._i32_call(load().sdrg_engine_resample_max_out, "resample_max_out")

    def resample_device(self, in_ptr: int, in_stride: int, n: int, out_ptr: int) -> int:
        """Device path: n_streams rows in_stride values apart in (float32, or complex64 at components = 2; the first n
        of every row are the call's), out [n_streams][resample_max_out()] float32, int16 or pairs of them out;
        asynchronous on the main stream.  Returns n_out."""
        return self._i32_call(load().sdrg_engine_resample_device, "resample_device", in_ptr, in_stride, n, out_ptr)

    def _resample_out(self) -> np.ndarray:
        c = self.resample_config()
        shape = (self.n_streams, self.resample_max_out()) + ((2,) if c["components"] == 2 else ())
        return np.empty(shape, RESAMPLE_OUT_DTYPE[c["out_format"]])

    def resample_host(self, rows: np.ndarray) -> np.ndarray:
        """Host path: rows is float32 [n_streams][n], or complex64 [n_streams][n] at components = 2, n <= max_in.
        Returns [n_streams][n_out] float32 or int16, with a last axis of 2 (re, im) at components = 2."""
        comps = self.resample_config()["components"]
        rows = np.ascontiguousarray(rows, np.complex64 if comps == 2 else np.float32)
        if rows.size % self.n_streams:
            raise SdrgError(f"rows has {rows.size} values, no multiple of {self.n_streams} streams")
        n = rows.size // self.n_streams
        if n == 0:  # a call without samples still wants a pointer
            rows = np.zeros((self.n_streams, 1), rows.dtype)
        out = self._resample_out()
        n_out = _I32()
        _check(load().sdrg_engine_resample_host(self._h, _ptr(rows), max(n, 1), n, _ptr(out), ctypes.byref(n_out)),
               "resample_host")
        return out[:, :n_out.value]

    def ddc_demod_resample_host(self, iq: np.ndarray, fmt: int = CS8) -> np.ndarray:
        """Tune and listen at the sound device's rate: iq [n_streams][samplesPerReading * 2] raw samples through the
        DDC, the demodulator (float32 out) and the resampler (components = 1), the channel and the audio left on the
        device; returns the resampled audio, int16 or float32 [n_streams][n_out]."""
        return self._iq_call(load().sdrg_engine_ddc_demod_resample_host, "ddc_demod_resample_host", iq, fmt,
                             self._resample_out)

    # ---- squelch stage ----------------------------------------------------------------------------
    def set_squelch(self, **fields) -> None:
        """sdrg_engine_set_squelch: open_db, close_db, tau_blocks, block, hang_blocks, max_in (fields left out are 0);
        set_squelch(off=True) switches the stage off."""
        self._set_stage(SquelchConfig, "squelch", fields)

    def squelch_config(self) -> dict:
        """The configuration in force, plus its design (open_thr, close_thr, beta as np.float32) and
        samples_consumed."""
        c, o, cl, beta, g = SquelchConfig(), _F(), _F(), _F(), ctypes.c_uint64()
        _check(load().sdrg_engine_get_squelch(self._h, ctypes.byref(c), ctypes.byref(o), ctypes.byref(cl),
                                              ctypes.byref(beta), ctypes.byref(g)), "get_squelch")
        return dict(_as_dict(c), open_thr=np.float32(o.value), close_thr=np.float32(cl.value),
                    beta=np.float32(beta.value), samples_consumed=g.value)

    def squelch_reset(self) -> None:
        _check(load().sdrg_engine_squelch_reset(self._h), "squelch_reset")

    def squelch_device(self, chan_ptr: int, in_stride: int, n: int, out_ptr: int, records_ptr: int | None = None) -> int:
        """Device path: chan [n_streams][in_stride] complex64 in (the first n of every row are the call's), the gated
        rows of the same shape out (out_ptr may be chan_ptr) and, unless records_ptr is None, [n_streams] SquelchRecord;
        asynchronous on the main stream.  Returns n_blocks, the blocks the call completed."""
        return self._i32_call(load().sdrg_engine_squelch_device, "squelch_device", chan_ptr, in_stride, n, out_ptr,
                              records_ptr)

    def _block_host(self, fn, what: str, chan: np.ndarray, record_dtype, want_records: bool):
        """The host call of a block stage (squelch_host, agc_host): (out [n_streams][n], records or None, n_blocks)."""
        chan = np.ascontiguousarray(chan, np.complex64).reshape(self.n_streams, -1)
        n = chan.shape[1]
        rows = chan if n else np.zeros((self.n_streams, 1), np.complex64)  # a call without samples still wants rows
        out = np.empty_like(rows)
        rec = np.empty(self.n_streams, record_dtype) if want_records else None
        n_blocks = self._i32_call(fn, what, _ptr(rows), rows.shape[1], n, _ptr(out), _ptr(rec))
        return out[:, :n], rec, n_blocks

    def squelch_host(self, chan: np.ndarray, want_records: bool = True):
        """Host path: chan is complex64 [n_streams][n], n <= max_in.  Returns (the gated complex64 [n_streams][n], the
        records [n_streams] SquelchRecord or None, n_blocks)."""
        return self._block_host(load().sdrg_engine_squelch_host, "squelch_host", chan, SquelchRecord, want_records)

    def _chain_with_records(self, fn, what: str, iq: np.ndarray, fmt: int, make_out):
        iq, out, rec, n_out = self._iq(iq, fmt), make_out(), np.empty(self.n_streams, SquelchRecord), _I32()
        _check(fn(self._h, _ptr(iq), fmt, _ptr(out), ctypes.byref(n_out), _ptr(rec)), what)
        return out[..., :n_out.value], rec

    def ddc_squelch_demod(self, iq: np.ndarray, fmt: int = CS8):
        """Tune, gate and listen: ddc_demod() with the squelch in place on the channel between the DDC and the
        demodulator; returns (the audio, int16 or float32 [n_streams][n_out], the records [n_streams] SquelchRecord)."""
        return self._chain_with_records(load().sdrg_engine_ddc_squelch_demod_host, "ddc_squelch_demod_host", iq, fmt,
                                        self._demod_out)

    def ddc_squelch_demod_resample_host(self, iq: np.ndarray, fmt: int = CS8):
        """ddc_demod_resample_host() with the squelch between the DDC and the demodulator; returns (the resampled
        audio, the records)."""
        return self._chain_with_records(load().sdrg_engine_ddc_squelch_demod_resample_host,
                                        "ddc_squelch_demod_resample_host", iq, fmt, self._resample_out)

    # ---- IQ correction stage ----------------------------------------------------------------------
    def set_iqcorr(self, **fields) -> None:
        """sdrg_engine_set_iqcorr: dc_tau_blocks, balance_tau_blocks, floor_db, mode, block, max_in (fields left out
        are 0); set_iqcorr(off=True) switches the stage off."""
        self._set_stage(IqcorrConfig, "iqcorr", fields)

    def iqcorr_config(self) -> dict:
        """The configuration in force, plus its design (beta_dc, beta_bal, floor_thr as np.float32) and
        samples_consumed."""
        c, bd, bb, fl, g = IqcorrConfig(), _F(), _F(), _F(), ctypes.c_uint64()
        _check(load().sdrg_engine_get_iqcorr(self._h, ctypes.byref(c), ctypes.byref(bd), ctypes.byref(bb),
                                             ctypes.byref(fl), ctypes.byref(g)), "get_iqcorr")
        return dict(_as_dict(c), beta_dc=np.float32(bd.value), beta_bal=np.float32(bb.value),
                    floor_thr=np.float32(fl.value), samples_consumed=g.value)

    def iqcorr_reset(self) -> None:
        _check(load().sdrg_engine_iqcorr_reset(self._h), "iqcorr_reset")

    def iqcorr_device(self, iq_ptr: int, fmt: int, in_stride: int, n: int, out_ptr: int,
                      records_ptr: int | None = None) -> int:
        """Device path: iq [n_streams][in_stride] raw samples in fmt (the first n of every row are the call's), the
        corrected rows [n_streams][in_stride] complex64 out (out_ptr may be iq_ptr at CF32 only) and, unless
        records_ptr is None, [n_streams] IqcorrRecord; asynchronous on the main stream.  Returns n_blocks."""
        return self._i32_call(load().sdrg_engine_iqcorr_device, "iqcorr_device", iq_ptr, fmt, in_stride, n, out_ptr,
                              records_ptr)

    def iqcorr_host(self, iq: np.ndarray, fmt: int = CS8, want_records: bool = True):
        """Host path: iq is [n_streams][n * 2] raw samples in the type of fmt, n <= max_in.  Returns (the corrected
        complex64 [n_streams][n], the records [n_streams] IqcorrRecord or None, n_blocks)."""
        iq = np.ascontiguousarray(iq, dtype=NUMPY_DTYPE[fmt])
        iq = iq.reshape(self.n_streams, iq.size // self.n_streams)
        n = iq.shape[1] // 2
        rows = iq if n else np.zeros((self.n_streams, 2), iq.dtype)  # a call without samples still wants rows
        out = np.empty((self.n_streams, rows.shape[1] // 2), np.complex64)
        rec = np.empty(self.n_streams, IqcorrRecord) if want_records else None
        n_blocks = self._i32_call(load().sdrg_engine_iqcorr_host, "iqcorr_host", _ptr(rows), fmt, rows.shape[1] // 2, n,
                                  _ptr(out), _ptr(rec))
        return out[:, :n], rec, n_blocks

    def iqcorr_process(self, iq: np.ndarray, fmt: int = CS8, stages: int = STAGE_ALL, now_ms: int = 0):
        """Correct, then look and listen: process() on the frame corrected on the device.  Returns (spectra, records,
        pcm, the correction's records [n_streams] IqcorrRecord)."""
        n = self.cfg.samplesPerReading
        iq = self._iq(iq, fmt)
        plen = self.pcm_len
        spec = np.empty((self.n_streams, n), np.float32) if stages & STAGE_SPECTRUM else None
        recs = np.zeros(self.n_streams, RECORD_DTYPE) if stages & STAGE_STATS else None
        pcm = np.empty((self.n_streams, max(plen, 0)), np.int16) if stages & STAGE_SSB else None
        iq_rec = np.empty(self.n_streams, IqcorrRecord)
        _check(load().sdrg_engine_iqcorr_process_host(self._h, _ptr(iq), fmt, stages, _ptr(spec), _ptr(recs),
                                                      _ptr(pcm) if plen > 0 else None, now_ms, _ptr(iq_rec)),
               "iqcorr_process_host")
        return spec, recs, pcm, iq_rec

    # ---- AFC stage --------------------------------------------------------------------------------
    def set_afc(self, **fields) -> None:
        """sdrg_engine_set_afc: channel_rate, max_offset_hz, tau_blocks, floor_db, lock_threshold, mode, block, max_in
        (fields left out are 0); set_afc(off=True) switches the stage off."""
        self._set_stage(AfcConfig, "afc", fields)

    def afc_config(self) -> dict:
        """The configuration in force, plus its design (afc_design's seven values as np.float32) and
        samples_consumed."""
        c, d, g = AfcConfig(), AfcDesign(), ctypes.c_uint64()
        _check(load().sdrg_engine_get_afc(self._h, ctypes.byref(c), ctypes.byref(d), ctypes.byref(g)), "get_afc")
        return dict(_as_dict(c), **_afc_design_dict(d), samples_consumed=g.value)

    def afc_reset(self) -> None:
        _check(load().sdrg_engine_afc_reset(self._h), "afc_reset")

    def afc_device(self, chan_ptr: int, in_stride: int, n: int, out_ptr: int | None,
                   records_ptr: int | None = None) -> int:
        """Device path: chan [n_streams][in_stride] complex64 in (the first n of every row are the call's), the
        corrected rows of the same shape out (out_ptr may be chan_ptr; None in AFC_MEASURE mode, which writes no rows)
        and, unless records_ptr is None, [n_streams] AfcRecord; asynchronous on the main stream.  Returns n_blocks."""
        return self._i32_call(load().sdrg_engine_afc_device, "afc_device", chan_ptr, in_stride, n, out_ptr, records_ptr)

    def afc_host(self, chan: np.ndarray, want_records: bool = True):
        """Host path: chan is complex64 [n_streams][n], n <= max_in.  Returns (the corrected complex64 [n_streams][n],
        or None in AFC_MEASURE mode; the records [n_streams] AfcRecord or None; n_blocks)."""
        chan = np.ascontiguousarray(chan, np.complex64).reshape(self.n_streams, -1)
        n = chan.shape[1]
        rows = chan if n else np.zeros((self.n_streams, 1), np.complex64)  # a call without samples still wants rows
        out = np.empty_like(rows) if self.afc_config()["mode"] == AFC_TRACK else None
        rec = np.empty(self.n_streams, AfcRecord) if want_records else None
        n_blocks = self._i32_call(load().sdrg_engine_afc_host, "afc_host", _ptr(rows), rows.shape[1], n, _ptr(out),
                                  _ptr(rec))
        return None if out is None else out[:, :n], rec, n_blocks

    def listen_afc(self, iq: np.ndarray, fmt: int = CS8, steps: int = 0):
        """sdrg_engine_listen_afc_host: listen() with the AFC first on the channel, DDC -> AFC -> [squelch] -> [AGC] ->
        demodulator -> [resampler].  Returns (the audio [n_streams][n_out], the squelch's records or None, the AGC's
        records or None, the AFC's records [n_streams] AfcRecord)."""
        iq, n_out = self._iq(iq, fmt), _I32()
        out = self._resample_out() if steps & LISTEN_RESAMPLE else self._demod_out()
        sq_rec = np.empty(self.n_streams, SquelchRecord) if steps & LISTEN_SQUELCH else None
        agc_rec = np.empty(self.n_streams, AGC_RECORD_DTYPE) if steps & LISTEN_AGC else None
        afc_rec = np.empty(self.n_streams, AfcRecord)
        _check(load().sdrg_engine_listen_afc_host(self._h, steps, _ptr(iq), fmt, _ptr(out), ctypes.byref(n_out),
                                                  _ptr(sq_rec), _ptr(agc_rec), _ptr(afc_rec)), "listen_afc_host")
        return out[..., :n_out.value], sq_rec, agc_rec, afc_rec

    # ---- symbol stage -----------------------------------------------------------------------------
    def set_symbols(self, **fields) -> None:
        """sdrg_engine_set_symbols: the fields of sdrg_symbols_config (fields left out are 0); set_symbols(off=True)
        switches the stage off."""
        self._set_stage(SymbolsConfig, "symbols", fields)

    def symbols_config(self) -> dict:
        """The configuration in force, plus its design (symbols_design's values but for the table), cap (the symbols
        per row) and samples_consumed."""
        c, d, g = SymbolsConfig(), SymbolsDesign(), ctypes.c_uint64()
        _check(load().sdrg_engine_get_symbols(self._h, ctypes.byref(c), ctypes.byref(d), ctypes.byref(g)), "get_symbols")
        return dict(_as_dict(c), **_symbols_design_dict(d), cap=self.symbols_max_out(), samples_consumed=g.value)

    def symbols_reset(self) -> None:
        _check(load().sdrg_engine_symbols_reset(self._h), "symbols_reset")

    def symbols_max_out(self) -> int:
        """cap = floor(inc max_in / 2^32) + 1: the symbols per row of `symbols`."""
        return self._i32_call(load().sdrg_engine_symbols_max_out, "symbols_max_out")

    def symbols_device(self, in_ptr: int, in_stride: int, n: int, symbols_ptr: int, records_ptr: int | None = None) -> int:
        """Device path: in [n_streams][in_stride] float32 (the first n of every row are the call's), symbols
        [n_streams][cap] uint8 (SYM_HARD) or float32 (SYM_SOFT) out and, unless records_ptr is None, [n_streams]
        SymbolsRecord; asynchronous on the main stream.  Returns n_sym, the symbols the call wrote per row."""
        return self._i32_call(load().sdrg_engine_symbols_device, "symbols_device", in_ptr, in_stride, n, symbols_ptr,
                              records_ptr)

    def _symbols_out(self) -> np.ndarray:
        c = SymbolsConfig()
        _check(load().sdrg_engine_get_symbols(self._h, ctypes.byref(c), None, None), "get_symbols")
        return np.empty((self.n_streams, self.symbols_max_out()), np.float32 if c.format == SYM_SOFT else np.uint8)

    def symbols_host(self, values: np.ndarray, want_records: bool = True):
        """Host path: values is float32 [n_streams][n], n <= max_in.  Returns (symbols [n_streams][n_sym] uint8 or
        float32, the records [n_streams] SymbolsRecord or None, n_sym)."""
        values = np.ascontiguousarray(values, np.float32).reshape(self.n_streams, -1)
        n = values.shape[1]
        rows = values if n else np.zeros((self.n_streams, 1), np.float32)  # a call without values still wants rows
        sym = self._symbols_out()
        rec = np.empty(self.n_streams, SymbolsRecord) if want_records else None
        n_sym = self._i32_call(load().sdrg_engine_symbols_host, "symbols_host", _ptr(rows), rows.shape[1], n, _ptr(sym),
                               _ptr(rec))
        return sym[:, :n_sym], rec, n_sym

    def listen_symbols(self, iq: np.ndarray, fmt: int = CS8, steps: int = 0, want_audio: bool = True,
                       want_records: bool = True):
        """sdrg_engine_listen_symbols_host: listen() with the symbol stage reading the demodulator's float audio on the
        device, ahead of the resampler.  Returns (the audio [n_streams][n_out], or None with want_audio False: it then
        stays on the device; the squelch's records or None, the AGC's records or None, symbols [n_streams][n_sym], the
        symbol records or None, n_sym)."""
        iq, n_out, n_sym = self._iq(iq, fmt), _I32(), _I32()
        out = None
        if want_audio:
            out = self._resample_out() if steps & LISTEN_RESAMPLE else self._demod_out()
        sq_rec = np.empty(self.n_streams, SquelchRecord) if steps & LISTEN_SQUELCH else None
        agc_rec = np.empty(self.n_streams, AGC_RECORD_DTYPE) if steps & LISTEN_AGC else None
        sym = self._symbols_out()
        rec = np.empty(self.n_streams, SymbolsRecord) if want_records else None
        _check(load().sdrg_engine_listen_symbols_host(self._h, steps, _ptr(iq), fmt, _ptr(out), ctypes.byref(n_out),
                                                      _ptr(sq_rec), _ptr(agc_rec), _ptr(sym), _ptr(rec),
                                                      ctypes.byref(n_sym)), "listen_symbols_host")
        return (None if out is None else out[..., :n_out.value]), sq_rec, agc_rec, sym[:, :n_sym.value], rec, n_sym.value

    # ---- noise blanker stage ----------------------------------------------------------------------
    def set_blanker(self, **fields) -> None:
        """sdrg_engine_set_blanker: tau_blocks, threshold_db, floor_db, block, lead, tail, max_in (fields left out are
        0); set_blanker(off=True) switches the stage off."""
        self._set_stage(BlankerConfig, "blanker", fields)

    def blanker_config(self) -> dict:
        """The configuration in force, plus its design (beta, ratio, floor_thr as np.float32) and samples_consumed."""
        c, beta, ratio, fl, g = BlankerConfig(), _F(), _F(), _F(), ctypes.c_uint64()
        _check(load().sdrg_engine_get_blanker(self._h, ctypes.byref(c), ctypes.byref(beta), ctypes.byref(ratio),
                                              ctypes.byref(fl), ctypes.byref(g)), "get_blanker")
        return dict(_as_dict(c), beta=np.float32(beta.value), ratio=np.float32(ratio.value),
                    floor_thr=np.float32(fl.value), samples_consumed=g.value)

    def blanker_reset(self) -> None:
        _check(load().sdrg_engine_blanker_reset(self._h), "blanker_reset")

    def blanker_device(self, iq_ptr: int, fmt: int, in_stride: int, n: int, out_ptr: int,
                       records_ptr: int | None = None) -> int:
        """Device path: iq [n_streams][in_stride] raw samples in fmt (the first n of every row are the call's), the
        blanked rows [n_streams][in_stride] complex64 out, delayed by lead samples (out must not overlap iq) and,
        unless records_ptr is None, [n_streams] BlankerRecord; asynchronous on the main stream.  Returns n_blocks."""
        return self._i32_call(load().sdrg_engine_blanker_device, "blanker_device", iq_ptr, fmt, in_stride, n, out_ptr,
                              records_ptr)

    def blanker_host(self, iq: np.ndarray, fmt: int = CS8, want_records: bool = True):
        """Host path: iq is [n_streams][n * 2] raw samples in the type of fmt, n <= max_in.  Returns (the blanked
        complex64 [n_streams][n], the records [n_streams] BlankerRecord or None, n_blocks)."""
        iq = np.ascontiguousarray(iq, dtype=NUMPY_DTYPE[fmt])
        iq = iq.reshape(self.n_streams, iq.size // self.n_streams)
        n = iq.shape[1] // 2
        rows = iq if n else np.zeros((self.n_streams, 2), iq.dtype)  # a call without samples still wants rows
        out = np.empty((self.n_streams, rows.shape[1] // 2), np.complex64)
        rec = np.empty(self.n_streams, BlankerRecord) if want_records else None
        n_blocks = self._i32_call(load().sdrg_engine_blanker_host, "blanker_host", _ptr(rows), fmt, rows.shape[1] // 2,
                                  n, _ptr(out), _ptr(rec))
        return out[:, :n], rec, n_blocks

    def clean_process_host(self, iq: np.ndarray, fmt: int = CS8, mask: int = 0, stages: int = STAGE_ALL,
                           now_ms: int = 0):
        """Clean, then look and listen: process() on the frame corrected (with CLEAN_IQCORR in mask) and blanked on the
        device.  Returns (spectra, records, pcm, the correction's records [n_streams] IqcorrRecord or None, the
        blanker's records [n_streams] BlankerRecord)."""
        n = self.cfg.samplesPerReading
        iq = self._iq(iq, fmt)
        plen = self.pcm_len
        spec = np.empty((self.n_streams, n), np.float32) if stages & STAGE_SPECTRUM else None
        recs = np.zeros(self.n_streams, RECORD_DTYPE) if stages & STAGE_STATS else None
        pcm = np.empty((self.n_streams, max(plen, 0)), np.int16) if stages & STAGE_SSB else None
        iq_rec = np.empty(self.n_streams, IqcorrRecord) if mask & CLEAN_IQCORR else None
        blank_rec = np.empty(self.n_streams, BlankerRecord)
        _check(load().sdrg_engine_clean_process_host(self._h, _ptr(iq), fmt, mask, stages, _ptr(spec), _ptr(recs),
                                                     _ptr(pcm) if plen > 0 else None, now_ms, _ptr(iq_rec),
                                                     _ptr(blank_rec)), "clean_process_host")
        return spec, recs, pcm, iq_rec, blank_rec

    # ---- tone detector stage ---------------------------------------------------------------------
    def set_tones(self, **fields) -> None:
        """sdrg_engine_set_tones: the fields of sdrg_tones_config (fields left out are 0; freq_hz a sequence, n_tones
        its length unless given); set_tones(off=True) switches the stage off."""
        fields = dict(fields)
        off = fields.pop("off", False)
        if off and fields:
            raise TypeError("off=True takes no other field")
        c = None if off else ctypes.byref(_tones_filled(fields))
        _check(load().sdrg_engine_set_tones(self._h, c), "set_tones")

    def tones_config(self) -> dict:
        """The configuration in force (freq_hz as a list of n_tones), plus its scalars (np.float32) and
        samples_consumed."""
        c, sc, g = TonesConfig(), TonesScalars(), ctypes.c_uint64()
        _check(load().sdrg_engine_get_tones(self._h, ctypes.byref(c), ctypes.byref(sc), ctypes.byref(g)), "get_tones")
        return dict(_tones_dict(c), **_scalars_dict(sc), samples_consumed=g.value)

    def tones_reset(self) -> None:
        _check(load().sdrg_engine_tones_reset(self._h), "tones_reset")

    def tones_max_blocks(self) -> int:
        """cap_blocks = ceil(max_in / S): the rows of powers per stream."""
        return self._i32_call(load().sdrg_engine_tones_max_blocks, "tones_max_blocks")

    def tones_device(self, in_ptr: int, in_stride: int, n: int, powers_ptr: int, records_ptr: int | None = None) -> int:
        """Device path: in [n_streams][in_stride] values, float32 or complex64 by components (the first n of every row
        are the call's), powers float32 [n_streams][cap_blocks][K] out and, unless records_ptr is None, [n_streams]
        TonesRecord; asynchronous on the main stream.  Returns n_blocks, the blocks the call completed."""
        return self._i32_call(load().sdrg_engine_tones_device, "tones_device", in_ptr, in_stride, n, powers_ptr,
                              records_ptr)

    def tones_host(self, values: np.ndarray, want_records: bool = True):
        """Host path: values is float32 (components 1) or complex64 (components 2) [n_streams][n], n <= max_in.
        Returns (powers float32 [n_streams][n_blocks][K], the records [n_streams] TonesRecord or None, n_blocks)."""
        cfg = self.tones_config()
        dtype = np.float32 if cfg["components"] == 1 else np.complex64
        values = np.ascontiguousarray(values, dtype).reshape(self.n_streams, -1)
        n = values.shape[1]
        rows = values if n else np.zeros((self.n_streams, 1), dtype)  # a call without values still wants rows
        powers = np.empty((self.n_streams, self.tones_max_blocks(), cfg["n_tones"]), np.float32)
        rec = np.empty(self.n_streams, TonesRecord) if want_records else None
        n_blocks = self._i32_call(load().sdrg_engine_tones_host, "tones_host", _ptr(rows), rows.shape[1], n,
                                  _ptr(powers), _ptr(rec))
        return powers[:, :n_blocks], rec, n_blocks

    def listen_tones(self, iq: np.ndarray, fmt: int = CS8, steps: int = 0, want_records: bool = True):
        """sdrg_engine_listen_tones_host: listen() with the tone detector reading the demodulator's float audio on the
        device, ahead of the resampler.  Returns (the audio [n_streams][n_out], the squelch's records or None, the
        AGC's records or None, powers float32 [n_streams][n_blocks][K], the tone records or None, n_blocks)."""
        iq, n_out, n_blocks = self._iq(iq, fmt), _I32(), _I32()
        out = self._resample_out() if steps & LISTEN_RESAMPLE else self._demod_out()
        sq_rec = np.empty(self.n_streams, SquelchRecord) if steps & LISTEN_SQUELCH else None
        agc_rec = np.empty(self.n_streams, AGC_RECORD_DTYPE) if steps & LISTEN_AGC else None
        c = TonesConfig()
        _check(load().sdrg_engine_get_tones(self._h, ctypes.byref(c), None, None), "get_tones")
        powers = np.empty((self.n_streams, self.tones_max_blocks(), c.n_tones), np.float32)
        rec = np.empty(self.n_streams, TonesRecord) if want_records else None
        _check(load().sdrg_engine_listen_tones_host(self._h, steps, _ptr(iq), fmt, _ptr(out), ctypes.byref(n_out),
                                                    _ptr(sq_rec), _ptr(agc_rec), _ptr(powers), _ptr(rec),
                                                    ctypes.byref(n_blocks)), "listen_tones_host")
        return out[..., :n_out.value], sq_rec, agc_rec, powers[:, :n_blocks.value], rec, n_blocks.value

    # ---- AGC stage --------------------------------------------------------------------------------
    def set_agc(self, **fields) -> None:
        """sdrg_engine_set_agc: the fields of sdrg_agc_config (fields left out are 0); set_agc(off=True) switches the
        stage off."""
        self._set_stage(AgcConfig, "agc", fields)

    def agc_config(self) -> dict:
        """The configuration in force, plus its design (max_gain, init_gain, floor_thr, alpha_a, alpha_d as np.float32)
        and samples_consumed."""
        c, g = AgcConfig(), ctypes.c_uint64()
        v = [_F() for _ in AGC_DESIGN_FIELDS]
        _check(load().sdrg_engine_get_agc(self._h, ctypes.byref(c), *[ctypes.byref(x) for x in v], ctypes.byref(g)),
               "get_agc")
        return dict(_as_dict(c), **{k: np.float32(x.value) for k, x in zip(AGC_DESIGN_FIELDS, v)},
                    samples_consumed=g.value)

    def agc_reset(self) -> None:
        _check(load().sdrg_engine_agc_reset(self._h), "agc_reset")

    def agc_device(self, chan_ptr: int, in_stride: int, n: int, out_ptr: int, records_ptr: int | None = None) -> int:
        """Device path: chan [n_streams][in_stride] complex64 in (the first n of every row are the call's), the levelled
        rows of the same shape out (out_ptr may be chan_ptr) and, unless records_ptr is None, [n_streams]
        AGC_RECORD_DTYPE; asynchronous on the main stream.  Returns n_blocks, the blocks the call completed."""
        return self._i32_call(load().sdrg_engine_agc_device, "agc_device", chan_ptr, in_stride, n, out_ptr, records_ptr)

    def agc_host(self, chan: np.ndarray, want_records: bool = True):
        """Host path: chan is complex64 [n_streams][n], n <= max_in.  Returns (the levelled complex64 [n_streams][n],
        the records [n_streams] AGC_RECORD_DTYPE or None, n_blocks)."""
        return self._block_host(load().sdrg_engine_agc_host, "agc_host", chan, AGC_RECORD_DTYPE, want_records)

    def listen(self, iq: np.ndarray, fmt: int = CS8, steps: int = 0):
        """sdrg_engine_listen_host: iq [n_streams][samplesPerReading * 2] raw samples through DDC -> [squelch] -> [AGC]
        -> demodulator -> [resampler], the steps in brackets by the mask (LISTEN_SQUELCH | LISTEN_AGC |
        LISTEN_RESAMPLE).  Returns (the audio [n_streams][n_out], the squelch's records or None, the AGC's records or
        None)."""
        iq, n_out = self._iq(iq, fmt), _I32()
        out = self._resample_out() if steps & LISTEN_RESAMPLE else self._demod_out()
        sq_rec = np.empty(self.n_streams, SquelchRecord) if steps & LISTEN_SQUELCH else None
        agc_rec = np.empty(self.n_streams, AGC_RECORD_DTYPE) if steps & LISTEN_AGC else None
        _check(load().sdrg_engine_listen_host(self._h, steps, _ptr(iq), fmt, _ptr(out), ctypes.byref(n_out),
                                              _ptr(sq_rec), _ptr(agc_rec)), "listen_host")
        return out[..., :n_out.value], sq_rec, agc_rec

    # ---- sideband stage ---------------------------------------------------------------------------
    def set_sideband(self, **fields) -> None:
        """sdrg_engine_set_sideband: the fields of sdrg_sideband_config (fields left out are 0); set_sideband(off=True)
        switches the stage off."""
        self._set_stage(SidebandConfig, "sideband", fields)

    def sideband_config(self) -> dict:
        """The configuration in force, plus its design (cr, ci) and samples_consumed."""
        c, g = SidebandConfig(), ctypes.c_uint64()
        cr, ci = np.zeros(SIDEBAND_MAX_TAPS, np.float32), np.zeros(SIDEBAND_MAX_TAPS, np.float32)
        _check(load().sdrg_engine_get_sideband(self._h, ctypes.byref(c), _ptr(cr), _ptr(ci), ctypes.byref(g)),
               "get_sideband")
        return dict(_as_dict(c), cr=cr[:c.taps].copy(), ci=ci[:c.taps].copy(), samples_consumed=g.value)

    def sideband_reset(self) -> None:
        _check(load().sdrg_engine_sideband_reset(self._h), "sideband_reset")

    def sideband_max_out(self) -> int:
        """ceil(max_in / audio_decimation): the row length of a sideband call's output."""
        return self._i32_call(load().sdrg_engine_sideband_max_out, "sideband_max_out")

    def sideband_device(self, chan_ptr: int, n: int, out_ptr: int) -> int:
        """Device path: chan [n_streams][max_in] complex64 in (the first n of every row are the call's), out
        [n_streams][sideband_max_out()] int16 or float32 out, pairs (upper, lower) of them at SIDEBAND_BOTH;
        asynchronous on the main stream.  Returns n_out."""
        return self._i32_call(load().sdrg_engine_sideband_device, "sideband_device", chan_ptr, n, out_ptr)

    def _sideband_out(self) -> np.ndarray:
        c = self.sideband_config()
        shape = (self.n_streams, self.sideband_max_out()) + ((2,) if c["mode"] == SIDEBAND_BOTH else ())
        return np.empty(shape, SIDEBAND_OUT_DTYPE[c["out_format"]])

    def sideband(self, chan: np.ndarray) -> np.ndarray:
        """Host path: chan is complex64 [n_streams][n], n <= max_in; returns int16 or float32 [n_streams][n_out], with
        a last axis of 2 (upper, lower) at SIDEBAND_BOTH."""
        chan = np.asarray(chan, np.complex64).reshape(self.n_streams, -1)
        n, max_in = chan.shape[1], self.sideband_config()["max_in"]
        if n > max_in:
            raise SdrgError(f"chan has {n} samples per stream, max_in is {max_in}")
        rows = np.zeros((self.n_streams, max_in), np.complex64)
        rows[:, :n] = chan
        out = self._sideband_out()
        return out[:, :self._i32_call(load().sdrg_engine_sideband_host, "sideband_host", _ptr(rows), n, _ptr(out))]

    def listen_sideband(self, iq: np.ndarray, fmt: int = CS8, steps: int = 0):
        """sdrg_engine_listen_sideband_host: listen() with the sideband stage in the demodulator's place, DDC ->
        [squelch] -> [AGC] -> sideband -> [resampler].  Returns (the audio [n_streams][n_out], with a last axis of 2
        at SIDEBAND_BOTH, the squelch's records or None, the AGC's records or None)."""
        iq, n_out = self._iq(iq, fmt), _I32()
        out = self._resample_out() if steps & LISTEN_RESAMPLE else self._sideband_out()
        sq_rec = np.empty(self.n_streams, SquelchRecord) if steps & LISTEN_SQUELCH else None
        agc_rec = np.empty(self.n_streams, AGC_RECORD_DTYPE) if steps & LISTEN_AGC else None
        _check(load().sdrg_engine_listen_sideband_host(self._h, steps, _ptr(iq), fmt, _ptr(out), ctypes.byref(n_out),
                                                       _ptr(sq_rec), _ptr(agc_rec)), "listen_sideband_host")
        return out[:, :n_out.value], sq_rec, agc_rec

    def process_device(self, iq_ptr: int, fmt: int, stages: int, spectra_ptr: int | None, records_ptr: int | None,
                       pcm_ptr: int | None, now_ms: int = 0) -> None:
        """Device path: raw device pointers (e.g. torch tensor .data_ptr()); asynchronous."""
        _check(load().sdrg_engine_process_device(self._h, iq_ptr, fmt, stages, spectra_ptr, records_ptr, pcm_ptr,
                                                 now_ms), "process_device")

    def synchronize(self) -> None:
        _check(load().sdrg_engine_synchronize(self._h), "synchronize")

    def wait_outputs(self, hip_stream: int | None = None) -> None:
        """Enqueue on hip_stream (None: the engine's main stream) a wait for every output of the last call."""
        _check(load().sdrg_engine_wait_outputs(self._h, hip_stream), "wait_outputs")

    def set_pipelining(self, mode) -> None:
        """Overlap each call's SSB stages with the next call's spectrum (see include/sdrg.h): False/PIPELINE_OFF,
        True/PIPELINE_ON, or PIPELINE_INPUTS_READY (iq complete at call time: no wait on the main stream); ON or
        INPUTS_READY | PIPELINE_STATS_ASYNC also runs each call's statistics beside the next call's spectrum."""
        _check(load().sdrg_engine_set_pipelining(self._h, int(mode)), "set_pipelining")

    def set_ssb_variant(self, nco_hz: float = 0.0, fir_taps: int = 0) -> None:
        """BUILD EXTENSION (not a reference interface): NCO mixer at nco_hz before the SSB chain and a
        fir_taps-long decimating FIR (0 = the reference's 255).  (0, 0) is the reference chain."""
        _check(load().sdrg_engine_set_ssb_variant(self._h, float(nco_hz), int(fir_taps)), "set_ssb_variant")

    def ssb_variant(self) -> dict:
        hz, taps, inc, ph = ctypes.c_double(), ctypes.c_int32(), ctypes.c_uint32(), ctypes.c_uint32()
        _check(load().sdrg_engine_get_ssb_variant(self._h, ctypes.byref(hz), ctypes.byref(taps), ctypes.byref(inc),
                                                  ctypes.byref(ph)), "get_ssb_variant")
        return {"nco_hz": hz.value, "fir_taps": taps.value, "nco_increment": inc.value, "nco_phase": ph.value}

    def gather(self, dist: "Dist", root: int = 0, records=None, records_out=None, focus_spectra=None, focus_out=None,
               spectra=None, spectra_out=None, pcm=None, pcm_out=None) -> None:
        """sdrg_engine_gather: gathers of this rank's per-frame outputs (device pointers, ints) to `root`, one RCCL group
        behind the last call's outputs on the engine stream that produced them (device copies on a one-rank
        communicator unless Dist.set_one_rank_rccl(True)); *_out only on the root."""
        b = _GatherBuffers(records, records_out, focus_spectra, focus_out, spectra, spectra_out, pcm, pcm_out)
        _check(load().sdrg_engine_gather(self._h, dist._h, root, ctypes.byref(b)), "sdrg_engine_gather")

    def set_stream(self, hip_stream: int | None) -> None:
        """Enqueue on the caller's HIP stream (e.g. torch.cuda.current_stream().cuda_stream); None = own."""
        _check(load().sdrg_engine_set_stream(self._h, hip_stream), "set_stream")

    def set_profiling(self, on: bool) -> None:
        _check(load().sdrg_engine_set_profiling(self._h, int(on)), "set_profiling")

    def timings(self) -> dict:
        t = _Timings()
        _check(load().sdrg_engine_get_timings(self._h, ctypes.byref(t)), "get_timings")
        return {"spectrum_ms": t.spectrum_ms, "stats_ms": t.stats_ms, "ssb_ms": t.ssb_ms, "total_ms": t.total_ms}

    def timing_stats(self) -> dict:
        t = _Timings()
        c = ctypes.c_int32()
        _check(load().sdrg_engine_get_timing_stats(self._h, ctypes.byref(t), ctypes.byref(c)), "get_timing_stats")
        return {"spectrum_ms": t.spectrum_ms, "stats_ms": t.stats_ms, "ssb_ms": t.ssb_ms, "total_ms": t.total_ms,
                "count": c.value}

    def reset_timing_stats(self) -> None:
        _check(load().sdrg_engine_reset_timing_stats(self._h), "reset_timing_stats")

    def close(self) -> None:
        if getattr(self, "_h", None):
            load().sdrg_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PulseBank:
    """n_streams beacon pulse detectors of one kind (SpectralPulseDetector or AudioPulseDetector) on one GPU."""

    def __init__(self, kind: int, n_streams: int, cfg: PulseConfig | None = None, device: int = 0):
        L = load()
        self.kind = kind
        self.n_streams = n_streams
        c = cfg if cfg is not None else PulseConfig.default(kind)
        h = ctypes.c_void_p()
        _check(L.sdrg_pulse_bank_create(kind, ctypes.byref(c), n_streams, device, ctypes.byref(h)),
               "sdrg_pulse_bank_create")
        self._h = h

    def configure(self, cfg: PulseConfig) -> None:
        _check(load().sdrg_pulse_bank_configure(self._h, ctypes.byref(cfg)), "pulse_bank_configure")

    def config(self) -> PulseConfig:
        c = PulseConfig()
        _check(load().sdrg_pulse_bank_get_config(self._h, ctypes.byref(c)), "pulse_bank_get_config")
        return c

    def reset(self) -> None:
        _check(load().sdrg_pulse_bank_reset(self._h), "pulse_bank_reset")

    def set_stream(self, hip_stream: int | None) -> None:
        _check(load().sdrg_pulse_bank_set_stream(self._h, hip_stream), "pulse_bank_set_stream")

    def process_spectral(self, snr_sigma: np.ndarray, freq_hz: np.ndarray) -> np.ndarray:
        a = np.ascontiguousarray(snr_sigma, np.float32)
        b = np.ascontiguousarray(freq_hz, np.float32)
        if a.size != self.n_streams or b.size != self.n_streams:
            raise SdrgError("one value per stream expected")
        out = np.zeros(self.n_streams, PULSE_OUTPUT_DTYPE)
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        _check(load().sdrg_pulse_bank_process_spectral_host(self._h, p(a), p(b), p(out)), "process_spectral_host")
        return out

    def process_audio(self, block: np.ndarray) -> np.ndarray:
        """block: [n_streams][n] int16 (or float32) samples, one block per stream."""
        a = np.ascontiguousarray(block)
        fmt = 0 if a.dtype == np.int16 else 1
        if fmt:
            a = np.ascontiguousarray(a, np.float32)
        if a.ndim != 2 or a.shape[0] != self.n_streams:
            raise SdrgError("block must be [n_streams][n]")
        out = np.zeros(self.n_streams, PULSE_OUTPUT_DTYPE)
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        _check(load().sdrg_pulse_bank_process_audio_host(self._h, p(a), fmt, a.shape[1], p(out)), "process_audio_host")
        return out

    def process_spectral_device(self, snr_ptr: int, freq_ptr: int, stride_bytes: int, out_ptr: int) -> None:
        _check(load().sdrg_pulse_bank_process_spectral_device(self._h, snr_ptr, freq_ptr, stride_bytes, out_ptr),
               "process_spectral_device")

    def process_audio_device(self, audio_ptr: int, sample_format: int, n: int, stride: int, out_ptr: int) -> None:
        _check(load().sdrg_pulse_bank_process_audio_device(self._h, audio_ptr, sample_format, n, stride, out_ptr),
               "process_audio_device")

    def synchronize(self) -> None:
        _check(load().sdrg_pulse_bank_synchronize(self._h), "pulse_bank_synchronize")

    def close(self) -> None:
        if getattr(self, "_h", None):
            load().sdrg_pulse_bank_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SSBProcessor:
    """SSBProcessor (src/ssb/ssb_processor.h:24-58): a worker thread fed through a queue of at most queue_max
    frames (the reference's 3) that drops the oldest frame when full; each frame runs the SSB chain and the audio
    pulse detector on the GPU, then pcm_cb(pcm int16 array) (only when non-empty) and pulse_cb(strength, live_etat)
    are called on the worker thread."""

    def __init__(self, device: int = 0, queue_max: int = 0):
        h = ctypes.c_void_p()
        _check(load().sdrg_ssb_processor_create(device, queue_max, ctypes.byref(h)), "sdrg_ssb_processor_create")
        self._h = h
        self._cbs = None

    def startProcessing(self, pcm_cb=None, pulse_cb=None) -> None:
        def pcm(_u, p, n):
            if pcm_cb is not None:
                pcm_cb(np.ctypeslib.as_array(p, shape=(n,)).copy())

        def pulse(_u, strength, live):
            if pulse_cb is not None:
                pulse_cb(strength, live)

        self._cbs = _SsbCallbacks(None, CB_SSB_PCM(pcm), CB_SSB_PULSE(pulse))
        _check(load().sdrg_ssb_processor_start(self._h, ctypes.byref(self._cbs)), "startProcessing")

    def stopProcessing(self) -> None:
        _check(load().sdrg_ssb_processor_stop(self._h), "stopProcessing")

    def enqueueData(self, iq: np.ndarray, sample_rate: int, fmt: int = CF32) -> None:
        """iq: one frame of raw samples in `fmt` (CF32: complex64 or interleaved float32)."""
        a = np.ascontiguousarray(iq)
        if fmt == CF32 and np.iscomplexobj(a):
            a = np.ascontiguousarray(a, np.complex64).view(np.float32)
        a = np.ascontiguousarray(a, NUMPY_DTYPE[fmt])
        _check(load().sdrg_ssb_processor_enqueue(self._h, a.ctypes.data_as(ctypes.c_void_p), fmt, a.size // 2,
                                                 sample_rate), "enqueueData")

    def setSoundMode(self, mode: int) -> None:
        _check(load().sdrg_ssb_processor_set_sound_mode(self._h, mode), "setSoundMode")

    def setPulseConfig(self, cfg: PulseConfig) -> None:
        _check(load().sdrg_ssb_processor_set_pulse_config(self._h, ctypes.byref(cfg)), "setPulseConfig")

    def getAmbientEnergy(self) -> float:
        return float(load().sdrg_ssb_processor_get_ambient_energy(self._h))

    def getCurrentRatio(self) -> float:
        return float(load().sdrg_ssb_processor_get_current_ratio(self._h))

    def drain(self) -> None:
        _check(load().sdrg_ssb_processor_drain(self._h), "drain")

    def counters(self) -> dict:
        e, d, p, st = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
        _check(load().sdrg_ssb_processor_counters(self._h, ctypes.byref(e), ctypes.byref(d), ctypes.byref(p),
                                                  ctypes.byref(st)), "counters")
        return {"enqueued": e.value, "dropped": d.value, "processed": p.value, "last_status": st.value}

    def close(self) -> None:
        if getattr(self, "_h", None):
            load().sdrg_ssb_processor_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


IN_BYTES_PER_SAMPLE = {CF32: 8, CS16: 4, CS8: 2, CU8: 2, CS12: 3}


class Ingest:
    """Exact-N re-chunking of raw reads per stream (rx_reading_thread, sdr-bridge-java-soapy.cpp:503-575)."""

    def __init__(self, n_streams: int, samples_per_reading: int, in_format: int = CS8, queue_max: int = 20):
        h = ctypes.c_void_p()
        _check(load().sdrg_ingest_create(n_streams, samples_per_reading, in_format, queue_max, ctypes.byref(h)),
               "sdrg_ingest_create")
        self._h = h
        self.n_streams, self.n, self.in_format = n_streams, samples_per_reading, in_format
        self.out_format = int(load().sdrg_ingest_output_format(h))

    def push(self, stream: int, raw: np.ndarray) -> None:
        """raw: the bytes of whole complex samples in the input format (any numpy dtype)."""
        b = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
        bps = IN_BYTES_PER_SAMPLE[self.in_format]
        if b.size % bps:
            raise SdrgError("partial sample")
        _check(load().sdrg_ingest_push(self._h, stream, b.ctypes.data_as(ctypes.c_void_p), b.size // bps),
               "ingest_push")

    def status(self, stream: int):
        q, p, d = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
        _check(load().sdrg_ingest_status(self._h, stream, ctypes.byref(q), ctypes.byref(p), ctypes.byref(d)),
               "ingest_status")
        return q.value, p.value, d.value

    def _frame_dtype(self):
        return NUMPY_DTYPE[self.out_format]

    def pop_batch(self):
        """[n_streams][N*2] frames in the output format, or None when some stream has no frame yet."""
        out = np.empty((self.n_streams, 2 * self.n), self._frame_dtype())
        got = ctypes.c_int32()
        _check(load().sdrg_ingest_pop_batch(self._h, out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(got)),
               "ingest_pop_batch")
        return out if got.value else None

    def pop(self, stream: int):
        out = np.empty(2 * self.n, self._frame_dtype())
        got = ctypes.c_int32()
        _check(load().sdrg_ingest_pop(self._h, stream, out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(got)),
               "ingest_pop")
        return out if got.value else None

    def set_samples_per_reading(self, n: int) -> None:
        _check(load().sdrg_ingest_set_samples_per_reading(self._h, n), "ingest_set_samples_per_reading")
        self.n = n

    def close(self) -> None:
        if getattr(self, "_h", None):
            load().sdrg_ingest_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
