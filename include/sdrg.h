/*
 * sdrg.h — C ABI of the MI355X (gfx950) IQ-stream DSP engine.
 *
 * This is the drop-in boundary for the reference's per-frame hot path
 * (alexandreGellibert/SDR-for-Android-lib, paths relative to the reference root):
 *
 *   FFTProcessor::configure / process / get*      src/dsp/fft_process.h:29-55, fft_process.cpp:20-379
 *   processSSB_opt(iq, fs, upper, pcm, pulse, mode) src/ssb/ssb_demod_opt.h:64-65, ssb_demod_opt.cpp:221-296
 *   SSBProcessor (queue + worker)                  src/ssb/ssb_processor.h:24-58
 *   JNI applyConfig / read / set*                  src/sdr-bridge-java-soapy.cpp:625-764, 878-1141
 *   SDRConfig fields                               java/fr/intuite/sdr/bridge/SDRBridge.kt:23-37
 *
 * The reference runs one receiver ("stream") per process and processes one frame of
 * samplesPerReading complex samples per call.  The engine generalises that to B independent
 * streams processed one frame each per call ("B streams x 1 frame per launch"): every piece of
 * per-stream state the reference keeps in FFTProcessor members or in processSSB_opt's
 * function statics is kept per stream in HBM, so stream s of a batch behaves exactly like a
 * reference process that was fed stream s's frames in order.
 *
 * Conventions: plain pointers and sizes, no exceptions across the boundary, every entry point
 * returns an sdrg_status (0 = OK).  A handle is not safe for concurrent calls from several
 * threads; configuration changes are applied at the next process call (frame boundary), which
 * replaces the reference's racy configure()-while-process() pattern (sdr-bridge-java-soapy.cpp:878-913).
 */
#ifndef SDRG_H
#define SDRG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDRG_ABI_VERSION 1

/* Status codes.  The reference's JNI layer reports failure as false/nullptr/0 plus a log line
 * (e.g. applyConfig returns false when a device call throws, sdr-bridge-java-soapy.cpp:1115-1118). */
typedef enum sdrg_status {
    SDRG_OK = 0,
    SDRG_E_INVALID = -1,      /* bad argument (null pointer, non-positive size, ...) */
    SDRG_E_UNSUPPORTED = -2,  /* e.g. a frame size outside [1, 2^20] */
    SDRG_E_NOMEM = -3,        /* device allocation failed */
    SDRG_E_HIP = -4,          /* a HIP runtime call failed (message via sdrg_last_error) */
    SDRG_E_NODEVICE = -5      /* no gfx950 device / HIP runtime not usable */
} sdrg_status;

/* Raw IQ sample formats.  The reference stream is always CF32 (sdr-bridge-java-soapy.cpp:263);
 * the device drivers convert their native CU8 / CS8 / CS16 to CF32 before the hot path.  The
 * engine fuses that conversion into its kernels with the convention
 *   CS8: v/128      CU8: (v - 127.4f) * (1/128)  (the in-tree convertIQ, ssb_demod_opt.cpp:33-44)
 *   CS16: v/32768   CF32: as is.  Samples are interleaved I,Q. */
typedef enum sdrg_iq_format {
    SDRG_IQ_CF32 = 0,
    SDRG_IQ_CS8 = 1,
    SDRG_IQ_CU8 = 2,
    SDRG_IQ_CS16 = 3,
    SDRG_IQ_CS12 = 4   /* packed 12-bit (3 bytes per complex sample): sdrg_ingest input only, repacked to CS16 */
} sdrg_iq_format;

/* Which stages a process call runs (bitmask). */
enum {
    SDRG_STAGE_SPECTRUM = 1,  /* FFT -> |X|^2 -> fftshift (fft_process.cpp:42-97) */
    SDRG_STAGE_STATS = 2,     /* evaluateSignalStrength (fft_process.cpp:122-379); needs SPECTRUM */
    SDRG_STAGE_SSB = 4,       /* processSSB_opt (ssb_demod_opt.cpp:221-296) */
    SDRG_STAGE_HOT_PATH = 7,  /* the three above: the accelerated per-frame DSP path */
    SDRG_STAGE_SPECTRAL_PULSE = 8,  /* SpectralPulseDetector::process(best1kHzSnrSigma, best1kHzCenterFreqHz)
                                       (sdr-bridge-java-soapy.cpp:477-488); needs STATS */
    SDRG_STAGE_AUDIO_PULSE = 16,    /* AudioPulseDetector::process(pcm) (ssb_processor.cpp:109-113); needs SSB */
    SDRG_STAGE_ALL = 31             /* everything soapyCallback + the SSB worker do per frame */
};

/* Mirror of Kotlin SDRConfig (SDRBridge.kt:23-37) / the 9 JNI applyConfig arguments
 * (sdr-bridge-java-soapy.cpp:1073-1085).  gain and refresh_* are carried for API parity only:
 * gain is a device setting and the refresh periods are stored but never read by the reference. */
typedef struct sdrg_config {
    int64_t center_frequency;          /* Hz; the reference stores it as uint32 (bridge-config.h:18) */
    int64_t sample_rate;               /* Hz; uint32 in the reference */
    int32_t samples_per_reading;       /* frame size N: any N in [1, 2^20] (fftwf_plan_dft_1d plans any N,
                                          fft_process.cpp:77-79; SDRBridge.kt:25 recommends multiples of 512) */
    int32_t freq_focus_range_khz;      /* focus half-width X in kHz */
    int32_t gain;
    int32_t sound_mode;                /* 0,1,2 (SDRBridge.kt:35-36); other values keep the last mode */
    int64_t refresh_fft_ms;
    int64_t refresh_peak_ms;
    int64_t refresh_signal_strength_ms;
} sdrg_config;

/* Per-frame, per-stream outputs: exactly what soapyCallback reads through the FFTProcessor getters
 * (sdr-bridge-java-soapy.cpp:446-455, fft_process.h:38-55), plus a few diagnostics for parity. */
typedef struct sdrg_frame_record {
    int64_t tracking_frequency;        /* getTrackingFrequency(): lround-ish of the float latch */
    float mean_snr_db;                 /* getMeanSnrDb */
    float mean_snr_sigma;              /* getMeanSnrSigma */
    float peak_above_noise_mean_db;    /* getPeakAboveNoiseMeanDb */
    float max_bin_snr_db;              /* getMaxBinSnrDb */
    float max_bin_snr_sigma;           /* getMaxBinSnrSigma */
    float best1khz_snr_db;             /* getBest1kHzSnrDb */
    float best1khz_snr_sigma;          /* getBest1kHzSnrSigma */
    float best1khz_center_freq_hz;     /* getBest1kHzCenterFreqHz */
    float per_bin_mean;                /* getPerBinMean (noiseLevel callback) */
    int32_t detection_flag;            /* getDetectionFlag: 0 or 3 */
    /* diagnostics (not reference getters) */
    int32_t peak_bin;                  /* focusLo + peakBinInFocus of this frame (-1 if no focus window) */
    float abs_peak_db;                 /* in-focus peak, 10*log10f(P+1e-20) */
    float signal_power_db;             /* focus-window mean power, dB */
    int32_t valid;                     /* nRef >= 2 (fft_process.cpp:218-225) */
    int32_t n_ref_windows;             /* reference windows collected */
} sdrg_frame_record;

/* Callback table mirroring the JNI read() callbacks (SDRBridge.kt:141-154,
 * sdr-bridge-java-soapy.cpp:625-693).  Any entry may be NULL.  `stream` is the stream index in the
 * batch.  The order of invocation per frame is soapyCallback's (sdr-bridge-java-soapy.cpp:458-475):
 * fft, detection_flag, mean_snr, mean_snr_sigma, peak_frequency, peak_above_noise_mean, max_bin,
 * best1khz, noise_level; pcm comes from the SSB worker (ssb_processor.cpp:103-113) and is invoked
 * after them, only when the frame produced samples.  spectral_pulse follows noise_level (:477-488, only
 * with SDRG_STAGE_SPECTRAL_PULSE); audio_pulse follows pcm (ssb_processor.cpp:109-113, every frame, only with
 * SDRG_STAGE_AUDIO_PULSE). */
typedef struct sdrg_callbacks {
    void *user;
    void (*fft)(void *user, int32_t stream, const float *power_shifted, int32_t n);        /* ([F)V  */
    void (*detection_flag)(void *user, int32_t stream, int32_t flag);                     /* (I)V   */
    void (*mean_snr)(void *user, int32_t stream, float mean_snr_db);                      /* (F)V   */
    void (*mean_snr_sigma)(void *user, int32_t stream, float mean_snr_sigma);             /* (F)V   */
    void (*peak_frequency)(void *user, int32_t stream, int64_t hz);                       /* (J)V   */
    void (*pcm)(void *user, int32_t stream, const int16_t *pcm, int32_t n);               /* ([S)V  */
    void (*peak_above_noise_mean)(void *user, int32_t stream, float db);                  /* (F)V   */
    void (*max_bin)(void *user, int32_t stream, float snr_db, float snr_sigma);           /* (FF)V  */
    void (*best1khz)(void *user, int32_t stream, float snr_db, float snr_sigma);          /* (FF)V  */
    void (*noise_level)(void *user, int32_t stream, float per_bin_mean);                  /* (F)V   */
    /* (FIJ)V: this frame's best1kHzSnrSigma, SpectralPulseDetector::liveEtat(), llround(estimatedFreqHz()) */
    void (*spectral_pulse)(void *user, int32_t stream, float snr_sigma, int32_t live_etat, int64_t freq_hz);
    /* (FI)V: AudioPulseDetector::lastPulseStrength(), liveEtat() */
    void (*audio_pulse)(void *user, int32_t stream, float strength, int32_t live_etat);
} sdrg_callbacks;

/* Per-kernel device times of the last process call, from hipEvents recorded on the stream each
 * kernel was launched on (only filled while profiling is enabled).  Pipelined, the SSB chain's start marker
 * would sit on the SSB stream, the step's critical path, so a pipelined call carries one only when the call before
 * it was not a profiled SSB call (the first call after a reset of the timing statistics, after profiling was
 * re-enabled, or after an unprofiled call); every other pipelined call's ssb_ms is the interval from the previous
 * call's SSB end marker to its own.  That interval is the SSB chain's own time (its kernels + the launch gaps
 * between them) in SDRG_PIPELINE_INPUTS_READY mode with the host keeping ahead of the GPU.  In SDRG_PIPELINE_ON
 * mode each call's SSB stream first waits for the call's start marker on the main stream, so the interval also
 * holds that wait (the step period rather than the chain), and in any mode it holds the time the host spends
 * blocked between two calls.  The audio pulse detector runs after the chain on a stream of its own. */
typedef struct sdrg_timings {
    float spectrum_ms;   /* unpack + FFT + |X|^2 + fftshift kernel */
    float stats_ms;      /* end of the spectrum -> end of the signal-strength kernel (+ spectral pulse detector when
                            requested), on the statistics' stream; never includes the SSB stream's work */
    float ssb_ms;        /* whole SSB chain (all its kernels; not the audio pulse detector, which runs on a stream
                            of its own after it); pipelined: the SSB stream's time per call, above */
    float total_ms;      /* call start -> end of the main stream's work; joined calls include the SSB stream */
} sdrg_timings;

/* ------------------------------------------------------------------------------------------------
 * Beacon pulse detectors.  One detector per stream, state in HBM, one wavefront per stream per frame:
 *   SpectralPulseDetector  src/dsp/spectral_pulse_detector.h:19-79, .cpp:1-196   (kind SDRG_PULSE_SPECTRAL)
 *     fed one (snrSigma, freqHz) pair per FFT frame (sdr-bridge-java-soapy.cpp:477-479)
 *   AudioPulseDetector     src/ssb/audio_pulse_detector.h:15-104, .cpp:1-256    (kind SDRG_PULSE_AUDIO)
 *     fed each SSB frame's PCM (ssb_processor.cpp:109)
 * Both run the reference's ROI / phase-lock / live-state logic with the same float (and, for the spectral
 * frequency estimate, double) operation order, so outputs are bit-identical to the reference classes.
 * ---------------------------------------------------------------------------------------------- */
enum { SDRG_PULSE_SPECTRAL = 0, SDRG_PULSE_AUDIO = 1 };

/* Union of SpectralPulseDetector::Config (spectral_pulse_detector.h:23-35) and AudioPulseDetector::Config
 * (audio_pulse_detector.h:19-37); sdrg_pulse_config_default() fills the reference defaults of a kind. */
typedef struct sdrg_pulse_config {
    float fs_energy;        /* energy frame rate, Hz (spectral 20, set to fs/N by applyConfig; audio 100) */
    float z_default_s;      /* local-max half-width while unlocked, s (0.666) */
    float t_target_init;    /* initial period, s (1.75) */
    float dt_tol_s;         /* rhythm / lock tolerance, s (0.150) */
    float snr_min;          /* spectral 1.5, audio 1.0 */
    float snr_rhythm;       /* spectral 2.5, audio 1.1 */
    float snr_strong;       /* spectral 4.0, audio 2.0 */
    float dispersion_max;   /* 1.3 */
    int32_t sum_n_max;      /* 7 */
    float live_window_t;    /* live-state look-back in periods (4.0) */
    float live_divisor;     /* 3.0 */
    /* audio front end only */
    float sample_rate;      /* PCM rate the filters are designed for (48000) */
    float f_min, f_max;     /* band-pass edges, Hz (1500, 4000) */
    float smooth_cutoff;    /* energy low-pass, Hz (5) */
    int32_t noise_ref_far;  /* noise reference [i-far, i-near) in energy frames (80, 40) */
    int32_t noise_ref_near;
} sdrg_pulse_config;

/* What the reference getters return after a frame (spectral_pulse_detector.h:41-48,
 * audio_pulse_detector.h:45-49), plus the callback arguments. */
typedef struct sdrg_pulse_output {
    float strength;            /* lastPulseStrength(): snr of the last admitted ROI */
    int32_t live_etat;         /* liveEtat(), 0..5 */
    int32_t level;             /* pulseDetected(): 0 NONE, 1 LOW, 2 MEDIUM, 3 STRONG */
    int32_t locked;            /* isLocked() */
    float period_s;            /* lockedPeriodS() */
    float est_freq_hz;         /* estimatedFreqHz() (spectral; 0 for audio) */
    int64_t est_freq_hz_rounded;  /* std::llround(estimatedFreqHz()), the spectralPulse callback's J */
    float input;               /* spectral: the snrSigma fed this frame (the callback's F); audio: strength */
    int32_t n_energy;          /* energy frames held (diagnostic) */
    int32_t n_rois;            /* ROIs held (diagnostic) */
    int32_t overflow;          /* ROI ring overflows (always 0 within the documented bound; diagnostic) */
} sdrg_pulse_output;

typedef struct sdrg_pulse_bank sdrg_pulse_bank;

/* Reference defaults of a detector kind. */
int32_t sdrg_pulse_config_default(int32_t kind, sdrg_pulse_config *out);
/* n_streams detectors of one kind on HIP device `device` (the reference constructor per stream). */
int32_t sdrg_pulse_bank_create(int32_t kind, const sdrg_pulse_config *cfg, int32_t n_streams, int32_t device,
                               sdrg_pulse_bank **out);
int32_t sdrg_pulse_bank_destroy(sdrg_pulse_bank *bank);
/* SPECTRAL: SpectralPulseDetector::configure (cfg replaced, detector state kept, :6-8).
 * AUDIO: a fresh AudioPulseDetector(cfg) per stream (what SSBProcessor::setPulseConfig does,
 * ssb_processor.cpp:70-95).  Applied in stream order with the process calls. */
int32_t sdrg_pulse_bank_configure(sdrg_pulse_bank *bank, const sdrg_pulse_config *cfg);
int32_t sdrg_pulse_bank_get_config(const sdrg_pulse_bank *bank, sdrg_pulse_config *out);
/* reset() of every detector (spectral_pulse_detector.cpp:179-196, audio_pulse_detector.cpp:242-256). */
int32_t sdrg_pulse_bank_reset(sdrg_pulse_bank *bank);
/* SPECTRAL, one frame per stream, device pointers: stream s reads *(float*)((char*)snr_sigma + s*stride_bytes)
 * and the same for freq_hz (so an sdrg_frame_record array can be passed directly); out: [n_streams]. */
int32_t sdrg_pulse_bank_process_spectral_device(sdrg_pulse_bank *bank, const float *snr_sigma,
                                                const float *freq_hz, int32_t stride_bytes,
                                                sdrg_pulse_output *out);
/* AUDIO, one PCM block per stream, device pointers: stream s has n samples at audio + s*stride samples;
 * sample_format 0 = int16 (process(vector<int16_t>), scaled by 1/32767), 1 = float (process(vector<float>)). */
int32_t sdrg_pulse_bank_process_audio_device(sdrg_pulse_bank *bank, const void *audio, int32_t sample_format,
                                             int32_t n, int32_t stride, sdrg_pulse_output *out);
/* Host-memory variants: copy in, run, copy out, synchronise. */
int32_t sdrg_pulse_bank_process_spectral_host(sdrg_pulse_bank *bank, const float *snr_sigma, const float *freq_hz,
                                              sdrg_pulse_output *out);
int32_t sdrg_pulse_bank_process_audio_host(sdrg_pulse_bank *bank, const void *audio, int32_t sample_format,
                                           int32_t n, sdrg_pulse_output *out);
int32_t sdrg_pulse_bank_synchronize(sdrg_pulse_bank *bank);
/* Run the device-pointer calls on the caller's HIP stream (a hipStream_t; NULL = the bank's own stream). */
int32_t sdrg_pulse_bank_set_stream(sdrg_pulse_bank *bank, void *hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Ingest: exact-N re-chunking of raw device reads (rx_reading_thread, sdr-bridge-java-soapy.cpp:503-575).
 * Reads of any length are appended per stream (accBuffer); every exact samples_per_reading block becomes a
 * frame in a per-stream queue of at most queue_max frames, the oldest dropped when full (RX_QUEUE_MAX = 20,
 * :121, :556-564).  Frames are popped one per stream into a [n_streams][N] batch in the engine format
 * (sdrg_ingest_output_format: the input format, except CS12 which is repacked to CS16).  Host-only.
 * ---------------------------------------------------------------------------------------------- */
typedef struct sdrg_ingest sdrg_ingest;
int32_t sdrg_ingest_create(int32_t n_streams, int32_t samples_per_reading, int32_t in_format, int32_t queue_max,
                           sdrg_ingest **out);
int32_t sdrg_ingest_destroy(sdrg_ingest *ing);
int32_t sdrg_ingest_output_format(const sdrg_ingest *ing);
/* readStream() returned n_samples complex samples in the input format for `stream` */
int32_t sdrg_ingest_push(sdrg_ingest *ing, int32_t stream, const void *raw, int64_t n_samples);
/* queued frames, samples of the partial frame, frames dropped from a full queue so far */
int32_t sdrg_ingest_status(const sdrg_ingest *ing, int32_t stream, int32_t *queued, int32_t *partial_samples,
                           int64_t *dropped_frames);
/* when every stream has a queued frame: pop one per stream into out [n_streams][N] and set *popped = 1;
 * otherwise *popped = 0 and nothing changes */
int32_t sdrg_ingest_pop_batch(sdrg_ingest *ing, void *out, int32_t *popped);
/* one stream's oldest frame (rx_process_thread's pop, :597-603) */
int32_t sdrg_ingest_pop(sdrg_ingest *ing, int32_t stream, void *out, int32_t *popped);
/* setSamplesPerReading: cut at n from now on (queued frames of the old size are discarded) */
int32_t sdrg_ingest_set_samples_per_reading(sdrg_ingest *ing, int32_t n);

/* ------------------------------------------------------------------------------------------------
 * SSBProcessor (src/ssb/ssb_processor.h:24-58, ssb_processor.cpp:26-115): the reference runs the SSB chain on a
 * worker thread fed by soapyCallback through a queue of at most 3 frames that drops its OLDEST frame when full
 * (:51-64); per popped frame, processSSB_opt with the frame's sample rate and the current sound mode, then the
 * PCM callback (only when the frame produced samples), then the audio pulse detector and its callback (:77-115).
 * This object is that worker over a one-stream engine (SSB + audio-pulse stages), so a consumer that falls behind
 * drops the same frames as the reference and the filter state continues over the frames that were processed.
 * Callbacks run on the worker thread.
 * ---------------------------------------------------------------------------------------------- */
typedef struct sdrg_ssb_processor sdrg_ssb_processor;
typedef struct sdrg_ssb_callbacks {
    void *user;
    void (*pcm)(void *user, const int16_t *pcm, int32_t n);                     /* pcmCallback, ([S)V */
    void (*pulse)(void *user, float strength, int32_t live_etat);               /* pulseCallback_, (FI)V */
} sdrg_ssb_callbacks;
/* queue_max: frames held before the oldest is dropped (0 = the reference's 3). */
int32_t sdrg_ssb_processor_create(int32_t device, int32_t queue_max, sdrg_ssb_processor **out);
int32_t sdrg_ssb_processor_destroy(sdrg_ssb_processor *p);   /* stopProcessing + release */
int32_t sdrg_ssb_processor_start(sdrg_ssb_processor *p, const sdrg_ssb_callbacks *cbs);  /* startProcessing */
int32_t sdrg_ssb_processor_stop(sdrg_ssb_processor *p);      /* stopProcessing: the worker finishes its frame */
/* enqueueData: copies the frame (n samples in `format`) with the rate it was read at; ignored when not started. */
int32_t sdrg_ssb_processor_enqueue(sdrg_ssb_processor *p, const void *iq, int32_t format, int32_t n,
                                   int64_t sample_rate);
/* BridgeConfig::getSoundMode() as the worker reads it per frame (:102); default 1. */
int32_t sdrg_ssb_processor_set_sound_mode(sdrg_ssb_processor *p, int32_t mode);
/* setPulseConfig (:70-75): a fresh AudioPulseDetector with cfg before the next frame. */
int32_t sdrg_ssb_processor_set_pulse_config(sdrg_ssb_processor *p, const sdrg_pulse_config *cfg);
float sdrg_ssb_processor_get_ambient_energy(const sdrg_ssb_processor *p);  /* getAmbientEnergy (ssb_processor.h:34) */
float sdrg_ssb_processor_get_current_ratio(const sdrg_ssb_processor *p);   /* getCurrentRatio (:35): always 0 */
/* Wait until the queue is empty and the worker idle (or stopped). */
int32_t sdrg_ssb_processor_drain(sdrg_ssb_processor *p);
/* Frames enqueued, dropped from a full queue, processed; status of the last failed frame (0 if none). */
int32_t sdrg_ssb_processor_counters(const sdrg_ssb_processor *p, int64_t *enqueued, int64_t *dropped,
                                    int64_t *processed, int32_t *last_status);

typedef struct sdrg_engine sdrg_engine;

/* Library identity. */
int32_t sdrg_abi_version(void);
const char *sdrg_last_error(void);      /* thread-local message for the last failing call */

/* Geometry helpers (host-only, no device needed). */
/* Frame size the SSB chain emits for a frame of n samples at sample_rate (0 if none):
 * (n - taps)/decim + 1 with taps = 255 (or n|1 when n < 255), decim = max(1, int(fs/48000.0f))
 * (ssb_demod_opt.cpp:121-143, :273). */
int32_t sdrg_ssb_pcm_len(int32_t n, int64_t sample_rate);

/* How the SSB launcher lays out a frame of n samples at sample_rate with fir_taps (0 = the reference's 255, else odd
 * in [3, 255], as sdrg_engine_set_ssb_variant takes it); answered by the launcher's own predicate, so tests that want
 * every layout cannot drift from it.  Host-only, launches nothing.
 *   decimation         max(1, int(fs / 48000.0f))
 *   taps               the FIR length actually used (fir_taps or 255, or n|1 when the frame is shorter)
 *   pcm_len            PCM samples per call, as sdrg_engine_pcm_len reports under that variant
 *   pipeline           1: the pipeline kernel; 0: the lane-per-stream kernels (the pipeline does not hold the shape)
 *   slots              FIR accumulators per stream in the pipeline kernel: (chunk + taps - 2) / decimation + 1 rounded
 *                      up to 4, 8, 16 or 32 (4 when pcm_len is 0); 0 when pipeline is 0
 *   chunk              samples per pipeline chunk
 *   chunk_outputs      FIR outputs one chunk can complete, ceil(chunk / decimation)
 *   max_chunk_outputs  the most the pipeline kernel holds; a larger chunk_outputs selects the lane-per-stream kernels */
typedef struct sdrg_ssb_layout_info {
    int32_t decimation, taps, pcm_len, pipeline, slots, chunk, chunk_outputs, max_chunk_outputs;
} sdrg_ssb_layout_info;
int32_t sdrg_ssb_layout(int64_t sample_rate, int32_t n, int32_t fir_taps, sdrg_ssb_layout_info *out);

/* The focus window of evaluateSignalStrength (fft_process.cpp:124-140) in the fftshifted spectrum the engine
 * writes: bins [*first_bin, *first_bin + *n_bins) hold offsets -focus_khz .. +focus_khz kHz around the
 * centre.  *n_bins = 0 when the window is empty (focus wider than the band, :218-247).  Host-only; used to
 * gather only the spectrum slice a consumer looks at (sdrg/shard.py gather_focus). */
int32_t sdrg_focus_window(int64_t sample_rate, int32_t n, int32_t focus_khz, int32_t *first_bin, int32_t *n_bins);

/* The SSB filter design the engine uses for a configuration, from the reference's own expressions:
 * rfFilter low-pass (iir2InitLowpass at (float)fs with the sound mode's fc/Q, ssb_demod_opt.cpp:60-73, :262),
 * HP/BP biquads (:148-175, :278-279) and the FIR taps (:121-134).  lpf/hp/bp: {a0, a1, a2, b1, b2};
 * taps must hold 255 floats; *n_taps receives the tap count.  Host-only. */
int32_t sdrg_ssb_design(int32_t samp_count, int64_t sample_rate, int32_t sound_mode, float *lpf, float *hp,
                        float *bp, float *taps, int32_t *n_taps);

/* Page-locked host memory (hipHostMalloc) for sdrg_engine_process_host's buffers: copies to and from it run at
 * the PCIe rate, while pageable buffers go through the runtime's staging.  The memory
 * stays valid until sdrg_host_free; any engine may use it. */
int32_t sdrg_host_alloc(size_t bytes, void **out);
int32_t sdrg_host_free(void *p);

/* Create an engine for n_streams independent receivers on HIP device `device`.
 * Replaces FFTProcessor() + configure() (fft_process.cpp:8-39) and BridgeConfig::initialize
 * (bridge-config.h:17-38) for each stream. */
int32_t sdrg_engine_create(const sdrg_config *cfg, int32_t n_streams, int32_t device, sdrg_engine **out);
int32_t sdrg_engine_destroy(sdrg_engine *eng);

/* JNI applyConfig (sdr-bridge-java-soapy.cpp:1073-1141): BridgeConfig::initialize + FFTProcessor::configure.
 * Per-stream tracking/detection/SSB state is kept, exactly as the reference keeps its members and
 * statics across applyConfig. */
int32_t sdrg_engine_apply_config(sdrg_engine *eng, const sdrg_config *cfg);
/* JNI setFrequency (:878-913): reconfigure + raise isCenterFrequencyChanged for every stream. */
int32_t sdrg_engine_set_frequency(sdrg_engine *eng, int64_t center_frequency);
/* JNI setFrequencyFocusRange (:1025-1040). */
int32_t sdrg_engine_set_frequency_focus_range(sdrg_engine *eng, int32_t khz);
/* JNI setSampleRate (:931-953): BridgeConfig only.  The SSB chain uses the new rate from the next frame (it is
 * handed BridgeConfig's rate per frame, :441-442); the statistics keep the rate of the last configure() point
 * (create / applyConfig / setFrequency / setFrequencyFocusRange), as FFTProcessor::config_ does.  The spectral
 * pulse detector is not reconfigured (only applyConfig does that, :1130-1138). */
int32_t sdrg_engine_set_sample_rate(sdrg_engine *eng, int64_t sample_rate);
/* JNI setSamplesPerReading (:1015-1021): BridgeConfig only; the frame size of the following calls (the reader cuts
 * frames at it, :541-573, and FFTProcessor::process plans whatever length it is handed, fft_process.cpp:42-79). */
int32_t sdrg_engine_set_samples_per_reading(sdrg_engine *eng, int32_t n);
/* JNI setSoundMode (:1066-1071). */
int32_t sdrg_engine_set_sound_mode(sdrg_engine *eng, int32_t mode);
/* processSSB_opt's upperSideband argument (default 1, which is what SSBProcessor always passes,
 * ssb_processor.cpp:103; 0 gives the reference's lower-sideband result, Re - Im of {y, y} = 0). */
int32_t sdrg_engine_set_upper_sideband(sdrg_engine *eng, int32_t upper);
/* BUILD EXTENSION, not a reference interface (BASELINE.json configs[2], "SSB (USB) NCO + FIR-decimate, 127-tap
 * FIR"; the reference chain has neither, ssb_demod_opt.cpp:122).  Off by default, and
 * every reference-parity result above assumes it off.
 *   nco_hz   : != 0 mixes each stream's IQ with a phase-continuous NCO before the chain: sample t of a call
 *              becomes Re((I + jQ) e^{-j 2 pi ph / 2^32}), ph = phase + inc t (mod 2^32), inc =
 *              round(nco_hz / sample_rate * 2^32) mod 2^32; the phasor is hi[ph >> 22] * lo[(ph >> 12) & 1023]
 *              from two 1024-entry tables of e^{-j 2 pi k / 2^10} and e^{-j 2 pi k / 2^20} rounded to float.
 *              The signal at +nco_hz lands at 0 Hz, where removeDC, the low-pass, AGC, FIR and EQ then run
 *              unchanged.  phase starts at 0 and advances by inc * samp_count per call (every stream of the
 *              engine sees the same calls).  0 = no mixer (the reference chain).
 *   fir_taps : decimating FIR length, odd in [3, 255] (Hann-sinc of :121-134 at that length); 0 = 255.
 *              The PCM frame length follows (sdrg_engine_pcm_len).
 * Takes effect at the next call; restarts the NCO phase; filter state is kept. */
int32_t sdrg_engine_set_ssb_variant(sdrg_engine *eng, double nco_hz, int32_t fir_taps);
/* The variant in force: nco_hz, the FIR length the next call uses, the NCO increment and the next call's
 * starting phase (any pointer may be NULL). */
int32_t sdrg_engine_get_ssb_variant(const sdrg_engine *eng, double *nco_hz, int32_t *fir_taps,
                                    uint32_t *nco_increment, uint32_t *nco_phase);
/* Current configuration (BridgeConfig getters, bridge-config.h:41-51). */
int32_t sdrg_engine_get_config(const sdrg_engine *eng, sdrg_config *out);
int32_t sdrg_engine_n_streams(const sdrg_engine *eng);
/* Samples per frame the SSB chain of every stream emits (constant for a configuration). */
int32_t sdrg_engine_pcm_len(const sdrg_engine *eng);

/* The engine's pulse detectors (one SPECTRAL and one AUDIO detector per stream, run by the
 * SDRG_STAGE_SPECTRAL_PULSE / SDRG_STAGE_AUDIO_PULSE stages).  applyConfig sets the spectral detector to
 * the default config with fs_energy = (float)sample_rate / (float)samples_per_reading
 * (sdr-bridge-java-soapy.cpp:1130-1138); create does the same.  set_spectral_pulse_config = configure();
 * set_audio_pulse_config = SSBProcessor::setPulseConfig (fresh detectors at the next frame). */
int32_t sdrg_engine_set_spectral_pulse_config(sdrg_engine *eng, const sdrg_pulse_config *cfg);
int32_t sdrg_engine_set_audio_pulse_config(sdrg_engine *eng, const sdrg_pulse_config *cfg);
/* Device arrays [n_streams] the last process call wrote (valid until the next call; either may be NULL). */
int32_t sdrg_engine_pulse_outputs(const sdrg_engine *eng, const sdrg_pulse_output **spectral,
                                  const sdrg_pulse_output **audio);

/* Reset every stream's cross-frame state (tracking latch, detection ring, SSB filter state, pulse
 * detectors) to the state of a freshly constructed reference process. */
int32_t sdrg_engine_reset_state(sdrg_engine *eng);

/* Process one frame of every stream, all buffers in device memory (HBM).
 *   iq       : [n_streams][samples_per_reading] samples in `format`
 *   spectra  : [n_streams][samples_per_reading] float, fftshifted linear power (fftCallback payload);
 *              may be NULL when STATS is not requested (then an internal buffer is used).  Odd N: element
 *              N-1 of each row is never written, as in the reference's fftshift loop (fft_process.cpp:92-97),
 *              whose member vector keeps its old value there (0 when fresh); a caller buffer should be zeroed
 *              once before its first use, since the statistics may read that bin
 *   records  : [n_streams] sdrg_frame_record (may be NULL if STATS not requested)
 *   pcm      : [n_streams][pcm_len] int16 (may be NULL if SSB not requested)
 *   now_ms   : monotonic clock in ms for the 300 ms frequency-tracking latch
 *              (fft_process.cpp:333-361 uses steady_clock; injected here so results are reproducible)
 * Work is enqueued on the engine's HIP streams and is complete when sdrg_engine_synchronize returns. */
int32_t sdrg_engine_process_device(sdrg_engine *eng, const void *iq, int32_t format, int32_t stages,
                                   float *spectra, sdrg_frame_record *records, int16_t *pcm,
                                   int64_t now_ms);
int32_t sdrg_engine_synchronize(sdrg_engine *eng);
/* evaluateSignalStrength alone (fft_process.cpp:122-379) on caller spectra: [n_streams][samples_per_reading]
 * fftshifted linear power (the FFTProcessor's power_shifted member after process()), records out, each stream's
 * statistics state (tracking latch, detection ring, stale outputs) advanced exactly as by a process() call with
 * STATS.  _device: both buffers in device memory, ordered on the main stream (complete after
 * sdrg_engine_synchronize).  _host: host buffers, synchronous. */
int32_t sdrg_engine_signal_strength_device(sdrg_engine *eng, const float *spectra, sdrg_frame_record *records,
                                           int64_t now_ms);
int32_t sdrg_engine_signal_strength_host(sdrg_engine *eng, const float *spectra, sdrg_frame_record *records,
                                         int64_t now_ms);
/* Enqueue the engine's work on the caller's HIP stream (a hipStream_t; NULL = the engine's own stream): the
 * SSB fork/join happens relative to it, so consumers on that stream (e.g. an RCCL gather of the records)
 * are ordered after each call without a host synchronisation.  Synchronises the previous stream first.
 * The stream must outlive the engine (or be unset with NULL before it is destroyed). */
int32_t sdrg_engine_set_stream(sdrg_engine *eng, void *hip_stream);
/* Pipelining across calls (default SDRG_PIPELINE_OFF).  Pipelined, sdrg_engine_process_device forks the SSB
 * stages at the start of each call and does not join them into the main stream at its end, so a call's SSB
 * pipeline runs beside the next call's spectrum.  The spectrum / statistics / spectral-pulse outputs are
 * ordered on the main stream as usual; the PCM and audio-pulse outputs are complete after
 * sdrg_engine_synchronize (or after the next call's SSB stage starts, which follows them on the SSB stream).
 * process_host always joins.  The input buffer stays in use until the SSB stage has read it: see
 * sdrg_engine_input_released below.
 *   SDRG_PIPELINE_ON: the SSB stage of a call starts after the work enqueued on the main stream before the
 *     call (the caller's producer work on iq), as the spectrum does.
 *   SDRG_PIPELINE_INPUTS_READY: the caller guarantees that iq is complete when the call is made (written by
 *     host-synchronised copies or earlier, already-finished work, e.g. a resident ring of input frames); the
 *     SSB stage then does not wait for the main stream at all, which saves its stream one cross-stream wait
 *     per call.  Work the caller enqueues on the main stream that writes iq is NOT waited for in this mode.
 * SDRG_PIPELINE_STATS_ASYNC may be added (OR) to ON or INPUTS_READY: a call's statistics and spectral pulse detector
 *   run on a stream of their own after the call's spectrum, beside the next call's spectrum, instead of after it
 *   on the main stream.  Every stage of every call still runs, in order per stream; the records and spectral-pulse
 *   outputs are complete after sdrg_engine_synchronize, or on a stream after sdrg_engine_wait_outputs.  The engine
 *   keeps the spectra a call's statistics read intact (a call writing the previous call's spectra buffer waits for
 *   those statistics on the GPU; the host waits for the statistics of the call two before), so a caller rotating
 *   two or more spectra buffers (and records buffers it reads back) overlaps the statistics fully.
 * Any other value returns SDRG_E_INVALID. */
enum { SDRG_PIPELINE_OFF = 0, SDRG_PIPELINE_ON = 1, SDRG_PIPELINE_INPUTS_READY = 2, SDRG_PIPELINE_STATS_ASYNC = 4 };
int32_t sdrg_engine_set_pipelining(sdrg_engine *eng, int32_t mode);
/* Enqueue on `hip_stream` (NULL = the engine's main stream) a wait for every output of the last call: spectra,
 * records and spectral-pulse outputs, PCM and audio-pulse outputs, whichever streams produce them (a consumer of a
 * pipelined call's outputs, e.g. an RCCL gather of the records, then follows them without a host synchronisation). */
int32_t sdrg_engine_wait_outputs(sdrg_engine *eng, void *hip_stream);
/* The INPUT of a call: the kernels read `iq` asynchronously after sdrg_engine_process_device returns -- the
 * spectrum on the main stream and the SSB pipeline on its own stream, which in pipelined mode runs on past the
 * call, beside the next call's spectrum.  The caller must not overwrite or free `iq` until the call has released
 * it.  input_released: *released = 1 once every kernel of the last call that reads its iq has finished (a
 * non-blocking query).  wait_input_released: enqueue on `hip_stream` (NULL = the engine's main stream) a wait for
 * that release, so a refill of the same buffer enqueued there afterwards (e.g. the next frame's host-to-device
 * copy) cannot overtake the readers -- without a host synchronisation and without joining the SSB stream into the
 * next call's spectrum (neither call is needed with a fresh buffer per call). */
int32_t sdrg_engine_input_released(const sdrg_engine *eng, int32_t *released);
int32_t sdrg_engine_wait_input_released(sdrg_engine *eng, void *hip_stream);

/* Same from host memory (PCIe-inclusive): copies iq in, runs, copies outputs back, synchronises,
 * then invokes the registered callbacks per stream in soapyCallback order.  Any output may be NULL. */
int32_t sdrg_engine_process_host(sdrg_engine *eng, const void *iq, int32_t format, int32_t stages,
                                 float *spectra, sdrg_frame_record *records, int16_t *pcm,
                                 int64_t now_ms);
/* Host copies of the last call's pulse outputs ([n_streams] each; either may be NULL); synchronises. */
int32_t sdrg_engine_get_pulse_outputs(sdrg_engine *eng, sdrg_pulse_output *spectral, sdrg_pulse_output *audio);

/* ------------------------------------------------------------------------------------------------
 * BUILD EXTENSION, not a reference interface: the display stage.  Per stream and frame, a span [lo, lo + nb) of the
 * fftshifted power spectrum (one row of N floats per stream, as sdrg_engine_process_device writes it) is reduced
 * to `width` columns, converted to dB and written as float dB or as 8-bit codes: the spectrum or waterfall row a
 * screen shows (16384 bins -> 1024 U8 columns: 1 KiB per frame instead of 64 KiB).
 *   span     FULL: lo = 0, nb = N.  FOCUS: sdrg_focus_window of the statistics' configuration in force (what
 *            sdrg_engine_gather_focus packs; clamped to the band when the focus is wider than it).  BINS: first_bin,
 *            n_bins.  Resolved at each display call (N and the focus may change between calls): an empty focus
 *            window (a 0 kHz focus), or lo + nb > N, fails that call with SDRG_E_INVALID and enqueues nothing.
 *   columns  column c of [0, width) covers the bins lo + j0 .. lo + j1 - 1, j0 = floor(c nb / width),
 *            j1 = floor((c + 1) nb / width) in 64-bit integers, and the one bin lo + j0 when that range is empty
 *            (width > nb: nearest-bin repetition).  width in [1, 2^20]; width = nb is the whole log-magnitude spectrum.
 *   value    MAX: the largest power of the column.  MEAN: (float)(S / (double)count), S the column's powers summed
 *            in double (in any order).  Defined for finite powers >= 0 and +inf.
 *   dB       d = 10.0f * log10f(v + 1e-20f) (fft_process.h:74-75 with refPower 1; glibc's log10f bit for bit).
 *   format   DB_F32: d, [n_streams][width] float.  U8: [n_streams][width] bytes, rows dense (stride width bytes):
 *            scale = 255.0f / (db_max - db_min); t = (d - db_min) * scale (two float operations); 255 if t >= 255,
 *            0 if t <= 0 or NaN, else (int)(t + 0.5f).
 * ---------------------------------------------------------------------------------------------- */
enum { SDRG_DISPLAY_SPAN_FULL = 0, SDRG_DISPLAY_SPAN_FOCUS = 1, SDRG_DISPLAY_SPAN_BINS = 2 };
enum { SDRG_DISPLAY_MAX = 0, SDRG_DISPLAY_MEAN = 1 };
enum { SDRG_DISPLAY_DB_F32 = 0, SDRG_DISPLAY_U8 = 1 };
typedef struct sdrg_display_config {
    int32_t span, first_bin, n_bins;   /* first_bin / n_bins: SPAN_BINS only */
    int32_t width, reduce, format;
    float db_min, db_max;              /* U8 only: finite, db_max > db_min */
} sdrg_display_config;

/* Host-only, no device: the bins [*first, *first + *count) of the span (span-relative) that column `column` of
 * `width` covers for a span of n_bins bins (n_bins and width in [1, 2^20], column in [0, width)). */
int32_t sdrg_display_column_range(int32_t n_bins, int32_t width, int32_t column, int32_t *first, int32_t *count);
/* Host-only: the U8 code of a dB value (db_min, db_max finite, db_max > db_min). */
int32_t sdrg_display_code(float db, float db_min, float db_max, uint8_t *code);

/* Set the configuration every later display call uses.  Checks what does not depend on N (known enum values, width
 * in [1, 2^20], BINS: first_bin >= 0 and n_bins >= 1, U8: the dB range); a rejected call leaves the previous
 * configuration in force.  A display call before any set_display returns SDRG_E_INVALID. */
int32_t sdrg_engine_set_display(sdrg_engine *eng, const sdrg_display_config *cfg);
int32_t sdrg_engine_get_display(const sdrg_engine *eng, sdrg_display_config *out);
/* The span and the bytes per output row the next display call would use (host-only; any pointer may be NULL). */
int32_t sdrg_engine_display_geometry(const sdrg_engine *eng, int32_t *first_bin, int32_t *n_bins, int32_t *row_bytes);
/* spectra [n_streams][samples_per_reading] float and out [n_streams][row_bytes] in device memory.  Runs on the main
 * stream (the caller's after sdrg_engine_set_stream): issued right after sdrg_engine_process_device it reads that
 * call's spectra without a host synchronisation, in every pipelining mode.  Complete after sdrg_engine_synchronize,
 * or on a stream after sdrg_engine_wait_outputs. */
int32_t sdrg_engine_display_device(sdrg_engine *eng, const float *spectra, void *out);
/* Host buffers, synchronous.  spectra == NULL: the spectra the last sdrg_engine_process_host call with
 * SDRG_STAGE_SPECTRUM left on the device (SDRG_E_INVALID without such a call, or when samples_per_reading has changed
 * since), so process_host(spectra = NULL, ...) + display_host(NULL, rows) copies back only the display rows. */
int32_t sdrg_engine_display_host(sdrg_engine *eng, const float *spectra, void *out);

/* ------------------------------------------------------------------------------------------------
 * BUILD EXTENSION, not a reference interface: the integration stage.  Per stream and bin, the mean or the largest of
 * the last `period` power spectra, or an exponential moving average: the non-coherent integration that the
 * reference's FFTProcessor prepares (integrationPeriod = 10 and a ring it fills and never reads) and does not do.
 * The engine keeps the history in device memory: one configuration and one history per engine, every call feeds one
 * frame per stream, so all streams advance together.
 *   in / out  spectra and out are [n_streams][N] float, N the samples_per_reading in force; all N elements of a row
 *             are plain data (also the element N - 1 the spectrum of an odd N never writes).  out == spectra is
 *             allowed (in place); any other overlap is undefined.
 *   t, c      t = 0, 1, ... counts the integrate calls since the last reset, x_t is this call's value of a bin and
 *             c = min(t + 1, period).
 *   MEAN      S, a double, is (double)x_i summed for i = t - c + 1 .. t in that order (oldest first), starting from
 *             the oldest value; out = (float)(S / (double)c).  Recomputed from the history at every call (a running
 *             sum would keep a residue of every strong frame that ever passed).  period = 1 returns the input's bits.
 *   MAX       the largest of those c values.
 *   EMA       t = 0: y = x.  Otherwise d = x - y; y = y + alpha * d (three float operations, no contraction).
 *             out = y; the engine keeps y.
 *   domain    MEAN and MAX: finite powers >= +0 and +inf.  EMA: finite powers >= +0.
 *   period    in [1, 64]; MEAN and MAX only (EMA neither reads nor checks it).
 *   alpha     finite, in (0, 1]; EMA only (MEAN and MAX neither read nor check it).
 *   reset     the next call is t = 0 after: every successful sdrg_engine_set_integration, sdrg_engine_integrate_reset,
 *             sdrg_engine_reset_state, and at an integrate call at which samples_per_reading, sample_rate or
 *             center_frequency of the configuration in force differ from those at the previous integrate call (the
 *             bins mean other frequencies; compared on the host, at the call).
 *   depth     the number of frames the last output integrates: c for MEAN and MAX, t + 1 for EMA, 0 after a reset.
 * A call that fails (a null pointer, no configuration set, SDRG_E_NOMEM) changes nothing and advances nothing.
 * ---------------------------------------------------------------------------------------------- */
enum { SDRG_INTEGRATE_MEAN = 0, SDRG_INTEGRATE_MAX = 1, SDRG_INTEGRATE_EMA = 2 };
enum { SDRG_INTEGRATE_MAX_PERIOD = 64 };
typedef struct sdrg_integrate_config {
    int32_t mode;
    int32_t period;   /* MEAN, MAX */
    float alpha;      /* EMA */
} sdrg_integrate_config;

/* Checks the mode and the field it uses; a rejected call leaves the previous configuration and history in force, an
 * accepted one resets the history.  An integrate call before any set_integration returns SDRG_E_INVALID. */
int32_t sdrg_engine_set_integration(sdrg_engine *eng, const sdrg_integrate_config *cfg);
/* The configuration in force and the depth of the last output; either pointer may be NULL.  SDRG_E_INVALID when
 * cfg_out is given and no configuration has been set. */
int32_t sdrg_engine_get_integration(const sdrg_engine *eng, sdrg_integrate_config *cfg_out, int32_t *depth_out);
int32_t sdrg_engine_integrate_reset(sdrg_engine *eng);
/* Device buffers.  Runs on the main stream (the caller's after sdrg_engine_set_stream): issued right after
 * sdrg_engine_process_device it follows that call's spectrum in every pipelining mode, and a following
 * sdrg_engine_signal_strength_device(out, ...) or sdrg_engine_display_device(out, ...) follows it.  Under
 * SDRG_PIPELINE_STATS_ASYNC, when out overlaps a spectra buffer whose statistics are still in flight, the kernel
 * waits (on the GPU) for them: integrating a call's spectra in place never changes what its statistics see.
 * Complete after sdrg_engine_synchronize, or on a stream after sdrg_engine_wait_outputs.  The ring (period x
 * n_streams x N floats) or the EMA state (n_streams x N floats) is allocated at the first call that needs it. */
int32_t sdrg_engine_integrate_device(sdrg_engine *eng, const float *spectra, float *out);
/* Host buffers, synchronous.  spectra == NULL: the spectra the last sdrg_engine_process_host call with
 * SDRG_STAGE_SPECTRUM left on the device (the rule and the refusals of sdrg_engine_display_host(NULL)).
 * out == NULL: the history advances and the integrated rows stay on the device only. */
int32_t sdrg_engine_integrate_host(sdrg_engine *eng, const float *spectra, float *out);
/* The display rows (current display configuration, [n_streams][row_bytes]) of the rows the last
 * sdrg_engine_integrate_host call left on the device; SDRG_E_INVALID when there are none or samples_per_reading has
 * changed since.  process_host(spectra = NULL) + integrate_host(NULL, NULL) + display_integrated_host(rows) copies
 * back only the display rows. */
int32_t sdrg_engine_display_integrated_host(sdrg_engine *eng, void *rows_out);

/* ------------------------------------------------------------------------------------------------
 * BUILD EXTENSION, not a reference interface: the peak table stage.  Per stream, the at most max_peaks strongest
 * local maxima of a span of one row x[0..N) of fftshifted linear power (a spectrum, or an integrated row), with a
 * minimum spacing and a threshold over the span's noise floor: the marker table of a spectrum display
 * (4096 x 16384: 16 max_peaks + 16 bytes per stream instead of 64 KiB).
 *   span       [lo, lo + nb): the display stage's three modes and rules (SDRG_DISPLAY_SPAN_FULL / FOCUS / BINS, above),
 *              resolved at each peaks call: an empty focus window, or lo + nb > N, fails that call with
 *              SDRG_E_INVALID and enqueues nothing.  p_j = x[lo + j], j in [0, nb).
 *   floor      F = the element of rank floor(nb / 2) (0-based) of p sorted ascending (the reference's gaps[size/2]
 *              convention, fft_process.cpp:256); an exact select.
 *   dB         dB(v) = 10.0f * log10f(v + 1e-20f), glibc's log10f bit for bit, as the display stage.  floor_db = dB(F).
 *   candidate  with d = min_separation, bin j is a candidate iff p_j > p_i for every i in [max(0, j - d), j) and
 *              p_j >= p_i for every i in (j, min(nb - 1, j + d)]: the first maximum of its window clipped to the span
 *              (d > nb is allowed).  Two candidates are more than d bins apart; a plateau yields its lowest bin, a
 *              constant row bin 0 only, a skirt falling monotonically from a strong bin nothing.
 *   threshold  db_j = dB(p_j); snr_j = db_j - floor_db (one float subtraction).  A candidate is above iff
 *              snr_j >= threshold_db (a NaN snr is not above).
 *   result     n_above = the number of above candidates; count = min(n_above, max_peaks); the peaks are the first
 *              `count` above candidates ordered by power descending, then bin ascending.
 *   domain     finite powers >= +0 and +inf; -0, negative powers and NaN are undefined.  All N elements of a row are
 *              data (also the element N - 1 the spectrum of an odd N never writes).
 *   config     max_peaks in [1, SDRG_PEAKS_MAX], min_separation in [1, SDRG_PEAKS_MAX_SEPARATION], threshold_db finite
 *              or -inf.
 *   outputs    peaks [n_streams][max_peaks] sdrg_peak and summary [n_streams] sdrg_peaks_summary; every byte of both
 *              is written by each call.  bin = lo + j (the row index), power = the bits read, db = db_j,
 *              snr_db = snr_j; the entries past count are {-1, 0, 0, 0}.
 * ---------------------------------------------------------------------------------------------- */
enum { SDRG_PEAKS_MAX = 64, SDRG_PEAKS_MAX_SEPARATION = 4096 };
typedef struct sdrg_peaks_config {
    int32_t span, first_bin, n_bins;   /* SDRG_DISPLAY_SPAN_*; first_bin / n_bins: SPAN_BINS only */
    int32_t max_peaks;
    int32_t min_separation;
    float threshold_db;
} sdrg_peaks_config;
typedef struct sdrg_peak {
    int32_t bin;
    float power, db, snr_db;
} sdrg_peak;
typedef struct sdrg_peaks_summary {
    int32_t count, n_above;
    float floor_power, floor_db;
} sdrg_peaks_summary;

/* Host-only, no device: the offset of bin `bin` of an fftshifted spectrum of n bins from the centre frequency, Hz:
 * ((double)(bin - n / 2) * (double)sample_rate) / (double)n  (n >= 1, bin in [0, n)). */
int32_t sdrg_bin_offset_hz(int32_t n, int64_t sample_rate, int32_t bin, double *out);

/* Set the configuration every later peaks call uses.  Checks what does not depend on N (a known span, BINS:
 * first_bin >= 0 and n_bins >= 1, max_peaks, min_separation, threshold_db); a rejected call leaves the previous
 * configuration in force.  A peaks call before any set_peaks returns SDRG_E_INVALID. */
int32_t sdrg_engine_set_peaks(sdrg_engine *eng, const sdrg_peaks_config *cfg);
int32_t sdrg_engine_get_peaks(const sdrg_engine *eng, sdrg_peaks_config *out);
/* spectra [n_streams][samples_per_reading] float, peaks [n_streams][max_peaks] and summary [n_streams] in device
 * memory.  Reads spectra only.  Runs on the main stream (the caller's after sdrg_engine_set_stream): issued right after
 * sdrg_engine_process_device or sdrg_engine_integrate_device it follows that call in every pipelining mode.  Complete
 * after sdrg_engine_synchronize, or on a stream after sdrg_engine_wait_outputs. */
int32_t sdrg_engine_peaks_device(sdrg_engine *eng, const float *spectra, sdrg_peak *peaks, sdrg_peaks_summary *summary);
/* Host buffers, synchronous.  spectra == NULL: the spectra the last sdrg_engine_process_host call with
 * SDRG_STAGE_SPECTRUM left on the device (the rule and the refusals of sdrg_engine_display_host(NULL)). */
int32_t sdrg_engine_peaks_host(sdrg_engine *eng, const float *spectra, sdrg_peak *peaks, sdrg_peaks_summary *summary);
/* The peak tables of the rows the last sdrg_engine_integrate_host call left on the device (the rule and the refusals of
 * sdrg_engine_display_integrated_host): process_host(spectra = NULL) + integrate_host(NULL, NULL) +
 * peaks_integrated_host copies back 16 max_peaks + 16 bytes per stream. */
int32_t sdrg_engine_peaks_integrated_host(sdrg_engine *eng, sdrg_peak *peaks, sdrg_peaks_summary *summary);

/* ------------------------------------------------------------------------------------------------
 * BUILD EXTENSION, not a reference interface: the DDC stage (digital down-converter).  Per stream, a channel at
 * offset_hz from the centre frequency: the raw IQ mixed down by a phase-continuous NCO, low-passed by a T-tap FIR and
 * decimated by D, as CF32.  Over the whole life of a stream (the calls' frames concatenated, whatever their lengths and
 * formats) y[m] = sum_k h[k] v[m D - k]; each call writes the outputs its frame completes.  All arithmetic is float
 * unless stated; fs = (uint32_t) of the bridge's current sample rate (the rate the SSB chain follows), N =
 * samples_per_reading at the call.
 *   config     offset_hz finite; decimation D in [1, SDRG_DDC_MAX_DECIMATION]; taps T odd in [1, SDRG_DDC_MAX_TAPS];
 *              0 < cutoff_hz <= fs / 2 with the fs at set_ddc.  A rejected set_ddc leaves the previous configuration and
 *              state in force; an accepted one, and sdrg_engine_ddc_reset, restart every stream: g0 = 0, history +0.
 *   per call   inc = round(frac(offset_hz / fs) * 2^32) mod 2^32 (the SSB variant's NCO increment) and the taps are
 *              resolved from the current fs; an fs other than the previous ddc call's restarts the streams first;
 *              cutoff_hz > fs / 2 fails the call with SDRG_E_INVALID and commits nothing (no restart either).  A change
 *              of samples_per_reading restarts nothing.
 *   taps       sdrg_ddc_design, in double: for k in [0, T): c = k - (T - 1) / 2, f = cutoff_hz / fs,
 *              ideal = 2 f if c == 0 else sin(2 pi f c) / (pi c), w = 0.5 - 0.5 cos(2 pi (k + 1) / (T + 1)),
 *              h[k] = (float)(ideal w / sum(ideal w)).
 *   unpack     CS8 (float)v * (1/128), CU8 ((float)v - 127.4f) * (1/128), CS16 (float)v * (1/32768), CF32 as is.
 *   mix        sample t of the frame has the global index g = g0 + t (uint64); ph = (uint32)(inc * g);
 *              H = hi[ph >> 22], L = lo[(ph >> 12) & 1023] of sdrg_nco_tables; wr = H.re L.re - H.im L.im,
 *              wi = H.re L.im + H.im L.re; vr = xr wr - xi wi, vi = xr wi + xi wr: every product and every sum
 *              rounded on its own.  inc = 0 goes through the table too (hi[0] lo[0] = 1).
 *   filter     for every m with g0 <= m D < g0 + N: acc = +0.0f, then for k = 0 .. T - 1 in this order
 *              acc = acc + h[k] * v[m D - k], each component on its own (a rounded multiply, then a rounded add);
 *              v[g] = +0 for g < 0.  n_out = ceil((g0 + N) / D) - ceil(g0 / D), the same for every stream, 0 when the
 *              frame holds no multiple of D.  The group delay of (T - 1) / 2 input samples is not compensated.
 *   output     out [n_streams][cap][2] float, cap = ceil(N / D); every byte is written by every call, the entries from
 *              n_out on are +0.  *n_out is set on the host before the call returns.
 *   state      per stream the last T - 1 mixed samples (floats, in device memory, allocated at the first ddc call), per
 *              engine g0, advanced by N once the call's launches have been issued: a failed call commits nothing.
 * ---------------------------------------------------------------------------------------------- */
#define SDRG_DDC_MAX_TAPS 511
#define SDRG_DDC_MAX_DECIMATION 512
typedef struct sdrg_ddc_config {
    double offset_hz;
    double cutoff_hz;
    int32_t decimation;
    int32_t taps;
} sdrg_ddc_config;

/* Host-only, no device.  The taps of cfg at sample_rate (cfg->taps floats), after the checks of set_ddc (offset_hz
 * included); sample_rate must be in [1, 2^32). */
int32_t sdrg_ddc_design(int64_t sample_rate, const sdrg_ddc_config *cfg, float *taps);
/* Host-only: the NCO's phasor tables, 4096 floats: hi[1024] then lo[1024], each {re, im}; hi[a] = e^{-j 2 pi a / 2^10},
 * lo[b] = e^{-j 2 pi b / 2^20}, computed in double and rounded to float (the tables of the SSB variant's NCO). */
int32_t sdrg_nco_tables(float *tab);
/* Host-only: how many consecutive outputs one workgroup of the DDC kernel computes for (decimation, taps): an output
 * index that is a multiple of it starts a new tile (for tests that want windows across every tile seam). */
int32_t sdrg_ddc_tile_outputs(int32_t decimation, int32_t taps, int32_t *tile);

/* Set (cfg != NULL) or switch off (cfg == NULL) the DDC.  A ddc call while it is off returns SDRG_E_INVALID and writes
 * nothing. */
int32_t sdrg_engine_set_ddc(sdrg_engine *eng, const sdrg_ddc_config *cfg);
/* The configuration in force (SDRG_E_INVALID when off), the NCO increment at the current sample rate and g0, the
 * samples every stream has consumed since the last restart; any pointer may be NULL. */
int32_t sdrg_engine_get_ddc(const sdrg_engine *eng, sdrg_ddc_config *cfg, uint32_t *nco_increment,
                            uint64_t *samples_consumed);
int32_t sdrg_engine_ddc_reset(sdrg_engine *eng);
/* cap = ceil(N / D) for the current samples_per_reading: the row length of `out`, in complex samples. */
int32_t sdrg_engine_ddc_max_out(const sdrg_engine *eng, int32_t *cap);
/* iq [n_streams][N] raw samples of format fmt (SDRG_IQ_*) and out [n_streams][cap][2] float in device memory.  Reads iq
 * only and shares nothing with sdrg_engine_process_device.  Runs on the main stream (the caller's after
 * sdrg_engine_set_stream); complete after sdrg_engine_synchronize, or on a stream after sdrg_engine_wait_outputs.  out
 * may be handed to another engine's sdrg_engine_process_device as CF32 input (samples_per_reading = cap there). */
int32_t sdrg_engine_ddc_device(sdrg_engine *eng, const void *iq, int32_t fmt, void *out, int32_t *n_out);
/* Host buffers, synchronous. */
int32_t sdrg_engine_ddc_host(sdrg_engine *eng, const void *iq, int32_t fmt, void *out, int32_t *n_out);

/* ------------------------------------------------------------------------------------------------
 * BUILD EXTENSION, not a reference interface: the DDC bank stage.  Per stream s and channel c < C, the stream's raw IQ
 * mixed down by offsets_hz[s][c], low-passed by one shared T-tap FIR and decimated by D, as CF32: C channels at their own
 * frequencies from one wideband capture.  Row s C + c of out holds, in bytes, what the DDC stage writes for stream s when
 * set to that offset with the same cutoff, D and T, so the whole out is the [n_streams C][cap][2] a second engine of
 * n_streams C streams takes on the device (demod_device, squelch_device, afc_device, tones_device, process_device as
 * CF32).  Opt-in and apart from the DDC: each has its own configuration and state.  All arithmetic is float unless
 * stated; fs and N as for the DDC.
 *   config     sdrg_bank_config and offsets_hz, n_streams * channels doubles, stream-major (offsets_hz[s * C + c]).
 *              decimation D, taps T and cutoff_hz under the DDC's rules and limits (SDRG_DDC_MAX_*); every offset finite;
 *              channels C in [1, SDRG_BANK_MAX_CHANNELS]; n_streams * C <= 65535.  A rejected set_bank leaves the
 *              previous configuration, offsets and state in force; an accepted one, and sdrg_engine_bank_reset, restart
 *              every stream: g0 = 0, history +0.
 *   per call   inc_c = round(frac(offset_c / fs) * 2^32) mod 2^32 and the taps are resolved from the current fs; an fs
 *              other than the previous bank call's restarts the streams first; cutoff_hz > fs / 2 fails the call with
 *              SDRG_E_INVALID and commits nothing (no restart either).  A change of samples_per_reading restarts nothing.
 *   taps       sdrg_ddc_design's formula with f = cutoff_hz / fs; the tables are sdrg_nco_tables.
 *   unpack     the DDC's: CS8 (float)v * (1/128), CU8 ((float)v - 127.4f) * (1/128), CS16 (float)v * (1/32768), CF32 as
 *              is.  x_s[g] is stream s's unpacked sample at the global index g (uint64), +0 for g < 0.
 *   mix        v_c[g] = x_s[g] * hi[ph >> 22] * lo[(ph >> 12) & 1023] with ph = (uint32)(inc_c * g), and the offsets in
 *              force at the call: H = hi[..], L = lo[..]; wr = H.re L.re - H.im L.im, wi = H.re L.im + H.im L.re;
 *              vr = xr wr - xi wi, vi = xr wi + xi wr: the DDC's products and order, each rounded on its own.
 *   filter     with g0 samples consumed before the call: for every m with g0 <= m D < g0 + N: acc = +0.0f, then for
 *              k = 0 .. T - 1 in this order acc = acc + h[k] * v_c[m D - k], each component on its own (a rounded
 *              multiply, then a rounded add).  n_out = ceil((g0 + N) / D) - ceil(g0 / D), the same for every row.
 *   output     out [n_streams][C][cap][2] float, cap = ceil(N / D); every byte is written by every call, the entries from
 *              n_out on of every row are +0.  *n_out is set on the host before the call returns.
 *   state      per stream the last T - 1 unpacked, *unmixed* samples (float pairs, 8 (T - 1) bytes whatever C is, in
 *              device memory), per engine g0, advanced by N once the call's launch has been issued: a failed call commits
 *              nothing.  v_c[g] is a function of g and x_s[g] alone, so mixing the history again gives the DDC's bytes
 *              (a +0 sample mixes to +-0, which moves no sum that starts at +0); the format may change between calls.
 *   retune     sdrg_engine_bank_retune replaces all offsets and restarts nothing: from the next call on, every row is
 *              what a bank set to the new offsets since the stream's start would write for the same raw samples (the
 *              phase at sample g is inc g whatever came before), the T - 1 samples of history included.  The filter is
 *              not flushed.  The phase of a channel is NOT continuous across a retune: the output steps from
 *              e^{-j 2 pi inc_old g} to e^{-j 2 pi inc_new g} at the call's first sample.  A refused retune (null,
 *              a non-finite offset, bank off) changes nothing.
 * ---------------------------------------------------------------------------------------------- */
#define SDRG_BANK_MAX_CHANNELS 4096
typedef struct sdrg_bank_config {
    double cutoff_hz;
    int32_t decimation;
    int32_t taps;
    int32_t channels;
} sdrg_bank_config;

/* Host-only: for a bank of `channels` channels on n_streams streams (the checks of set_bank on these four), how many
 * consecutive outputs one workgroup computes (an output index that is a multiple of it starts a new tile) and how many
 * consecutive channels of a stream it computes them for (a channel index that is a multiple of it starts a new group):
 * for tests that want windows across tile seams and channel counts across group seams.  No output byte depends on
 * either.  Either pointer may be NULL. */
int32_t sdrg_bank_geometry(int32_t decimation, int32_t taps, int32_t channels, int32_t n_streams, int32_t *tile_outputs,
                           int32_t *channels_per_group);
/* Set (cfg != NULL, offsets_hz [n_streams * cfg->channels]) or switch off (cfg == NULL; offsets_hz is not read) the
 * bank.  A bank call while it is off returns SDRG_E_INVALID and writes nothing. */
int32_t sdrg_engine_set_bank(sdrg_engine *eng, const sdrg_bank_config *cfg, const double *offsets_hz);
/* Replace all n_streams * channels offsets; see `retune` above. */
int32_t sdrg_engine_bank_retune(sdrg_engine *eng, const double *offsets_hz);
/* The configuration in force (SDRG_E_INVALID when off) and g0, the samples every stream has consumed since the last
 * restart; either pointer may be NULL. */
int32_t sdrg_engine_get_bank(const sdrg_engine *eng, sdrg_bank_config *cfg, uint64_t *samples_consumed);
/* The offsets in force and their NCO increments at the current sample rate, n_streams * channels values each; either
 * pointer may be NULL. */
int32_t sdrg_engine_bank_offsets(const sdrg_engine *eng, double *offsets_hz, uint32_t *increments);
int32_t sdrg_engine_bank_reset(sdrg_engine *eng);
/* cap = ceil(N / D) for the current samples_per_reading: the row length of `out`, in complex samples. */
int32_t sdrg_engine_bank_max_out(const sdrg_engine *eng, int32_t *cap);
/* iq [n_streams][N] raw samples of format fmt (SDRG_IQ_*) and out [n_streams][C][cap][2] float in device memory.  Reads
 * iq only and shares nothing with sdrg_engine_process_device or sdrg_engine_ddc_device.  Stream rules and waiting as
 * sdrg_engine_ddc_device: runs on the main stream (the caller's after sdrg_engine_set_stream); complete after
 * sdrg_engine_synchronize, or on a stream after sdrg_engine_wait_outputs.  A retune issued after the call does not
 * disturb it. */
int32_t sdrg_engine_bank_device(sdrg_engine *eng, const void *iq, int32_t fmt, void *out, int32_t *n_out);
/* Host buffers, synchronous. */
int32_t sdrg_engine_bank_host(sdrg_engine *eng, const void *iq, int32_t fmt, void *out, int32_t *n_out);

/* ------------------------------------------------------------------------------------------------
 * BUILD EXTENSION, not a reference interface: the demodulator stage.  Per stream, the n CF32 channel samples of a call
 * (the DDC's out, or any [n_streams][max_in][2] float rows in device memory) become audio at channel_rate / R: detector
 * (AM envelope or FM phase step), DC block, de-emphasis, a T2-tap real FIR decimating by R, gain, and int16 PCM or
 * float.  Over the whole life of a stream (the calls' samples concatenated, whatever their lengths) the result is that
 * of one call; each call writes the outputs its samples complete.  All arithmetic is float, every product, sum,
 * quotient and root rounded on its own, unless "double" is stated; denormals are kept.  A non-finite input sample makes
 * that stream's output unspecified from then on (the recurrences and the history carry it).  fc = channel_rate_hz.
 *   config     mode SDRG_DEMOD_AM or SDRG_DEMOD_FM; fc > 0, finite; deviation_hz > 0 and finite with (float) kf finite
 *              (FM only, ignored for AM); dc_cutoff_hz >= 0, finite (0: no DC block); deemphasis_us >= 0, finite (0: no
 *              de-emphasis); audio_decimation R in [1, SDRG_DEMOD_MAX_DECIMATION]; audio_taps T2 odd in
 *              [1, SDRG_DEMOD_MAX_TAPS]; 0 < audio_cutoff_hz <= fc / 2; gain finite; out_format SDRG_DEMOD_OUT_S16 or
 *              SDRG_DEMOD_OUT_F32; max_in in [1, 2^20]: the row length of the input in complex samples, every call's
 *              n <= max_in.  A rejected set_demod leaves the previous configuration and state in force; an accepted one,
 *              and sdrg_engine_demod_reset, restart every stream: g = 0 and every state +0.
 *   design     sdrg_demod_design, in double, each result then rounded to float: kf = fc / (2 pi deviation_hz) (FM; +0 for
 *              AM); alpha = 1 - exp(-2 pi dc_cutoff_hz / fc); a = 1 - exp(-1 / (fc deemphasis_us 1e-6)), +0 when
 *              deemphasis_us is 0; the taps are the formula of sdrg_ddc_design with f = audio_cutoff_hz / fc, T = T2.
 *   detector   sample i of the call has the global index g + i; z = (zr, zi) is the sample, w = (wr, wi) the stream's
 *              previous sample (the last one of the previous call at i = 0).
 *              AM: e = sqrtf(zr zr + zi zi), the root correctly rounded.
 *              FM: pr = zr wr + zi wi; pi = zi wr - zr wi; e = sdrg_atan2f(pi, pr) * kf.  At global index 0 there is no
 *              previous sample and e = +0 (the sign of a zero product would otherwise decide between 0 and pi).
 *   atan2f     sdrg_atan2f(y, x): ax = |x|, ay = |y|, mx = max(ax, ay), mn = min(ax, ay); q = mx > 0 ? mn / mx : 0, the
 *              quotient correctly rounded; s = q q; p = c7, then p = p s + c_k for k = 6 .. 0; r = p q; if ay > ax,
 *              r = 0x1.921fb6p+0f - r; if the sign bit of x is set, r = 0x1.921fb6p+1f - r; the result is
 *              copysignf(r, y).  c0 = 0x1.ffffecp-1f, c1 = -0x1.554ce6p-2f, c2 = 0x1.988d5p-3f, c3 = -0x1.1d09a6p-3f,
 *              c4 = 0x1.8bc022p-4f, c5 = -0x1.cbe51p-5f, c6 = 0x1.68671ep-6f, c7 = -0x1.0bce58p-8f.  Within 3.6e-7 rad
 *              of atan2 (about 1.5 ulp of pi).
 *   DC block   if alpha != 0: u = e - m, then m = m + alpha u; otherwise u = e.
 *   de-emph    if a != 0: t = u - s, then s = s + a t, and v = s; otherwise v = u.
 *   filter     for every m with g <= m R < g + n: acc = +0.0f, then for k = 0 .. T2 - 1 in this order
 *              acc = acc + h[k] * v[m R - k] (a rounded multiply, then a rounded add); v[j] = +0 for j < 0.
 *              n_out = ceil((g + n) / R) - ceil(g / R), the same for every stream, 0 when the call holds no multiple
 *              of R.  The group delay of (T2 - 1) / 2 channel samples is not compensated.
 *   output     o = y * gain.  SDRG_DEMOD_OUT_F32 writes o; SDRG_DEMOD_OUT_S16 writes
 *              (int16_t) rintf(fminf(fmaxf(o, -1.0f), 1.0f) * 32767.0f), ties to even.  out [n_streams][cap],
 *              cap = ceil(max_in / R); every byte is written by every call, the entries from n_out on are zero.  n = 0 is
 *              a valid call: no outputs, the state unchanged.  *n_out is set on the host before the call returns.
 *   state      per stream w (2 floats), m, s and the last T2 - 1 values of v, in device memory (allocated at the first
 *              demod call), in two halves a call reads and writes in turn; per engine g, advanced by n once the call's
 *              launches have been issued: a failed call commits nothing.
 * ---------------------------------------------------------------------------------------------- */
#define SDRG_DEMOD_AM 0
#define SDRG_DEMOD_FM 1
#define SDRG_DEMOD_OUT_S16 0
#define SDRG_DEMOD_OUT_F32 1
#define SDRG_DEMOD_MAX_TAPS 255
#define SDRG_DEMOD_MAX_DECIMATION 64
#define SDRG_DEMOD_MAX_IN 1048576
typedef struct sdrg_demod_config {
    double channel_rate_hz;
    double deviation_hz;
    double dc_cutoff_hz;
    double deemphasis_us;
    double audio_cutoff_hz;
    int32_t mode;
    int32_t audio_decimation;
    int32_t audio_taps;
    int32_t out_format;
    int32_t max_in;
    float gain;
} sdrg_demod_config;

/* Host-only, no device.  After the checks of set_demod: *kf, *alpha, *a and taps[cfg->audio_taps] of the design above;
 * any of the four pointers may be NULL. */
int32_t sdrg_demod_design(const sdrg_demod_config *cfg, float *kf, float *alpha, float *a, float *taps);
/* Host-only: *tile, how many consecutive FIR outputs one workgroup computes for (R, T2) (an output index that is a
 * multiple of it starts a new tile), and *chunk, how many samples of a stream the recurrence kernel takes per step (a
 * sample index that is a multiple of it starts a new step): for tests that want data across every seam. */
int32_t sdrg_demod_geometry(int32_t audio_decimation, int32_t audio_taps, int32_t *tile, int32_t *chunk);

/* Set (cfg != NULL) or switch off (cfg == NULL) the demodulator.  A demod call while it is off returns SDRG_E_INVALID
 * and writes nothing. */
int32_t sdrg_engine_set_demod(sdrg_engine *eng, const sdrg_demod_config *cfg);
/* The configuration in force (SDRG_E_INVALID when off), its four design results (taps: audio_taps floats) and g, the
 * samples every stream has consumed since the last restart; any pointer may be NULL. */
int32_t sdrg_engine_get_demod(const sdrg_engine *eng, sdrg_demod_config *cfg, float *kf, float *alpha, float *a,
                              float *taps, uint64_t *samples_consumed);
int32_t sdrg_engine_demod_reset(sdrg_engine *eng);
/* cap = ceil(max_in / R): the row length of `out`, in int16 or float by out_format. */
int32_t sdrg_engine_demod_max_out(const sdrg_engine *eng, int32_t *cap);
/* chan [n_streams][max_in][2] float, of which the first n complex samples of every row are this call's (0 <= n <=
 * max_in), and out [n_streams][cap] in device memory.  Reads chan only.  Stream rules and waiting as
 * sdrg_engine_ddc_device: runs on the main stream (the caller's after sdrg_engine_set_stream); complete after
 * sdrg_engine_synchronize, or on a stream after sdrg_engine_wait_outputs. */
int32_t sdrg_engine_demod_device(sdrg_engine *eng, const void *chan, int32_t n, void *out, int32_t *n_out);
/* Host buffers of the same shapes, synchronous. */
int32_t sdrg_engine_demod_host(sdrg_engine *eng, const void *chan, int32_t n, void *out, int32_t *n_out);
/* Tune and listen: sdrg_engine_ddc_host's iq through the DDC and the demodulator, the channel left on the device (the
 * demodulator's n is the DDC call's n_out); only the audio rows out [n_streams][cap] come back.  SDRG_E_INVALID if
 * either stage is off or max_in is smaller than the DDC's cap; a refused call commits nothing in either stage. */
int32_t sdrg_engine_ddc_demod_host(sdrg_engine *eng, const void *iq, int32_t fmt, void *out, int32_t *n_out);

/* ------------------------------------------------------------------------------------------------
 * BUILD EXTENSION, not a reference interface: the channelizer stage, a uniform polyphase filter bank.  Per stream, M
 * channels spaced fs / M apart share one prototype low-pass of L = M P taps and come out at the rate O fs / M
 * (D = M / O), as CF32: one read of the wideband frame for every channel of the band.  Nothing depends on the sample
 * rate in Hz: a rate change restarts nothing, and neither does a change of samples_per_reading.  N =
 * samples_per_reading at the call.
 *   config     cutoff_rel, the prototype's cutoff in units of the channel spacing fs / M, 0 < cutoff_rel <= M / 2;
 *              channels M a power of two in [2, SDRG_CHANNELIZER_MAX_CHANNELS]; taps_per_channel P in
 *              [1, SDRG_CHANNELIZER_MAX_TAPS_PER_CHANNEL] with L = M P <= SDRG_CHANNELIZER_MAX_TAPS; oversample O 1 or
 *              2; the rows written are [first_channel, first_channel + n_channels) of the fftshifted channel order,
 *              n_channels >= 1, first_channel >= 0, first_channel + n_channels <= M.  A rejected set_channelizer
 *              leaves the previous configuration and state in force; an accepted one, and
 *              sdrg_engine_channelizer_reset, restart every stream: g0 = 0, history +0.
 *   prototype  sdrg_channelizer_design, in double: h[0 .. L - 2] is the formula of sdrg_ddc_design with
 *              f = cutoff_rel / M and T = L - 1 (odd), and h[L - 1] = +0.  So at cutoff_hz / fs == cutoff_rel / M the
 *              bank's taps are sdrg_ddc_design's for T = L - 1.
 *   unpack     the DDC's: CS8 (float)v * (1/128), CU8 ((float)v - 127.4f) * (1/128), CS16 (float)v * (1/32768), CF32
 *              as is.
 *   channel    c in [0, M) is centred at c fs / M (c >= M / 2: negative).  Over the whole life of a stream (the calls'
 *              frames concatenated, whatever their lengths and formats), x[g] = +0 for g < 0, the output time m sits
 *              at the input index m D:
 *                u_p[m] = sum_{q = 0}^{P - 1} h[p + q M] x[m D - p - q M], p in [0, M)    (the branch sums)
 *                Y_c[m] = sum_p u_p[m] e^{+j 2 pi c p / M}
 *                y_c[m] = Y_c[m] at O = 1, (-1)^{c m} Y_c[m] at O = 2.
 *              This is sum_n h[n] v_c[m D - n] with v_c[g] = x[g] e^{-j 2 pi c g / M}: the DDC at offset_hz = c fs / M
 *              with the same taps and decimation D, in its phase convention; the group delay of (L - 2) / 2 input
 *              samples is not compensated.
 *   arithmetic float throughout; fused multiply-adds, any association of the sums and any FFT algorithm are allowed:
 *              the result is specified by the bound below, not by its bytes.  With eps = 2^-24, per output and channel
 *                |y - exact| <= (P + 2) eps sum_n |h[n]| |x[m D - n]| + 8 log2(M) eps sqrt(M) ||u[m]||_2.
 *              Two properties hold byte for byte all the same: an output depends only on its window of L samples (and
 *              on c and m), so a stream cut into calls anywhere gives the bytes of one call; and the same call on the
 *              same state gives the same bytes.  After a non-finite CF32 sample a stream's output is unspecified.
 *   output     out [n_streams][n_channels][cap][2] float, cap = ceil(N / D).  Row r is channel k = first_channel + r
 *              of the fftshifted order, c = (k + M / 2) mod M; sdrg_bin_offset_hz(M, fs, k) is its centre's offset.
 *              With g0 samples consumed before it, a call writes the outputs with g0 <= m D < g0 + N:
 *              n_out = ceil((g0 + N) / D) - ceil(g0 / D) of them, the same for every stream and row.  Every byte of
 *              out is written by every call, +0 from n_out on in every row.  *n_out is set on the host before the
 *              call returns.  Viewed as [n_streams n_channels][cap][2], out is what an engine of that many streams
 *              takes as sdrg_engine_demod_device input (max_in = cap, n = n_out) or as CF32 process_device input.
 *   state      per stream the last L - 1 unpacked samples as float pairs, in device memory, in two halves a call reads
 *              and writes in turn (allocated at the first call); per engine g0, advanced by N once the call's launch
 *              has been issued: a failed call commits nothing.  The taps live in a device buffer written by
 *              set_channelizer, never by a call.
 * ---------------------------------------------------------------------------------------------- */
#define SDRG_CHANNELIZER_MAX_CHANNELS 256
#define SDRG_CHANNELIZER_MAX_TAPS_PER_CHANNEL 32
#define SDRG_CHANNELIZER_MAX_TAPS 4096
typedef struct sdrg_channelizer_config {
    double cutoff_rel;
    int32_t channels;
    int32_t taps_per_channel;
    int32_t oversample;
    int32_t first_channel;
    int32_t n_channels;
} sdrg_channelizer_config;

/* Host-only, no device.  The prototype of cfg (channels * taps_per_channel floats), after the checks of
 * set_channelizer. */
int32_t sdrg_channelizer_design(const sdrg_channelizer_config *cfg, float *taps);
/* Host-only: how many consecutive output times one workgroup of the channelizer kernel computes for cfg: an output
 * index that is a multiple of it starts a new tile (for tests that want windows across every tile seam). */
int32_t sdrg_channelizer_tile_outputs(const sdrg_channelizer_config *cfg, int32_t *tile);

/* Set (cfg != NULL) or switch off (cfg == NULL) the channelizer.  A channelizer call while it is off returns
 * SDRG_E_INVALID and writes nothing. */
int32_t sdrg_engine_set_channelizer(sdrg_engine *eng, const sdrg_channelizer_config *cfg);
/* The configuration in force (SDRG_E_INVALID when off) and g0, the samples every stream has consumed since the last
 * restart; either pointer may be NULL. */
int32_t sdrg_engine_get_channelizer(const sdrg_engine *eng, sdrg_channelizer_config *cfg, uint64_t *samples_consumed);
int32_t sdrg_engine_channelizer_reset(sdrg_engine *eng);
/* cap = ceil(N / D) for the current samples_per_reading: the row length of `out`, in complex samples. */
int32_t sdrg_engine_channelizer_max_out(const sdrg_engine *eng, int32_t *cap);
/* iq [n_streams][N] raw samples of format fmt (SDRG_IQ_*) and out [n_streams][n_channels][cap][2] float in device
 * memory.  Reads iq only and shares nothing with sdrg_engine_process_device or the DDC.  Stream rules and waiting as
 * sdrg_engine_ddc_device: runs on the main stream (the caller's after sdrg_engine_set_stream); complete after
 * sdrg_engine_synchronize, or on a stream after sdrg_engine_wait_outputs. */
int32_t sdrg_engine_channelizer_device(sdrg_engine *eng, const void *iq, int32_t fmt, void *out, int32_t *n_out);
/* Host buffers, synchronous. */
int32_t sdrg_engine_channelizer_host(sdrg_engine *eng, const void *iq, int32_t fmt, void *out, int32_t *n_out);

/* ------------------------------------------------------------------------------------------------
 * BUILD EXTENSION, not a reference interface: the resampler stage, a polyphase rational resampler.  Per stream, the n
 * values of a call (the demodulator's float audio, the DDC's or the channelizer's CF32 channel, or any rows in device
 * memory) come out at exactly L / M times their rate: fs = 2 000 000 / 41 Hz audio through 123 / 125 is 48 000 Hz.
 * Nothing depends on a rate in Hz.  Over the whole life of a stream (the calls' values concatenated, whatever their
 * lengths) the result is that of one call; each call writes the outputs its values complete.  All arithmetic is float,
 * every product and sum rounded on its own, unless "double" is stated; denormals are kept.  A non-finite input value
 * makes that stream's output unspecified from then on (the history carries it).
 *   config     interp L and decim M in [1, SDRG_RESAMPLE_MAX_FACTOR] with gcd(L, M) = 1 (a reducible pair is refused;
 *              sdrg_resample_ratio reduces one) and 1/8 <= L / M <= 8 (larger decimations belong to the DDC and the
 *              demodulator); taps_per_phase P in [1, SDRG_RESAMPLE_MAX_TAPS_PER_PHASE] with L P <=
 *              SDRG_RESAMPLE_MAX_TAPS; 0 < cutoff_rel <= 1, the prototype's cutoff in units of the narrower Nyquist
 *              band, min(in, out) rate / 2; components 1 (real float rows [n_streams][max_in]) or 2 (CF32 rows
 *              [n_streams][max_in][2], each component resampled on its own); out_format SDRG_RESAMPLE_OUT_S16 or
 *              SDRG_RESAMPLE_OUT_F32, applied to each component; gain finite; max_in in [1, 2^20]: the row length of
 *              the input, every call's n <= max_in.  A rejected set_resample leaves the previous configuration and
 *              state in force; an accepted one, and sdrg_engine_resample_reset, restart every stream: g = 0, history +0.
 *   prototype  sdrg_resample_design, in double: with n = L P and T = n if n is odd, else n - 1, h[0 .. T - 1] is the
 *              formula of sdrg_ddc_design with f = cutoff_rel / (2 max(L, M)) cycles per upsampled sample, scaled to
 *              the DC gain L before its single rounding: h[k] = (float)((double)L v[k] / sum).  h[T .. n - 1] = +0.
 *   filter     x[i] is the stream's input since the restart, x[i] = +0 for i < 0.  Output m has q = floor(m M / L) and
 *              phi = (m M) mod L: acc = +0.0f, then for k = 0 .. P - 1 in this order
 *              acc = acc + h[phi + k L] * x[q - k] (a rounded multiply, then a rounded add), per component.  With g
 *              values consumed before it, a call of n writes the outputs with g <= q < g + n, the m in
 *              [ceil(g L / M), ceil((g + n) L / M)): n_out of them, the same for every stream, possibly 0 when M > L
 *              (the call still advances the history).  The group delay of (T - 1) / 2 upsampled samples is not
 *              compensated.
 *   output     o = y * gain.  SDRG_RESAMPLE_OUT_F32 writes o; SDRG_RESAMPLE_OUT_S16 writes the demodulator's
 *              (int16_t) rintf(fminf(fmaxf(o, -1.0f), 1.0f) * 32767.0f), ties to even.  out [n_streams][cap] of float
 *              or int16, or of pairs of them at components = 2; cap = ceil(max_in L / M).  Every byte is written by
 *              every call, zero from n_out on.  n = 0 is a valid call: no outputs, the state unchanged.  *n_out is set
 *              on the host before the call returns.
 *   state      per stream the last P - 1 input values, in device memory (allocated at the first resample call), in two
 *              halves a call reads and writes in turn; per engine g, advanced by n once the call's launch has been
 *              issued: a failed call commits nothing.  The taps live in a device buffer, in the order [phi][k], written
 *              by set_resample, never by a call.
 * ---------------------------------------------------------------------------------------------- */
#define SDRG_RESAMPLE_OUT_S16 0
#define SDRG_RESAMPLE_OUT_F32 1
#define SDRG_RESAMPLE_MAX_FACTOR 512
#define SDRG_RESAMPLE_MAX_TAPS_PER_PHASE 64
#define SDRG_RESAMPLE_MAX_TAPS 8192
#define SDRG_RESAMPLE_MAX_IN 1048576
typedef struct sdrg_resample_config {
    double cutoff_rel;
    int32_t interp;
    int32_t decim;
    int32_t taps_per_phase;
    int32_t components;
    int32_t out_format;
    int32_t max_in;
    float gain;
} sdrg_resample_config;

/* Host-only, no device.  The prototype of cfg (interp * taps_per_phase floats), after the checks of set_resample. */
int32_t sdrg_resample_design(const sdrg_resample_config *cfg, float *taps);
/* Host-only: how many consecutive outputs one workgroup of the resampler kernel computes for cfg: an output index of a
 * call that is a multiple of it starts a new tile (for tests that want windows across every tile seam). */
int32_t sdrg_resample_tile_outputs(const sdrg_resample_config *cfg, int32_t *tile);
/* Host-only: *interp / *decim = out_hz * in_den / in_num in lowest terms, the ratio that takes the rate in_num / in_den
 * Hz to out_hz Hz: (2 000 000, 41, 48 000) gives 123 / 125.  SDRG_E_INVALID, and nothing written, if an argument is 0
 * or the reduced pair is outside the limits of the configuration. */
int32_t sdrg_resample_ratio(uint64_t in_num, uint64_t in_den, uint64_t out_hz, int32_t *interp, int32_t *decim);

/* Set (cfg != NULL) or switch off (cfg == NULL) the resampler.  A resample call while it is off returns SDRG_E_INVALID
 * and writes nothing. */
int32_t sdrg_engine_set_resample(sdrg_engine *eng, const sdrg_resample_config *cfg);
/* The configuration in force (SDRG_E_INVALID when off), its prototype (taps: interp * taps_per_phase floats) and g, the
 * values every stream has consumed since the last restart; any pointer may be NULL. */
int32_t sdrg_engine_get_resample(const sdrg_engine *eng, sdrg_resample_config *cfg, float *taps,
                                 uint64_t *samples_consumed);
int32_t sdrg_engine_resample_reset(sdrg_engine *eng);
/* cap = ceil(max_in L / M): the row length of `out`, in floats or int16, or pairs of them, by the configuration. */
int32_t sdrg_engine_resample_max_out(const sdrg_engine *eng, int32_t *cap);
/* in: n_streams rows in_stride values apart (a value is a float, or a float pair at components = 2), of which the
 * first n of every row are this call's (0 <= n <= max_in, in_stride >= n), and out [n_streams][cap], in device memory.
 * Reads `in` only.  Stream rules and waiting as sdrg_engine_ddc_device: runs on the main stream (the caller's after
 * sdrg_engine_set_stream); complete after sdrg_engine_synchronize, or on a stream after sdrg_engine_wait_outputs. */
int32_t sdrg_engine_resample_device(sdrg_engine *eng, const void *in, int32_t in_stride, int32_t n, void *out,
                                    int32_t *n_out);
/* Host buffers of the same shapes, synchronous; all n_streams * in_stride values of `in` are copied. */
int32_t sdrg_engine_resample_host(sdrg_engine *eng, const void *in, int32_t in_stride, int32_t n, void *out,
                                  int32_t *n_out);
/* Tune and listen at the sound device's rate: sdrg_engine_ddc_demod_host's iq through the DDC, the demodulator and the
 * resampler, the channel and the audio left on the device (the resampler's n is the demodulator's n_out); only the
 * resampled rows out [n_streams][cap] come back.  SDRG_E_INVALID if a stage is off, the demodulator's max_in is smaller
 * than the DDC's cap, the demodulator does not write SDRG_DEMOD_OUT_F32, or the resampler has components != 1 or a
 * max_in smaller than the demodulator's cap; a refused call commits nothing in any stage. */
int32_t sdrg_engine_ddc_demod_resample_host(sdrg_engine *eng, const void *iq, int32_t fmt, void *out, int32_t *n_out);

/* ------------------------------------------------------------------------------------------------
 * BUILD EXTENSION, not a reference interface: the squelch stage, a power gate with hysteresis and a level read-out per
 * channel.  Per stream, the n CF32 channel samples of a call (the DDC's out, a row of the channelizer's, or any rows in
 * device memory) are cut into blocks of S samples at the global indices that are multiples of S.  Each completed
 * block's mean power updates a smoothed level; a hysteresis gate with a hang time decides from that level how the next
 * block passes; a transition is ramped over one block; a record per stream reports the level and the gate.  A decision
 * never reaches back into the block that produced it: the stage adds no delay and out has one sample per input sample.
 * Over the whole life of a stream (the calls' samples concatenated, whatever their lengths) the result is that of one
 * call.  A sample gated to (+0, +0) is silence in both detectors of the demodulator (sqrtf(0) = +0, sdrg_atan2f(+-0,
 * +-0) kf = +-0), so one gate in front of it serves every mode.  All arithmetic is float, every product and sum rounded
 * on its own, unless "double" is stated; denormals are kept.  A non-finite input sample makes that stream's outputs and
 * records unspecified from then on.
 *   config     open_db, close_db finite with close_db <= open_db; tau_blocks finite, >= 0; block S a power of two in
 *              [SDRG_SQUELCH_MIN_BLOCK, SDRG_SQUELCH_MAX_BLOCK]; hang_blocks H in [0, SDRG_SQUELCH_MAX_HANG]; max_in in
 *              [1, 2^20]: every call's n <= in_stride <= max_in.  A rejected set_squelch changes nothing; an accepted
 *              one, and sdrg_engine_squelch_reset, restart every stream: g = 0, L = +0, closed, hang 0, the current
 *              block's code 0.
 *   design     sdrg_squelch_design, in double, each result rounded to float once: open_thr = 10^(open_db / 10),
 *              close_thr = 10^(close_db / 10), refused if either is not finite and positive as a float; beta =
 *              1 - exp(-1 / tau_blocks), and beta = 1.0f exactly when tau_blocks is 0.  0 dB is a channel of mean
 *              power 1.
 *   power      sample j of a block (its in-block index: the global index mod S) has p_j = zr zr + zi zi: two rounded
 *              products, one rounded sum.  The block's sum is the adjacent-pair tree over its S powers: q'[i] =
 *              q[2 i] + q[2 i + 1], repeated until one value is left; P = q[0] * (1 / S).
 *   level      for each completed block, in order: if beta == 1, L = P; otherwise d = P - L, then L = L + beta * d.
 *   gate       then was = open, and: if open and L >= close_thr, hang = H; else if open and hang > 0, hang = hang - 1;
 *              else if open, open = 0; if closed and L >= open_thr, open = 1 and hang = H.  The next block's code is
 *              2 was + open: 0 closed, 1 ramp up, 2 ramp down, 3 open.  Global block 0 has code 0.
 *   output     the sample at in-block index i under its block's code, r = 1 / S: code 0 (+0, +0); code 3 the input's
 *              eight bytes; code 1 w = (float)(i + 1) * r and (zr * w, zi * w); code 2 w = (float)(S - 1 - i) * r and
 *              (zr * w, zi * w).  out [n_streams][in_stride][2] float: every byte is written by every call, zero from n
 *              on.  out may be chan itself (gating in place); any other overlap is undefined.  n = 0 is a valid call:
 *              it writes out and the records and leaves the state where it is.
 *   records    sdrg_squelch_record [n_streams], written by every call: level is L after the last block completed so far
 *              (+0 before the first); level_db = 10.0f * log10f(level + 1e-20f) with glibc's log10f bit for bit (the
 *              display stage's rule); open is the gate after that block; open_blocks is how many of the blocks this
 *              call completed left the gate open.  *n_blocks = floor((g + n) / S) - floor(g / S), the blocks this call
 *              completed, is set on the host before the call returns.
 *   state      per stream the powers of the block in progress (S - 1 floats), L, open, hang and the current block's
 *              code, in device memory (allocated at the first squelch call), in two halves a call reads and writes in
 *              turn; per engine g, advanced by n once the call's launches have been issued: a failed call commits
 *              nothing.  Calls shorter than a block accumulate; any number of calls may share one block.
 * ---------------------------------------------------------------------------------------------- */
#define SDRG_SQUELCH_MIN_BLOCK 16
#define SDRG_SQUELCH_MAX_BLOCK 1024
#define SDRG_SQUELCH_MAX_HANG 65535
#define SDRG_SQUELCH_MAX_IN 1048576
typedef struct sdrg_squelch_config {
    double open_db;
    double close_db;
    double tau_blocks;
    int32_t block;
    int32_t hang_blocks;
    int32_t max_in;
} sdrg_squelch_config;

typedef struct sdrg_squelch_record {
    float level;
    float level_db;
    int32_t open;
    int32_t open_blocks;
} sdrg_squelch_record;

/* Host-only, no device.  After the checks of set_squelch: the three design values above; any of the three pointers may
 * be NULL. */
int32_t sdrg_squelch_design(const sdrg_squelch_config *cfg, float *open_thr, float *close_thr, float *beta);
/* Host-only: *tile = max(512, block), how many consecutive samples one workgroup takes: of the power kernel those of
 * the global indices [k tile, (k + 1) tile), of the gate kernel those of the call's indices [k tile, (k + 1) tile) (for
 * tests that want data across every seam). */
int32_t sdrg_squelch_geometry(int32_t block, int32_t *tile);

/* Set (cfg != NULL) or switch off (cfg == NULL) the squelch.  A squelch call while it is off returns SDRG_E_INVALID and
 * writes nothing. */
int32_t sdrg_engine_set_squelch(sdrg_engine *eng, const sdrg_squelch_config *cfg);
/* The configuration in force (SDRG_E_INVALID when off), its three design values and g, the samples every stream has
 * consumed since the last restart; any pointer may be NULL. */
int32_t sdrg_engine_get_squelch(const sdrg_engine *eng, sdrg_squelch_config *cfg, float *open_thr, float *close_thr,
                                float *beta, uint64_t *samples_consumed);
int32_t sdrg_engine_squelch_reset(sdrg_engine *eng);
/* chan and out: n_streams rows of in_stride complex samples ([n_streams][in_stride][2] float), of which the first n of
 * every row are this call's (0 <= n <= in_stride <= max_in); records [n_streams] or NULL; all in device memory.  The
 * rows of a channelizer's out [B][n_channels][cap][2] are those of an engine of B n_channels streams (in_stride = cap).
 * Stream rules and waiting as sdrg_engine_demod_device: runs on the main stream (the caller's after
 * sdrg_engine_set_stream); complete after sdrg_engine_synchronize, or on a stream after sdrg_engine_wait_outputs. */
int32_t sdrg_engine_squelch_device(sdrg_engine *eng, const void *chan, int32_t in_stride, int32_t n, void *out,
                                   sdrg_squelch_record *records, int32_t *n_blocks);
/* Host buffers of the same shapes, synchronous; all n_streams * in_stride samples of chan are copied. */
int32_t sdrg_engine_squelch_host(sdrg_engine *eng, const void *chan, int32_t in_stride, int32_t n, void *out,
                                 sdrg_squelch_record *records, int32_t *n_blocks);
/* Tune, gate and listen: sdrg_engine_ddc_demod_host with the squelch between the DDC and the demodulator, in place on
 * the channel the chain keeps on the device (in_stride = the DDC's cap, n = the DDC call's n_out).  Only the audio rows
 * and, unless records is NULL, the records [n_streams] come back.  SDRG_E_INVALID under sdrg_engine_ddc_demod_host's
 * conditions, or if the squelch is off or its max_in is smaller than the DDC's cap; a refused call commits nothing in
 * any stage.  sdrg_engine_ddc_demod_host itself never gates, whether or not a squelch is set. */
int32_t sdrg_engine_ddc_squelch_demod_host(sdrg_engine *eng, const void *iq, int32_t fmt, void *out, int32_t *n_out,
                                           sdrg_squelch_record *records);
/* The same for sdrg_engine_ddc_demod_resample_host. */
int32_t sdrg_engine_ddc_squelch_demod_resample_host(sdrg_engine *eng, const void *iq, int32_t fmt, void *out,
                                                    int32_t *n_out, sdrg_squelch_record *records);

/* ------------------------------------------------------------------------------------------------
 * BUILD EXTENSION, not a reference interface: the AGC stage, one block-ramped gain per channel ahead of the
 * demodulator.  Per stream, the n CF32 channel samples of a call (the DDC's out, the squelch's out, a row of the
 * channelizer's, or any rows in device memory) are cut into blocks of S samples at the global indices that are multiples
 * of S, as the squelch's are.  Each completed block's statistic (its mean power or its peak power) moves the stream's
 * gain by an attack / hang / decay law; block b is multiplied by a ramp from the gain after block b - 2 to the gain after
 * block b - 1.  The gain is therefore continuous across the seams of the blocks, and a decision never reaches back into
 * the block that produced it: the stage adds no delay and out has one sample per input sample.  Over the whole life of a
 * stream (the calls' samples concatenated, whatever their lengths) the result is that of one call.  All arithmetic is
 * float, every product, sum, quotient and root rounded on its own (IEEE, correctly rounded), unless "double" is stated;
 * denormals are kept.  A non-finite input sample makes that stream's outputs and records unspecified from then on.
 *   config     target, the wanted RMS (detector MEAN) or peak (PEAK) amplitude of the output, finite and positive as a
 *              float; max_gain_db and initial_gain_db finite; floor_db finite or -INFINITY; attack_blocks and
 *              decay_blocks finite, >= 0; detector SDRG_AGC_DET_MEAN or SDRG_AGC_DET_PEAK; block S a power of two in
 *              [SDRG_AGC_MIN_BLOCK, SDRG_AGC_MAX_BLOCK]; hang_blocks H in [0, SDRG_AGC_MAX_HANG]; max_in in [1, 2^20]:
 *              every call's n <= in_stride <= max_in.  A rejected set_agc changes nothing; an accepted one, and
 *              sdrg_engine_agc_reset, restart every stream: g = 0, G = G_prev = init_gain, hang 0, P_last = +0.
 *   design     sdrg_agc_design, in double, each result rounded to float once: max_gain = 10^(max_gain_db / 20) and
 *              init_gain = 10^(initial_gain_db / 20), refused unless both are finite and positive as floats and
 *              init_gain <= max_gain; floor_thr = 10^(floor_db / 10), which may be +0 (floor_db = -INFINITY gives +0) and
 *              must be finite; alpha_a = 1 - exp(-1 / attack_blocks) and alpha_d = 1 - exp(-1 / decay_blocks), each
 *              1.0f exactly when its time is 0.  target is rounded to float once.
 *   statistic  sample j of a block has p_j = zr zr + zi zi: two rounded products, one rounded sum.  MEAN: P is the
 *              squelch's: the adjacent-pair tree over the S powers (q'[i] = q[2 i] + q[2 i + 1] until one value is left),
 *              times 1 / S.  PEAK: P = max_j p_j.
 *   step       for each completed block k, in order: P_last = P.  If P < floor_thr, nothing else changes (the hold: the
 *              squelch's zeros give P = +0, so behind a closed gate the gain stays where it was).  Otherwise
 *              a = sqrtf(P), want = fminf(target / a, max_gain) (a = 0 gives max_gain), d = want - G, and: if want < G,
 *              G = want if alpha_a == 1, else G = G + alpha_a * d, hang = H, and the block counts as an attack; else if
 *              hang > 0, hang = hang - 1; else G = want if alpha_d == 1, else G = G + alpha_d * d.  gain[k] is G after
 *              the step (the hold included); gain[-1] = gain[-2] = init_gain.
 *   output     sample i (in-block index) of global block b, with r = 1 / S, g0 = gain[b - 2], g1 = gain[b - 1]:
 *              t = (float)(i + 1) * r, w = g0 + (g1 - g0) * t, and the output is (zr * w, zi * w).  Block 0 runs at
 *              init_gain.  out [n_streams][in_stride][2] float: every byte is written by every call, zero from n on.  out
 *              may be chan itself (in place); any other overlap is undefined.  n = 0 is a valid call: it writes out and
 *              the records and leaves the state where it is.
 *   records    sdrg_agc_record [n_streams], written by every call: gain is gain[k] of the last block completed so far
 *              (init_gain before the first); gain_db = 20.0f * log10f(gain); level_db = 10.0f * log10f(P_last + 1e-20f),
 *              P_last the statistic of that block (+0 before the first), both with glibc's log10f bit for bit (the
 *              display stage's rule); attacks is how many of the blocks this call completed took the attack branch.
 *              *n_blocks = floor((g + n) / S) - floor(g / S) is set on the host before the call returns.
 *   state      per stream {G, G_prev, hang, P_last} and the powers of the block in progress (S - 1 floats), in device
 *              memory (allocated at the first agc call), in two halves a call reads and writes in turn; per engine g,
 *              advanced by n once the call's launches have been issued: a failed call commits nothing.  Calls shorter
 *              than a block accumulate; any number of calls may share one block.
 * ---------------------------------------------------------------------------------------------- */
#define SDRG_AGC_MIN_BLOCK 16
#define SDRG_AGC_MAX_BLOCK 1024
#define SDRG_AGC_MAX_HANG 65535
#define SDRG_AGC_MAX_IN 1048576
#define SDRG_AGC_DET_MEAN 0
#define SDRG_AGC_DET_PEAK 1
typedef struct sdrg_agc_config {
    double target;
    double max_gain_db;
    double initial_gain_db;
    double floor_db;
    double attack_blocks;
    double decay_blocks;
    int32_t detector;
    int32_t block;
    int32_t hang_blocks;
    int32_t max_in;
} sdrg_agc_config;

typedef struct sdrg_agc_record {
    float gain;
    float gain_db;
    float level_db;
    int32_t attacks;
} sdrg_agc_record;

/* Host-only, no device.  After the checks of set_agc: the five design values above; any of the five pointers may be
 * NULL. */
int32_t sdrg_agc_design(const sdrg_agc_config *cfg, float *max_gain, float *init_gain, float *floor_thr, float *alpha_a,
                        float *alpha_d);
/* Host-only: *tile = max(512, block), how many consecutive samples one workgroup takes: of the power kernel those of
 * the positions [k tile, (k + 1) tile) counted from the start of the block in progress, of the apply kernel those of the
 * call's indices [k tile, (k + 1) tile) (for tests that want data across every seam). */
int32_t sdrg_agc_geometry(int32_t block, int32_t *tile);

/* Set (cfg != NULL) or switch off (cfg == NULL) the AGC.  An agc call while it is off returns SDRG_E_INVALID and writes
 * nothing. */
int32_t sdrg_engine_set_agc(sdrg_engine *eng, const sdrg_agc_config *cfg);
/* The configuration in force (SDRG_E_INVALID when off), its five design values and g, the samples every stream has
 * consumed since the last restart; any pointer may be NULL. */
int32_t sdrg_engine_get_agc(const sdrg_engine *eng, sdrg_agc_config *cfg, float *max_gain, float *init_gain,
                            float *floor_thr, float *alpha_a, float *alpha_d, uint64_t *samples_consumed);
int32_t sdrg_engine_agc_reset(sdrg_engine *eng);
/* chan and out: n_streams rows of in_stride complex samples ([n_streams][in_stride][2] float), of which the first n of
 * every row are this call's (0 <= n <= in_stride <= max_in); records [n_streams] or NULL; all in device memory.  Stream
 * rules and waiting as sdrg_engine_squelch_device. */
int32_t sdrg_engine_agc_device(sdrg_engine *eng, const void *chan, int32_t in_stride, int32_t n, void *out,
                               sdrg_agc_record *records, int32_t *n_blocks);
/* Host buffers of the same shapes, synchronous; all n_streams * in_stride samples of chan are copied. */
int32_t sdrg_engine_agc_host(sdrg_engine *eng, const void *chan, int32_t in_stride, int32_t n, void *out,
                             sdrg_agc_record *records, int32_t *n_blocks);

/* Tune and listen, with the steps the mask names: iq through DDC -> [squelch] -> [AGC] -> demodulator -> [resampler].
 * The squelch and the AGC run in place on the channel the chain keeps on the device (in_stride = the DDC's cap, n = the
 * DDC call's n_out); only the last stage's rows and, for each record pointer that is not NULL and whose stage is in the
 * mask, that stage's records [n_streams] come back (a record pointer whose stage is not in the mask is ignored).  The
 * four chain calls above are this call with the masks 0, SDRG_LISTEN_RESAMPLE, SDRG_LISTEN_SQUELCH and
 * SDRG_LISTEN_SQUELCH | SDRG_LISTEN_RESAMPLE: they never run the AGC, whether or not one is set.  SDRG_E_INVALID, in
 * this order: a null engine, iq, out or n_out; a mask with other bits; the demodulator off; the resampler, the squelch,
 * the AGC off while in the mask; the DDC's own refusals; the demodulator's max_in, then the squelch's, then the AGC's
 * smaller than the DDC's cap; with the resampler, a demodulator that does not write SDRG_DEMOD_OUT_F32, a resampler
 * with components != 1 or a max_in smaller than the demodulator's cap.  A refused call commits nothing in any stage. */
#define SDRG_LISTEN_SQUELCH 1
#define SDRG_LISTEN_AGC 2
#define SDRG_LISTEN_RESAMPLE 4
int32_t sdrg_engine_listen_host(sdrg_engine *eng, int32_t steps, const void *iq, int32_t fmt, void *out, int32_t *n_out,
                                sdrg_squelch_record *squelch_records, sdrg_agc_record *agc_records);

/* ------------------------------------------------------------------------------------------------
 * BUILD EXTENSION, not a reference interface: the sideband stage.  Per stream, the n CF32 channel samples of a call
 * (the DDC's out, the squelch's or the AGC's, or any [n_streams][max_in][2] float rows in device memory) become the
 * audio of one sideband, or of both, at channel_rate / R: the real part of a T-tap complex band-pass over
 * [low_hz, high_hz] above the channel's centre (upper) or below it (lower), decimated by R, gain, and int16 PCM or
 * float.  CW is the upper sideband of a channel tuned 700 Hz below the signal with a narrow band around 700 Hz.  Over
 * the whole life of a stream (the calls' samples concatenated, whatever their lengths) the result is that of one call;
 * each call writes the outputs its samples complete.  All arithmetic is float, every product and sum rounded on its
 * own, unless "double" is stated; denormals are kept.  A non-finite input sample makes that stream's output
 * unspecified from then on (the history carries it).  fc = channel_rate_hz.
 *   config     fc > 0, finite; low_hz and high_hz finite with 0 <= low_hz < high_hz <= fc / 2; mode
 *              SDRG_SIDEBAND_UPPER, SDRG_SIDEBAND_LOWER or SDRG_SIDEBAND_BOTH; audio_decimation R in
 *              [1, SDRG_SIDEBAND_MAX_DECIMATION]; taps T odd in [1, SDRG_SIDEBAND_MAX_TAPS]; out_format
 *              SDRG_SIDEBAND_OUT_S16 or SDRG_SIDEBAND_OUT_F32; max_in in [1, 2^20]: the row length of the input in
 *              complex samples, every call's n <= max_in; gain finite.  A rejected set_sideband leaves the previous
 *              configuration and state in force; an accepted one, and sdrg_engine_sideband_reset, restart every
 *              stream: g = 0 and the history +0.
 *   design     sdrg_sideband_design, in double, each result then rounded to float once: p[k], k in [0, T), is the
 *              formula of sdrg_ddc_design with f = (high_hz - low_hz) / (2 fc), normalised to sum 1 and not rounded;
 *              fm = (low_hz + high_hz) / 2; theta_k = 2 pi fm (k - (T - 1) / 2) / fc;
 *              cr[k] = (float) (p[k] cos theta_k), ci[k] = (float) (p[k] sin theta_k).  T = 1 gives cr = 1, ci = 0.
 *              c = cr + j ci passes [low_hz, high_hz] and stops [-high_hz, -low_hz]; its conjugate does the reverse.
 *   filter     sample i of the call has the global index g + i; z[j] = (zr[j], zi[j]) is the stream's sample at the
 *              global index j, (+0, +0) for j < 0.  For every m with g <= m R < g + n: acc = (+0, +0), then for
 *              k = 0 .. T - 1 in this order acc.x = acc.x + cr[k] * zr[m R - k] and acc.y = acc.y + ci[k] * zi[m R - k]
 *              (a rounded multiply, then a rounded add, each).  Then u = acc.x - acc.y, the upper sideband
 *              Re(c * z), and l = acc.x + acc.y, the lower, Re(conj(c) * z).  n_out = ceil((g + n) / R) -
 *              ceil(g / R), the same for every stream, 0 when the call holds no multiple of R.  The group delay of
 *              (T - 1) / 2 channel samples is not compensated.
 *   output     o = u * gain (UPPER) or l * gain (LOWER); BOTH writes the pair (u * gain, l * gain) interleaved.
 *              SDRG_SIDEBAND_OUT_F32 writes o; SDRG_SIDEBAND_OUT_S16 writes
 *              (int16_t) rintf(fminf(fmaxf(o, -1.0f), 1.0f) * 32767.0f), ties to even.  out [n_streams][cap], at BOTH
 *              [n_streams][cap][2], cap = ceil(max_in / R); every byte is written by every call, the entries from
 *              n_out on are zero.  n = 0 is a valid call: no outputs, the state unchanged.  *n_out is set on the host
 *              before the call returns.
 *   state      per stream the last T - 1 samples as float pairs, in device memory (allocated at the first sideband
 *              call), in two halves a call reads and writes in turn; per engine g, advanced by n once the call's launch
 *              has been issued: a failed call commits nothing.  The first call after a restart reads no half.
 * ---------------------------------------------------------------------------------------------- */
#define SDRG_SIDEBAND_UPPER 0
#define SDRG_SIDEBAND_LOWER 1
#define SDRG_SIDEBAND_BOTH 2
#define SDRG_SIDEBAND_OUT_S16 0
#define SDRG_SIDEBAND_OUT_F32 1
#define SDRG_SIDEBAND_MAX_TAPS 511
#define SDRG_SIDEBAND_MAX_DECIMATION 64
#define SDRG_SIDEBAND_MAX_IN 1048576
typedef struct sdrg_sideband_config {
    double channel_rate_hz;
    double low_hz;
    double high_hz;
    int32_t mode;
    int32_t audio_decimation;
    int32_t taps;
    int32_t out_format;
    int32_t max_in;
    float gain;
} sdrg_sideband_config;

/* Host-only, no device.  After the checks of set_sideband: cr[cfg->taps] and ci[cfg->taps] of the design above; either
 * pointer may be NULL. */
int32_t sdrg_sideband_design(const sdrg_sideband_config *cfg, float *cr, float *ci);
/* Host-only: *tile, how many consecutive outputs one workgroup computes for (R, T) (an output index that is a multiple
 * of it starts a new tile): for tests that want data across every seam. */
int32_t sdrg_sideband_geometry(int32_t audio_decimation, int32_t taps, int32_t *tile);

/* Set (cfg != NULL) or switch off (cfg == NULL) the sideband stage.  A sideband call while it is off returns
 * SDRG_E_INVALID and writes nothing. */
int32_t sdrg_engine_set_sideband(sdrg_engine *eng, const sdrg_sideband_config *cfg);
/* The configuration in force (SDRG_E_INVALID when off), its design (cr, ci: taps floats each) and g, the samples every
 * stream has consumed since the last restart; any pointer may be NULL. */
int32_t sdrg_engine_get_sideband(const sdrg_engine *eng, sdrg_sideband_config *cfg, float *cr, float *ci,
                                 uint64_t *samples_consumed);
int32_t sdrg_engine_sideband_reset(sdrg_engine *eng);
/* cap = ceil(max_in / R): the row length of `out`, in outputs (int16 or float by out_format, pairs of them at BOTH). */
int32_t sdrg_engine_sideband_max_out(const sdrg_engine *eng, int32_t *cap);
/* chan [n_streams][max_in][2] float, of which the first n complex samples of every row are this call's (0 <= n <=
 * max_in), and out [n_streams][cap] ([n_streams][cap][2] at BOTH) in device memory.  Reads chan only.  Stream rules and
 * waiting as sdrg_engine_demod_device: runs on the main stream (the caller's after sdrg_engine_set_stream); complete
 * after sdrg_engine_synchronize, or on a stream after sdrg_engine_wait_outputs. */
int32_t sdrg_engine_sideband_device(sdrg_engine *eng, const void *chan, int32_t n, void *out, int32_t *n_out);
/* Host buffers of the same shapes, synchronous. */
int32_t sdrg_engine_sideband_host(sdrg_engine *eng, const void *chan, int32_t n, void *out, int32_t *n_out);
/* Tune and listen to a sideband: sdrg_engine_listen_host with the sideband stage in the demodulator's place, iq through
 * DDC -> [squelch] -> [AGC] -> sideband -> [resampler], the same mask bits, records and buffers kept on the device;
 * the demodulator takes no part, whether or not one is set.  SDRG_E_INVALID, in this order: a null engine, iq, out or
 * n_out; a mask with other bits; the sideband stage off; the resampler, the squelch, the AGC off while in the mask; the
 * DDC's own refusals; the sideband stage's max_in, then the squelch's, then the AGC's smaller than the DDC's cap; with
 * the resampler, a sideband stage that does not write SDRG_SIDEBAND_OUT_F32, a resampler whose components are not 1 for
 * UPPER and LOWER and 2 for BOTH (the interleaved pair is filtered per component by the same real taps), or one with a
 * max_in smaller than the sideband stage's cap.  A refused call commits nothing in any stage. */
int32_t sdrg_engine_listen_sideband_host(sdrg_engine *eng, int32_t steps, const void *iq, int32_t fmt, void *out,
                                         int32_t *n_out, sdrg_squelch_record *squelch_records,
                                         sdrg_agc_record *agc_records);

/* ------------------------------------------------------------------------------------------------
 * BUILD EXTENSION, not a reference interface: the IQ correction stage, the DC offset and the gain / phase imbalance of a
 * receiver's quadrature mixer estimated and removed per stream, ahead of every other stage.  Per stream, the n raw
 * samples of a call, in any of the four formats (the format may change from call to call), are cut into blocks of S
 * samples at the global indices that are multiples of S.  Each completed block's moments move a DC estimate (dr, di)
 * and a balance estimate (wr, wi); block k is corrected under a ramp from the parameters after block k - 2 to those after
 * block k - 1, so there is no step at a block seam and no decision reaches back into the block that produced it: the
 * stage adds no delay and out has one CF32 sample per input sample.  Over the whole life of a stream (the calls'
 * samples concatenated, whatever their lengths) the result is that of one call.  All arithmetic is float, every
 * product, sum and quotient rounded on its own, unless "double" is stated; denormals are kept.  A non-finite sample
 * makes that stream's outputs and records unspecified from then on.  The balance rule is the blind estimate for
 * x = K1 z + K2 conj(z) with circular z: E[x^2] / E|x|^2 = 2 w / (1 + |w|^2) with w = K2 / conj(K1), and
 * y = x - w conj(x) cancels the image.  The balance is one complex number per stream: it does not depend on frequency.
 *   config     dc_tau_blocks, balance_tau_blocks finite, >= 0; floor_db finite; mode SDRG_IQCORR_DC, SDRG_IQCORR_BALANCE
 *              or both (0 and other bits are refused); block S a power of two in [SDRG_IQCORR_MIN_BLOCK,
 *              SDRG_IQCORR_MAX_BLOCK]; max_in in [1, 2^20]: every call's n <= in_stride <= max_in.  A rejected
 *              set_iqcorr changes nothing; an accepted one, and sdrg_engine_iqcorr_reset, restart every stream: g = 0
 *              and the state dr, di, wr, wi, A, B, P, seeded all zero.
 *   design     sdrg_iqcorr_design, in double, each result rounded to float once: beta_x = 1 - exp(-1 / tau_x), and
 *              exactly 1.0f at tau_x = 0; floor_thr = 10^(floor_db / 10), refused unless it is a finite positive float.
 *   sample     z = (zr, zi) is the format's scaled value, as the DDC reads it: CS8 v / 128, CU8 (v - 127.4f) * (1 /
 *              128), CS16 v / 32768, CF32 as it lies.
 *   moments    T(.) is the adjacent-pair tree over a block's S values in order: q'[i] = q[2 i] + q[2 i + 1] until one
 *              value is left; r = 1 / S.  Per sample q1 = zr zr, q2 = zi zi, e = q1 - q2, s = q1 + q2, c = zr zi.  Per
 *              block mr = T(zr) r, mi = T(zi) r, E = T(e) r, W = T(s) r, C = T(c) r, and, centred on the block's own
 *              mean, a = E - (mr mr - mi mi), b = C - mr mi, p = W - (mr mr + mi mi).  A block's moments depend on its
 *              own samples only.
 *   step       for each completed block, in order.  With SDRG_IQCORR_DC: dr = dr + beta_dc (mr - dr), or dr = mr when
 *              beta_dc is 1; the same for di with mi.  With SDRG_IQCORR_BALANCE: if p < floor_thr the block is held
 *              (nothing of the balance moves, held counts one); otherwise, if not yet seeded, (A, B, P) = (a, b, p) and
 *              seeded = 1, else A = A + beta_bal (a - A) and the same for B with b and P with p (also at beta_bal = 1);
 *              then cr = A / P, ci = (2 B) / P, m = cr cr + ci ci; if m <= 0.25f, d = 1 + sqrtf(1 - m), wr = cr / d,
 *              wi = ci / d; if m > 0.25f the block is held: wr and wi stay where they are and held counts one.
 *              theta_k = (dr, di, wr, wi) after global block k; theta_-1 = theta_-2 = 0.
 *   output     the sample at in-block index i of global block k: t = (float)(i + 1) * r; each of the four parameters is
 *              theta_(k-2) + (theta_(k-1) - theta_(k-2)) * t; ur = zr - dr, ui = zi - di; yr = ur - (wr ur + wi ui),
 *              yi = ui - (wi ur - wr ui).  With DC only the w terms are still evaluated, with w = +0; with BALANCE only
 *              dr = di = +0.  out [n_streams][in_stride][2] float, 8-byte aligned: every byte is written by every
 *              call, zero from n on.  out may be iq itself only when fmt is CF32; any other overlap is undefined.  n = 0
 *              is a valid call: it writes out and the records and leaves the state where it is.
 *   records    sdrg_iqcorr_record [n_streams], written by every call: dc_re, dc_im, w_re, w_im are theta after the last
 *              block completed so far; power is P; image_db = 10.0f * log10f(wr wr + wi wi + 1e-20f) with glibc's
 *              log10f bit for bit (the squelch's); held_blocks is how many of the blocks this call completed were held;
 *              seeded is the state's flag.  *n_blocks = floor((g + n) / S) - floor(g / S) is set on the host before the
 *              call returns.
 *   state      per stream the scaled samples of the block in progress (S - 1 pairs of floats), the two last theta, A,
 *              B, P and seeded, in device memory (allocated at the first iqcorr call), in two halves a call reads and
 *              writes in turn; per engine g, advanced by n once the call's launches have been issued: a failed call
 *              commits nothing.  Calls shorter than a block accumulate; any number of calls may share one block.
 * ---------------------------------------------------------------------------------------------- */
#define SDRG_IQCORR_DC 1
#define SDRG_IQCORR_BALANCE 2
#define SDRG_IQCORR_MIN_BLOCK 64
#define SDRG_IQCORR_MAX_BLOCK 1024
#define SDRG_IQCORR_MAX_IN 1048576
typedef struct sdrg_iqcorr_config {
    double dc_tau_blocks;
    double balance_tau_blocks;
    double floor_db;       /* blocks whose centred power is under 10^(floor_db / 10) do not move the balance */
    int32_t mode;
    int32_t block;
    int32_t max_in;
} sdrg_iqcorr_config;

typedef struct sdrg_iqcorr_record {
    float dc_re, dc_im, w_re, w_im;
    float power;
    float image_db;
    int32_t held_blocks;
    int32_t seeded;
} sdrg_iqcorr_record;

/* Host-only, no device.  After the checks of set_iqcorr: the three design values above; any of the three pointers may
 * be NULL. */
int32_t sdrg_iqcorr_design(const sdrg_iqcorr_config *cfg, float *beta_dc, float *beta_bal, float *floor_thr);
/* Host-only: *tile = max(512, block), how many consecutive samples one workgroup takes: of the moments kernel those of
 * the global indices [k tile, (k + 1) tile), of the pass kernel those of the call's indices [k tile, (k + 1) tile). */
int32_t sdrg_iqcorr_geometry(int32_t block, int32_t *tile);

/* Set (cfg != NULL) or switch off (cfg == NULL) the stage.  An iqcorr call while it is off returns SDRG_E_INVALID and
 * writes nothing. */
int32_t sdrg_engine_set_iqcorr(sdrg_engine *eng, const sdrg_iqcorr_config *cfg);
/* The configuration in force (SDRG_E_INVALID when off), its three design values and g, the samples every stream has
 * consumed since the last restart; any pointer may be NULL. */
int32_t sdrg_engine_get_iqcorr(const sdrg_engine *eng, sdrg_iqcorr_config *cfg, float *beta_dc, float *beta_bal,
                               float *floor_thr, uint64_t *samples_consumed);
int32_t sdrg_engine_iqcorr_reset(sdrg_engine *eng);
/* iq: n_streams rows of in_stride raw samples in fmt, aligned as the format's components, of which the first n of every
 * row are this call's (0 <= n <= in_stride <= max_in); out [n_streams][in_stride][2] float; records [n_streams] or
 * NULL; all in device memory.  Stream rules and waiting as sdrg_engine_squelch_device.  To correct ahead of the DDC or
 * the channelizer, pass out to their _device calls as SDRG_IQ_CF32. */
int32_t sdrg_engine_iqcorr_device(sdrg_engine *eng, const void *iq, int32_t fmt, int32_t in_stride, int32_t n, void *out,
                                  sdrg_iqcorr_record *records, int32_t *n_blocks);
/* Host buffers of the same shapes, synchronous; all n_streams * in_stride samples of iq are copied. */
int32_t sdrg_engine_iqcorr_host(sdrg_engine *eng, const void *iq, int32_t fmt, int32_t in_stride, int32_t n, void *out,
                                sdrg_iqcorr_record *records, int32_t *n_blocks);
/* Correct, then look and listen: one frame per stream (n = in_stride = samples_per_reading) is corrected into a device
 * buffer the engine owns, sdrg_engine_process_host's stages run on those rows as SDRG_IQ_CF32, and what process_host
 * copies back comes back, plus iq_records [n_streams] unless NULL.  SDRG_E_INVALID, with no stage moved, if the stage
 * is off or its max_in is smaller than the frame, and under sdrg_engine_process_host's own conditions.
 * sdrg_engine_process_host itself never corrects, whether or not the stage is set. */
int32_t sdrg_engine_iqcorr_process_host(sdrg_engine *eng, const void *iq, int32_t fmt, int32_t stages, float *spectra,
                                        sdrg_frame_record *records, int16_t *pcm, int64_t now_ms,
                                        sdrg_iqcorr_record *iq_records);

/* ------------------------------------------------------------------------------------------------
 * BUILD EXTENSION, not a reference interface: the noise blanker stage, impulse noise (ignition, switching supplies,
 * radar sidelobes: pulses of a few samples far over everything else) zeroed per stream in the wideband samples, ahead of
 * the first filter.  Per stream, the n raw samples of a call, in any of the four formats (the format may change from call
 * to call), are cut into blocks of S samples at the global indices that are multiples of S.  Each completed block gives
 * a floor F, the least of its sub-blocks' mean powers, which a pulse leaves alone; the floors move a level L, and a
 * sample whose power is over ratio times the level of the block before its own is a hit.  A hit blanks itself, the lead
 * samples before it and the tail samples after it, so the stage delays the stream by exactly lead samples; out has one
 * CF32 sample per input sample.  Over the whole life of a stream (the calls' samples concatenated, whatever their
 * lengths) the result is that of one call.  All arithmetic is float, every product and sum rounded on its own, unless
 * "double" is stated; denormals are kept.  A non-finite sample makes that stream's outputs and records unspecified from
 * then on.
 *   config     tau_blocks finite, >= 0; threshold_db and floor_db finite; block S a power of two in
 *              [SDRG_BLANKER_MIN_BLOCK, SDRG_BLANKER_MAX_BLOCK]; lead in [0, SDRG_BLANKER_MAX_LEAD]; tail in [0,
 *              SDRG_BLANKER_MAX_TAIL]; max_in in [1, 2^20]: every call's n <= in_stride <= max_in.  Each bad field is
 *              refused on its own.  A rejected set_blanker changes nothing; an accepted one, and
 *              sdrg_engine_blanker_reset, restart every stream: g = 0, unseeded.
 *   design     sdrg_blanker_design, in double, each result rounded to float once: beta = 1 - exp(-1 / tau_blocks), and
 *              exactly 1.0f at tau_blocks = 0; ratio = 10^(threshold_db / 10); floor_thr = 10^(floor_db / 10); the last
 *              two are refused unless they are finite positive floats.  Advice: L sits under the mean power even on
 *              noise alone (by 1.2 dB at S = 64, 2.9 dB at S = 1024: DESIGN.md §3.20), so threshold_db counts from the
 *              floor, not from the mean; on Gaussian noise alone 13 dB gives under one false hit in 10^4 samples at
 *              every S, and 16 dB gave none in 2 * 10^6.
 *   sample     z = (zr, zi) is the format's scaled value, as the IQ correction reads it: CS8 v / 128, CU8 (v - 127.4f)
 *              * (1 / 128), CS16 v / 32768, CF32 as it lies.  q = zr zr + zi zi: two products and one sum.
 *   floor      a block is cut into S / 16 sub-blocks of 16 samples; f_j is the adjacent-pair tree over sub-block j's 16
 *              powers in order (q'[i] = q[2 i] + q[2 i + 1] until one value is left); F = min_j(f_j) * 0.0625f.  A
 *              block's F depends on its own samples only.
 *   step       for each completed block, in order: if the stream is not seeded, L = F and seeded = 1; otherwise L = L +
 *              beta (F - L), also at beta = 1.  thr_k = fmaxf(L, floor_thr) * ratio after global block k; thr_-1 = +inf:
 *              nothing is blanked before the first block completes.
 *   hit        the input at global index v, in block k, is a hit iff q[v] > thr_(k-1): the decision never reaches into
 *              the block that produced it.
 *   output     the output at global index j carries the input i = j - lead.  If i < 0 it is (+0, +0); if any v in
 *              [max(i - tail, 0), i + lead] is a hit it is (+0, +0); otherwise it is z[i] as scaled.  Every index an
 *              output needs is <= j.  out [n_streams][in_stride][2] float, 8-byte aligned: every byte is written by
 *              every call, zero from n on.  out must not overlap iq in any format: a workgroup reads raw samples that
 *              lie where another's outputs go; an overlap is not detected and its result is undefined.  n = 0 is a
 *              valid call: it writes out and the records and leaves the state where it is.
 *   records    sdrg_blanker_record [n_streams], written by every call: level is L after the last block completed so
 *              far; level_db = 10.0f * log10f(L + 1e-20f) with glibc's log10f bit for bit (the squelch's); hits is how
 *              many of this call's n inputs were hits; blanked is how many of this call's n outputs with i >= 0 the
 *              rule zeroed (it differs from hits by the windows, and by lead at the call's two ends).  *n_blocks =
 *              floor((g + n) / S) - floor(g / S) is set on the host before the call returns.
 *   state      per stream the powers of the block in progress, L, seeded and the threshold in force for the block in
 *              progress, the hit flags of the last lead + tail inputs and the last lead scaled samples, in device
 *              memory (allocated at the first blanker call), in two halves a call reads and writes in turn; per engine
 *              g, advanced by n once the call's launches have been issued: a failed call commits nothing.
 * ---------------------------------------------------------------------------------------------- */
#define SDRG_BLANKER_MIN_BLOCK 64
#define SDRG_BLANKER_MAX_BLOCK 1024
#define SDRG_BLANKER_MAX_LEAD 16
#define SDRG_BLANKER_MAX_TAIL 64
#define SDRG_BLANKER_MAX_IN 1048576
#define SDRG_CLEAN_IQCORR 1 /* sdrg_engine_clean_process_host's mask: the IQ correction ahead of the blanker */
typedef struct sdrg_blanker_config {
    double tau_blocks;
    double threshold_db;   /* a hit is a sample over 10^(threshold_db / 10) times the level */
    double floor_db;       /* the level counts as at least 10^(floor_db / 10) */
    int32_t block;
    int32_t lead;
    int32_t tail;
    int32_t max_in;
} sdrg_blanker_config;

typedef struct sdrg_blanker_record {
    float level;
    float level_db;
    int32_t hits;
    int32_t blanked;
} sdrg_blanker_record;

/* Host-only, no device.  After the checks of set_blanker: the three design values above; any of the three pointers may
 * be NULL. */
int32_t sdrg_blanker_design(const sdrg_blanker_config *cfg, float *beta, float *ratio, float *floor_thr);
/* Host-only: *floor_tile = max(512, block), how many consecutive positions, counted from the start of the block in
 * progress, one workgroup of the floor kernel takes; *pass_tile = 512, how many consecutive outputs of the call one
 * workgroup of the pass kernel writes (it decides the hits of as many inputs, and again those of the lead + tail inputs
 * before them).  Either pointer may be NULL, not both. */
int32_t sdrg_blanker_geometry(int32_t block, int32_t *floor_tile, int32_t *pass_tile);

/* Set (cfg != NULL) or switch off (cfg == NULL) the stage.  A blanker call while it is off returns SDRG_E_INVALID and
 * writes nothing. */
int32_t sdrg_engine_set_blanker(sdrg_engine *eng, const sdrg_blanker_config *cfg);
/* The configuration in force (SDRG_E_INVALID when off), its three design values and g, the samples every stream has
 * consumed since the last restart; any pointer may be NULL. */
int32_t sdrg_engine_get_blanker(const sdrg_engine *eng, sdrg_blanker_config *cfg, float *beta, float *ratio,
                                float *floor_thr, uint64_t *samples_consumed);
int32_t sdrg_engine_blanker_reset(sdrg_engine *eng);
/* iq: n_streams rows of in_stride raw samples in fmt, aligned as the format's components, of which the first n of every
 * row are this call's (0 <= n <= in_stride <= max_in); out [n_streams][in_stride][2] float, not overlapping iq; records
 * [n_streams] or NULL; all in device memory.  Stream rules and waiting as sdrg_engine_squelch_device.  To blank ahead
 * of the DDC or the channelizer, pass out to their _device calls as SDRG_IQ_CF32; to correct first, pass
 * sdrg_engine_iqcorr_device's out here as SDRG_IQ_CF32. */
int32_t sdrg_engine_blanker_device(sdrg_engine *eng, const void *iq, int32_t fmt, int32_t in_stride, int32_t n, void *out,
                                   sdrg_blanker_record *records, int32_t *n_blocks);
/* Host buffers of the same shapes, synchronous; all n_streams * in_stride samples of iq are copied. */
int32_t sdrg_engine_blanker_host(sdrg_engine *eng, const void *iq, int32_t fmt, int32_t in_stride, int32_t n, void *out,
                                 sdrg_blanker_record *records, int32_t *n_blocks);
/* Clean, then look and listen: one frame per stream (n = in_stride = samples_per_reading) goes raw -> [IQ correction,
 * with SDRG_CLEAN_IQCORR in mask] -> blanker into device buffers the engine owns, sdrg_engine_process_host's stages run
 * on the cleaned rows as SDRG_IQ_CF32, and what process_host copies back comes back, plus iq_records [n_streams] (only
 * with SDRG_CLEAN_IQCORR) and blank_records [n_streams], each unless NULL.  The spectra and the audio are of the stream
 * delayed by lead samples.  SDRG_E_INVALID, with no stage moved, for a mask with other bits, if the blanker (or, in the
 * mask, the IQ correction) is off or its max_in is smaller than the frame, and under sdrg_engine_process_host's own
 * conditions; each stage's cursor moves only once everything behind it is enqueued.  sdrg_engine_process_host and
 * sdrg_engine_iqcorr_process_host never blank, whether or not the stage is set. */
int32_t sdrg_engine_clean_process_host(sdrg_engine *eng, const void *iq, int32_t fmt, int32_t mask, int32_t stages,
                                       float *spectra, sdrg_frame_record *records, int16_t *pcm, int64_t now_ms,
                                       sdrg_iqcorr_record *iq_records, sdrg_blanker_record *blank_records);

/* ------------------------------------------------------------------------------------------------
 * BUILD EXTENSION, not a reference interface: the tone detector stage, the power at K configured frequencies per block
 * of a stream and a latched decision that survives a noisy block: the sub-audible tone of an FM channel, a call tone, a
 * keyed carrier, the mark and space of an FSK signal, a pilot.  Per stream, the n values of a call are cut into blocks
 * of S = 64 Q values at the global indices that are multiples of S.  At components = 1 a value is a real float (the
 * audio of the demodulator or of the sideband stage at *_OUT_F32), at components = 2 a CF32 sample (the DDC's channel, a
 * row of the channelizer's).  Over the whole life of a stream (the calls' values concatenated, whatever their lengths)
 * the result is that of one call.  All arithmetic is float, every product, sum and quotient rounded on its own, unless
 * "double" is stated; denormals are kept.  A non-finite value makes that stream's outputs unspecified from then on.
 *   config     rate_hz fa > 0, finite; components 1 or 2; n_tones K in [1, SDRG_TONES_MAX_TONES]; freq_hz (the first K
 *              are used) each finite, 0 < f < fa / 2 at components 1, |f| <= fa / 2 at components 2, equal frequencies
 *              allowed; sub_blocks Q in [1, SDRG_TONES_MAX_SUB_BLOCKS]; window SDRG_TONES_RECT or SDRG_TONES_HANN; min_db
 *              and dominance_db finite, dominance_db >= 0; share in [0, 1]; confirm_blocks in [1, 255]; release_blocks in
 *              [0, 255]; max_in in [1, SDRG_TONES_MAX_IN]: every call's n <= in_stride <= max_in.  Each bad field is
 *              refused on its own.  A rejected set_tones changes nothing; an accepted one, and sdrg_engine_tones_reset,
 *              restart every stream.
 *   design     sdrg_tones_design, in double, each result rounded to float once: w[i] = 1 (RECT) or 0.5 - 0.5 cos(2 pi
 *              (i + 1) / (S + 1)) (HANN) for i in [0, S); t = f_k i / fa, theta = 2 pi (t - floor(t)); c[k][i] = (float)
 *              (w[i] cos theta), s[k][i] = (float)(w[i] sin theta); wf[i] = (float)w[i]; W1 = sum w, W2 = sum w^2; at
 *              components 1 pnorm = (float)(4 / W1^2) and enorm = (float)(2 / W2), at components 2 pnorm = (float)(1 /
 *              W1^2) and enorm = (float)(1 / W2); min_power = (float)10^(min_db / 10), dom = (float)10^(dominance_db /
 *              10), share_thr = (float)share.  A tone of amplitude A at f_k then reads power_k ~ A^2, and its share of
 *              the block's energy ~ 1.
 *   products   at in-block index i.  components 1: C_i = x c, S_i = x s, e_i = (x wf) (x wf).  components 2: C_i = xr c
 *              + xi s and S_i = xi c - xr s, each two products then one sum or difference; a = xr wf, b = xi wf, e_i = a
 *              a + b b.
 *   sums       the 64 products of sub-block j (the indices [64 j, 64 j + 64)) are joined by the adjacent-pair tree
 *              (q'[i] = q[2 i] + q[2 i + 1] until one value is left); a block's accumulators start at +0 and take the
 *              sub-block sums in ascending j, acc = acc + sub_j: 2 K + 1 accumulators, C_k, S_k and E.
 *   block      per completed block: P_k = (C_k C_k + S_k S_k) pnorm; Et = E enorm; k* the smallest k with the largest
 *              P_k; P2 the largest P_k over k != k*, +0 at K = 1; share_b = P_k* / fmaxf(Et, 1e-30f); the candidate is
 *              k* if P_k* >= min_power and P_k* >= share_thr Et and P_k* >= dom P2, else -1.
 *   latch      in this order: if cand >= 0 and cand == last then run = min(run + 1, 65535), otherwise run = (cand >= 0)
 *              ? 1 : 0; last = cand; if cand >= 0 and run >= confirm_blocks then tone = cand, miss = 0; else if tone >=
 *              0: if cand == tone then miss = 0, else miss = miss + 1 and, if miss > release_blocks, tone = -1 and miss
 *              = 0.  A fresh stream has tone = last = -1, run = miss = 0.
 *   outputs    powers [n_streams][cap_blocks][K] float, cap_blocks = ceil(max_in / S) (sdrg_engine_tones_max_blocks):
 *              row b is P_0 .. P_(K-1) of the b-th block this call completed; every byte is written by every call, +0
 *              from n_blocks on.  records [n_streams] (NULL allowed): tone, the latched tone or -1; candidate, that of
 *              the last block completed so far (-1 before the first); power, P_k* of that block (+0 before the first);
 *              power_db = 10.0f * log10f(power + 1e-20f) with glibc's log10f bit for bit; share, share_b of that block
 *              (+0 before the first); tone_blocks, the blocks of this call after which a tone was latched; changes, the
 *              blocks of this call after which tone differs from before them; run.  *n_blocks = floor((g + n) / S) -
 *              floor(g / S) is set on the host.  n = 0 is a valid call: it writes powers and the records and leaves the
 *              state where it is.
 *   state      per stream the at most 63 values of the sub-block in progress, the 2 K + 1 accumulators, the latch's
 *              words and what the record repeats, in device memory, in two halves a call reads and writes in turn; per
 *              engine g, advanced by n once the call's launches have been issued: a failed call commits nothing.
 *   memory     besides the state and the design ((2 K + 1) S floats), a call of n values needs n_streams * ceil(n /
 *              64) * (2 K + 1) floats of device scratch, kept and grown as needed: 43 MB at 4096 streams, n = 1639 and K
 *              = 50, but 2.2 GB at 4096 streams, n = 65536 and K = 64.  A call that cannot have it returns SDRG_E_NOMEM
 *              and commits nothing; a caller short of memory feeds long rows in several calls, whose result is the same.
 * ---------------------------------------------------------------------------------------------- */
#define SDRG_TONES_MAX_TONES 64
#define SDRG_TONES_MAX_SUB_BLOCKS 256
#define SDRG_TONES_MAX_IN 65536
#define SDRG_TONES_RECT 0
#define SDRG_TONES_HANN 1
typedef struct sdrg_tones_config {
    double rate_hz;
    double freq_hz[SDRG_TONES_MAX_TONES];
    double min_db;        /* a candidate's power is at least 10^(min_db / 10) */
    double dominance_db;  /* and at least 10^(dominance_db / 10) times the second largest */
    double share;         /* and at least this share of the block's energy */
    int32_t components;
    int32_t n_tones;
    int32_t sub_blocks;
    int32_t window;
    int32_t confirm_blocks;
    int32_t release_blocks;
    int32_t max_in;
    int32_t reserved;     /* ignored */
} sdrg_tones_config;

typedef struct sdrg_tones_record {
    int32_t tone;
    int32_t candidate;
    float power;
    float power_db;
    float share;
    int32_t tone_blocks;
    int32_t changes;
    int32_t run;
} sdrg_tones_record;

typedef struct sdrg_tones_scalars {
    float pnorm, enorm, min_power, dom, share_thr;
} sdrg_tones_scalars;

/* Host-only, no device.  After the checks of set_tones: table [K][S][2] (c, s), wf [S] and the five scalars; any of the
 * three pointers may be NULL. */
int32_t sdrg_tones_design(const sdrg_tones_config *cfg, float *table, float *wf, sdrg_tones_scalars *scalars);
/* Host-only: *sub_blocks_per_group, how many consecutive sub-blocks of 64 values, counted from the start of the
 * sub-block in progress, one workgroup of the correlate kernel takes. */
int32_t sdrg_tones_geometry(int32_t *sub_blocks_per_group);

/* Set (cfg != NULL) or switch off (cfg == NULL) the stage; an accepted set uploads the design.  A tones call while it
 * is off returns SDRG_E_INVALID and writes nothing. */
int32_t sdrg_engine_set_tones(sdrg_engine *eng, const sdrg_tones_config *cfg);
/* The configuration in force (SDRG_E_INVALID when off), its scalars and g, the values every stream has consumed since
 * the last restart; any pointer may be NULL. */
int32_t sdrg_engine_get_tones(const sdrg_engine *eng, sdrg_tones_config *cfg, sdrg_tones_scalars *scalars,
                              uint64_t *samples_consumed);
int32_t sdrg_engine_tones_reset(sdrg_engine *eng);
/* cap_blocks = ceil(max_in / S): the rows of powers per stream */
int32_t sdrg_engine_tones_max_blocks(const sdrg_engine *eng, int32_t *cap_blocks);
/* in: n_streams rows of in_stride values (floats at components 1, float pairs aligned to 8 bytes at components 2), of
 * which the first n of every row are this call's (0 <= n <= in_stride <= max_in); powers [n_streams][cap_blocks][K]
 * float; records [n_streams] or NULL; all in device memory.  Stream rules and waiting as sdrg_engine_squelch_device. */
int32_t sdrg_engine_tones_device(sdrg_engine *eng, const void *in, int32_t in_stride, int32_t n, void *powers,
                                 sdrg_tones_record *records, int32_t *n_blocks);
/* Host buffers of the same shapes, synchronous; all n_streams * in_stride values of in are copied. */
int32_t sdrg_engine_tones_host(sdrg_engine *eng, const void *in, int32_t in_stride, int32_t n, void *powers,
                               sdrg_tones_record *records, int32_t *n_blocks);
/* sdrg_engine_listen_host with the tone stage reading the demodulator's float rows on the device, ahead of the
 * resampler: besides what listen_host returns, powers [n_streams][cap_blocks][K], tone_records [n_streams] unless NULL
 * and *n_blocks.  SDRG_E_INVALID, with no stage moved, under listen_host's conditions, for a null powers or n_blocks, if
 * the tone stage is off, its components is not 1, the demodulator does not write SDRG_DEMOD_OUT_F32, or the tone
 * stage's max_in is under the demodulator's row length; a call that fails for want of memory commits nothing in any
 * stage either.  The other chain calls never run the tone stage, whether or not it is set. */
int32_t sdrg_engine_listen_tones_host(sdrg_engine *eng, int32_t steps, const void *iq, int32_t fmt, void *out,
                                      int32_t *n_out, sdrg_squelch_record *squelch_records,
                                      sdrg_agc_record *agc_records, float *powers, sdrg_tones_record *tone_records,
                                      int32_t *n_blocks);

/* ------------------------------------------------------------------------------------------------
 * BUILD EXTENSION, not a reference interface: the AFC stage, automatic frequency control: the carrier offset of a CF32
 * channel estimated block by block and removed per stream.  Per stream, the n CF32 channel samples of a call (the DDC's
 * out, a row of the channelizer's, or any rows in device memory) are cut into blocks of S samples at the global indices
 * that are multiples of S, as the squelch's are.  Each completed block's lag-1 product sum (the mean of z[i] conj(z[i -
 * 1]), whose angle is the phase step per sample) moves a smoothed estimate; its coherence against the smoothed power
 * decides whether the stream is locked, and while it is, the estimate sets the frequency of a phase-continuous NCO that
 * mixes the following blocks down.  The estimate comes from the input, not from the corrected output (feed-forward): no
 * decision reaches back into the block that produced it, the stage adds no delay and out has one sample per input
 * sample.  Over the whole life of a stream (the calls' samples concatenated, whatever their lengths) the result is that
 * of one call.  All arithmetic is float, every product, sum, quotient and root rounded on its own, unless "double" is
 * stated; denormals are kept.  A non-finite sample makes that stream's outputs and records unspecified from then on.
 *   config     channel_rate finite, > 0; max_offset_hz in (0, channel_rate / 4]; tau_blocks finite, >= 0; floor_db
 *              finite; lock_threshold in [0, 1]; mode SDRG_AFC_TRACK or SDRG_AFC_MEASURE (anything else is refused);
 *              block S a power of two in [SDRG_AFC_MIN_BLOCK, SDRG_AFC_MAX_BLOCK]; max_in in [1, 2^20]: every call's
 *              n <= in_stride <= max_in.  A rejected set_afc changes nothing; an accepted one, and
 *              sdrg_engine_afc_reset, restart every stream: g = 0, A = B = P = +0, unseeded, unlocked, coh = +0,
 *              inc = 0, Phi = 0.
 *   design     sdrg_afc_design, in double, each result rounded to float once: beta = 1 - exp(-1 / tau_blocks), and
 *              exactly 1.0f at tau_blocks = 0; floor_thr = 10^(floor_db / 10), refused unless it is a finite positive
 *              float; lock_thr = (float)lock_threshold; max_s = (float)(2^32 max_offset_hz / channel_rate), at most
 *              2^30; K = (float)(2^31 / pi); hz_per_inc = (float)(channel_rate / 2^32); rad_per_inc =
 *              (float)(pi / 2^31).
 *   products   for the sample z = (zr, zi) at in-block index i >= 1, with z' = (zr', zi') the sample before it:
 *              pr = zr zr' + zi zi', pi = zi zr' - zr zi' (the demodulator's FM products, in its order); at i = 0,
 *              pr = pi = +0: a block's statistics depend on its own samples only, and a block seam costs one product
 *              in S.  q = zr zr + zi zi.
 *   block      T(.) is the adjacent-pair tree over a block's S values in order (q'[i] = q[2 i] + q[2 i + 1] until one
 *              value is left), r = 1 / S: Rr = T(pr) r, Ri = T(pi) r, W = T(q) r.
 *   step       for each completed block, in order: if W < floor_thr the block is held (nothing moves, held counts one).
 *              Otherwise, if not yet seeded, (A, B, P) = (Rr, Ri, W) and seeded = 1, else A = A + beta (Rr - A) and the
 *              same for B with Ri and P with W (also at beta = 1); then coh = sqrtf(A A + B B) / P and
 *              locked = coh >= lock_thr.  If locked: phi = sdrg_atan2f(B, A) (the demodulator's), s = phi K,
 *              s = fminf(fmaxf(s, -max_s), max_s), inc = (int32_t) rintf(s), ties to even; if not, inc stays where it
 *              is.  inc_k is inc after global block k; inc_-1 = 0.
 *   phase      Phi_0 = 0, Phi_(k+1) = (uint32)(Phi_k + (uint32) inc_(k-1) * S); the sample at in-block index i of global
 *              block k has ph = (uint32)(Phi_k + (uint32) inc_(k-1) * i): the frequency moves at a block seam only, and
 *              the phase never jumps.  Block k is mixed by the estimate after block k - 1.
 *   output     SDRG_AFC_TRACK: H = hi[ph >> 22], L = lo[(ph >> 12) & 1023] of sdrg_nco_tables; wr = H.re L.re -
 *              H.im L.im, wi = H.re L.im + H.im L.re; yr = zr wr - zi wi, yi = zr wi + zi wr (the DDC's mix, in its
 *              order): a positive measured offset is mixed down.  inc = 0 goes through the table too, and hi[0] lo[0]
 *              = 1 leaves the sample's bits but for the sign of a zero.  out [n_streams][in_stride][2] float, 8-byte
 *              aligned: every byte is written by every call, zero from n on.  out may be chan itself; any other overlap
 *              is undefined.  SDRG_AFC_MEASURE: out must be NULL, and nothing is written but the records.  n = 0 is a
 *              valid call: it writes out and the records and leaves the state where it is.
 *   records    sdrg_afc_record [n_streams], written by every call: offset_hz = (float) inc * hz_per_inc and
 *              step = (float) inc * rad_per_inc (radians per sample) of inc after the last block completed so far;
 *              inc itself; coherence is the last computed coh (+0 before the first); level = P; level_db = 10.0f *
 *              log10f(P + 1e-20f) with glibc's log10f bit for bit (the squelch's); held_blocks is how many of the
 *              blocks this call completed were held; flags = locked | seeded << 1.  *n_blocks = floor((g + n) / S) -
 *              floor(g / S) is set on the host before the call returns.
 *   state      per stream the samples of the block in progress (S - 1 pairs of floats), A, B, P, coh, inc, Phi and the
 *              two flags, in device memory (allocated at the first afc call), in two halves a call reads and writes in
 *              turn; per engine g, advanced by n once the call's launches have been issued: a failed call commits
 *              nothing.  Calls shorter than a block accumulate; any number of calls may share one block.
 * ---------------------------------------------------------------------------------------------- */
#define SDRG_AFC_TRACK 1
#define SDRG_AFC_MEASURE 2
#define SDRG_AFC_LOCKED 1 /* sdrg_afc_record.flags */
#define SDRG_AFC_SEEDED 2
#define SDRG_AFC_MIN_BLOCK 16
#define SDRG_AFC_MAX_BLOCK 1024
#define SDRG_AFC_MAX_IN 1048576
typedef struct sdrg_afc_config {
    double channel_rate;   /* Hz: the rate of the channel's samples */
    double max_offset_hz;  /* the estimate is clamped to +- this */
    double tau_blocks;
    double floor_db;       /* blocks whose mean power is under 10^(floor_db / 10) move nothing */
    double lock_threshold; /* the coherence from which the estimate steers the NCO */
    int32_t mode;
    int32_t block;
    int32_t max_in;
} sdrg_afc_config;

typedef struct sdrg_afc_design_values {
    float beta, floor_thr, lock_thr, max_s, K, hz_per_inc, rad_per_inc;
} sdrg_afc_design_values;

typedef struct sdrg_afc_record {
    float offset_hz;
    float step;
    int32_t inc;
    float coherence;
    float level;
    float level_db;
    int32_t held_blocks;
    int32_t flags;
} sdrg_afc_record;

/* Host-only, no device.  After the checks of set_afc: the seven design values above. */
int32_t sdrg_afc_design(const sdrg_afc_config *cfg, sdrg_afc_design_values *design);
/* Host-only: *tile = max(512, block), how many consecutive samples one workgroup takes at a time: of the moments kernel
 * those of the positions [k tile, (k + 1) tile) counted from the start of the block in progress; the pass kernel's
 * workgroup k takes the four tiles of the call's indices [4 k tile, 4 (k + 1) tile) one after the other. */
int32_t sdrg_afc_geometry(int32_t block, int32_t *tile);
/* Host-only: inc * channel_rate / 2^32 in double: a record's inc in Hz without the float's rounding (to feed a DDC's
 * offset_hz, for instance).  NaN for a channel_rate that is not finite and positive. */
double sdrg_afc_offset_hz(int32_t inc, double channel_rate);

/* Set (cfg != NULL) or switch off (cfg == NULL) the stage.  An afc call while it is off returns SDRG_E_INVALID and
 * writes nothing. */
int32_t sdrg_engine_set_afc(sdrg_engine *eng, const sdrg_afc_config *cfg);
/* The configuration in force (SDRG_E_INVALID when off), its design values and g, the samples every stream has consumed
 * since the last restart; any pointer may be NULL. */
int32_t sdrg_engine_get_afc(const sdrg_engine *eng, sdrg_afc_config *cfg, sdrg_afc_design_values *design,
                            uint64_t *samples_consumed);
int32_t sdrg_engine_afc_reset(sdrg_engine *eng);
/* chan and out: n_streams rows of in_stride complex samples ([n_streams][in_stride][2] float), of which the first n of
 * every row are this call's (0 <= n <= in_stride <= max_in); records [n_streams] or NULL; all in device memory.  In
 * SDRG_AFC_TRACK mode out must not be NULL, in SDRG_AFC_MEASURE mode it must be: either is refused with SDRG_E_INVALID.
 * Stream rules and waiting as sdrg_engine_squelch_device. */
int32_t sdrg_engine_afc_device(sdrg_engine *eng, const void *chan, int32_t in_stride, int32_t n, void *out,
                               sdrg_afc_record *records, int32_t *n_blocks);
/* Host buffers of the same shapes, synchronous; all n_streams * in_stride samples of chan are copied. */
int32_t sdrg_engine_afc_host(sdrg_engine *eng, const void *chan, int32_t in_stride, int32_t n, void *out,
                             sdrg_afc_record *records, int32_t *n_blocks);
/* sdrg_engine_listen_host with the AFC first on the channel: iq through DDC -> AFC -> [squelch] -> [AGC] -> demodulator
 * -> [resampler], the same mask bits, records and buffers kept on the device; the AFC runs in place on the channel
 * (in_stride = the DDC's cap, n = the DDC call's n_out) and its records [n_streams] come back unless afc_records is
 * NULL.  SDRG_E_INVALID, with no stage moved, under listen_host's conditions in its order, with the AFC's among them: the
 * AFC off, or in SDRG_AFC_MEASURE mode, after the mask's stages' own; its max_in smaller than the DDC's cap, after the
 * AGC's.  Every buffer is reserved before the first launch: a call that fails for want of memory commits nothing in any
 * stage either.  The other chain calls never run the AFC, whether or not it is set. */
int32_t sdrg_engine_listen_afc_host(sdrg_engine *eng, int32_t steps, const void *iq, int32_t fmt, void *out,
                                    int32_t *n_out, sdrg_squelch_record *squelch_records, sdrg_agc_record *agc_records,
                                    sdrg_afc_record *afc_records);

/* ------------------------------------------------------------------------------------------------
 * BUILD EXTENSION, not a reference interface: the symbol stage: the symbol clock of FM audio recovered block by block
 * and the audio sliced to 2 or 4 levels per stream, one byte (or one float) per symbol.  Per stream, the n real floats
 * of a call (the demodulator's SDRG_DEMOD_OUT_F32 rows, or any rows in device memory) are cut into blocks of S values
 * at the global indices that are multiples of S, as the AFC's are.  A clock that is a function of the global index alone
 * cuts the stream into cells of 2^32 / inc samples; each completed block's squared differences, correlated with that
 * clock, move a smoothed estimate of where the transmitter's cells meet, and while its coherence says the stream is
 * locked the estimate sets the fraction of the cell at which the following blocks are sampled (feed-forward: no
 * decision reaches back into the block that produced it, and a symbol is written by the call that holds the sample
 * ending its cell).  Over the whole life of a stream (the calls' values concatenated, whatever their lengths) the
 * result is that of one call.  All arithmetic is float, every product, sum, quotient and root rounded on its own,
 * unless "double" or "integer" is stated; denormals are kept.  A non-finite value makes that stream's outputs and
 * records unspecified from then on.
 *   input      [n_streams][in_stride] float, 4-byte aligned, 0 <= n <= in_stride <= max_in.  g is the number of values
 *              every stream has consumed; x[i] is the value at global index i, and x[i] = +0 for i < 0.
 *   config     sample_rate and symbol_rate finite, > 0, sample_rate / symbol_rate in [2, 64]; levels 2 or 4; block S a
 *              power of two in [SDRG_SYM_MIN_BLOCK, SDRG_SYM_MAX_BLOCK]; tau_blocks and tau_level_blocks finite, >= 0;
 *              floor_db finite; lock_threshold in [0, 1]; phase_trim in [-0.5, 0.5]; level_mode SDRG_SYM_LEVEL_TRACK or
 *              SDRG_SYM_LEVEL_FIXED; level_scale finite, > 0; fixed_centre finite; fixed_threshold finite, > 0 (the
 *              last three are checked in either level_mode); format SDRG_SYM_HARD or SDRG_SYM_SOFT; max_in in
 *              [1, 2^20].  Each is refused on its own.  A rejected set_symbols changes nothing; an accepted one, and
 *              sdrg_engine_symbols_reset, restart every stream: g = 0, A = B = U = M = Q = +0, coh = +0, unseeded,
 *              unlocked, slips = 0, tau = (uint32)(2^31 + trim), and centre = +0, thr = 1 (SDRG_SYM_LEVEL_TRACK) or the
 *              two configured floats (SDRG_SYM_LEVEL_FIXED).
 *   design     sdrg_symbols_design, in double, each result rounded once: inc = rint(2^32 symbol_rate / sample_rate) as
 *              uint32, refused outside [2^26, 2^31]; rinc = (float)(1.0 / inc); beta = 1 - exp(-1 / tau_blocks) and
 *              beta_level the same of tau_level_blocks, each exactly 1.0f at 0; floor_thr = 10^(floor_db / 10), refused
 *              unless it is a finite positive float; lock_thr = (float)lock_threshold; K = (float)(2^31 / pi); trim =
 *              (int64) rint(phase_trim 2^32); rs = (float)(1.0 / S); scale, centre and threshold, the floats of level_scale,
 *              fixed_centre and fixed_threshold; and the table tab[k] = ((float)cos, (float)sin)(2 pi (k + 0.5) / 1024), k in [0, 1024).
 *   clock      c_i = (uint32)(inc i): integer, wrapping, a function of the global index only.  Sample i >= 1 *emits*
 *              when c_i < inc: the clock wrapped between i - 1 and i, so the cells' edges never depend on the data.
 *              The emitting samples in [0, g) number K(g) = floor(inc (g - 1) / 2^32) for g >= 1, K(0) = 0; a call
 *              writes n_sym = K(g + n) - K(g) symbols (sdrg_symbols_count, in 128-bit integers), and rows of cap =
 *              floor(inc max_in / 2^32) + 1 symbols (sdrg_engine_symbols_max_out) hold any call's.
 *   products   at in-block index j >= 1: dx = x[i] - x[i - 1], u = dx dx, (tc, ts) = tab[c_i >> 22], a = u tc,
 *              b = u ts; at j = 0, u = a = b = +0: a block's statistics depend on its own values only, and a block
 *              seam costs one product in S.  q = x x at every j.
 *   block      T(.) is the adjacent-pair tree over a block's S values in order (v'[i] = v[2 i] + v[2 i + 1] until one
 *              value is left), rs = 1 / S: Ab = T(a) rs, Bb = T(b) rs, Ub = T(u) rs, Mb = T(x) rs, Qb = T(q) rs.
 *   step       for each completed block, in order: if Qb < floor_thr the block is held (nothing moves, the levels
 *              included; held counts one): a closed squelch's zeros.  Otherwise, if not yet seeded, (A, B, U, M, Q) =
 *              (Ab, Bb, Ub, Mb, Qb) and seeded = 1, else A = A + beta (Ab - A) and the same for B and U, and M = M +
 *              beta_level (Mb - M) and the same for Q (also at beta = 1); then coh = sqrtf(A A + B B) / U, +0 when U
 *              is 0, and locked = coh >= lock_thr.  If locked: ang = (int64) rintf(sdrg_atan2f(B, A) K), tau' =
 *              (uint32)(ang - (inc >> 1) + 2^31 + trim) in 64-bit integers, wrapped; with d = (int32)(tau' - tau), one
 *              slip is counted when d >= 0 && tau' < tau or d < 0 && tau' > tau (the sampling point went round the
 *              cell's edge: one symbol is sampled twice or not at all); tau = tau'.  If not, tau stays.  Then the
 *              levels: SDRG_SYM_LEVEL_TRACK: centre = M, w = Q - M M, thr = level_scale sqrtf(fmaxf(w, +0));
 *              SDRG_SYM_LEVEL_FIXED: the two configured floats, always.  Block k is sampled with (tau, centre, thr,
 *              locked) after block k - 1.  (u is largest where the cells meet, and sits half a sample before i:
 *              - inc / 2; the sampling point is half a cell after the edge: + 2^31; u does not see a DC offset.)
 *   symbol     for an emitting sample i of global block k: num = (uint64) c_i + (2^32 - tau), qd = num / inc, r = num
 *              - qd inc, in integers (qd <= 65); nu = (float) r rinc; x0 = x[i - qd], x1 = x[i - qd - 1]; y = x0 - nu
 *              (x0 - x1); v = y - centre: the cell that ended at i, sampled linearly at the fraction tau / 2^32 of its
 *              length from the 66 values before i and none after.  SDRG_SYM_HARD, levels 2: s = v >= 0; levels 4: s =
 *              v < -thr ? 0 : v < 0 ? 1 : v < thr ? 2 : 3; the byte is s | (locked ? 0 : SDRG_SYM_UNLOCKED).
 *              SDRG_SYM_SOFT: the float thr > 0 ? v / thr : +0.  Its place in the call's row is K(i) - K(g).
 *   output     symbols [n_streams][cap], uint8 (SDRG_SYM_HARD) or float (SDRG_SYM_SOFT, 4-byte aligned): every byte is
 *              written by every call, zero from n_sym on.  *n_sym is set on the host before the call returns.  n = 0 is
 *              a valid call: it writes symbols and the records and leaves the state where it is.
 *   records    sdrg_symbols_record [n_streams] (32 bytes each) or NULL, written by every call: tau_frac = (float) tau
 *              2^-32, tau, coherence the last computed coh (+0 before the first), centre, threshold, slips since the
 *              last restart, held_blocks of the blocks this call completed, flags = locked | seeded << 1.
 *   state      per stream the 66 values before the block in progress and that block's values so far, and the step's
 *              words, in device memory (allocated at the first call), in two halves a call reads and writes in turn;
 *              per engine g, advanced by n once the call's launches have been issued: a failed call commits nothing.
 * ---------------------------------------------------------------------------------------------- */
#define SDRG_SYM_LEVEL_TRACK 1
#define SDRG_SYM_LEVEL_FIXED 2
#define SDRG_SYM_HARD 1
#define SDRG_SYM_SOFT 2
#define SDRG_SYM_LOCKED 1 /* sdrg_symbols_record.flags */
#define SDRG_SYM_SEEDED 2
#define SDRG_SYM_UNLOCKED 0x80 /* a SDRG_SYM_HARD byte sampled while unlocked */
#define SDRG_SYM_MIN_BLOCK 64
#define SDRG_SYM_MAX_BLOCK 1024
#define SDRG_SYM_MAX_IN 1048576
#define SDRG_SYM_HISTORY 66
#define SDRG_SYM_TABLE 1024
typedef struct sdrg_symbols_config {
    double sample_rate;      /* Hz: the rate of the input's values */
    double symbol_rate;      /* symbols per second */
    double tau_blocks;       /* the time constant of A, B and U */
    double tau_level_blocks; /* of M and Q */
    double floor_db;         /* blocks whose mean square is under 10^(floor_db / 10) move nothing */
    double lock_threshold;
    double phase_trim;       /* cells: added to the sampling point */
    double level_scale;      /* SDRG_SYM_LEVEL_TRACK: thr = level_scale * the standard deviation */
    double fixed_centre;     /* SDRG_SYM_LEVEL_FIXED */
    double fixed_threshold;
    int32_t levels;
    int32_t block;
    int32_t level_mode;
    int32_t format;
    int32_t max_in;
} sdrg_symbols_config;

typedef struct sdrg_symbols_design_values {
    int64_t trim;
    uint32_t inc;
    float rinc, beta, beta_level, floor_thr, lock_thr, K, rs, scale, centre, threshold;
} sdrg_symbols_design_values;

typedef struct sdrg_symbols_record {
    float tau_frac;
    uint32_t tau;
    float coherence;
    float centre;
    float threshold;
    int32_t slips;
    int32_t held_blocks;
    int32_t flags;
} sdrg_symbols_record;

/* Host-only, no device.  After the checks of set_symbols: the design values above and, unless table is NULL, the
 * SDRG_SYM_TABLE pairs (cos, sin). */
int32_t sdrg_symbols_design(const sdrg_symbols_config *cfg, sdrg_symbols_design_values *design, float *table);
/* Host-only: *tile = max(512, block), the consecutive values one workgroup of the moments kernel takes, by position
 * counted from the start of the block in progress; *pass_tile, the consecutive symbols of a row one workgroup of the
 * pass kernel writes.  Either pointer may be NULL. */
int32_t sdrg_symbols_geometry(int32_t block, int32_t *tile, int32_t *pass_tile);
/* Host-only: K(g + n) - K(g), the symbols a call of n values writes at stream position g, in 128-bit integers; -1 for
 * an inc outside [2^26, 2^31]. */
int64_t sdrg_symbols_count(uint32_t inc, uint64_t g, uint64_t n);

/* Set (cfg != NULL) or switch off (cfg == NULL) the stage; the table is uploaded before the configuration is committed.
 * A symbols call while it is off returns SDRG_E_INVALID and writes nothing. */
int32_t sdrg_engine_set_symbols(sdrg_engine *eng, const sdrg_symbols_config *cfg);
/* The configuration in force (SDRG_E_INVALID when off), its design values and g; any pointer may be NULL. */
int32_t sdrg_engine_get_symbols(const sdrg_engine *eng, sdrg_symbols_config *cfg, sdrg_symbols_design_values *design,
                                uint64_t *samples_consumed);
int32_t sdrg_engine_symbols_reset(sdrg_engine *eng);
/* *cap = floor(inc max_in / 2^32) + 1: the symbols per row of `symbols`. */
int32_t sdrg_engine_symbols_max_out(const sdrg_engine *eng, int32_t *cap);
/* in: n_streams rows of in_stride floats, of which the first n of every row are this call's; symbols [n_streams][cap]
 * uint8 or float by format; records [n_streams] or NULL; all in device memory.  Stream rules and waiting as
 * sdrg_engine_squelch_device. */
int32_t sdrg_engine_symbols_device(sdrg_engine *eng, const void *in, int32_t in_stride, int32_t n, void *symbols,
                                   sdrg_symbols_record *records, int32_t *n_sym);
/* Host buffers of the same shapes, synchronous; all n_streams * in_stride values of in are copied. */
int32_t sdrg_engine_symbols_host(sdrg_engine *eng, const void *in, int32_t in_stride, int32_t n, void *symbols,
                                 sdrg_symbols_record *records, int32_t *n_sym);
/* sdrg_engine_listen_host with the symbol stage reading the demodulator's float audio where it lies on the device,
 * ahead of the resampler (in_stride = the demodulator's cap, n = its call's n_out): symbols [n_streams][cap] and, unless
 * symbol_records is NULL, the records [n_streams] come back in addition, and *n_sym.  out may be NULL: the audio then
 * stays on the device (n_out is still set).  SDRG_E_INVALID, with no stage moved, under listen_host's conditions in its
 * order, then: the symbol stage off; the demodulator not writing SDRG_DEMOD_OUT_F32; the stage's max_in under the
 * demodulator's row length.  Every buffer is reserved before the first launch: a call that fails for want of memory
 * commits nothing in any stage either.  The other chain calls never run the symbol stage, whether or not it is set. */
int32_t sdrg_engine_listen_symbols_host(sdrg_engine *eng, int32_t steps, const void *iq, int32_t fmt, void *out,
                                        int32_t *n_out, sdrg_squelch_record *squelch_records,
                                        sdrg_agc_record *agc_records, void *symbols,
                                        sdrg_symbols_record *symbol_records, int32_t *n_sym);

/* JNI read(): register the callback table (copied). NULL clears it. */
int32_t sdrg_engine_set_callbacks(sdrg_engine *eng, const sdrg_callbacks *cbs);

/* Profiling: when enabled, every process call records hipEvents around each kernel group (a ring of
 * event sets, so back-to-back calls are timed without host synchronisation). */
int32_t sdrg_engine_set_profiling(sdrg_engine *eng, int32_t enabled);
/* Timings of the most recent profiled call (waits for it to finish). */
int32_t sdrg_engine_get_timings(const sdrg_engine *eng, sdrg_timings *out);
/* Mean timings over every profiled call since the last reset (waits for them); *count = calls averaged. */
int32_t sdrg_engine_get_timing_stats(const sdrg_engine *eng, sdrg_timings *mean, int32_t *count);
int32_t sdrg_engine_reset_timing_stats(sdrg_engine *eng);

/* ------------------------------------------------------------------------------------------------
 * Multi-GPU: one process per GPU (rank), each with its own engine for its block of streams (rank r owns the
 * global streams [r*B, (r+1)*B): frames and per-stream state are independent, so nothing else is exchanged), and
 * the per-frame results gathered to a root rank with RCCL (ncclGather over xGMI).  The reference is one receiver
 * in one process; what is gathered is what its soapyCallback hands to Kotlin per frame
 * (sdr-bridge-java-soapy.cpp:456-466: the fftCallback spectrum, the getters' values with the peak) and the SSB
 * worker's PCM (ssb_processor.cpp:103-108).  RCCL is loaded at run time (librccl.so.1) by the first call below;
 * without it they return SDRG_E_UNSUPPORTED and nothing else is affected.
 * ---------------------------------------------------------------------------------------------- */
#define SDRG_DIST_ID_BYTES 128
typedef struct sdrg_dist sdrg_dist;
/* ncclGetUniqueId, on one rank: the caller hands these bytes to every rank (a file, a socket, MPI, ...). */
int32_t sdrg_dist_unique_id(void *id, int32_t bytes);
/* ncclCommInitRank on `device` (collective: every rank of the job calls it with the same id). */
int32_t sdrg_dist_create(const void *id, int32_t world_size, int32_t rank, int32_t device, sdrg_dist **out);
int32_t sdrg_dist_destroy(sdrg_dist *d);
/* Rank, world size, the RCCL version in use and whether the gathers move their bytes through RCCL (1) or, for a
 * one-rank communicator, as hipMemcpyAsync device copies (0).  Any pointer may be NULL. */
int32_t sdrg_dist_info(const sdrg_dist *d, int32_t *rank, int32_t *world_size, int32_t *rccl_version,
                       int32_t *rccl_data);
/* A one-rank communicator's gathers are device copies by default (RCCL's one-rank gather kernel runs beside the SSB
 * pipeline and slows the step: DESIGN.md §7); on = 1 routes them through ncclGather as at world size > 1. */
int32_t sdrg_dist_set_one_rank_rccl(sdrg_dist *d, int32_t on);

/* What one gather moves.  Each selected pair gathers this rank's n_streams rows to the root's output, which
 * holds world_size x n_streams rows in rank order (= global stream order); the *_out pointers are read on the
 * root only (NULL elsewhere).  A NULL source skips the pair; every rank selects the same pairs.  All device memory
 * of the engine's device.
 *   records       [n_streams] sdrg_frame_record  -> records_out [world][n_streams]
 *   focus_spectra [n_streams][N] (a call's spectra) -> focus_out [world][n_streams][n_bins]: each frame's focus
 *                 window (sdrg_focus_window of the statistics' configuration), packed on the device first
 *   spectra       [n_streams][N]                 -> spectra_out [world][n_streams][N]: the whole fftshifted spectra
 *                 (268 MB per rank at 4096 x 16384)
 *   pcm           [n_streams][pcm_len] int16     -> pcm_out [world][n_streams][pcm_len] */
typedef struct sdrg_gather_buffers {
    const sdrg_frame_record *records;
    sdrg_frame_record *records_out;
    const float *focus_spectra;  /* the focus-window slices of these spectra */
    float *focus_out;
    const float *spectra;        /* the whole spectra */
    float *spectra_out;
    const int16_t *pcm;
    int16_t *pcm_out;
} sdrg_gather_buffers;
/* Enqueue the gathers (one RCCL group) behind the last process call's outputs they read, on the engine stream that
 * produced them: the statistics stream when that call ran its statistics asynchronously (its records, and the spectra
 * those statistics waited for), else the main stream; with PCM, the audio detector's stream (after the SSB stage).
 * No host synchronisation; a later call that writes any byte a gather reads (byte ranges overlap: the same buffer, a
 * slice of it, or an offset into it) waits for that gather on the GPU first, and nothing else waits, so a caller
 * rotating its output buffers overlaps the gathers with its next calls.  Every rank calls it with the same selection
 * (the stream choice above depends on it, and RCCL matches the ranks' gathers in issue order).  At world_size > 1 the
 * path is compiled and checked only on one-rank communicators and on the world-2 CPU rehearsal: no two-GPU run has
 * executed it.  Complete after sdrg_engine_synchronize (or on a stream after
 * sdrg_engine_wait_outputs).  Replaces nothing in the reference (one receiver per process): BASELINE configs[3]. */
int32_t sdrg_engine_gather(sdrg_engine *eng, sdrg_dist *d, int32_t root, const sdrg_gather_buffers *bufs);
/* Single-pair forms of sdrg_engine_gather. */
int32_t sdrg_engine_gather_records(sdrg_engine *eng, sdrg_dist *d, int32_t root, const sdrg_frame_record *records,
                                   sdrg_frame_record *records_out);
int32_t sdrg_engine_gather_focus(sdrg_engine *eng, sdrg_dist *d, int32_t root, const float *spectra, float *focus_out);
int32_t sdrg_engine_gather_spectra(sdrg_engine *eng, sdrg_dist *d, int32_t root, const float *spectra,
                                   float *spectra_out);
int32_t sdrg_engine_gather_pcm(sdrg_engine *eng, sdrg_dist *d, int32_t root, const int16_t *pcm, int16_t *pcm_out);

/* Device memory for a host that has no other GPU allocator (the C/C++ side of the JNI boundary): hipMalloc /
 * hipFree on `device`, and a synchronous copy in any direction (hipMemcpyDefault; it is not ordered with the
 * engine's streams -- call sdrg_engine_synchronize before reading an engine output back). */
int32_t sdrg_device_alloc(int32_t device, size_t bytes, void **out);
int32_t sdrg_device_free(int32_t device, void *p);
int32_t sdrg_memcpy(int32_t device, void *dst, const void *src, size_t bytes);
/* Measurement (bench.py's roofline basis, not part of the reference's surface): the read + write GB/s of a float4
 * streaming copy of `bytes` on `device` (nontemporal loads and stores, 16 workgroups per CU, `reps` timed launches
 * after one untimed), the achievable HBM rate a memory-bound kernel is priced against beside the 8 TB/s spec. */
int32_t sdrg_measure_hbm_copy(int32_t device, size_t bytes, int32_t reps, double *gbs);

#ifdef __cplusplus
}
#endif

#endif /* SDRG_H */
