"""Lab: the host calls of the stages that read caller spectra, and of the streaming stages, timed whole.
python tools/lab/host_stage_time.py [calls] [warmup]  (SDRG_LIB_PATH selects a variant library, SDRG_PKG_PATH the
directory that holds a variant of the sdrg package)

display(spectra), integrate(spectra) and peaks(spectra) at 64 x 16384 from pageable host memory: the wall time of each
of `calls` calls after `warmup`, which is the wrapper's argument handling, the copy of the spectra to the device, the
kernel, the copy of the result back and the wait.  Then the six host calls of the streaming stages at the same shape,
CS8: ddc, demod (400 channel samples per stream), channelizer, resample_host (400 audio samples per stream), ddc_demod
and ddc_demod_resample_host.  One JSON line per kind: the median, the least and the mean, us."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.environ.get("SDRG_PKG_PATH") or
                os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "sdr-for-android-lib_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402, F401  (before libsdrg.so is loaded: DESIGN.md "HIP runtime")
import sdrg  # noqa: E402

CALLS = int(sys.argv[1]) if len(sys.argv) > 1 else 200
WARMUP = int(sys.argv[2]) if len(sys.argv) > 2 else 20
B, N = 64, 16384

eng = sdrg.Engine(sdrg.SDRConfig(centerFrequency=100_000_000, samplesPerReading=N, sampleRate=2_000_000,
                                 freqFocusRangeKhz=5, soundMode=1), B)
eng.set_display(span=sdrg.DISPLAY_SPAN_FULL, width=1024, reduce=sdrg.DISPLAY_MAX, format=sdrg.DISPLAY_U8, db_min=-120.0,
                db_max=0.0)
eng.set_integration(mode=sdrg.INTEGRATE_MEAN, period=8)
eng.set_peaks(span=sdrg.DISPLAY_SPAN_FULL, max_peaks=16, min_separation=8, threshold_db=10.0)
eng.set_ddc(offset_hz=250e3, cutoff_hz=12e3, decimation=41, taps=255)
eng.set_demod(mode=sdrg.DEMOD_FM, channel_rate_hz=2_000_000 / 41, deviation_hz=5000.0, dc_cutoff_hz=20.0,
              deemphasis_us=0.0, audio_decimation=1, audio_taps=31, audio_cutoff_hz=8000.0, gain=1.0,
              out_format=sdrg.DEMOD_OUT_F32, max_in=400)
eng.set_channelizer(cutoff_rel=0.5, channels=64, taps_per_channel=8, oversample=1, first_channel=0, n_channels=64)
eng.set_resample(interp=123, decim=125, taps_per_phase=16, cutoff_rel=0.9, components=1,
                 out_format=sdrg.RESAMPLE_OUT_S16, gain=1.0, max_in=400)
rng = np.random.default_rng(1)
spectra = rng.exponential(1.0, size=(B, N)).astype(np.float32)
iq = rng.integers(-128, 128, size=(B, 2 * N), dtype=np.int8)
chan = (rng.uniform(-0.9, 0.9, size=(B, 800)).astype(np.float32)).view(np.complex64)
audio = rng.uniform(-0.9, 0.9, size=(B, 400)).astype(np.float32)

KINDS = (("display", eng.display, spectra), ("integrate", eng.integrate, spectra), ("peaks", eng.peaks, spectra),
         ("ddc", eng.ddc, iq), ("demod", eng.demod, chan), ("channelizer", eng.channelizer, iq),
         ("resample", eng.resample_host, audio), ("ddc_demod", eng.ddc_demod, iq),
         ("ddc_demod_resample", eng.ddc_demod_resample_host, iq))
for name, call, arg in KINDS:
    for _ in range(WARMUP):
        call(arg)
    us = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        call(arg)
        us.append((time.perf_counter() - t0) * 1e6)
    print(json.dumps(dict(kind=name + "_host", streams=B, n=N, calls=CALLS, warmup=WARMUP,
                          median_us=round(statistics.median(us), 1), min_us=round(min(us), 1),
                          mean_us=round(statistics.fmean(us), 1), library=os.environ.get("SDRG_LIB_PATH", "product"),
                          package=os.environ.get("SDRG_PKG_PATH", "product"))), flush=True)
eng.close()
