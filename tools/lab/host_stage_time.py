"""Lab: the host calls of the stages that read caller spectra, timed whole.
python tools/lab/host_stage_time.py [calls] [warmup]  (SDRG_LIB_PATH selects a variant library, SDRG_PKG_PATH the
directory that holds a variant of the sdrg package)

display(spectra), integrate(spectra) and peaks(spectra) at 64 x 16384 from pageable host memory: the wall time of each
of `calls` calls after `warmup`, which is the wrapper's argument handling, the copy of the spectra to the device, the
kernel, the copy of the result back and the wait.  One JSON line per stage: the median, the least and the mean, us."""
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
spectra = np.random.default_rng(1).exponential(1.0, size=(B, N)).astype(np.float32)

for name, call in (("display", eng.display), ("integrate", eng.integrate), ("peaks", eng.peaks)):
    for _ in range(WARMUP):
        call(spectra)
    us = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        call(spectra)
        us.append((time.perf_counter() - t0) * 1e6)
    print(json.dumps(dict(kind=name + "_host", streams=B, n=N, calls=CALLS, warmup=WARMUP,
                          median_us=round(statistics.median(us), 1), min_us=round(min(us), 1),
                          mean_us=round(statistics.fmean(us), 1), library=os.environ.get("SDRG_LIB_PATH", "product"),
                          package=os.environ.get("SDRG_PKG_PATH", "product"))), flush=True)
eng.close()
