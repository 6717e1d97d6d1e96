"""Lab: the host's share of a process_device call, the path bench.py measures.
python tools/lab/engine_core_time.py [calls] [warmup]  (SDRG_LIB_PATH selects a variant library)

16 x 16384 CS8, every stage, pipelining as bench.py sets it for its headline (SDRG_PIPELINE_INPUTS_READY |
SDRG_PIPELINE_STATS_ASYNC), two sets of output buffers in rotation, profiling off and then on: the wall time of the
process_device call alone (the wrapper, enqueue() and the launches it makes), with Engine.synchronize() after each call
outside the timed interval, so no call waits for an earlier one.  One JSON line per profiling setting: the median, the
least and the mean of `calls` calls after `warmup`, us."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "sdr-for-android-lib_amd"))
import torch  # noqa: E402  (before libsdrg.so is loaded: DESIGN.md "HIP runtime")
import sdrg  # noqa: E402

CALLS = int(sys.argv[1]) if len(sys.argv) > 1 else 200
WARMUP = int(sys.argv[2]) if len(sys.argv) > 2 else 20
B, N = 16, 16384

dev = torch.device("cuda:0")
eng = sdrg.Engine(sdrg.SDRConfig(centerFrequency=100_000_000, samplesPerReading=N, sampleRate=2_000_000,
                                 freqFocusRangeKhz=5, soundMode=1), B, device=0)
eng.set_pipelining(sdrg.PIPELINE_INPUTS_READY | sdrg.PIPELINE_STATS_ASYNC)
torch.manual_seed(1)
iq = torch.randint(-128, 128, (B, 2 * N), dtype=torch.int8, device=dev)
spec = [torch.empty((B, N), dtype=torch.float32, device=dev) for _ in range(2)]
rec = [torch.zeros((B, sdrg.RECORD_DTYPE.itemsize), dtype=torch.uint8, device=dev) for _ in range(2)]
pcm = torch.empty((B, eng.pcm_len), dtype=torch.int16, device=dev)
torch.cuda.synchronize()

for prof in (False, True):
    eng.set_profiling(prof)
    us = []
    for k in range(WARMUP + CALLS):
        t0 = time.perf_counter()
        eng.process_device(iq.data_ptr(), sdrg.CS8, sdrg.STAGE_ALL, spec[k % 2].data_ptr(), rec[k % 2].data_ptr(),
                           pcm.data_ptr(), 1000 + 10 * k)
        t1 = time.perf_counter()
        eng.synchronize()
        if k >= WARMUP:
            us.append((t1 - t0) * 1e6)
    print(json.dumps(dict(kind="process_device_host", profiling=prof, streams=B, n=N, calls=CALLS, warmup=WARMUP,
                          median_us=round(statistics.median(us), 1), min_us=round(min(us), 1),
                          mean_us=round(statistics.fmean(us), 1), library=os.environ.get("SDRG_LIB_PATH", "product"))),
          flush=True)
eng.close()
