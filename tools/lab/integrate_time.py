"""Lab: the integration stage (csrc/integrate.hip) timed on resident spectra.
python tools/lab/integrate_time.py [calls] [out.jsonl]  (SDRG_LIB_PATH selects a variant library)

sdrg_engine_integrate_device alone at 4096 x 16384: HIP events around `calls` launches once the ring is full, on input
buffers rotated so that no call finds its spectra in the Infinity Cache (3 buffers of 256 MiB), out of place (one
output buffer) and in place (each input buffer is also the output).  Per line: us per launch, the bytes the model moves
(4c + 8 per bin for MEAN / MAX at depth c, 16 for EMA), the rate that gives, and its share of sdrg_measure_hbm_copy's
read + write rate taken before and after in the same run."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "sdr-for-android-lib_amd"))
import torch  # noqa: E402
import sdrg  # noqa: E402

CALLS = int(sys.argv[1]) if len(sys.argv) > 1 else 60
OUT = sys.argv[2] if len(sys.argv) > 2 else None
LIBRARY = os.path.basename(os.environ.get("SDRG_LIB_PATH", "product"))
dev = torch.device("cuda", 0)
lib = sdrg.load()
lines = []


def emit(**r):
    lines.append(r)
    print(json.dumps(r), flush=True)


def kernel_alone(B, n, in_place, rotate=3, **integ):
    eng = sdrg.Engine(sdrg.SDRConfig(centerFrequency=100_000_000, samplesPerReading=n, sampleRate=2_000_000,
                                     freqFocusRangeKhz=5, soundMode=1), B)
    eng.set_integration(**integ)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    spec = [torch.empty((B, n), dtype=torch.float32, device=dev).exponential_(1.0, generator=g) for _ in range(rotate)]
    out = None if in_place else torch.zeros((B, n), dtype=torch.float32, device=dev)
    work = torch.cuda.Stream(dev)
    eng.set_stream(work.cuda_stream)
    torch.cuda.synchronize()

    def call(k):
        x = spec[k % rotate].data_ptr()
        rc = lib.sdrg_engine_integrate_device(eng._h, ctypes.c_void_p(x), ctypes.c_void_p(x if in_place else out.data_ptr()))
        assert rc == 0, rc

    ema = integ["mode"] == sdrg.INTEGRATE_EMA
    for k in range((2 if ema else integ["period"]) + 2 * rotate):  # the ring fills: every timed call has depth = period
        call(k)
    depth = eng.integration_depth()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(work):
        a.record()
        for k in range(CALLS):
            call(k)
        b.record()
    b.synchronize()
    us = a.elapsed_time(b) / CALLS * 1e3
    per_bin = 16 if ema else 4 * depth + 8
    gbs = B * n * per_bin / (us * 1e-6) / 1e9
    emit(kind="kernel", library=LIBRARY, streams=B, n=n, mode=("MEAN", "MAX", "EMA")[integ["mode"]],
         period=None if ema else integ["period"], in_place=in_place, us_per_launch=round(us, 2), bytes_per_bin=per_bin,
         model_mb=round(B * n * per_bin / 1e6, 1), gb_s=round(gbs, 1))
    eng.set_stream(None)
    eng.close()
    del spec, out
    torch.cuda.empty_cache()


hbm = [sdrg.measure_hbm_copy(0, 1 << 30, 10)]
emit(kind="hbm_copy", library=LIBRARY, read_plus_write_gb_s=round(hbm[0], 1))
MEAN, MAXM, EMA = sdrg.INTEGRATE_MEAN, sdrg.INTEGRATE_MAX, sdrg.INTEGRATE_EMA
for in_place in (False, True):
    for integ in (dict(mode=MEAN, period=2), dict(mode=MEAN, period=10), dict(mode=MEAN, period=16), dict(mode=MAXM, period=10),
                  dict(mode=EMA, alpha=0.1)):
        kernel_alone(4096, 16384, in_place, **integ)
hbm.append(sdrg.measure_hbm_copy(0, 1 << 30, 10))
emit(kind="hbm_copy", library=LIBRARY, read_plus_write_gb_s=round(hbm[1], 1))
copy = sum(hbm) / 2
for r in lines:
    if r["kind"] == "kernel":
        r["share_of_copy"] = round(r["gb_s"] / copy, 3)
if OUT:
    with open(OUT, "a") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")
