"""Lab: the resampler stage (csrc/resample.hip) timed on resident rows.
python tools/lab/resample_time.py [calls]  (SDRG_LIB_PATH selects a variant library)

sdrg_engine_resample_device alone: HIP events around K calls on three rotating input buffers, us per call (its one
launch), beside sdrg_measure_hbm_copy's read + write rate (a float4 streaming copy) before and after in the same run.
The yardstick of a shape is its input read plus its output write at the copy's rate (the mean of the two measurements);
`share` is yardstick / measured.  Inputs: uniform noise in (-1, 1), float output."""
import ctypes
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "sdr-for-android-lib_amd"))
import torch  # noqa: E402
import sdrg  # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 40
dev = torch.device("cuda", 0)
lib = sdrg.load()
results = []


def sha256(t):
    """The hash of a device tensor's bytes once the work on it is done: two libraries that compute the same agree on it."""
    torch.cuda.synchronize()
    return hashlib.sha256(t.cpu().numpy()).hexdigest()


def hbm():
    gbs = sdrg.measure_hbm_copy(0, 1 << 30, 10)
    print(json.dumps(dict(kind="hbm_copy", read_plus_write_gb_s=round(gbs, 1),
                          library=os.environ.get("SDRG_LIB_PATH", "product"))), flush=True)
    return gbs


def timed(work, call, rotate):
    for k in range(2 * rotate):
        call(k)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(work):
        a.record()
        for k in range(K):
            call(k)
        b.record()
    b.synchronize()
    return a.elapsed_time(b) / K * 1e3


def kernel_alone(B, n, L, M, P, components):
    eng = sdrg.Engine(sdrg.SDRConfig(centerFrequency=100_000_000, samplesPerReading=1024, sampleRate=2_000_000,
                                     freqFocusRangeKhz=5, soundMode=1), B)
    eng.set_resample(interp=L, decim=M, taps_per_phase=P, cutoff_rel=0.9, components=components,
                     out_format=sdrg.RESAMPLE_OUT_F32, gain=1.0, max_in=n)
    cap = eng.resample_max_out()
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    bufs = [torch.rand((B, n, components), device=dev, generator=g, dtype=torch.float32) * 2 - 1 for _ in range(3)]
    out = torch.zeros((B, cap, components), dtype=torch.float32, device=dev)
    n_out = ctypes.c_int32()
    work = torch.cuda.Stream(dev)
    eng.set_stream(work.cuda_stream)
    torch.cuda.synchronize()

    def call(k):
        rc = lib.sdrg_engine_resample_device(eng._h, ctypes.c_void_p(bufs[k % 3].data_ptr()), n, n,
                                             ctypes.c_void_p(out.data_ptr()), ctypes.byref(n_out))
        assert rc == 0, rc

    us = timed(work, call, 3)
    in_bytes, out_bytes = B * n * 4 * components, B * cap * 4 * components
    r = dict(kind="resample", library=os.path.basename(os.environ.get("SDRG_LIB_PATH", "product")), streams=B, n=n,
             interp=L, decim=M, taps_per_phase=P, components=components, buffers=3, calls=K,
             tile_outputs=sdrg.resample_tile_outputs(interp=L, decim=M, taps_per_phase=P, cutoff_rel=0.9,
                                                     components=components, out_format=sdrg.RESAMPLE_OUT_F32,
                                                     gain=1.0, max_in=n),
             us_per_call=round(us, 2), in_bytes=in_bytes, out_bytes=out_bytes,
             macs=B * cap * P * components, gmacs_per_s=round(B * cap * P * components / (us * 1e-6) / 1e9, 1),
             read_plus_write_gb_s=round((in_bytes + out_bytes) / (us * 1e-6) / 1e9, 1), out_sha256=sha256(out))
    results.append(r)
    eng.set_stream(None)
    eng.close()
    del bufs, out
    torch.cuda.empty_cache()


before = hbm()
kernel_alone(4096, 1639, 123, 125, 16, 1)   # audio behind D = 41: 48 780.49 Hz to 48 000 Hz
kernel_alone(4096, 1639, 147, 160, 24, 1)   # 48 000 Hz to 44 100 Hz
kernel_alone(4096, 16384, 3, 2, 8, 2)       # a CF32 channel up by 3 / 2
kernel_alone(4096, 16384, 2, 3, 8, 2)       # and down by 2 / 3
kernel_alone(4096, 1639, 512, 511, 16, 1)   # the widest tap table: every tile stages 256 rows
after = hbm()
copy = (before + after) / 2
for r in results:
    floor_us = (r["in_bytes"] + r["out_bytes"]) / (copy * 1e9) * 1e6
    r.update(copy_gb_s=round(copy, 1), yardstick_us=round(floor_us, 2), share=round(floor_us / r["us_per_call"], 3))
    print(json.dumps(r), flush=True)
