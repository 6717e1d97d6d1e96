"""Lab: the IQ correction stage (csrc/iqcorr.hip) timed on resident raw rows, beside the squelch at the same shape.
python tools/lab/iqcorr_time.py [calls] [out.jsonl]  (SDRG_LIB_PATH selects a variant library)

sdrg_engine_iqcorr_device alone: HIP events around K calls on three rotating input buffers, us per call (its three
launches), beside sdrg_measure_hbm_copy's read + write rate (a float4 streaming copy) before and after in the same run.
A call reads its raw samples twice (the moments kernel, then the pass kernel) and writes CF32 once: the yardstick of a
shape is bps + 8 + bps bytes per sample at the copy's rate (the mean of the two measurements); `share` is yardstick /
measured.  Every shape is timed with records at S = 256: CS8 and CF32 out of place, and CF32 in place (the rotating
buffers are then corrected again and again, which changes the data, not the work).  Beside each shape, the squelch
(sdrg_engine_squelch_device, out of place) at the same streams, n and S in the same run, and the ratio of the two times.
Inputs: uniform noise in (-1, 1) with a Q gain of 1.05 and an offset, so that every block moves both estimates."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "sdr-for-android-lib_amd"))
import torch  # noqa: E402
import sdrg  # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 40
OUT = sys.argv[2] if len(sys.argv) > 2 else None
S = 256
dev = torch.device("cuda", 0)
lib = sdrg.load()
results = []
BPS = {sdrg.CS8: 2, sdrg.CF32: 8}


def emit(r):
    line = json.dumps(r)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def hbm():
    gbs = sdrg.measure_hbm_copy(0, 1 << 30, 10)
    emit(dict(kind="hbm_copy", read_plus_write_gb_s=round(gbs, 1), library=os.environ.get("SDRG_LIB_PATH", "product")))
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


def engine(B):
    return sdrg.Engine(sdrg.SDRConfig(centerFrequency=100_000_000, samplesPerReading=1024, sampleRate=2_000_000,
                                      freqFocusRangeKhz=5, soundMode=1), B)


def rows(B, n, fmt, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    z = torch.rand((B, n, 2), device=dev, generator=g, dtype=torch.float32) * 2 - 1
    z[..., 1] *= 1.05
    z = z * 0.4 + 0.05
    return z if fmt == sdrg.CF32 else torch.round(z * 100).to(torch.int8)


def squelch_alone(B, n):
    eng = engine(B)
    eng.set_squelch(open_db=-9.0, close_db=-15.0, tau_blocks=2.0, block=S, hang_blocks=2, max_in=n)
    bufs = [rows(B, n, sdrg.CF32, s) for s in range(3)]
    out = torch.zeros((B, n, 2), dtype=torch.float32, device=dev)
    rec = torch.zeros((B, 4), dtype=torch.int32, device=dev)
    n_blocks = ctypes.c_int32()
    work = torch.cuda.Stream(dev)
    eng.set_stream(work.cuda_stream)
    torch.cuda.synchronize()

    def call(k):
        rc = lib.sdrg_engine_squelch_device(eng._h, ctypes.c_void_p(bufs[k % 3].data_ptr()), n, n,
                                            ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(rec.data_ptr()),
                                            ctypes.byref(n_blocks))
        assert rc == 0, rc

    us = timed(work, call, 3)
    torch.cuda.synchronize()
    eng.set_stream(None)
    eng.close()
    return us


def kernel_alone(B, n, fmt, in_place, squelch_us):
    eng = engine(B)
    eng.set_iqcorr(dc_tau_blocks=16.0, balance_tau_blocks=16.0, floor_db=-60.0, mode=3, block=S, max_in=n)
    bufs = [rows(B, n, fmt, s) for s in range(3)]
    out = torch.zeros((B, n, 2), dtype=torch.float32, device=dev)
    rec = torch.zeros((B, 8), dtype=torch.int32, device=dev)
    n_blocks = ctypes.c_int32()
    work = torch.cuda.Stream(dev)
    eng.set_stream(work.cuda_stream)
    torch.cuda.synchronize()

    def call(k):
        src = bufs[k % 3].data_ptr()
        rc = lib.sdrg_engine_iqcorr_device(eng._h, ctypes.c_void_p(src), fmt, n, n,
                                           ctypes.c_void_p(src if in_place else out.data_ptr()),
                                           ctypes.c_void_p(rec.data_ptr()), ctypes.byref(n_blocks))
        assert rc == 0, rc

    us = timed(work, call, 3)
    torch.cuda.synchronize()
    seeded = int(rec[:, 7].sum().item())
    moved = B * n * (BPS[fmt] + 8 + BPS[fmt])
    r = dict(kind="iqcorr", library=os.path.basename(os.environ.get("SDRG_LIB_PATH", "product")), streams=B, n=n,
             fmt={sdrg.CS8: "cs8", sdrg.CF32: "cf32"}[fmt], block=S, in_place=in_place, buffers=3, calls=K,
             tile=sdrg.iqcorr_geometry(S), seeded_streams=seeded, us_per_call=round(us, 2), bytes=moved,
             gb_s=round(moved / (us * 1e-6) / 1e9, 1), squelch_us_per_call=round(squelch_us, 2),
             over_squelch=round(us / squelch_us, 3))
    results.append(r)
    eng.set_stream(None)
    eng.close()
    del bufs, out
    torch.cuda.empty_cache()


before = hbm()
for n in (400, 1639, 16384):  # the squelch's shapes: a narrow-band channel, a broadcast channel, a frame
    sq_us = squelch_alone(4096, n)
    kernel_alone(4096, n, sdrg.CS8, False, sq_us)
    kernel_alone(4096, n, sdrg.CF32, False, sq_us)
    kernel_alone(4096, n, sdrg.CF32, True, sq_us)
after = hbm()
copy = (before + after) / 2
for r in results:
    floor_us = r["bytes"] / (copy * 1e9) * 1e6
    r.update(copy_gb_s=round(copy, 1), yardstick_us=round(floor_us, 2), share=round(floor_us / r["us_per_call"], 3))
    emit(r)
