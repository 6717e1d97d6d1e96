"""Lab: the AFC stage (csrc/afc.hip) timed on resident CF32 rows, beside the squelch at the same shape.
python tools/lab/afc_time.py [calls] [out.jsonl]  (SDRG_LIB_PATH selects a variant library)

sdrg_engine_afc_device alone: HIP events around K calls on three rotating input buffers, us per call (its three
launches, two when it measures), beside sdrg_measure_hbm_copy's read + write rate (a float4 streaming copy) before and
after in the same run.  A tracking call reads its samples twice (the moments kernel, then the pass kernel) and writes
them once: the yardstick of a shape is 8 + 8 + 8 bytes per sample at the copy's rate (the mean of the two measurements),
8 for a measuring call, which reads them once and writes none; `share` is yardstick / measured.  Every shape is timed
with records at S = 256: TRACK out of place, TRACK in place (the rotating buffers are then turned again and again, which
changes the data, not the work) and MEASURE.  Beside each shape, the squelch (sdrg_engine_squelch_device, out of place)
at the same streams, n and S in the same run, and the ratio of the two times.
Inputs: per stream a carrier of 0.5 at its own offset within +-4 kHz of a 48 kHz channel under uniform noise, so that
every stream locks and every sample is turned by its own phase."""
import ctypes
import json
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "sdr-for-android-lib_amd"))
import torch  # noqa: E402
import sdrg  # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 40
OUT = sys.argv[2] if len(sys.argv) > 2 else None
S = 256
RATE = 48000.0
dev = torch.device("cuda", 0)
lib = sdrg.load()
results = []


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


def rows(B, n, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    hz = (torch.arange(B, device=dev, dtype=torch.float64) % 81 - 40) * 100.0
    ph = 2 * math.pi * hz[:, None] * torch.arange(n, device=dev, dtype=torch.float64)[None, :] / RATE
    z = torch.stack([0.5 * torch.cos(ph), 0.5 * torch.sin(ph)], dim=-1).to(torch.float32)
    return (z + 0.1 * (torch.rand((B, n, 2), device=dev, generator=g, dtype=torch.float32) * 2 - 1)).contiguous()


def squelch_alone(B, n):
    eng = engine(B)
    eng.set_squelch(open_db=-9.0, close_db=-15.0, tau_blocks=2.0, block=S, hang_blocks=2, max_in=n)
    bufs = [rows(B, n, s) for s in range(3)]
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


def kernel_alone(B, n, mode, in_place, squelch_us):
    eng = engine(B)
    eng.set_afc(channel_rate=RATE, max_offset_hz=5000.0, tau_blocks=16.0, floor_db=-60.0, lock_threshold=0.25, mode=mode,
                block=S, max_in=n)
    track = mode == sdrg.AFC_TRACK
    bufs = [rows(B, n, s) for s in range(3)]
    out = torch.zeros((B, n, 2), dtype=torch.float32, device=dev)
    rec = torch.zeros((B, 8), dtype=torch.int32, device=dev)
    n_blocks = ctypes.c_int32()
    work = torch.cuda.Stream(dev)
    eng.set_stream(work.cuda_stream)
    torch.cuda.synchronize()

    def call(k):
        src = bufs[k % 3].data_ptr()
        dst = ctypes.c_void_p(src if in_place else out.data_ptr()) if track else None
        rc = lib.sdrg_engine_afc_device(eng._h, ctypes.c_void_p(src), n, n, dst, ctypes.c_void_p(rec.data_ptr()),
                                        ctypes.byref(n_blocks))
        assert rc == 0, rc

    us = timed(work, call, 3)
    torch.cuda.synchronize()
    locked = int((rec[:, 7] & 1).sum().item())
    moved = B * n * (24 if track else 8)
    r = dict(kind="afc", library=os.path.basename(os.environ.get("SDRG_LIB_PATH", "product")), streams=B, n=n,
             mode="track" if track else "measure", block=S, in_place=in_place, buffers=3, calls=K,
             tile=sdrg.afc_geometry(S), locked_streams=locked, us_per_call=round(us, 2), bytes=moved,
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
    kernel_alone(4096, n, sdrg.AFC_TRACK, False, sq_us)
    kernel_alone(4096, n, sdrg.AFC_TRACK, True, sq_us)
    kernel_alone(4096, n, sdrg.AFC_MEASURE, False, sq_us)
after = hbm()
copy = (before + after) / 2
for r in results:
    floor_us = r["bytes"] / (copy * 1e9) * 1e6
    r.update(copy_gb_s=round(copy, 1), yardstick_us=round(floor_us, 2), share=round(floor_us / r["us_per_call"], 3))
    emit(r)
