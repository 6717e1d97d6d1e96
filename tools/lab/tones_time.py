"""Lab: the tone detector stage (csrc/tones.hip) timed on resident rows, beside the squelch on rows of the same length.
python tools/lab/tones_time.py [calls] [out.jsonl]  (SDRG_LIB_PATH selects a variant library)

sdrg_engine_tones_device alone: HIP events around `calls` calls on three rotating input buffers, us per call (its two
launches), with records, at 4096 streams x n = 100, 400 and 1639 values, K = 1, 8 and 50 tones, Q = 1 and 64 sub-blocks a
block, real and complex values.  Three rounds; in every round each tones shape is followed by sdrg_engine_squelch_device
(block = 64, out of place, with records) on complex rows of the same n, so the two alternate through the run.  Every
round is a line (kind "round"); the summary lines (kind "tones") carry the medians, the ratio to the squelch's median at
that n, and the yardstick: the call's input bytes plus the table once, at sdrg_measure_hbm_copy's read + write rate (a
float4 streaming copy; the mean of a measurement before and one after).  `share` is yardstick / measured."""
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "sdr-for-android-lib_amd"))
import torch  # noqa: E402
import sdrg  # noqa: E402

CALLS = int(sys.argv[1]) if len(sys.argv) > 1 else 40
OUT = sys.argv[2] if len(sys.argv) > 2 else None
B, ROUNDS, FA = 4096, 3, 12195.0
dev = torch.device("cuda", 0)
lib = sdrg.load()


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


def timed(work, call):
    for k in range(6):
        call(k)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(work):
        a.record()
        for k in range(CALLS):
            call(k)
        b.record()
    b.synchronize()
    return a.elapsed_time(b) / CALLS * 1e3


def engine():
    return sdrg.Engine(sdrg.SDRConfig(centerFrequency=100_000_000, samplesPerReading=1024, sampleRate=2_000_000,
                                      freqFocusRangeKhz=5, soundMode=1), B)


def rows(n, width, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return (torch.rand((B, n, width), device=dev, generator=g, dtype=torch.float32) * 2 - 1) * 0.3


def tones_us(n, K, Q, comp):
    bufs = [rows(n, comp, s) for s in range(3)]
    eng = engine()
    lo = 60.0 if comp == 1 else -3000.0
    eng.set_tones(rate_hz=FA, components=comp, freq_hz=[lo + 5900.0 * k / 64 for k in range(K)], sub_blocks=Q,
                  window=sdrg.TONES_HANN, min_db=-30.0, dominance_db=10.0, share=0.05, confirm_blocks=2, release_blocks=1,
                  max_in=n)
    powers = torch.zeros((B, eng.tones_max_blocks(), K), dtype=torch.float32, device=dev)
    rec = torch.zeros((B, 8), dtype=torch.int32, device=dev)
    n_blocks = ctypes.c_int32()
    work = torch.cuda.Stream(dev)
    eng.set_stream(work.cuda_stream)
    torch.cuda.synchronize()

    def call(k):
        rc = lib.sdrg_engine_tones_device(eng._h, ctypes.c_void_p(bufs[k % 3].data_ptr()), n, n,
                                          ctypes.c_void_p(powers.data_ptr()), ctypes.c_void_p(rec.data_ptr()),
                                          ctypes.byref(n_blocks))
        assert rc == 0, rc

    us = timed(work, call)
    torch.cuda.synchronize()
    eng.set_stream(None)
    eng.close()
    del bufs, powers
    torch.cuda.empty_cache()
    return us


def squelch_us(n):
    bufs = [rows(n, 2, s) for s in range(3)]
    out = torch.zeros((B, n, 2), dtype=torch.float32, device=dev)
    rec = torch.zeros((B, 4), dtype=torch.int32, device=dev)
    n_blocks = ctypes.c_int32()
    eng = engine()
    eng.set_squelch(open_db=-12.0, close_db=-18.0, tau_blocks=4.0, block=64, hang_blocks=2, max_in=n)
    work = torch.cuda.Stream(dev)
    eng.set_stream(work.cuda_stream)
    torch.cuda.synchronize()

    def call(k):
        rc = lib.sdrg_engine_squelch_device(eng._h, ctypes.c_void_p(bufs[k % 3].data_ptr()), n, n,
                                            ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(rec.data_ptr()),
                                            ctypes.byref(n_blocks))
        assert rc == 0, rc

    us = timed(work, call)
    torch.cuda.synchronize()
    eng.set_stream(None)
    eng.close()
    del bufs, out
    torch.cuda.empty_cache()
    return us


SHAPES = [(n, K, Q, comp) for n in (100, 400, 1639) for K in (1, 8, 50) for Q in (1, 64) for comp in (1, 2)]
before = hbm()
seen, squelch = {s: [] for s in SHAPES}, {n: [] for n in (100, 400, 1639)}
for rnd in range(ROUNDS):
    for s in SHAPES:
        n, K, Q, comp = s
        t, q = tones_us(*s), squelch_us(n)
        seen[s].append(t)
        squelch[n].append(q)
        emit(dict(kind="round", round=rnd, streams=B, n=n, tones=K, sub_blocks=Q, components=comp, calls=CALLS,
                  us_per_call=round(t, 2), squelch_us_per_call=round(q, 2)))
after = hbm()
copy = (before + after) / 2
for s in SHAPES:
    n, K, Q, comp = s
    us, sq_us = statistics.median(seen[s]), statistics.median(squelch[n])
    moved = B * n * comp * 4 + (K * 64 * Q * 2 + 64 * Q) * 4
    yard = moved / (copy * 1e9) * 1e6
    emit(dict(kind="tones", library=os.path.basename(os.environ.get("SDRG_LIB_PATH", "product")), streams=B, n=n, tones=K,
              sub_blocks=Q, components=comp, buffers=3, calls=CALLS, rounds=ROUNDS,
              sub_blocks_per_group=sdrg.tones_geometry(), us_per_call=round(us, 2), squelch_us_per_call=round(sq_us, 2),
              over_squelch=round(us / sq_us, 3), bytes=moved, copy_gb_s=round(copy, 1), yardstick_us=round(yard, 2),
              share=round(yard / us, 4)))
