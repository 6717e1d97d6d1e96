"""Lab: the symbol stage (csrc/symbols.hip) timed on resident float rows, beside the AFC measuring and the squelch at
the same shape.
python tools/lab/symbols_time.py [calls] [out.jsonl]  (SDRG_LIB_PATH selects a variant library)

sdrg_engine_symbols_device alone: HIP events around K calls on three rotating input buffers, with records, us per call
(its three launches), the median of three rounds, beside sdrg_measure_hbm_copy's read + write rate (a float4 streaming
copy) before and after in the same run.  The yardstick of a shape is 4 bytes per value read twice at the copy's rate
(the mean of the two measurements): once for the moments, once as if the pass read every value again (it reads two
values per symbol, so this is generous to the stage); `share` is yardstick / measured.  Every shape is timed HARD and
SOFT at S = 256 and 10 samples per symbol.  Beside each shape, in the same run and at the same streams, n and S: the
AFC measuring (sdrg_engine_afc_device, SDRG_AFC_MEASURE, on complex rows of n) and the squelch
(sdrg_engine_squelch_device, out of place), and the ratios of the times.
Inputs: per stream 4-level rectangular cells of 10 samples at its own start, smoothed over 6 values, plus a DC offset
and uniform noise, so that every stream locks."""
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "sdr-for-android-lib_amd"))
import torch  # noqa: E402
import sdrg  # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 40
OUT = sys.argv[2] if len(sys.argv) > 2 else None
S = 256
RATE = 48000.0
ROUNDS = 3
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
    us = []
    for _ in range(ROUNDS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(work):
            a.record()
            for k in range(K):
                call(k)
            b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) / K * 1e3)
    return statistics.median(us)


def engine(B):
    return sdrg.Engine(sdrg.SDRConfig(centerFrequency=100_000_000, samplesPerReading=1024, sampleRate=2_000_000,
                                      freqFocusRangeKhz=5, soundMode=1), B)


def audio(B, n, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    cells = n // 10 + 3
    lev = (torch.randint(0, 4, (B, cells), device=dev, generator=g) * 2 - 3).to(torch.float32)
    x = lev.repeat_interleave(10, dim=1)
    start = (torch.arange(B, device=dev) % 10)[:, None] + torch.arange(n + 5, device=dev)[None, :]
    x = torch.gather(x, 1, start)
    x = torch.nn.functional.avg_pool1d(x[:, None, :], 6, stride=1)[:, 0, :n]
    return (x + 0.7 + 0.1 * (torch.rand((B, n), device=dev, generator=g, dtype=torch.float32) * 2 - 1)).contiguous()


def complex_rows(B, n, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return (0.5 * (torch.rand((B, n, 2), device=dev, generator=g, dtype=torch.float32) * 2 - 1)).contiguous()


def run(eng, call):
    work = torch.cuda.Stream(dev)
    eng.set_stream(work.cuda_stream)
    torch.cuda.synchronize()
    us = timed(work, call, 3)
    torch.cuda.synchronize()
    eng.set_stream(None)
    eng.close()
    return us


def squelch_alone(B, n):
    eng = engine(B)
    eng.set_squelch(open_db=-9.0, close_db=-15.0, tau_blocks=2.0, block=S, hang_blocks=2, max_in=n)
    bufs = [complex_rows(B, n, s) for s in range(3)]
    out = torch.zeros((B, n, 2), dtype=torch.float32, device=dev)
    rec = torch.zeros((B, 4), dtype=torch.int32, device=dev)
    nb = ctypes.c_int32()

    def call(k):
        rc = lib.sdrg_engine_squelch_device(eng._h, ctypes.c_void_p(bufs[k % 3].data_ptr()), n, n,
                                            ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(rec.data_ptr()), ctypes.byref(nb))
        assert rc == 0, rc

    return run(eng, call)


def afc_measure_alone(B, n):
    eng = engine(B)
    eng.set_afc(channel_rate=RATE, max_offset_hz=5000.0, tau_blocks=16.0, floor_db=-60.0, lock_threshold=0.25,
                mode=sdrg.AFC_MEASURE, block=S, max_in=n)
    bufs = [complex_rows(B, n, s) for s in range(3)]
    rec = torch.zeros((B, 8), dtype=torch.int32, device=dev)
    nb = ctypes.c_int32()

    def call(k):
        rc = lib.sdrg_engine_afc_device(eng._h, ctypes.c_void_p(bufs[k % 3].data_ptr()), n, n, None,
                                        ctypes.c_void_p(rec.data_ptr()), ctypes.byref(nb))
        assert rc == 0, rc

    return run(eng, call)


def symbols_alone(B, n, fmt, afc_us, squelch_us):
    eng = engine(B)
    eng.set_symbols(sample_rate=RATE, symbol_rate=4800.0, tau_blocks=8.0, tau_level_blocks=8.0, floor_db=-60.0,
                    lock_threshold=0.1, phase_trim=0.0, level_scale=0.894427191, fixed_centre=0.0, fixed_threshold=1.0,
                    levels=4, block=S, level_mode=sdrg.SYM_LEVEL_TRACK, format=fmt, max_in=n)
    cap = eng.symbols_max_out()
    bufs = [audio(B, n, s) for s in range(3)]
    width = 4 if fmt == sdrg.SYM_SOFT else 1
    out = torch.zeros((B * cap * width,), dtype=torch.uint8, device=dev)
    rec = torch.zeros((B, 8), dtype=torch.int32, device=dev)
    ns = ctypes.c_int32()

    def call(k):
        rc = lib.sdrg_engine_symbols_device(eng._h, ctypes.c_void_p(bufs[k % 3].data_ptr()), n, n,
                                            ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(rec.data_ptr()), ctypes.byref(ns))
        assert rc == 0, rc

    us = run(eng, call)
    locked = int((rec[:, 7] & 1).sum().item())
    moved = B * n * 8
    results.append(dict(kind="symbols", library=os.path.basename(os.environ.get("SDRG_LIB_PATH", "product")), streams=B, n=n,
                        format="soft" if fmt == sdrg.SYM_SOFT else "hard", block=S, samples_per_symbol=10, cap=cap,
                        buffers=3, calls=K, rounds=ROUNDS, tiles=list(sdrg.symbols_geometry(S)), locked_streams=locked,
                        us_per_call=round(us, 2), bytes=moved, gb_s=round(moved / (us * 1e-6) / 1e9, 1),
                        afc_measure_us_per_call=round(afc_us, 2), over_afc_measure=round(us / afc_us, 3),
                        squelch_us_per_call=round(squelch_us, 2), over_squelch=round(us / squelch_us, 3)))
    del bufs, out
    torch.cuda.empty_cache()


before = hbm()
for n in (400, 1639, 16384):  # the squelch's shapes: a narrow-band channel, a broadcast channel, a frame
    sq_us = squelch_alone(4096, n)
    afc_us = afc_measure_alone(4096, n)
    symbols_alone(4096, n, sdrg.SYM_HARD, afc_us, sq_us)
    symbols_alone(4096, n, sdrg.SYM_SOFT, afc_us, sq_us)
after = hbm()
copy = (before + after) / 2
for r in results:
    floor_us = r["bytes"] / (copy * 1e9) * 1e6
    r.update(copy_gb_s=round(copy, 1), yardstick_us=round(floor_us, 2), share=round(floor_us / r["us_per_call"], 3))
    emit(r)
