"""Lab: the noise blanker stage (csrc/blanker.hip) timed on resident raw rows, beside the IQ correction at the same shape.
python tools/lab/blanker_time.py [calls] [out.jsonl]  (SDRG_LIB_PATH selects a variant library)

sdrg_engine_blanker_device alone: HIP events around K calls on three rotating input buffers, us per call (its three
launches), beside sdrg_measure_hbm_copy's read + write rate (a float4 streaming copy) before and after in the same run.
A call reads its raw samples twice (the floor kernel, then the pass kernel) and writes CF32 once: the yardstick of a
shape is bps + 8 + bps bytes per sample at the copy's rate (the mean of the two measurements); `share` is yardstick /
measured.  Every shape is timed with records at S = 256, lead 2 and tail 8, CS8 and CF32.  Beside each shape, the IQ
correction (sdrg_engine_iqcorr_device, out of place, the same three dependent launches) at the same streams, n, S and
format in the same run, and the ratio of the two times.  Inputs: uniform noise in (-0.1, 0.1) with a pulse of 0.9 every
997 samples, so that calls have hits, windows and atomics as a pulsed band gives them."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "sdr-for-android-lib_amd"))
import torch  # noqa: E402
import sdrg  # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 40
OUT = sys.argv[2] if len(sys.argv) > 2 else None
S, LEAD, TAIL = 256, 2, 8
dev = torch.device("cuda", 0)
lib = sdrg.load()
results = []
BPS = {sdrg.CS8: 2, sdrg.CF32: 8}
NAME = {sdrg.CS8: "cs8", sdrg.CF32: "cf32"}


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
    z = (torch.rand((B, n, 2), device=dev, generator=g, dtype=torch.float32) * 2 - 1) * 0.1
    z.view(-1, 2)[seed + 300::997, 0] += 0.9
    return z if fmt == sdrg.CF32 else torch.round(z * 100).to(torch.int8)


def stage_alone(B, n, fmt, device_call, words):
    """us per call of a stage's device call on three rotating buffers, and its last records [B][words] int32."""
    bufs = [rows(B, n, fmt, s) for s in range(3)]
    out = torch.zeros((B, n, 2), dtype=torch.float32, device=dev)
    rec = torch.zeros((B, words), dtype=torch.int32, device=dev)
    n_blocks = ctypes.c_int32()
    work = torch.cuda.Stream(dev)
    eng = engine(B)
    eng.set_iqcorr(dc_tau_blocks=16.0, balance_tau_blocks=16.0, floor_db=-60.0, mode=3, block=S, max_in=n)
    eng.set_blanker(tau_blocks=16.0, threshold_db=13.0, floor_db=-100.0, block=S, lead=LEAD, tail=TAIL, max_in=n)
    eng.set_stream(work.cuda_stream)
    torch.cuda.synchronize()

    def call(k):
        rc = device_call(eng._h, ctypes.c_void_p(bufs[k % 3].data_ptr()), fmt, n, n, ctypes.c_void_p(out.data_ptr()),
                         ctypes.c_void_p(rec.data_ptr()), ctypes.byref(n_blocks))
        assert rc == 0, rc

    us = timed(work, call, 3)
    torch.cuda.synchronize()
    rec = rec.cpu()
    eng.set_stream(None)
    eng.close()
    del bufs, out
    torch.cuda.empty_cache()
    return us, rec


def shape(B, n, fmt):
    iq_us, _ = stage_alone(B, n, fmt, lib.sdrg_engine_iqcorr_device, 8)
    us, rec = stage_alone(B, n, fmt, lib.sdrg_engine_blanker_device, 4)
    moved = B * n * (BPS[fmt] + 8 + BPS[fmt])
    floor_tile, pass_tile = sdrg.blanker_geometry(S)
    results.append(dict(kind="blanker", library=os.path.basename(os.environ.get("SDRG_LIB_PATH", "product")), streams=B,
                        n=n, fmt=NAME[fmt], block=S, lead=LEAD, tail=TAIL, buffers=3, calls=K, floor_tile=floor_tile,
                        pass_tile=pass_tile, hits_per_stream=round(float(rec[:, 2].float().mean()), 2),
                        blanked_per_stream=round(float(rec[:, 3].float().mean()), 2), us_per_call=round(us, 2),
                        bytes=moved, gb_s=round(moved / (us * 1e-6) / 1e9, 1), iqcorr_us_per_call=round(iq_us, 2),
                        over_iqcorr=round(us / iq_us, 3)))


before = hbm()
for n in (400, 1639, 16384):  # the IQ correction's shapes: a narrow-band channel, a broadcast channel, a frame
    shape(4096, n, sdrg.CS8)
    shape(4096, n, sdrg.CF32)
after = hbm()
copy = (before + after) / 2
for r in results:
    floor_us = r["bytes"] / (copy * 1e9) * 1e6
    r.update(copy_gb_s=round(copy, 1), yardstick_us=round(floor_us, 2), share=round(floor_us / r["us_per_call"], 3))
    emit(r)
