"""Lab: the AGC stage (csrc/agc.hip) timed on a resident CF32 channel.
python tools/lab/agc_time.py [calls] [out.jsonl]  (SDRG_LIB_PATH selects a variant library)

sdrg_engine_agc_device alone, as tools/lab/squelch_time.py times the squelch: HIP events around K calls on three
rotating input buffers, us per call (its three launches), beside sdrg_measure_hbm_copy's read + write rate (a float4
streaming copy) before and after in the same run.  The yardstick of a shape is its input read plus its output write at
the copy's rate (the mean of the two measurements); `share` is yardstick / measured.  Every shape is timed with records,
out of place and in place (out == chan: the rotating buffers are then levelled again and again, which changes the data,
not the work), at S = 64 and at S = 16 (four times the blocks for the serial step).  Two rows for attribution: the long
shape with n = 0 (the zero rows and the records only) and with the peak detector.  Inputs: uniform noise in (-1, 1),
eight blocks loud and eight at a tenth of the amplitude in turn, so that the gain attacks, hangs and decays within a long
call."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "sdr-for-android-lib_amd"))
import torch  # noqa: E402
import sdrg  # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 40
OUT = sys.argv[2] if len(sys.argv) > 2 else None
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


def kernel_alone(B, n, S, in_place, n_call=None, detector=sdrg.AGC_DET_MEAN):
    n_call = n if n_call is None else n_call
    eng = sdrg.Engine(sdrg.SDRConfig(centerFrequency=100_000_000, samplesPerReading=1024, sampleRate=2_000_000,
                                     freqFocusRangeKhz=5, soundMode=1), B)
    eng.set_agc(target=0.25, max_gain_db=40.0, initial_gain_db=0.0, floor_db=-60.0, attack_blocks=0.5, decay_blocks=4.0,
                detector=detector, block=S, hang_blocks=2, max_in=n)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    loud = ((torch.arange(n, device=dev) // (8 * S)) % 2 == 0).to(torch.float32) * 0.9 + 0.1
    bufs = [(torch.rand((B, n, 2), device=dev, generator=g, dtype=torch.float32) * 2 - 1) * loud[None, :, None]
            for _ in range(3)]
    out = torch.zeros((B, n, 2), dtype=torch.float32, device=dev)
    rec = torch.zeros((B, 4), dtype=torch.int32, device=dev)
    n_blocks = ctypes.c_int32()
    work = torch.cuda.Stream(dev)
    eng.set_stream(work.cuda_stream)
    torch.cuda.synchronize()

    def call(k):
        src = bufs[k % 3].data_ptr()
        rc = lib.sdrg_engine_agc_device(eng._h, ctypes.c_void_p(src), n, n_call,
                                        ctypes.c_void_p(src if in_place else out.data_ptr()),
                                        ctypes.c_void_p(rec.data_ptr()), ctypes.byref(n_blocks))
        assert rc == 0, rc

    us = timed(work, call, 3)
    torch.cuda.synchronize()
    attacks = int(rec[:, 3].sum().item())
    in_bytes, out_bytes = B * n_call * 8, B * n * 8
    r = dict(kind="agc", library=os.path.basename(os.environ.get("SDRG_LIB_PATH", "product")), streams=B, n=n_call,
             in_stride=n, block=S, detector=detector, in_place=in_place, buffers=3, calls=K, tile=sdrg.agc_geometry(S),
             attacks_in_the_last_call=attacks, us_per_call=round(us, 2), in_bytes=in_bytes, out_bytes=out_bytes,
             read_plus_write_gb_s=round((in_bytes + out_bytes) / (us * 1e-6) / 1e9, 1))
    results.append(r)
    eng.set_stream(None)
    eng.close()
    del bufs, out
    torch.cuda.empty_cache()


before = hbm()
for S in (64, 16):
    for in_place in (False, True):
        kernel_alone(4096, 400, S, in_place)     # a narrow-band channel behind D = 41
        kernel_alone(4096, 1639, S, in_place)    # a broadcast channel behind D = 10
        kernel_alone(4096, 16384, S, in_place)   # 256 (S = 64) or 1024 (S = 16) blocks per stream and call
kernel_alone(4096, 16384, 64, False, n_call=0)   # attribution: the zero rows and the step kernel's records only
kernel_alone(4096, 16384, 64, False, detector=sdrg.AGC_DET_PEAK)  # attribution: the maximum in place of the sum
after = hbm()
copy = (before + after) / 2
for r in results:
    floor_us = (r["in_bytes"] + r["out_bytes"]) / (copy * 1e9) * 1e6
    r.update(copy_gb_s=round(copy, 1), yardstick_us=round(floor_us, 2), share=round(floor_us / r["us_per_call"], 3))
    emit(r)
