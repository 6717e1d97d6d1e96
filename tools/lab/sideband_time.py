"""Lab: the sideband stage (csrc/sideband.hip) timed on a resident CF32 channel, beside the DDC on the same rows.
python tools/lab/sideband_time.py [calls] [out.jsonl]  (SDRG_LIB_PATH selects a variant library)

sdrg_engine_sideband_device alone: HIP events around K calls on three rotating input buffers, us per call, beside
sdrg_measure_hbm_copy's read + write rate (a float4 streaming copy) before and after in the same run.  The yardstick of a
shape is its input read plus its output write at the copy's rate (the mean of the two measurements); `share` is
yardstick / measured.  sdrg_engine_ddc_device is timed on the same CF32 rows with (D, T) = (R, T) in the same run, the
two alternating over three rounds; each figure is the median of its three.  Inputs: uniform noise in (-1, 1), float
output, UPPER and BOTH."""
import ctypes
import hashlib
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "sdr-for-android-lib_amd"))
import torch  # noqa: E402
import sdrg  # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 40
OUT = sys.argv[2] if len(sys.argv) > 2 else None
ROUNDS = 3
FS = 2_000_000
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


def shape(B, n, R, T, mode):
    eng = sdrg.Engine(sdrg.SDRConfig(centerFrequency=100_000_000, samplesPerReading=n, sampleRate=FS,
                                     freqFocusRangeKhz=5, soundMode=1), B)
    eng.set_sideband(channel_rate_hz=float(FS), low_hz=300.0, high_hz=0.4 * FS / R, mode=mode, audio_decimation=R, taps=T,
                     out_format=sdrg.SIDEBAND_OUT_F32, max_in=n, gain=1.0)
    eng.set_ddc(offset_hz=0.1 * FS, cutoff_hz=0.4 * FS / R, decimation=R, taps=T)
    cap, width = eng.sideband_max_out(), 2 if mode == sdrg.SIDEBAND_BOTH else 1
    assert eng.ddc_max_out() == cap
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    bufs = [torch.rand((B, n, 2), device=dev, generator=g, dtype=torch.float32) * 2 - 1 for _ in range(3)]
    out = torch.zeros((B, cap, width), dtype=torch.float32, device=dev)
    ddc_out = torch.zeros((B, cap, 2), dtype=torch.float32, device=dev)
    n_out = ctypes.c_int32()
    work = torch.cuda.Stream(dev)
    eng.set_stream(work.cuda_stream)
    torch.cuda.synchronize()

    def sideband_call(k):
        rc = lib.sdrg_engine_sideband_device(eng._h, ctypes.c_void_p(bufs[k % 3].data_ptr()), n,
                                             ctypes.c_void_p(out.data_ptr()), ctypes.byref(n_out))
        assert rc == 0, rc

    def ddc_call(k):
        rc = lib.sdrg_engine_ddc_device(eng._h, ctypes.c_void_p(bufs[k % 3].data_ptr()), sdrg.CF32,
                                        ctypes.c_void_p(ddc_out.data_ptr()), ctypes.byref(n_out))
        assert rc == 0, rc

    sb_us, ddc_us = [], []
    for _ in range(ROUNDS):
        sb_us.append(timed(work, sideband_call, 3))
        ddc_us.append(timed(work, ddc_call, 3))
    us, d_us = statistics.median(sb_us), statistics.median(ddc_us)
    in_bytes, out_bytes = B * n * 8, B * cap * width * 4
    r = dict(kind="sideband", library=os.path.basename(os.environ.get("SDRG_LIB_PATH", "product")), streams=B, n=n,
             mode="BOTH" if width == 2 else "UPPER", decimation=R, taps=T, buffers=3, calls=K, rounds=ROUNDS,
             tile_outputs=sdrg.sideband_geometry(R, T), us_per_call=round(us, 2),
             us_rounds=[round(x, 2) for x in sb_us], ddc_us_per_call=round(d_us, 2),
             ddc_us_rounds=[round(x, 2) for x in ddc_us], sideband_over_ddc=round(us / d_us, 3), in_bytes=in_bytes,
             out_bytes=out_bytes, ddc_out_bytes=B * cap * 8,
             read_plus_write_gb_s=round((in_bytes + out_bytes) / (us * 1e-6) / 1e9, 1), out_sha256=sha256(out))
    results.append(r)
    eng.set_stream(None)
    eng.close()
    del bufs, out, ddc_out
    torch.cuda.empty_cache()


before = hbm()
for mode in (sdrg.SIDEBAND_UPPER, sdrg.SIDEBAND_BOTH):
    for n in (400, 1639, 16384):
        for R, T in ((1, 255), (4, 511), (1, 1)):
            shape(4096, n, R, T, mode)
after = hbm()
copy = (before + after) / 2
lines = []
for r in results:
    floor_us = (r["in_bytes"] + r["out_bytes"]) / (copy * 1e9) * 1e6
    r.update(copy_gb_s=round(copy, 1), yardstick_us=round(floor_us, 2), share=round(floor_us / r["us_per_call"], 3))
    lines.append(json.dumps(r))
    print(lines[-1], flush=True)
if OUT:
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
