"""Lab: the DDC stage (csrc/ddc.hip) timed on resident raw IQ.
python tools/lab/ddc_time.py [calls]  (SDRG_LIB_PATH selects a variant library)

sdrg_engine_ddc_device alone: HIP events around K calls on three rotating input buffers, us per launch, beside
sdrg_measure_hbm_copy's read + write rate (a float4 streaming copy) before and after in the same run.  The yardstick of a
shape is its input read plus its output write at the copy's rate (the mean of the two measurements); `share` is
yardstick / measured.  Inputs: uniform noise over the format's whole range."""
import ctypes
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "sdr-for-android-lib_amd"))
import torch  # noqa: E402
import sdrg  # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 60
dev = torch.device("cuda", 0)
lib = sdrg.load()
TORCH_DTYPE = {sdrg.CS8: torch.int8, sdrg.CS16: torch.int16}
NAME = {sdrg.CS8: "CS8", sdrg.CS16: "CS16"}
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


def kernel_alone(B, n, fmt, taps, decimation, offset_hz=250_000.0):
    fs = 2_000_000
    eng = sdrg.Engine(sdrg.SDRConfig(centerFrequency=100_000_000, samplesPerReading=n, sampleRate=fs,
                                     freqFocusRangeKhz=5, soundMode=1), B)
    eng.set_ddc(offset_hz=offset_hz, cutoff_hz=0.4 * fs / decimation, decimation=decimation, taps=taps)
    cap = eng.ddc_max_out()
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    info = torch.iinfo(TORCH_DTYPE[fmt])
    bufs = [torch.randint(info.min, info.max + 1, (B, 2 * n), device=dev, generator=g, dtype=torch.int32)
            .to(TORCH_DTYPE[fmt]) for _ in range(3)]
    out = torch.zeros((B, cap, 2), dtype=torch.float32, device=dev)
    n_out = ctypes.c_int32()
    work = torch.cuda.Stream(dev)
    eng.set_stream(work.cuda_stream)
    torch.cuda.synchronize()

    def call(k):
        rc = lib.sdrg_engine_ddc_device(eng._h, ctypes.c_void_p(bufs[k % 3].data_ptr()), fmt,
                                        ctypes.c_void_p(out.data_ptr()), ctypes.byref(n_out))
        assert rc == 0, rc

    us = timed(work, call, 3)
    in_bytes, out_bytes = B * n * sdrg.BYTES_PER_SAMPLE[fmt], B * cap * 8
    r = dict(kind="ddc", library=os.path.basename(os.environ.get("SDRG_LIB_PATH", "product")), streams=B, n=n,
             format=NAME[fmt], taps=taps, decimation=decimation, buffers=3, calls=K,
             tile_outputs=sdrg.ddc_tile_outputs(decimation, taps), us_per_launch=round(us, 2), in_bytes=in_bytes,
             out_bytes=out_bytes, read_plus_write_gb_s=round((in_bytes + out_bytes) / (us * 1e-6) / 1e9, 1),
             out_sha256=sha256(out))
    results.append(r)
    eng.set_stream(None)
    eng.close()
    del bufs, out
    torch.cuda.empty_cache()


before = hbm()
kernel_alone(4096, 16384, sdrg.CS8, 255, 41)
kernel_alone(4096, 16384, sdrg.CS8, 127, 16)
kernel_alone(4096, 16384, sdrg.CS8, 63, 8)
kernel_alone(1024, 65536, sdrg.CS16, 255, 41)
kernel_alone(4096, 16384, sdrg.CS8, 1, 41)     # attribution: staging alone (one tap)
kernel_alone(4096, 16384, sdrg.CS8, 255, 512)  # attribution: the same staging, a sixteenth of the taps' work
after = hbm()
copy = (before + after) / 2
for r in results:
    floor_us = (r["in_bytes"] + r["out_bytes"]) / (copy * 1e9) * 1e6
    r.update(copy_gb_s=round(copy, 1), yardstick_us=round(floor_us, 2), share=round(floor_us / r["us_per_launch"], 3))
    print(json.dumps(r), flush=True)
