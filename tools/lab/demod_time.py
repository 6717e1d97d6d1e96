"""Lab: the demodulator stage (csrc/demod.hip) timed on a resident CF32 channel.
python tools/lab/demod_time.py [calls]  (SDRG_LIB_PATH selects a variant library)

sdrg_engine_demod_device alone: HIP events around K calls on three rotating input buffers, us per call (its two or three
launches), beside sdrg_measure_hbm_copy's read + write rate (a float4 streaming copy) before and after in the same run.
The yardstick of a shape is its input read plus its output write at the copy's rate (the mean of the two measurements);
`share` is yardstick / measured.  Every shape is timed with both recurrences on and, for attribution, with both off (the
recurrence kernel is then not launched: the difference is its time).  Inputs: uniform noise in (-1, 1), float output."""
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


def kernel_alone(B, n, fc, R, T2, recurrences, mode=sdrg.DEMOD_FM):
    eng = sdrg.Engine(sdrg.SDRConfig(centerFrequency=100_000_000, samplesPerReading=1024, sampleRate=2_000_000,
                                     freqFocusRangeKhz=5, soundMode=1), B)
    eng.set_demod(mode=mode, channel_rate_hz=fc, deviation_hz=fc / 4, dc_cutoff_hz=20.0 if recurrences else 0.0,
                  deemphasis_us=75.0 if recurrences else 0.0, audio_decimation=R, audio_taps=T2,
                  audio_cutoff_hz=0.4 * fc / R, gain=1.0, out_format=sdrg.DEMOD_OUT_F32, max_in=n)
    cap = eng.demod_max_out()
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    bufs = [torch.rand((B, n, 2), device=dev, generator=g, dtype=torch.float32) * 2 - 1 for _ in range(3)]
    out = torch.zeros((B, cap), dtype=torch.float32, device=dev)
    n_out = ctypes.c_int32()
    work = torch.cuda.Stream(dev)
    eng.set_stream(work.cuda_stream)
    torch.cuda.synchronize()

    def call(k):
        rc = lib.sdrg_engine_demod_device(eng._h, ctypes.c_void_p(bufs[k % 3].data_ptr()), n,
                                          ctypes.c_void_p(out.data_ptr()), ctypes.byref(n_out))
        assert rc == 0, rc

    us = timed(work, call, 3)
    tile, chunk = sdrg.demod_geometry(R, T2)
    in_bytes, out_bytes = B * n * 8, B * cap * 4
    r = dict(kind="demod", library=os.path.basename(os.environ.get("SDRG_LIB_PATH", "product")), streams=B, n=n,
             mode="FM" if mode == sdrg.DEMOD_FM else "AM", decimation=R, taps=T2, recurrences=recurrences, buffers=3,
             calls=K, tile_outputs=tile, chunk=chunk, us_per_call=round(us, 2), in_bytes=in_bytes, out_bytes=out_bytes,
             read_plus_write_gb_s=round((in_bytes + out_bytes) / (us * 1e-6) / 1e9, 1), out_sha256=sha256(out))
    results.append(r)
    eng.set_stream(None)
    eng.close()
    del bufs, out
    torch.cuda.empty_cache()


before = hbm()
for rec in (True, False):
    kernel_alone(4096, 400, 2_000_000 / 41, 1, 1, rec)    # narrow-band FM behind D = 41
    kernel_alone(4096, 1639, 200_000.0, 4, 127, rec)      # broadcast FM behind D = 10
    kernel_alone(4096, 16384, 2_000_000.0, 1, 1, rec)     # the serial kernel at its worst
after = hbm()
copy = (before + after) / 2
for r in results:
    floor_us = (r["in_bytes"] + r["out_bytes"]) / (copy * 1e9) * 1e6
    r.update(copy_gb_s=round(copy, 1), yardstick_us=round(floor_us, 2), share=round(floor_us / r["us_per_call"], 3))
    print(json.dumps(r), flush=True)
