"""Lab: the display stage (csrc/display.hip) timed on resident spectra, and the host path it shortens.
python tools/lab/display_time.py [calls] [all|kernel]  (SDRG_LIB_PATH selects a variant library; kernel: part (a) only)

(a) sdrg_engine_display_device alone: HIP events around K calls on input buffers rotated so that no call finds its
    spectra in the Infinity Cache (3 buffers, at least 256 MiB each apart), us per launch and the read rate nb * 4 bytes
    per frame gives, beside sdrg_measure_hbm_copy's read + write rate from the same run.
(b) the host path on page-locked buffers at 4096 x 16384, SPECTRUM | STATS: sdrg_engine_process_host returning the
    full spectra against process_host(spectra = NULL) + sdrg_engine_display_host(NULL), ms per call."""
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "sdr-for-android-lib_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import sdrg  # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 60
PARTS = sys.argv[2] if len(sys.argv) > 2 else "all"
dev = torch.device("cuda", 0)
lib = sdrg.load()


def config(n, focus=5):
    return sdrg.SDRConfig(centerFrequency=100_000_000, samplesPerReading=n, sampleRate=2_000_000,
                          freqFocusRangeKhz=focus, soundMode=1)


def kernel_alone(B, n, rotate=3, **disp):
    eng = sdrg.Engine(config(n), B)
    eng.set_display(db_min=-120.0, db_max=0.0, **disp)
    lo, nb, row_bytes = eng.display_geometry()
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    spec = [torch.empty((B, n), dtype=torch.float32, device=dev).exponential_(1.0, generator=g) for _ in range(rotate)]
    out = torch.zeros((B * row_bytes,), dtype=torch.uint8, device=dev)
    work = torch.cuda.Stream(dev)
    eng.set_stream(work.cuda_stream)
    torch.cuda.synchronize()

    def call(k):
        rc = lib.sdrg_engine_display_device(eng._h, ctypes.c_void_p(spec[k % rotate].data_ptr()),
                                            ctypes.c_void_p(out.data_ptr()))
        assert rc == 0, rc

    for k in range(2 * rotate):
        call(k)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(work):
        a.record()
        for k in range(K):
            call(k)
        b.record()
    b.synchronize()
    us = a.elapsed_time(b) / K * 1e3
    read_gbs = B * nb * 4 / (us * 1e-6) / 1e9
    r = dict(kind="kernel", streams=B, n=n, first_bin=lo, n_bins=nb, row_bytes=row_bytes, us_per_launch=round(us, 2),
             read_gb_s=round(read_gbs, 1), **disp)
    print(json.dumps(r), flush=True)
    eng.set_stream(None)
    eng.close()
    del spec, out
    torch.cuda.empty_cache()


def host_path(B, n, calls):
    rng = np.random.default_rng(2)
    iq = sdrg.HostBuffer((B, 2 * n), np.int8)
    iq.array[:] = rng.integers(-100, 100, size=(B, 2 * n), dtype=np.int8)
    spec = sdrg.HostBuffer((B, n), np.float32)
    rec = sdrg.HostBuffer((B,), sdrg.RECORD_DTYPE)
    rows = sdrg.HostBuffer((B, 1024), np.uint8)
    stages = sdrg.STAGE_SPECTRUM | sdrg.STAGE_STATS
    eng = sdrg.Engine(config(n), B)
    eng.set_display(span=sdrg.DISPLAY_SPAN_FULL, width=1024, reduce=sdrg.DISPLAY_MAX, format=sdrg.DISPLAY_U8, db_min=-120.0,
                    db_max=0.0)
    p = lambda h: h.array.ctypes.data_as(ctypes.c_void_p)  # noqa: E731

    def full(k):
        assert lib.sdrg_engine_process_host(eng._h, p(iq), sdrg.CS8, stages, p(spec), p(rec), None, 1000 + k) == 0

    def rows_only(k):
        assert lib.sdrg_engine_process_host(eng._h, p(iq), sdrg.CS8, stages, None, p(rec), None, 1000 + k) == 0
        assert lib.sdrg_engine_display_host(eng._h, None, p(rows)) == 0

    for name, fn in (("process_host, full spectra back", full), ("process_host(NULL) + display_host(NULL)", rows_only),
                     ("process_host, full spectra back", full), ("process_host(NULL) + display_host(NULL)", rows_only)):
        for k in range(3):
            fn(k)
        t0 = time.perf_counter()
        for k in range(calls):
            fn(3 + k)
        ms = (time.perf_counter() - t0) / calls * 1e3
        r = dict(kind="host", path=name, streams=B, n=n, ms_per_call=round(ms, 3))
        print(json.dumps(r), flush=True)
    eng.close()
    for h in (iq, spec, rec, rows):
        h.close()


hbm = sdrg.measure_hbm_copy(0, 1 << 30, 10)
print(json.dumps(dict(kind="hbm_copy", read_plus_write_gb_s=round(hbm, 1), library=os.environ.get("SDRG_LIB_PATH", "product"))),
      flush=True)
U8, F32, MAXR, MEANR = sdrg.DISPLAY_U8, sdrg.DISPLAY_DB_F32, sdrg.DISPLAY_MAX, sdrg.DISPLAY_MEAN
for reduce in (MAXR, MEANR):
    kernel_alone(4096, 16384, span=sdrg.DISPLAY_SPAN_FULL, width=1024, reduce=reduce, format=U8)
    kernel_alone(4096, 16384, span=sdrg.DISPLAY_SPAN_FULL, width=1000, reduce=reduce, format=U8)
    kernel_alone(1024, 65536, span=sdrg.DISPLAY_SPAN_FULL, width=1920, reduce=reduce, format=U8)
    kernel_alone(4096, 16384, span=sdrg.DISPLAY_SPAN_FOCUS, width=64, reduce=reduce, format=U8)
kernel_alone(4096, 16384, span=sdrg.DISPLAY_SPAN_FOCUS, width=1024, reduce=MAXR, format=U8)
kernel_alone(4096, 16384, span=sdrg.DISPLAY_SPAN_FULL, width=16384, reduce=MAXR, format=F32)
if PARTS == "all":
    host_path(4096, 16384, max(5, K // 6))
hbm2 = sdrg.measure_hbm_copy(0, 1 << 30, 10)
print(json.dumps(dict(kind="hbm_copy", read_plus_write_gb_s=round(hbm2, 1))), flush=True)
