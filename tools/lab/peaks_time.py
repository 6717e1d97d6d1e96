"""Lab: the peak table stage (csrc/peaks.hip) timed on resident spectra.
python tools/lab/peaks_time.py [calls]  (SDRG_LIB_PATH selects a variant library)

sdrg_engine_peaks_device alone: HIP events around K calls on input buffers rotated so that no call finds its spectra in
the Infinity Cache (3 buffers, at least 256 MiB each), us per launch and the read rate nb * 4 bytes per frame gives,
beside sdrg_measure_hbm_copy's read + write rate before and after, and the display stage's MAX row (1024 U8 columns) of
the same spectra in the same run.  Inputs: exponential noise of mean 1, and the same with 20 tones per row (1000 over the
mean, a skirt of two bins on each side)."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "sdr-for-android-lib_amd"))
import torch  # noqa: E402
import sdrg  # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 60
dev = torch.device("cuda", 0)
lib = sdrg.load()


def config(n, focus=5):
    return sdrg.SDRConfig(centerFrequency=100_000_000, samplesPerReading=n, sampleRate=2_000_000,
                          freqFocusRangeKhz=focus, soundMode=1)


def spectra(B, n, tones, rotate):
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    bufs = []
    for _ in range(rotate):  # 256 MiB each at 4096 x 16384 and 1024 x 65536
        s = torch.empty((B, n), dtype=torch.float32, device=dev).exponential_(1.0, generator=g)
        if tones:
            at = torch.randint(2, n - 2, (B, tones), device=dev, generator=g)
            for k in (-2, -1, 0, 1, 2):
                s.scatter_add_(1, at + k, torch.full((B, tones), 1000.0 / (1 + 4 * k * k), device=dev))
        bufs.append(s)
    return bufs


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


def kernel_alone(B, n, tones, span, max_peaks=16, min_separation=8, threshold_db=10.0, display=False):
    eng = sdrg.Engine(config(n), B)
    eng.set_peaks(span=span, max_peaks=max_peaks, min_separation=min_separation, threshold_db=threshold_db)
    eng.set_display(span=span, width=1024, reduce=sdrg.DISPLAY_MAX, format=sdrg.DISPLAY_U8, db_min=-120.0, db_max=0.0)
    lo, nb, row_bytes = eng.display_geometry()
    spec = spectra(B, n, tones, 3)
    rotate = len(spec)
    pk = torch.zeros((B * max_peaks * 16,), dtype=torch.uint8, device=dev)
    sm = torch.zeros((B * 16,), dtype=torch.uint8, device=dev)
    rows = torch.zeros((B * row_bytes,), dtype=torch.uint8, device=dev)
    work = torch.cuda.Stream(dev)
    eng.set_stream(work.cuda_stream)
    torch.cuda.synchronize()

    def peaks_call(k):
        rc = lib.sdrg_engine_peaks_device(eng._h, ctypes.c_void_p(spec[k % rotate].data_ptr()), ctypes.c_void_p(pk.data_ptr()),
                                          ctypes.c_void_p(sm.data_ptr()))
        assert rc == 0, rc

    def display_call(k):
        rc = lib.sdrg_engine_display_device(eng._h, ctypes.c_void_p(spec[k % rotate].data_ptr()),
                                            ctypes.c_void_p(rows.data_ptr()))
        assert rc == 0, rc

    us = timed(work, peaks_call, rotate)
    summary = sm.cpu().numpy().view(sdrg.PEAKS_SUMMARY_DTYPE)
    r = dict(kind="peaks", streams=B, n=n, first_bin=lo, n_bins=nb, tones=tones, max_peaks=max_peaks,
             min_separation=min_separation, threshold_db=threshold_db, buffers=rotate, us_per_launch=round(us, 2),
             read_gb_s=round(B * nb * 4 / (us * 1e-6) / 1e9, 1), mean_n_above=round(float(summary["n_above"].mean()), 2))
    print(json.dumps(r), flush=True)
    if display:
        us = timed(work, display_call, rotate)
        r = dict(kind="display_max_1024_u8", streams=B, n=n, n_bins=nb, tones=tones, us_per_launch=round(us, 2),
                 read_gb_s=round(B * nb * 4 / (us * 1e-6) / 1e9, 1))
        print(json.dumps(r), flush=True)
    eng.set_stream(None)
    eng.close()
    del spec, pk, sm, rows
    torch.cuda.empty_cache()


def hbm():
    gbs = sdrg.measure_hbm_copy(0, 1 << 30, 10)
    print(json.dumps(dict(kind="hbm_copy", read_plus_write_gb_s=round(gbs, 1),
                          library=os.environ.get("SDRG_LIB_PATH", "product"))), flush=True)


FULL, FOCUS = sdrg.DISPLAY_SPAN_FULL, sdrg.DISPLAY_SPAN_FOCUS
hbm()
for tones in (0, 20):
    kernel_alone(4096, 16384, tones, FULL, display=True)
    kernel_alone(4096, 16384, tones, FULL, min_separation=1)
    kernel_alone(4096, 16384, tones, FULL, min_separation=4096)
# attribution: one top-K round instead of 16, and a threshold nothing reaches (no candidate scan, no top-K round)
kernel_alone(4096, 16384, 0, FULL, max_peaks=1)
kernel_alone(4096, 16384, 0, FULL, threshold_db=300.0)
kernel_alone(4096, 16384, 0, FOCUS, display=True)
kernel_alone(1024, 65536, 0, FULL, display=True)
kernel_alone(1024, 65536, 20, FULL)
hbm()
