"""GPU tests of the display stage (csrc/display.hip, sdrg_engine_display_*): dB rows decimated to W columns, against
the NumPy restatement in tests/display_cases.py.  MAX results, and both output formats, are compared as bytes; MEAN
is bit-exact where the sums are (powers k * 2^-10) and within the stated tolerance on the engine's own spectra.

The launcher picks one of three kernels (direct: W >= nb; shuffle: nb / W a power of two in [4, 256] on 16-byte
aligned rows; tiled LDS accumulators: every other W < nb, several frames per workgroup for small spans): the shapes
below reach each of them, with aligned and misaligned spans, odd N, odd row lengths of bytes and column tiles."""
import ctypes

import numpy as np
import pytest

import display_cases as dc

pytestmark = pytest.mark.gpu

FS = 2_000_000
DB_MIN, DB_MAX = -120.0, 0.0


@pytest.fixture(scope="module")
def S():
    import sdrg
    return sdrg


@pytest.fixture(scope="module")
def O():
    import oracle
    return oracle


@pytest.fixture(scope="module")
def T():
    import torch
    return torch


def engine(S, n, B, focus=5, fs=FS):
    return S.Engine(S.SDRConfig(centerFrequency=100_000_000, samplesPerReading=n, sampleRate=fs, freqFocusRangeKhz=focus,
                                soundMode=1), B)


def invalid(S, fn, *a, **k):
    with pytest.raises(S.SdrgError) as ei:
        fn(*a, **k)
    assert "SDRG_E_INVALID" in str(ei.value)


GUARD = 64


def display_device(T, eng, spec_t, **cfg):
    """set_display(**cfg), display_device on a 0xAA-filled buffer with GUARD bytes after it; returns the rows as the
    configured dtype [B][W] after checking the guard."""
    cfg.setdefault("db_min", DB_MIN)
    cfg.setdefault("db_max", DB_MAX)
    eng.set_display(**cfg)
    _, _, rb = eng.display_geometry()
    B = eng.n_streams
    out = T.full((B * rb + GUARD,), 0xAA, dtype=T.uint8, device=spec_t.device)
    T.cuda.synchronize()
    eng.display_device(spec_t.data_ptr(), out.data_ptr())
    eng.synchronize()
    raw = out.cpu().numpy()
    assert np.all(raw[B * rb:] == 0xAA), "bytes written past the last row"
    u8 = cfg.get("format", 0) == dc.U8
    return raw[:B * rb].view(np.uint8 if u8 else np.float32).reshape(B, cfg["width"])


def want_rows(spec, lo, nb, cfg):
    return dc.rows(spec, lo, nb, cfg["width"], cfg.get("reduce", 0), cfg.get("format", 0), DB_MIN, DB_MAX)


def check_exact(T, eng, spec_t, spec, lo, nb, **cfg):
    got = display_device(T, eng, spec_t, **cfg)
    want = want_rows(spec, lo, nb, cfg)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert got.tobytes() == want.tobytes(), (cfg, np.argwhere(got.view(np.uint8) != want.view(np.uint8))[:8])


def caller_spectra(T, a):
    return T.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda:0")


@pytest.fixture(scope="module")
def engine_spectra(S, O, T):
    """Case 1's spectra: 5 CS8 streams at N = 16384 through the engine's own spectrum kernel (shared, read-only)."""
    n, B = 16384, 5
    raw = np.stack([O.synth_frames(1, n, O.CS8, tone_hz=700.0 * b - 1500.0, fs=FS, seed=40 + b)[0] for b in range(B)])
    return n, B, raw


FULL_WIDTHS = (1024, 1000, 16384, 20000)


@pytest.mark.parametrize("fmt", (dc.DB_F32, dc.U8), ids=("f32", "u8"))
@pytest.mark.parametrize("W", FULL_WIDTHS)
def test_engine_spectra_full_span_max(S, T, engine_spectra, W, fmt):
    """process_device then display_device with no synchronisation between: the rows are those of that call's spectra."""
    n, B, raw = engine_spectra
    eng = engine(S, n, B)
    iq = T.from_numpy(raw).to("cuda:0")
    spec = T.zeros((B, n), dtype=T.float32, device="cuda:0")
    out = T.full((B * W * 4 + GUARD,), 0xAA, dtype=T.uint8, device="cuda:0")
    eng.set_display(span=S.DISPLAY_SPAN_FULL, width=W, reduce=S.DISPLAY_MAX, format=fmt, db_min=DB_MIN, db_max=DB_MAX)
    assert eng.display_geometry() == (0, n, W * (1 if fmt == dc.U8 else 4))
    T.cuda.synchronize()
    eng.process_device(iq.data_ptr(), S.CS8, S.STAGE_SPECTRUM, spec.data_ptr(), None, None, 1000)
    eng.display_device(spec.data_ptr(), out.data_ptr())
    eng.synchronize()
    rb = W * (1 if fmt == dc.U8 else 4)
    got = out.cpu().numpy()
    want = dc.rows(spec.cpu().numpy(), 0, n, W, dc.MAX, fmt, DB_MIN, DB_MAX)
    assert got[:B * rb].tobytes() == want.tobytes()
    assert np.all(got[B * rb:] == 0xAA)
    eng.close()


@pytest.mark.parametrize("W", (64, 4099, 5000))
def test_odd_n(S, O, T, W):
    n, B = 4099, 3
    raw = np.stack([O.synth_frames(1, n, O.CS8, tone_hz=300.0 * b, fs=FS, seed=7 + b)[0] for b in range(B)])
    eng = engine(S, n, B)
    iq = T.from_numpy(raw).to("cuda:0")
    spec_t = T.zeros((B, n), dtype=T.float32, device="cuda:0")  # bin N-1 of an odd N is never written
    T.cuda.synchronize()
    eng.process_device(iq.data_ptr(), S.CS8, S.STAGE_SPECTRUM, spec_t.data_ptr(), None, None, 1000)
    eng.synchronize()
    spec = spec_t.cpu().numpy()
    for fmt in (dc.DB_F32, dc.U8):
        check_exact(T, eng, spec_t, spec, 0, n, span=S.DISPLAY_SPAN_FULL, width=W, reduce=dc.MAX, format=fmt)
    eng.close()


@pytest.mark.parametrize("n_bins", (81, 16383))
@pytest.mark.parametrize("first_bin", (1, 8151, 8153))
def test_misaligned_spans_and_dense_rows(S, T, first_bin, n_bins):
    """Spans that start off a 16-byte boundary and rows of 7, 81, ... bytes: exact rows, nothing written beyond them.
    The powers are exactly summable, so MEAN has one right answer too."""
    n, B = 16384, 9
    spec = dc.summable_spectra(B, n, seed=first_bin + n_bins)
    spec_t = caller_spectra(T, spec)
    eng = engine(S, n, B)
    for W in (7, 64, 81, 128):
        cfg = dict(span=S.DISPLAY_SPAN_BINS, first_bin=first_bin, n_bins=n_bins, width=W, format=dc.U8, db_min=-30.0,
                   db_max=10.0)
        if first_bin + n_bins > n:  # resolved at the call: rejected, nothing enqueued
            eng.set_display(**cfg)
            invalid(S, eng.display_geometry)
            out = T.full((B * W,), 0xAA, dtype=T.uint8, device="cuda:0")
            T.cuda.synchronize()
            invalid(S, eng.display_device, spec_t.data_ptr(), out.data_ptr())
            eng.synchronize()
            assert bool((out == 0xAA).all())
            continue
        for reduce in (dc.MAX, dc.MEAN):
            got = display_device(T, eng, spec_t, reduce=reduce, **cfg)
            want = dc.rows(spec, first_bin, n_bins, W, reduce, dc.U8, -30.0, 10.0)
            assert got.tobytes() == want.tobytes(), (W, reduce)
    eng.close()


@pytest.mark.parametrize("W", (7, 1500))
def test_column_boundaries(S, T, W):
    """Row b is zero except a 1.0 at bin b: exactly the columns whose range holds bin b light up."""
    n = B = 1000
    spec = np.eye(n, dtype=np.float32)
    eng = engine(S, n, B)
    got = display_device(T, eng, caller_spectra(T, spec), span=S.DISPLAY_SPAN_FULL, width=W, reduce=dc.MAX, format=dc.U8)
    bounds = dc.column_bounds(n, W)
    first, count = bounds[:-1], np.maximum(bounds[1:] - bounds[:-1], 1)
    bins = np.arange(n)[:, None]
    lit = (first[None, :] <= bins) & (bins < (first + count)[None, :])
    assert lit.sum(axis=1).min() >= 1
    np.testing.assert_array_equal(got, np.where(lit, 255, 0).astype(np.uint8))
    eng.close()


def test_focus_span_follows_the_statistics_window(S, T):
    """FOCUS is sdrg_focus_window of the statistics' configuration at each call: 81 bins at 16384 / 2 MHz / 5 kHz, it
    follows setFrequencyFocusRange, is the whole band for a focus wider than the band (the window is clamped, not
    empty) and fails the call where the window is empty (0 kHz)."""
    n, B = 16384, 4
    spec = dc.noise_spectra(B, n, seed=5)
    spec_t = caller_spectra(T, spec)
    eng = engine(S, n, B, focus=5)
    for focus in (5, 50):
        if focus != 5:
            eng.setFrequencyFocusRange(focus)
        lo, nb = S.focus_window(FS, n, focus)
        assert nb > 0
        cfg = dict(width=64, reduce=dc.MAX, format=dc.DB_F32)
        got = display_device(T, eng, spec_t, span=S.DISPLAY_SPAN_FOCUS, **cfg)
        assert eng.display_geometry() == (lo, nb, 64 * 4)
        as_bins = display_device(T, eng, spec_t, span=S.DISPLAY_SPAN_BINS, first_bin=lo, n_bins=nb, **cfg)
        assert got.tobytes() == as_bins.tobytes()
        assert got.tobytes() == dc.rows(spec, lo, nb, 64, dc.MAX, dc.DB_F32).tobytes()
    assert S.focus_window(FS, n, 5) == (8151, 81)
    eng.set_display(span=S.DISPLAY_SPAN_FOCUS, width=64)
    # a focus wider than the band: the statistics clamp their window to the band (fft_process.cpp:131-140), which
    # sdrg_focus_window reports and sdrg_engine_gather_focus packs, so the display shows the whole band
    eng.setFrequencyFocusRange(2000)
    assert S.focus_window(FS, n, 2000) == (0, n)
    assert eng.display_geometry() == (0, n, 64 * 4)
    got = display_device(T, eng, spec_t, span=S.DISPLAY_SPAN_FOCUS, width=64)
    assert got.tobytes() == dc.rows(spec, 0, n, 64, dc.MAX, dc.DB_F32).tobytes()
    # the window is empty at 0 kHz: rejected at the call
    eng.setFrequencyFocusRange(0)
    assert S.focus_window(FS, n, 0)[1] == 0
    invalid(S, eng.display_geometry)
    out = T.zeros((B * 64,), dtype=T.float32, device="cuda:0")
    T.cuda.synchronize()
    invalid(S, eng.display_device, spec_t.data_ptr(), out.data_ptr())
    eng.close()


@pytest.mark.parametrize("n,B,W,fmt", [(1, 3, 1, dc.DB_F32), (1, 3, 4, dc.U8), (64, 3, 1024, dc.DB_F32),
                                       (2 ** 20, 1, 64, dc.DB_F32), (2 ** 20, 1, 2 ** 20, dc.U8)],
                         ids=("1to1", "1to4", "64to1024", "1Mto64", "1Mto1M-u8"))
def test_sizes(S, T, n, B, W, fmt):
    spec = dc.noise_spectra(B, n, seed=n + W)
    eng = engine(S, n, B)
    check_exact(T, eng, caller_spectra(T, spec), spec, 0, n, span=S.DISPLAY_SPAN_FULL, width=W, reduce=dc.MAX, format=fmt)
    eng.close()


@pytest.mark.parametrize("W", (1280, 320, 100), ids=("direct", "shuffle", "tiled"))
def test_values(S, T, W):
    """Zeros, denormals, FLT_MAX, +inf and the boundary sweep's powers through the dB expression and the quantiser, at
    W = nb (every value its own column) and through the two reducing kernels."""
    n, B = 1280, 2
    vals = np.concatenate([dc.special_powers(), dc.boundary_sweep_powers()])
    spec = np.zeros((B, n), np.float32)
    spec[0, :vals.size] = vals
    spec[1, :vals.size] = vals[::-1]
    spec_t = caller_spectra(T, spec)
    eng = engine(S, n, B)
    check_exact(T, eng, spec_t, spec, 0, n, span=S.DISPLAY_SPAN_FULL, width=W, reduce=dc.MAX, format=dc.DB_F32)
    for lo_db, hi_db in ((DB_MIN, DB_MAX), (dc.SWEEP_DB_MIN, dc.SWEEP_DB_MAX)):
        got = display_device(T, eng, spec_t, span=S.DISPLAY_SPAN_FULL, width=W, reduce=dc.MAX, format=dc.U8, db_min=lo_db,
                             db_max=hi_db)
        want = dc.rows(spec, 0, n, W, dc.MAX, dc.U8, lo_db, hi_db)
        assert got.tobytes() == want.tobytes(), (lo_db, hi_db)
    if W == n:  # a zero power is about -200 dB and code 0, +inf is +inf dB and code 255
        d = display_device(T, eng, spec_t, span=S.DISPLAY_SPAN_FULL, width=W, reduce=dc.MAX, format=dc.DB_F32)
        assert abs(d[0, 0] + 200.0) < 1e-3 and np.isposinf(d[0, dc.special_powers().size - 1])
        assert got[0, 0] == 0 and got[0, dc.special_powers().size - 1] == 255
    eng.close()


@pytest.mark.parametrize("n,B,W", [(16384, 3, 1000), (16384, 3, 1024), (2 ** 20, 1, 64)], ids=("tiled", "shuffle", "16384-per-column"))
def test_mean_exactly_summable(S, T, n, B, W):
    """Powers k * 2^-10: every double sum is exact in any order, so the rows are bit-exact.  At 2^20 -> 64 a column holds
    16384 bins: a float accumulator rounds, a double one does not."""
    spec = dc.summable_spectra(B, n, seed=n + W)
    spec_t = caller_spectra(T, spec)
    eng = engine(S, n, B)
    for fmt in (dc.DB_F32, dc.U8):
        got = display_device(T, eng, spec_t, span=S.DISPLAY_SPAN_FULL, width=W, reduce=dc.MEAN, format=fmt, db_min=-10.0,
                             db_max=10.0)
        want = dc.rows(spec, 0, n, W, dc.MEAN, fmt, -10.0, 10.0)
        assert got.tobytes() == want.tobytes(), fmt
    eng.close()


@pytest.mark.parametrize("W", FULL_WIDTHS)
def test_mean_engine_spectra(S, T, engine_spectra, W):
    """|got - want| <= 6e-7 + 4 spacing(|want|): two double sums of a column can differ by a float ulp of the mean
    (5.2e-7 dB), then come the roundings of log10f and of the multiply.  Codes differ by at most 1, and at least 99 % of
    the columns are bit-equal."""
    n, B, raw = engine_spectra
    eng = engine(S, n, B)
    iq = T.from_numpy(raw).to("cuda:0")
    spec_t = T.zeros((B, n), dtype=T.float32, device="cuda:0")
    T.cuda.synchronize()
    eng.process_device(iq.data_ptr(), S.CS8, S.STAGE_SPECTRUM, spec_t.data_ptr(), None, None, 1000)
    eng.synchronize()
    spec = spec_t.cpu().numpy()
    cfg = dict(span=S.DISPLAY_SPAN_FULL, width=W, reduce=dc.MEAN)
    got = display_device(T, eng, spec_t, format=dc.DB_F32, **cfg)
    want = dc.rows(spec, 0, n, W, dc.MEAN, dc.DB_F32)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    bound = 6e-7 + 4 * np.spacing(np.abs(want)).astype(np.float64)
    print(f"W={W}: max |got - want| {err.max():.3e}, bit-equal {np.mean(got.view(np.uint32) == want.view(np.uint32)):.5f}")
    assert np.all(err <= bound), float((err - bound).max())
    assert np.mean(got.view(np.uint32) == want.view(np.uint32)) >= 0.99
    got8 = display_device(T, eng, spec_t, format=dc.U8, **cfg)
    want8 = dc.code(want, DB_MIN, DB_MAX)
    assert np.abs(got8.astype(np.int32) - want8.astype(np.int32)).max() <= 1
    assert np.mean(got8 == want8) >= 0.99
    eng.close()


def test_pipelined_calls_equal_the_joined_schedule(S, O, T):
    """PIPELINE_ON | PIPELINE_STATS_ASYNC, two rotating spectra buffers, four calls each followed by display_device:
    the rows are those of the joined schedule."""
    n, B, F, W = 16384, 4, 4, 1000
    raws = np.stack([np.stack([O.synth_frames(1, n, O.CS8, tone_hz=400.0 * b - 900.0, fs=FS, seed=100 * f + b)[0]
                               for b in range(B)]) for f in range(F)])

    def run(mode):
        eng = engine(S, n, B)
        eng.set_pipelining(mode)
        eng.set_display(span=S.DISPLAY_SPAN_FULL, width=W, reduce=S.DISPLAY_MAX, format=S.DISPLAY_DB_F32)
        iq = [T.from_numpy(raws[f]).to("cuda:0") for f in range(F)]
        spec = [T.zeros((B, n), dtype=T.float32, device="cuda:0") for _ in range(2)]
        rec = [T.zeros((B, S.RECORD_DTYPE.itemsize), dtype=T.uint8, device="cuda:0") for _ in range(2)]
        pcm = [T.zeros((B, eng.pcm_len), dtype=T.int16, device="cuda:0") for _ in range(F)]
        rows = [T.zeros((B, W), dtype=T.float32, device="cuda:0") for _ in range(F)]
        T.cuda.synchronize()
        for f in range(F):
            eng.process_device(iq[f].data_ptr(), S.CS8, S.STAGE_ALL, spec[f % 2].data_ptr(), rec[f % 2].data_ptr(),
                               pcm[f].data_ptr(), 1000 + 10 * f)
            eng.display_device(spec[f % 2].data_ptr(), rows[f].data_ptr())
        eng.synchronize()
        out = T.stack(rows).cpu().numpy()
        last = spec[(F - 1) % 2].cpu().numpy()
        eng.close()
        return out, last

    joined, last = run(S.PIPELINE_OFF)
    piped, _ = run(S.PIPELINE_ON | S.PIPELINE_STATS_ASYNC)
    assert piped.tobytes() == joined.tobytes()
    assert joined[F - 1].tobytes() == dc.rows(last, 0, n, W, dc.MAX, dc.DB_F32).tobytes()
    assert len({joined[f].tobytes() for f in range(F)}) == F  # four different frames


def test_wait_outputs_orders_a_consumer_stream(S, O, T):
    """A consumer on another stream follows the display rows through sdrg_engine_wait_outputs, with no host
    synchronisation between the calls and its copy."""
    n, B, W = 16384, 64, 1024
    raw = np.stack([O.synth_frames(1, n, O.CS8, tone_hz=100.0 * b - 3000.0, fs=FS, seed=300 + b)[0] for b in range(B)])
    eng = engine(S, n, B)
    eng.set_display(span=S.DISPLAY_SPAN_FULL, width=W, reduce=S.DISPLAY_MAX, format=S.DISPLAY_U8, db_min=DB_MIN, db_max=DB_MAX)
    iq = T.from_numpy(raw).to("cuda:0")
    spec = T.zeros((B, n), dtype=T.float32, device="cuda:0")
    rows = T.zeros((B, W), dtype=T.uint8, device="cuda:0")
    copy = T.zeros((B, W), dtype=T.uint8, device="cuda:0")
    consumer = T.cuda.Stream("cuda:0")
    T.cuda.synchronize()
    for k in range(3):  # the second and third wait reuse the engine's marker
        eng.process_device(iq.data_ptr(), S.CS8, S.STAGE_SPECTRUM, spec.data_ptr(), None, None, 1000 + k)
        eng.display_device(spec.data_ptr(), rows.data_ptr())
        eng.wait_outputs(consumer.cuda_stream)
        with T.cuda.stream(consumer):
            copy.copy_(rows)
    consumer.synchronize()
    eng.synchronize()
    assert copy.cpu().numpy().tobytes() == dc.rows(spec.cpu().numpy(), 0, n, W, dc.MAX, dc.U8, DB_MIN, DB_MAX).tobytes()
    eng.close()


def test_host_path(S, O):
    """process_host(spectra = NULL) then display() gives the rows of the spectra an identical engine returns, and
    display(spectra) the rows of caller spectra; display() needs such a call, at the frame size still in force."""
    n, B, W = 4096, 3, 500
    raw = np.stack([O.synth_frames(1, n, O.CS8, tone_hz=900.0 * b - 800.0, fs=FS, seed=21 + b)[0] for b in range(B)])
    ref = engine(S, n, B)
    spec, _, _ = ref.process(raw, fmt=S.CS8, stages=S.STAGE_SPECTRUM | S.STAGE_STATS, now_ms=1000)
    ref.close()
    eng = engine(S, n, B)
    eng.set_display(span=S.DISPLAY_SPAN_FULL, width=W, reduce=S.DISPLAY_MAX, format=S.DISPLAY_U8, db_min=DB_MIN, db_max=DB_MAX)
    invalid(S, eng.display)  # no process_host call yet
    rec = np.zeros(B, S.RECORD_DTYPE)
    rc = S.load().sdrg_engine_process_host(eng._h, raw.ctypes.data_as(ctypes.c_void_p), S.CS8, S.STAGE_SPECTRUM | S.STAGE_STATS,
                                           None, rec.ctypes.data_as(ctypes.c_void_p), None, 1000)
    assert rc == 0
    want = dc.rows(spec, 0, n, W, dc.MAX, dc.U8, DB_MIN, DB_MAX)
    got = eng.display()
    assert got.dtype == np.uint8 and got.shape == (B, W) and got.tobytes() == want.tobytes()
    eng.set_display(span=S.DISPLAY_SPAN_FULL, width=W, reduce=S.DISPLAY_MAX, format=S.DISPLAY_DB_F32)
    got = eng.display()
    assert got.dtype == np.float32 and got.tobytes() == dc.rows(spec, 0, n, W, dc.MAX, dc.DB_F32).tobytes()
    other = dc.noise_spectra(B, n, seed=3)
    assert eng.display(other).tobytes() == dc.rows(other, 0, n, W, dc.MAX, dc.DB_F32).tobytes()
    assert eng.display().tobytes() == got.tobytes()  # the caller's spectra went through a buffer of their own
    eng.setSamplesPerReading(2048)
    invalid(S, eng.display)  # the spectra on the device are 4096 bins wide
    small = dc.noise_spectra(B, 2048, seed=4)
    assert eng.display(small).tobytes() == dc.rows(small, 0, 2048, W, dc.MAX, dc.DB_F32).tobytes()
    eng.close()


def test_contract(S, T):
    n, B = 4096, 2
    spec = dc.noise_spectra(B, n, seed=9)
    spec_t = caller_spectra(T, spec)
    eng = engine(S, n, B)
    out = T.zeros((B * 256,), dtype=T.float32, device="cuda:0")
    T.cuda.synchronize()
    invalid(S, eng.display_geometry)  # before any set_display
    invalid(S, eng.display_config)
    invalid(S, eng.display_device, spec_t.data_ptr(), out.data_ptr())
    invalid(S, eng.display, spec)
    good = dict(span=S.DISPLAY_SPAN_BINS, first_bin=3000, n_bins=1000, width=256, reduce=S.DISPLAY_MAX,
                format=S.DISPLAY_DB_F32, db_min=0.0, db_max=0.0)  # the dB range matters for U8 only
    eng.set_display(**good)
    assert eng.display_config() == good
    for bad in (dict(span=3), dict(reduce=2), dict(format=-1), dict(width=0), dict(width=2 ** 20 + 1), dict(first_bin=-1),
                dict(n_bins=0), dict(format=S.DISPLAY_U8), dict(format=S.DISPLAY_U8, db_min=1.0, db_max=float("inf")),
                dict(format=S.DISPLAY_U8, db_min=float("nan"), db_max=0.0)):
        invalid(S, eng.set_display, **{**good, **bad})
        assert eng.display_config() == good  # a rejected configuration leaves the previous one in force
    invalid(S, eng.display_device, None, out.data_ptr())
    invalid(S, eng.display_device, spec_t.data_ptr(), None)
    assert eng.display_geometry() == (3000, 1000, 1024)
    want = dc.rows(spec, 3000, 1000, 256, dc.MAX, dc.DB_F32)
    assert eng.display(spec).tobytes() == want.tobytes()
    eng.setSamplesPerReading(3500)  # the span [3000, 4000) no longer fits: fails at the call, enqueues nothing
    invalid(S, eng.display_geometry)
    invalid(S, eng.display_device, spec_t.data_ptr(), out.data_ptr())
    eng.synchronize()
    assert float(out.abs().max()) == 0.0
    eng.setSamplesPerReading(n)  # the next valid call works
    eng.display_device(spec_t.data_ptr(), out.data_ptr())
    eng.synchronize()
    assert out.cpu().numpy().reshape(B, 256).tobytes() == want.tobytes()
    eng.close()
