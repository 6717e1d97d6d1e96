"""GPU tests of the peak table stage (csrc/peaks.hip, sdrg_engine_peaks_*): the K strongest local maxima of each row
against the NumPy restatement in tests/peaks_cases.py.  Every comparison is of the bytes of both outputs (the stage is
specified operation by operation: no tolerances), and 64 guard bytes follow each buffer.

The launcher picks one of three kernels by the span: one wave (nb <= 2048), 1024 threads on an LDS copy (nb <= 16384),
1024 threads on the row in memory with the candidate scan in tiles of 16384 bins (above).  The kernel turns the
threshold into a lowest power by a search (the restatement evaluates every candidate's log), and its candidate scan tests
j +- 1 .. 3 first, then the rest of the bin's 32-bin (64 from memory) block, whole blocks through their maxima and the
partial blocks at the window's ends: the shapes below put ties, plateaus and window ends on each of those seams, and
thresholds on a candidate's own snr and its float neighbours."""
import ctypes

import numpy as np
import pytest

import display_cases as dc
import integrate_cases as ic
import peaks_cases as pc

pytestmark = pytest.mark.gpu

FS = 2_000_000
GUARD = 64
f32 = np.float32
INF = float("inf")


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


def caller_spectra(T, a):
    return T.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda:0")


def out_buffers(T, B, K):
    pk = T.full((B * K * 16 + GUARD,), 0xAA, dtype=T.uint8, device="cuda:0")
    sm = T.full((B * 16 + GUARD,), 0xAA, dtype=T.uint8, device="cuda:0")
    return pk, sm


def read_buffers(pk_t, sm_t, B, K):
    pk, sm = pk_t.cpu().numpy(), sm_t.cpu().numpy()
    assert np.all(pk[B * K * 16:] == 0xAA) and np.all(sm[B * 16:] == 0xAA), "bytes written past the tables"
    return pk[:B * K * 16].view(pc.PEAK_DTYPE).reshape(B, K), sm[:B * 16].view(pc.SUMMARY_DTYPE)


def peaks_device(T, eng, spec_t, **cfg):
    """set_peaks(**cfg), peaks_device into 0xAA-filled buffers with guard bytes; (peaks [B][K], summary [B])."""
    eng.set_peaks(**cfg)
    B, K = eng.n_streams, cfg["max_peaks"]
    pk_t, sm_t = out_buffers(T, B, K)
    T.cuda.synchronize()
    eng.peaks_device(spec_t.data_ptr(), pk_t.data_ptr(), sm_t.data_ptr())
    eng.synchronize()
    return read_buffers(pk_t, sm_t, B, K)


def same(got, want, what=None):
    pk, sm = got
    wpk, wsm = want
    assert pk.shape == wpk.shape and sm.shape == wsm.shape
    assert sm.tobytes() == wsm.tobytes(), (what, [(int(b), sm[b], wsm[b]) for b in np.flatnonzero(sm != wsm)[:3]])
    bad = np.argwhere(pk != wpk)
    assert pk.tobytes() == wpk.tobytes(), (what, [(tuple(i), pk[tuple(i)], wpk[tuple(i)]) for i in bad[:3]])


def check(T, S, eng, spec_t, spec, lo, nb, **cfg):
    cfg.setdefault("span", S.DISPLAY_SPAN_FULL)
    got = peaks_device(T, eng, spec_t, **cfg)
    same(got, pc.tables(spec, lo, nb, cfg["min_separation"], cfg["max_peaks"], cfg["threshold_db"]), cfg)
    return got


SEPARATIONS = (1, 2, 63, 64, 65, 4096)


@pytest.fixture(scope="module")
def seam_rows():
    """Rows of 4230 bins (shared, read-only) that put ties on the seams of the candidate scan."""
    n = 4230
    rows = {}
    for d in SEPARATIONS:
        r = np.zeros((8, n), np.float32)
        r[0, 10] = r[0, 10 + d] = 5.0              # equal maxima exactly d apart: the second is inside the window
        r[1, 10] = r[1, 10 + d + 1] = 5.0          # d + 1 apart: both
        r[2, 60:70] = 2.0                          # a plateau across a 64-bin (and 32-bin) block boundary
        r[2, 130:134] = 2.0                        # and one across a 16-byte boundary only
        r[2, 1000] = np.nextafter(f32(2.0), f32(0))
        r[3, 0] = r[3, n - 1] = 3.0                # candidates at j = 0 and j = nb - 1
        r[4] = np.arange(n, 0, -1)                 # a falling skirt: its top only
        r[4, 2000] = r[4, 1999]                    # with a two-bin shelf in it
        r[5] = np.arange(n)                        # a rising ramp: the last bin only
        r[6] = 0.75                                # a constant row: bin 0
        r[7] = pc.quantised_rows(1, n, seed=d)[0]
        rows[d] = r
    return n, rows


@pytest.mark.parametrize("d", SEPARATIONS)
def test_ties_and_spacing(S, T, seam_rows, d):
    n, rows = seam_rows
    spec = rows[d]
    B = spec.shape[0]
    eng = engine(S, n, B)
    spec_t = caller_spectra(T, spec)
    pk, sm = check(T, S, eng, spec_t, spec, 0, n, max_peaks=64, min_separation=d, threshold_db=-INF)
    assert pk["bin"][0][pk["power"][0] == 5].tolist() == [10]
    assert pk["bin"][1][pk["power"][1] == 5].tolist() == [10, 10 + d + 1]
    assert pk["bin"][3, :3].tolist() == [0, n - 1, -1]
    assert sm["n_above"][4:7].tolist() == [1, 1, 1] and pk["bin"][4:7, 0].tolist() == [0, n - 1, 0]
    if d == 1:
        assert sm["n_above"][7] > 64 and sm["count"][7] == 64
    check(T, S, eng, spec_t, spec, 0, n, max_peaks=3, min_separation=d, threshold_db=0.0)
    # the same rows from a span that starts off 16 bytes and ends inside a block
    check(T, S, eng, spec_t, spec, 3, n - 100, span=S.DISPLAY_SPAN_BINS, first_bin=3, n_bins=n - 100, max_peaks=64,
          min_separation=d, threshold_db=-INF)
    eng.close()


@pytest.mark.parametrize("d", SEPARATIONS)
def test_quantised_rows(S, T, d):
    """B = 5, N = 1024, eight levels: ties everywhere; 4096 is d > nb."""
    n, B = 1024, 5
    spec = pc.quantised_rows(B, n, seed=100 + d)
    eng = engine(S, n, B)
    spec_t = caller_spectra(T, spec)
    for K, thr in ((64, -INF), (3, 2.0)):
        check(T, S, eng, spec_t, spec, 0, n, max_peaks=K, min_separation=d, threshold_db=thr)
    eng.close()


def test_ordering_and_table_sizes(S, T):
    """Equal powers come lower bin first, ulp neighbours that share a dB value by power; max_peaks 1, 3 and 64 with three
    candidates above the threshold."""
    n, B = 256, 2
    a, b = pc.ulp_pair_sharing_db()
    spec = np.zeros((B, n), np.float32)
    spec[0, [200, 40, 120]] = 7.0
    spec[1, [30, 90, 150]] = a, b, a
    eng = engine(S, n, B)
    spec_t = caller_spectra(T, spec)
    for K in (1, 3, 64):
        pk, sm = check(T, S, eng, spec_t, spec, 0, n, max_peaks=K, min_separation=4, threshold_db=10.0)
        assert sm["n_above"].tolist() == [3, 3] and sm["count"].tolist() == [min(K, 3)] * 2
        assert pk["bin"][:, 0].tolist() == [40, 90]
    pk, _ = check(T, S, eng, spec_t, spec, 0, n, max_peaks=3, min_separation=4, threshold_db=10.0)
    assert pk["bin"].tolist() == [[40, 120, 200], [90, 30, 150]]
    assert pk["db"][1, 0] == pk["db"][1, 1] and pk["power"][1, 0] > pk["power"][1, 1]
    eng.close()


def test_threshold(S, T):
    """A candidate whose snr equals the threshold exactly is above, one float above it is not; -inf takes every
    candidate; zeros (floor 0, -200 dB), subnormals, two +inf bins, and a row more than half +inf (snr NaN: nothing)."""
    n, B, d = 300, 6, 5
    spec = np.zeros((B, n), np.float32)
    spec[0] = pc.noise_rows(1, n, seed=7)[0]
    spec[0, 77] = 0.25
    # row 1: zeros
    spec[2] = np.arange(1, n + 1).astype(np.uint32).view(np.float32)  # subnormals 1 .. 300 ulps
    spec[2, 100] = np.array([0x7FFFFF], np.uint32).view(np.float32)[0]
    spec[3] = pc.noise_rows(1, n, seed=8)[0]
    spec[3, [50, 250]] = np.inf
    spec[4, :200] = np.inf
    spec[4, 200:] = pc.noise_rows(1, 100, seed=9)[0]
    spec[5, ::2] = np.inf  # exactly half: rank nb / 2 is +inf
    eng = engine(S, n, B)
    spec_t = caller_spectra(T, spec)
    snr = f32(dc.db(f32(0.25)) - dc.db(pc.floor_power(spec[0])))
    for thr, n0 in ((snr, 1), (np.nextafter(snr, f32(INF)), 0), (np.nextafter(snr, f32(-INF)), 1)):
        pk, sm = check(T, S, eng, spec_t, spec, 0, n, max_peaks=4, min_separation=d, threshold_db=float(thr))
        assert sm["n_above"][0] == n0 and (pk["bin"][0, 0] == 77) == bool(n0)
        if n0:
            assert pk["snr_db"][0, 0] == snr
        assert sm["n_above"][1] == 0 and sm["floor_power"][1] == 0 and abs(sm["floor_db"][1] + 200.0) < 1e-3
        assert sm["n_above"][3] == 2 and pk["bin"][3, :2].tolist() == [50, 250] and np.all(np.isposinf(pk["snr_db"][3, :2]))
        assert np.isposinf(sm["floor_db"][4]) and sm["n_above"][4] == 0 and sm["n_above"][5] == 0
    pk, sm = check(T, S, eng, spec_t, spec, 0, n, max_peaks=64, min_separation=d, threshold_db=-INF)
    assert pk["bin"][1].tolist() == [0] + [-1] * 63 and pk["snr_db"][1, 0] == 0  # the zero row: bin 0, 0 dB over the floor
    assert sm["n_above"][2] >= 2 and pk["bin"][2, 0] == 100
    check(T, S, eng, spec_t, spec, 0, n, max_peaks=2, min_separation=1, threshold_db=0.0)
    eng.close()


@pytest.mark.parametrize("nb", (1000, 1001, 5000, 5001))
def test_floor(S, T, nb):
    """The exact select: even and odd spans, rows that are mostly the median's value, rows whose values share all high
    bits (the first digit starts at the highest bit that differs), a row of one value and a row of two."""
    n, B = 5008, 6
    rng = np.random.default_rng(nb)
    spec = pc.noise_rows(B, n, seed=nb)
    spec[1] = rng.choice(np.array([0.5, 0.5, 0.5, 0.25, 1.0], np.float32), size=n)  # duplicates of the median
    spec[2] = pc.shared_high_bits_rows(1, n, seed=nb)[0]
    spec[3] = 0.125
    spec[4] = rng.choice(np.array([0.125, np.nextafter(f32(0.125), f32(1))], np.float32), size=n)
    spec[5] = np.sort(spec[5])
    eng = engine(S, n, B)
    spec_t = caller_spectra(T, spec)
    _, sm = check(T, S, eng, spec_t, spec, 3, nb, span=S.DISPLAY_SPAN_BINS, first_bin=3, n_bins=nb, max_peaks=8,
                  min_separation=8, threshold_db=3.0)
    assert sm["floor_power"].tolist() == [np.sort(r[3:3 + nb])[nb // 2] for r in spec]
    eng.close()


SPANS = [(1, 1, 6), (2, 2, 9), (81, 3, 17), (2048, 5, 9), (2049, 1, 6), (16384, 3, 6), (16385, 2, 6), (65536, 5, 1)]


@pytest.mark.parametrize("nb,lo,B", SPANS, ids=[f"{nb}at{lo}x{B}" for nb, lo, B in SPANS])
def test_spans(S, T, nb, lo, B):
    """BINS spans that start 1, 2, 3 and 5 floats off a 16-byte boundary, at the sizes where the launcher changes kernel
    (2048 | 2049, 16384 | 16385) and over four tiles; the bins outside the span hold larger powers than any inside."""
    n = nb + 8
    spec = pc.noise_rows(B, n, seed=nb, tones=min(20, nb // 4))
    spec[:, :lo] = 50.0
    spec[:, lo + nb:] = 60.0
    if B > 1:
        spec[1] = pc.quantised_rows(1, n, seed=nb)[0]
    eng = engine(S, n, B)
    spec_t = caller_spectra(T, spec)
    for d, K, thr in ((8, 16, 10.0), (4096, 64, -INF), (1, 64, 6.0)):
        pk, _ = check(T, S, eng, spec_t, spec, lo, nb, span=S.DISPLAY_SPAN_BINS, first_bin=lo, n_bins=nb, max_peaks=K,
                      min_separation=d, threshold_db=thr)
        assert np.all((pk["bin"] == -1) | ((pk["bin"] >= lo) & (pk["bin"] < lo + nb)))
    eng.close()


@pytest.mark.parametrize("n,B", [(1001, 9), (4099, 17), (2 ** 20, 1)], ids=("1001", "4099", "1M"))
def test_full_span(S, T, n, B):
    """Odd N (element N - 1 is data) and the largest frame."""
    spec = pc.noise_rows(B, n, seed=n, tones=20)
    spec[0, n - 1] = 30.0
    eng = engine(S, n, B)
    spec_t = caller_spectra(T, spec)
    pk, _ = check(T, S, eng, spec_t, spec, 0, n, max_peaks=16, min_separation=8, threshold_db=10.0)
    assert pk["bin"][0, 0] == n - 1
    check(T, S, eng, spec_t, spec, 0, n, max_peaks=64, min_separation=4096, threshold_db=-INF)
    eng.close()


def test_focus_span_follows_the_statistics_window(S, T):
    n, B = 16384, 9
    spec = pc.noise_rows(B, n, seed=5, tones=40)
    spec_t = caller_spectra(T, spec)
    eng = engine(S, n, B, focus=5)
    cfg = dict(max_peaks=8, min_separation=2, threshold_db=3.0)
    for focus in (5, 50, 2000):  # 2000 kHz: wider than the band, the window is the whole band
        if focus != 5:
            eng.setFrequencyFocusRange(focus)
        lo, nb = S.focus_window(FS, n, focus)
        got = check(T, S, eng, spec_t, spec, lo, nb, span=S.DISPLAY_SPAN_FOCUS, **cfg)
        as_bins = peaks_device(T, eng, spec_t, span=S.DISPLAY_SPAN_BINS, first_bin=lo, n_bins=nb, **cfg)
        same(got, as_bins)
    assert S.focus_window(FS, n, 5) == (8151, 81)
    eng.set_peaks(span=S.DISPLAY_SPAN_FOCUS, **cfg)
    eng.setFrequencyFocusRange(0)  # an empty window: rejected at the call, nothing enqueued
    pk_t, sm_t = out_buffers(T, B, 8)
    T.cuda.synchronize()
    invalid(S, eng.peaks_device, spec_t.data_ptr(), pk_t.data_ptr(), sm_t.data_ptr())
    eng.synchronize()
    assert bool((pk_t == 0xAA).all()) and bool((sm_t == 0xAA).all())
    eng.close()


# ---- engine composition -------------------------------------------------------------------------------------------

TONE_BINS = (10, -20, 30, -40, 50)


def tone_frames(O, n, F, seed=0):
    """[F][B][...] CS8 frames, stream b a tone exactly on bin n / 2 + TONE_BINS[b]."""
    return np.stack([np.stack([O.synth_frames(1, n, O.CS8, tone_hz=k * FS / n, fs=FS, seed=seed + 10 * f + b)[0]
                               for b, k in enumerate(TONE_BINS)]) for f in range(F)])


def test_process_then_peaks_then_integrate_then_peaks(S, O, T):
    """process_device -> peaks_device on its spectra with no synchronisation between: the strongest peak is the tone's
    bin; -> integrate_device (MEAN, 4) -> peaks_device on the integrated rows."""
    n, B, F, K = 16384, len(TONE_BINS), 4, 16
    raws = tone_frames(O, n, F)
    eng = engine(S, n, B)
    eng.set_peaks(span=S.DISPLAY_SPAN_FULL, max_peaks=K, min_separation=8, threshold_db=10.0)
    eng.set_integration(S.INTEGRATE_MEAN, period=4)
    iq = [T.from_numpy(raws[f]).to("cuda:0") for f in range(F)]
    spec = [T.zeros((B, n), dtype=T.float32, device="cuda:0") for _ in range(F)]
    integ = [T.zeros((B, n), dtype=T.float32, device="cuda:0") for _ in range(F)]
    outs = [(out_buffers(T, B, K), out_buffers(T, B, K)) for _ in range(F)]
    T.cuda.synchronize()
    for f in range(F):
        eng.process_device(iq[f].data_ptr(), S.CS8, S.STAGE_SPECTRUM, spec[f].data_ptr(), None, None, 1000 + f)
        eng.peaks_device(spec[f].data_ptr(), outs[f][0][0].data_ptr(), outs[f][0][1].data_ptr())
        eng.integrate_device(spec[f].data_ptr(), integ[f].data_ptr())
        eng.peaks_device(integ[f].data_ptr(), outs[f][1][0].data_ptr(), outs[f][1][1].data_ptr())
    eng.synchronize()
    for f in range(F):
        got = read_buffers(*outs[f][0], B, K)
        same(got, pc.tables(spec[f].cpu().numpy(), 0, n, 8, K, 10.0), f)
        assert got[0]["bin"][:, 0].tolist() == [n // 2 + k for k in TONE_BINS]
        assert [S.bin_offset_hz(n, FS, int(b)) for b in got[0]["bin"][:, 0]] == [k * FS / n for k in TONE_BINS]
        got = read_buffers(*outs[f][1], B, K)
        same(got, pc.tables(integ[f].cpu().numpy(), 0, n, 8, K, 10.0), f)
        assert got[0]["bin"][:, 0].tolist() == [n // 2 + k for k in TONE_BINS]
    mean = ic.Integrator(ic.MEAN, period=4)
    for f in range(F):
        want = mean.push(spec[f].cpu().numpy())
    assert integ[F - 1].cpu().numpy().tobytes() == want.tobytes()
    eng.close()


def test_pipelined_calls_equal_the_joined_schedule(S, O, T):
    """PIPELINE_ON | PIPELINE_STATS_ASYNC, two rotating spectra buffers, four calls each followed by peaks_device: the
    tables are those of the joined schedule."""
    n, B, F, K = 16384, len(TONE_BINS), 4, 8
    raws = tone_frames(O, n, F, seed=500)

    def run(mode):
        eng = engine(S, n, B)
        eng.set_pipelining(mode)
        eng.set_peaks(span=S.DISPLAY_SPAN_FULL, max_peaks=K, min_separation=16, threshold_db=8.0)
        iq = [T.from_numpy(raws[f]).to("cuda:0") for f in range(F)]
        spec = [T.zeros((B, n), dtype=T.float32, device="cuda:0") for _ in range(2)]
        rec = [T.zeros((B, S.RECORD_DTYPE.itemsize), dtype=T.uint8, device="cuda:0") for _ in range(2)]
        pcm = [T.zeros((B, eng.pcm_len), dtype=T.int16, device="cuda:0") for _ in range(F)]
        outs = [out_buffers(T, B, K) for _ in range(F)]
        T.cuda.synchronize()
        for f in range(F):
            eng.process_device(iq[f].data_ptr(), S.CS8, S.STAGE_ALL, spec[f % 2].data_ptr(), rec[f % 2].data_ptr(),
                               pcm[f].data_ptr(), 1000 + 10 * f)
            eng.peaks_device(spec[f % 2].data_ptr(), outs[f][0].data_ptr(), outs[f][1].data_ptr())
        eng.synchronize()
        got = [read_buffers(*outs[f], B, K) for f in range(F)]
        last = spec[(F - 1) % 2].cpu().numpy()
        eng.close()
        return got, last

    joined, last = run(S.PIPELINE_OFF)
    piped, _ = run(S.PIPELINE_ON | S.PIPELINE_STATS_ASYNC)
    for f in range(F):
        same(piped[f], joined[f], f)
    same(joined[F - 1], pc.tables(last, 0, n, 16, K, 8.0))
    assert len({joined[f][0].tobytes() for f in range(F)}) == F  # four different frames


def test_wait_outputs_orders_a_consumer_stream(S, O, T):
    n, B, K = 16384, len(TONE_BINS), 8
    raw = tone_frames(O, n, 1, seed=900)[0]
    eng = engine(S, n, B)
    eng.set_peaks(span=S.DISPLAY_SPAN_FULL, max_peaks=K, min_separation=8, threshold_db=10.0)
    iq = T.from_numpy(raw).to("cuda:0")
    spec = T.zeros((B, n), dtype=T.float32, device="cuda:0")
    pk_t, sm_t = out_buffers(T, B, K)
    pk_copy, sm_copy = T.zeros_like(pk_t), T.zeros_like(sm_t)
    consumer = T.cuda.Stream("cuda:0")
    T.cuda.synchronize()
    for k in range(3):
        eng.process_device(iq.data_ptr(), S.CS8, S.STAGE_SPECTRUM, spec.data_ptr(), None, None, 1000 + k)
        eng.peaks_device(spec.data_ptr(), pk_t.data_ptr(), sm_t.data_ptr())
        eng.wait_outputs(consumer.cuda_stream)
        with T.cuda.stream(consumer):
            pk_copy.copy_(pk_t)
            sm_copy.copy_(sm_t)
    consumer.synchronize()
    eng.synchronize()
    same(read_buffers(pk_copy, sm_copy, B, K), pc.tables(spec.cpu().numpy(), 0, n, 8, K, 10.0))
    eng.close()


# ---- host path and contract ---------------------------------------------------------------------------------------

def test_host_path(S, O):
    """process_host(spectra = NULL) then peaks() gives the tables of the spectra an identical engine returns, peaks(spectra)
    those of caller spectra through a buffer of their own; integrate(NULL, NULL) then peaks_integrated() those of the
    integrated rows."""
    n, B, K = 4096, 3, 8
    raws = np.stack([np.stack([O.synth_frames(1, n, O.CS8, tone_hz=900.0 * b - 800.0, fs=FS, seed=21 + b + 7 * f)[0]
                               for b in range(B)]) for f in range(2)])
    ref = engine(S, n, B)
    specs = [ref.process(raws[f], fmt=S.CS8, stages=S.STAGE_SPECTRUM | S.STAGE_STATS, now_ms=1000 + f)[0].copy()
             for f in range(2)]
    ref.close()
    eng = engine(S, n, B)
    cfg = dict(span=S.DISPLAY_SPAN_FULL, max_peaks=K, min_separation=8, threshold_db=10.0)
    eng.set_peaks(**cfg)
    invalid(S, eng.peaks)             # no process_host call yet
    invalid(S, eng.peaks_integrated)  # no integrate_host call yet
    eng.set_integration(S.INTEGRATE_MEAN, period=2)
    mean = ic.Integrator(ic.MEAN, period=2)
    rec = np.zeros(B, S.RECORD_DTYPE)
    for f in range(2):
        rc = S.load().sdrg_engine_process_host(eng._h, raws[f].ctypes.data_as(ctypes.c_void_p), S.CS8,
                                               S.STAGE_SPECTRUM | S.STAGE_STATS, None, rec.ctypes.data_as(ctypes.c_void_p),
                                               None, 1000 + f)
        assert rc == 0
        got = eng.peaks()
        assert got[0].dtype == S.PEAK_DTYPE and got[0].shape == (B, K) and got[1].dtype == S.PEAKS_SUMMARY_DTYPE
        same(got, pc.tables(specs[f], 0, n, 8, K, 10.0), f)
        assert eng.integrate(None, want_output=False) is None
        same(eng.peaks_integrated(), pc.tables(mean.push(specs[f]), 0, n, 8, K, 10.0), f)
    other = pc.noise_rows(B, n, seed=3, tones=5)
    same(eng.peaks(other), pc.tables(other, 0, n, 8, K, 10.0))
    same(eng.peaks(), got)  # the caller's spectra went through a buffer of their own
    eng.setSamplesPerReading(2048)
    invalid(S, eng.peaks)             # the spectra on the device are 4096 bins wide
    invalid(S, eng.peaks_integrated)  # and so are the integrated rows
    small = pc.noise_rows(B, 2048, seed=4, tones=5)
    same(eng.peaks(small), pc.tables(small, 0, 2048, 8, K, 10.0))
    eng.close()


def test_contract(S, T):
    n, B = 4096, 2
    spec = pc.noise_rows(B, n, seed=9, tones=6)
    spec_t = caller_spectra(T, spec)
    eng = engine(S, n, B)
    pk_t, sm_t = out_buffers(T, B, 4)
    T.cuda.synchronize()
    args = (spec_t.data_ptr(), pk_t.data_ptr(), sm_t.data_ptr())
    invalid(S, eng.peaks_config)  # before any set_peaks
    invalid(S, eng.peaks_device, *args)
    invalid(S, eng.peaks, spec)
    invalid(S, eng.peaks_integrated)
    good = dict(span=S.DISPLAY_SPAN_BINS, first_bin=3000, n_bins=1000, max_peaks=4, min_separation=5, threshold_db=6.0)
    eng.set_peaks(**good)
    assert eng.peaks_config() == good
    for bad in (dict(span=3), dict(span=-1), dict(max_peaks=0), dict(max_peaks=65), dict(min_separation=0),
                dict(min_separation=4097), dict(threshold_db=float("nan")), dict(threshold_db=INF), dict(first_bin=-1),
                dict(n_bins=0)):
        invalid(S, eng.set_peaks, **{**good, **bad})
        assert eng.peaks_config() == good  # a rejected configuration leaves the previous one in force
    for ok in (dict(max_peaks=64, min_separation=4096, threshold_db=-INF), dict(max_peaks=1, min_separation=1)):
        eng.set_peaks(**{**good, **ok})
    eng.set_peaks(**good)
    for k in range(3):
        invalid(S, eng.peaks_device, *[None if i == k else a for i, a in enumerate(args)])
    want = pc.tables(spec, 3000, 1000, 5, 4, 6.0)
    same(eng.peaks(spec), want)
    eng.setSamplesPerReading(3500)  # the span [3000, 4000) no longer fits: fails at the call, enqueues nothing
    invalid(S, eng.peaks_device, *args)
    eng.synchronize()
    assert bool((pk_t == 0xAA).all()) and bool((sm_t == 0xAA).all())
    eng.setSamplesPerReading(n)  # the next valid call works
    eng.peaks_device(*args)
    eng.synchronize()
    same(read_buffers(pk_t, sm_t, B, 4), want)
    eng.close()
