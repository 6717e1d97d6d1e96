"""GPU tests of the integration stage (csrc/integrate.hip, sdrg_engine_integrate_*): the mean, the maximum and the
EMA of the last spectra, compared as bytes, after every call, with the NumPy restatement in tests/integrate_cases.py.

The kernel works on float4s of the flat [n_streams * N] array with a scalar launch for the last count % 4 floats (and
for everything when a caller's pointer is off 16 bytes), loads the ring in batches of 8 slots, and wraps the ring at
`period`: the shapes below have counts of every residue mod 4, more than one workgroup, periods on both sides of a
batch, and 2 * period + 3 calls each, so the ring wraps twice."""
import ctypes

import numpy as np
import pytest

import display_cases as dc
import integrate_cases as ic

pytestmark = pytest.mark.gpu

FS = 2_000_000
FC = 100_000_000
GUARD = 16  # floats after the output
PATTERN = 0x55AA55AA


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


def engine(S, n, B, fs=FS, fc=FC):
    return S.Engine(S.SDRConfig(centerFrequency=fc, samplesPerReading=n, sampleRate=fs, freqFocusRangeKhz=5, soundMode=1), B)


def invalid(S, fn, *a, **k):
    with pytest.raises(S.SdrgError) as ei:
        fn(*a, **k)
    assert "SDRG_E_INVALID" in str(ei.value)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def upload(T, a):
    return T.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda:0")


class Output:
    """[count] floats followed by GUARD floats of PATTERN; `offset` floats into a 16-byte aligned allocation."""

    def __init__(self, T, count, offset=0):
        self.T, self.count = T, count
        self.buf = T.full((offset + count + GUARD,), PATTERN, dtype=T.int32, device="cuda:0")
        self.view = self.buf[offset:]
        self.ptr = self.view.data_ptr()

    def load(self, dev_rows):  # for in-place calls
        self.view[:self.count].copy_(dev_rows.reshape(-1).view(self.T.int32))

    def read(self):
        raw = self.view.cpu().numpy()
        assert np.all(raw[self.count:] == PATTERN), "floats written past the output"
        return raw[:self.count].view(np.float32)


def check_calls(T, eng, it, frames, in_place=False, offset=0, out=None):
    """One integrate_device call per frame of `frames` [F][B][n]: after every call the output equals the restatement's as
    bytes, the guard is intact, the input is as it was and depth is the restatement's."""
    F, B, n = frames.shape
    dev = upload(T, frames if not offset else np.concatenate([np.zeros(offset, np.float32), frames.reshape(-1)]))
    dev = dev[offset:].reshape(F, B, n)
    out = out or Output(T, B * n, offset)
    for t in range(F):
        if in_place:
            out.load(dev[t])
        T.cuda.synchronize()
        eng.integrate_device(out.ptr if in_place else dev[t].data_ptr(), out.ptr)
        eng.synchronize()
        want = it.push(frames[t])
        got = out.read().reshape(B, n)
        assert got.tobytes() == want.tobytes(), (t, np.argwhere(bits(got) != bits(want))[:8])
        assert eng.integration_depth() == it.depth
    if not in_place:
        assert dev.cpu().numpy().tobytes() == frames.tobytes()


RING_SHAPES = [  # (N, B, K): a cover of N in {1 .. 16384}, B in {1, 3, 5, 37}, K in {1 .. 64}; N * B of every residue mod 4
    (1, 1, 1), (1, 3, 2), (3, 5, 3), (3, 37, 7), (64, 37, 7), (64, 1, 17), (1000, 3, 10), (1001, 5, 16), (1002, 1, 17),
    (1003, 37, 3), (1003, 3, 64), (4096, 3, 64), (4096, 37, 1), (16384, 5, 10), (16384, 1, 2), (16384, 3, 16),
]


@pytest.mark.parametrize("mode", (ic.MEAN, ic.MAX), ids=("mean", "max"))
@pytest.mark.parametrize("n,B,K", RING_SHAPES, ids=lambda v: str(v))
def test_ring_and_tails(S, T, n, B, K, mode):
    frames = ic.spread_frames(2 * K + 3, B, n, seed=1000 * K + n + B)
    frames[K // 2 + 1, B // 2] = 0.0  # a silent frame of one stream
    eng = engine(S, n, B)
    eng.set_integration(mode=mode, period=K)
    assert eng.integration() == dict(mode=mode, period=K, alpha=0.0, depth=0)
    check_calls(T, eng, ic.Integrator(mode, period=K), frames)
    eng.close()


@pytest.mark.parametrize("alpha", (1.0, 0.5, float(np.float32(0.1))), ids=("1", "0.5", "0.1f"))
@pytest.mark.parametrize("n,B", [(1, 1), (3, 5), (64, 37), (1000, 3), (1001, 5), (1002, 1), (1003, 37), (4096, 3), (16384, 5)],
                         ids=lambda v: str(v))
def test_ema(S, T, n, B, alpha):
    frames = ic.spread_frames(7, B, n, seed=n + B) if alpha != 0.5 else ic.dyadic_frames(7, B, n, seed=n + B)
    eng = engine(S, n, B)
    eng.set_integration(mode=S.INTEGRATE_EMA, alpha=alpha)
    check_calls(T, eng, ic.Integrator(ic.EMA, alpha=alpha), frames)
    assert eng.integration()["depth"] == 7
    eng.close()


@pytest.mark.parametrize("mode", (ic.MEAN, ic.MAX, ic.EMA), ids=("mean", "max", "ema"))
def test_one_large_row(S, T, mode):
    n, B, K = 2 ** 20, 1, 2
    frames = ic.spread_frames(2 * K + 3, B, n, seed=20)
    eng = engine(S, n, B)
    eng.set_integration(mode=mode, period=K, alpha=0.25)
    check_calls(T, eng, ic.Integrator(mode, period=K, alpha=0.25), frames)
    eng.close()


@pytest.mark.parametrize("n,B", [(1003, 3), (16384, 3), (5, 2)], ids=lambda v: str(v))
@pytest.mark.parametrize("K", (4, 16, 64))
def test_order_probes(S, T, K, n, B):
    """The probes in the row's first and last bin and on both sides of a float4 boundary: every call that ends a period
    integrates exactly the probe, whose mean differs by a float ulp when the doubles are added in another order."""
    F = 2 * K + 3
    frames = ic.place_order_probes(ic.spread_frames(F, B, n, seed=K + n), K)
    a, b = ic.probe_bins(n)
    eng = engine(S, n, B)
    eng.set_integration(mode=S.INTEGRATE_MEAN, period=K)
    it = ic.Integrator(ic.MEAN, period=K)
    dev = upload(T, frames)
    out = Output(T, B * n)
    for t in range(F):
        T.cuda.synchronize()
        eng.integrate_device(dev[t].data_ptr(), out.ptr)
        eng.synchronize()
        got = out.read().reshape(B, n)
        assert got.tobytes() == it.push(frames[t]).tobytes(), t
        if t % K == K - 1:
            assert np.all(got[:, a + b] == ic.order_probes(K)[2]), (t, got[:, a + b])
    eng.close()


@pytest.mark.parametrize("mode,kw", [(ic.MEAN, dict(period=5)), (ic.MAX, dict(period=5)), (ic.EMA, dict(alpha=0.1))],
                         ids=("mean", "max", "ema"))
def test_zero_rows_stay_zero(S, T, mode, kw):
    n, B = 1001, 3
    frames = ic.spread_frames(9, B, n, seed=3)
    frames[:, 1] = 0.0  # stream 1 is silent throughout
    frames[2:, 2] = 0.0  # stream 2 falls silent: MEAN and MAX are exactly 0 five calls later
    eng = engine(S, n, B)
    eng.set_integration(mode=mode, **kw)
    it = ic.Integrator(mode, **kw)
    check_calls(T, eng, it, frames)
    last = it.push(np.zeros((B, n), np.float32))
    assert not bits(last[1]).any()
    if mode != ic.EMA:
        assert not bits(last[2]).any()
    eng.close()


@pytest.mark.parametrize("K", (2, 10))
@pytest.mark.parametrize("mode", (ic.MEAN, ic.MAX), ids=("mean", "max"))
def test_no_residue(S, T, mode, K):
    """+inf, then 1e30f, then K frames around 1e-20f: K frames later the output is exactly the mean (the maximum) of
    those K, as an integrator that never saw the strong frames gives it."""
    n, B = 1003, 3
    frames = ic.residue_frames(K, B, n, seed=K)
    eng = engine(S, n, B)
    eng.set_integration(mode=mode, period=K)
    out = Output(T, B * n)
    check_calls(T, eng, ic.Integrator(mode, period=K), frames, out=out)
    fresh = ic.Integrator(mode, period=K)
    for f in frames[2:]:
        want = fresh.push(f)
    got = out.read().reshape(B, n)
    assert got.tobytes() == want.tobytes() and got.max() < 3e-20
    eng.close()


@pytest.mark.parametrize("mode,kw", [(ic.MEAN, dict(period=3)), (ic.MAX, dict(period=9)), (ic.EMA, dict(alpha=0.25))],
                         ids=("mean", "max", "ema"))
@pytest.mark.parametrize("offset", (0, 1), ids=("aligned", "off16"))
def test_in_place_equals_out_of_place(S, T, mode, kw, offset):
    """out == spectra, and both pointers 4 bytes off a 16-byte boundary (the scalar instance takes the whole array)."""
    n, B = 1002, 5
    frames = ic.spread_frames(12, B, n, seed=8)
    for in_place in (False, True):
        eng = engine(S, n, B)
        eng.set_integration(mode=mode, **kw)
        check_calls(T, eng, ic.Integrator(mode, **kw), frames, in_place=in_place, offset=offset)
        eng.close()


def cs8_frames(O, F, B, n, seed):
    return np.stack([np.stack([O.synth_frames(1, n, O.CS8, tone_hz=400.0 * b - 900.0, fs=FS, seed=seed + 100 * f + b)[0]
                               for b in range(B)]) for f in range(F)])


@pytest.mark.parametrize("n", (4096, 4099))
def test_engine_spectra(S, O, T, n):
    """process_device then integrate_device with no synchronisation between them: the rows integrate that call's
    spectra (odd N: the element N - 1 the spectrum never writes is data like any other)."""
    B, K, F = 3, 3, 8
    raws = cs8_frames(O, F, B, n, seed=11)
    eng = engine(S, n, B)
    eng.set_integration(mode=S.INTEGRATE_MEAN, period=K)
    it = ic.Integrator(ic.MEAN, period=K)
    iq = T.from_numpy(raws).to("cuda:0")
    spec = T.zeros((B, n), dtype=T.float32, device="cuda:0")
    out = Output(T, B * n)
    T.cuda.synchronize()
    for f in range(F):
        eng.process_device(iq[f].data_ptr(), S.CS8, S.STAGE_SPECTRUM, spec.data_ptr(), None, None, 1000 + f)
        eng.integrate_device(spec.data_ptr(), out.ptr)
        eng.synchronize()
        x = spec.cpu().numpy()
        assert x.max() > 0
        assert out.read().reshape(B, n).tobytes() == it.push(x).tobytes(), f
    eng.close()


def test_composition_on_two_engines(S, O, T):
    """Engine A integrates and hands the rows to signal_strength_device and display_device on the device; engine B is
    given the restated rows: the records and the display rows are equal as bytes, call after call."""
    n, B, K, F, W = 4096, 4, 3, 6, 500
    raws = cs8_frames(O, F, B, n, seed=31)
    spec_eng = engine(S, n, B)
    spectra = np.stack([spec_eng.process(raws[f], fmt=S.CS8, stages=S.STAGE_SPECTRUM, now_ms=0)[0] for f in range(F)])
    spec_eng.close()
    a, b = engine(S, n, B), engine(S, n, B)
    a.set_integration(mode=S.INTEGRATE_MEAN, period=K)
    for e in (a, b):
        e.set_display(span=S.DISPLAY_SPAN_FULL, width=W, reduce=S.DISPLAY_MAX, format=S.DISPLAY_U8, db_min=-120.0, db_max=0.0)
    it = ic.Integrator(ic.MEAN, period=K)
    dev = upload(T, spectra)
    rows = T.zeros((B, n), dtype=T.float32, device="cuda:0")
    rec = [T.zeros((B, S.RECORD_DTYPE.itemsize), dtype=T.uint8, device="cuda:0") for _ in range(2)]
    disp = [T.zeros((B, W), dtype=T.uint8, device="cuda:0") for _ in range(2)]
    for f in range(F):
        want = upload(T, it.push(spectra[f]))
        T.cuda.synchronize()
        a.integrate_device(dev[f].data_ptr(), rows.data_ptr())
        S._check(S.load().sdrg_engine_signal_strength_device(a._h, rows.data_ptr(), rec[0].data_ptr(), 1000 + 10 * f), "ss")
        a.display_device(rows.data_ptr(), disp[0].data_ptr())
        S._check(S.load().sdrg_engine_signal_strength_device(b._h, want.data_ptr(), rec[1].data_ptr(), 1000 + 10 * f), "ss")
        b.display_device(want.data_ptr(), disp[1].data_ptr())
        a.synchronize()
        b.synchronize()
        assert rec[0].cpu().numpy().tobytes() == rec[1].cpu().numpy().tobytes(), f
        assert disp[0].cpu().numpy().tobytes() == disp[1].cpu().numpy().tobytes(), f
    assert rec[0].cpu().numpy().any()
    a.close()
    b.close()


def test_in_place_under_asynchronous_statistics(S, O, T):
    """PIPELINE_ON | PIPELINE_STATS_ASYNC, every call's spectra integrated in place right after the call: the records
    are those of the joined schedule with out-of-place integration (the statistics saw the spectrum, not the integrated
    rows), and the integrated rows are the restatement's."""
    n, B, K, F = 16384, 64, 3, 5
    raws = cs8_frames(O, F, B, n, seed=51)

    def run(mode, in_place):
        eng = engine(S, n, B)
        eng.set_pipelining(mode)
        eng.set_integration(mode=S.INTEGRATE_MEAN, period=K)
        iq = T.from_numpy(raws).to("cuda:0")
        spec = [T.zeros((B, n), dtype=T.float32, device="cuda:0") for _ in range(F)]
        outs = spec if in_place else [T.zeros((B, n), dtype=T.float32, device="cuda:0") for _ in range(F)]
        rec = [T.zeros((B, S.RECORD_DTYPE.itemsize), dtype=T.uint8, device="cuda:0") for _ in range(F)]
        pcm = [T.zeros((B, eng.pcm_len), dtype=T.int16, device="cuda:0") for _ in range(F)]
        T.cuda.synchronize()
        for f in range(F):
            eng.process_device(iq[f].data_ptr(), S.CS8, S.STAGE_ALL, spec[f].data_ptr(), rec[f].data_ptr(), pcm[f].data_ptr(),
                               1000 + 10 * f)
            eng.integrate_device(spec[f].data_ptr(), outs[f].data_ptr())
        eng.synchronize()
        res = (T.stack(rec).cpu().numpy(), T.stack(outs).cpu().numpy(), T.stack(spec).cpu().numpy())
        eng.close()
        return res

    rec_j, out_j, spec_j = run(S.PIPELINE_OFF, False)
    rec_p, out_p, _ = run(S.PIPELINE_ON | S.PIPELINE_STATS_ASYNC, True)
    assert rec_p.tobytes() == rec_j.tobytes()
    assert out_p.tobytes() == out_j.tobytes()
    it = ic.Integrator(ic.MEAN, period=K)
    for f in range(F):
        assert out_j[f].tobytes() == it.push(spec_j[f]).tobytes(), f
    assert len({rec_j[f].tobytes() for f in range(F)}) == F


def test_wait_outputs_orders_a_consumer_stream(S, O, T):
    n, B, K = 16384, 64, 2
    raws = cs8_frames(O, 1, B, n, seed=71)
    eng = engine(S, n, B)
    eng.set_integration(mode=S.INTEGRATE_MAX, period=K)
    it = ic.Integrator(ic.MAX, period=K)
    iq = T.from_numpy(raws[0]).to("cuda:0")
    spec = T.zeros((B, n), dtype=T.float32, device="cuda:0")
    rows = T.zeros((B, n), dtype=T.float32, device="cuda:0")
    copy = T.zeros((B, n), dtype=T.float32, device="cuda:0")
    consumer = T.cuda.Stream("cuda:0")
    T.cuda.synchronize()
    for k in range(3):
        eng.process_device(iq.data_ptr(), S.CS8, S.STAGE_SPECTRUM, spec.data_ptr(), None, None, 1000 + k)
        eng.integrate_device(spec.data_ptr(), rows.data_ptr())
        eng.wait_outputs(consumer.cuda_stream)
        with T.cuda.stream(consumer):
            copy.copy_(rows)
        consumer.synchronize()  # the next call rewrites rows
    eng.synchronize()
    x = spec.cpu().numpy()
    for k in range(3):
        want = it.push(x)
    assert copy.cpu().numpy().tobytes() == want.tobytes()
    eng.close()


def test_reset_rules(S, T):
    n, B, K = 64, 2, 3
    frames = ic.spread_frames(40, B, n, seed=5)
    small = ic.spread_frames(4, B, 32, seed=6)
    eng = engine(S, n, B)
    eng.set_integration(mode=S.INTEGRATE_MEAN, period=K)
    it = ic.Integrator(ic.MEAN, period=K)
    assert eng.integration_depth() == 0
    state = dict(f=0)

    def calls(count, expect_depths, src=frames):
        got = []
        k = state["f"]
        check = src[k:k + count]
        dev = upload(T, check)
        out = Output(T, check[0].size)
        for t in range(count):
            T.cuda.synchronize()
            eng.integrate_device(dev[t].data_ptr(), out.ptr)
            eng.synchronize()
            assert out.read().tobytes() == it.push(check[t]).tobytes()
            got.append(eng.integration_depth())
        state["f"] = k + count
        assert got == expect_depths, got

    calls(5, [1, 2, 3, 3, 3])
    for cause in (lambda: eng.set_integration(mode=S.INTEGRATE_MEAN, period=K), eng.integrate_reset, eng.reset_state,
                  lambda: eng.setSampleRate(FS + 1000), lambda: eng.setFrequency(FC + 5000)):
        cause()
        if cause in (eng.integrate_reset, eng.reset_state):
            assert eng.integration_depth() == 0
        it.reset()  # the restatement forgets: the next output is the input's bits
        calls(4, [1, 2, 3, 3])
    eng.setFrequency(FC + 5000)  # the value in force: no reset
    eng.setSampleRate(FS + 1000)
    calls(2, [3, 3])
    eng.setSamplesPerReading(32)
    it.reset()
    state["f"] = 0
    calls(4, [1, 2, 3, 3], src=small)
    eng.setSamplesPerReading(n)  # and back: the history of 64-bin rows is not taken up again
    it.reset()
    state["f"] = 30
    calls(4, [1, 2, 3, 3])
    eng.close()


def test_host_path(S, O):
    n, B, K, W = 4096, 3, 2, 500
    raws = cs8_frames(O, 3, B, n, seed=91)
    ref = engine(S, n, B)
    spectra = [ref.process(raws[f], fmt=S.CS8, stages=S.STAGE_SPECTRUM | S.STAGE_STATS, now_ms=1000 + f)[0] for f in range(3)]
    ref.close()
    eng = engine(S, n, B)
    eng.set_integration(mode=S.INTEGRATE_MEAN, period=K)
    eng.set_display(span=S.DISPLAY_SPAN_FULL, width=W, reduce=S.DISPLAY_MAX, format=S.DISPLAY_U8, db_min=-120.0, db_max=0.0)
    it = ic.Integrator(ic.MEAN, period=K)
    invalid(S, eng.integrate)  # spectra = NULL before any process_host call
    invalid(S, eng.display_integrated)  # no integrate_host call yet
    assert eng.integration_depth() == 0
    other = ic.spread_frames(1, B, n, seed=92)[0]
    got = eng.integrate(other)  # caller spectra
    assert got.dtype == np.float32 and got.shape == (B, n) and got.tobytes() == it.push(other).tobytes()
    rec = np.zeros(B, S.RECORD_DTYPE)
    for f in range(3):  # NULL after process_host(spectra = NULL); out = NULL keeps the rows on the device
        rc = S.load().sdrg_engine_process_host(eng._h, raws[f].ctypes.data_as(ctypes.c_void_p), S.CS8,
                                               S.STAGE_SPECTRUM | S.STAGE_STATS, None, rec.ctypes.data_as(ctypes.c_void_p),
                                               None, 1000 + f)
        assert rc == 0
        want = it.push(spectra[f])
        if f == 1:
            assert eng.integrate(None, want_output=False) is None
        else:
            assert eng.integrate().tobytes() == want.tobytes(), f
        assert eng.display_integrated().tobytes() == dc.rows(want, 0, n, W, dc.MAX, dc.U8, -120.0, 0.0).tobytes(), f
    eng.setSamplesPerReading(2048)
    invalid(S, eng.integrate)  # the spectra on the device are 4096 bins wide
    invalid(S, eng.display_integrated)  # and so are the integrated rows
    assert eng.integration_depth() == K  # the refused calls advanced nothing
    it.reset()
    small = ic.spread_frames(1, B, 2048, seed=93)[0]
    want = it.push(small)
    assert eng.integrate(small).tobytes() == want.tobytes()
    assert eng.display_integrated().tobytes() == dc.rows(want, 0, 2048, W, dc.MAX, dc.U8, -120.0, 0.0).tobytes()
    eng.close()


def test_contract(S, T):
    n, B, K = 1000, 2, 4
    frames = ic.spread_frames(8, B, n, seed=13)
    dev = upload(T, frames)
    out = Output(T, B * n)
    eng = engine(S, n, B)
    T.cuda.synchronize()
    invalid(S, eng.integration)  # before any set_integration
    invalid(S, eng.integrate_device, dev[0].data_ptr(), out.ptr)
    invalid(S, eng.integrate, frames[0])
    assert eng.integration_depth() == 0
    eng.set_integration(mode=S.INTEGRATE_MEAN, period=K, alpha=7.0)  # MEAN does not read alpha
    good = eng.integration()
    assert good == dict(mode=S.INTEGRATE_MEAN, period=K, alpha=7.0, depth=0)
    it = ic.Integrator(ic.MEAN, period=K)
    check_calls(T, eng, it, frames[:3], out=out)
    good["depth"] = 3
    nan, inf = float("nan"), float("inf")
    for bad in (dict(mode=3), dict(mode=-1), dict(mode=S.INTEGRATE_MEAN, period=0), dict(mode=S.INTEGRATE_MAX, period=65),
                dict(mode=S.INTEGRATE_MAX, period=-1), dict(mode=S.INTEGRATE_EMA, alpha=0.0),
                dict(mode=S.INTEGRATE_EMA, alpha=-0.5), dict(mode=S.INTEGRATE_EMA, alpha=nan),
                dict(mode=S.INTEGRATE_EMA, alpha=1.5), dict(mode=S.INTEGRATE_EMA, alpha=inf)):
        invalid(S, eng.set_integration, **bad)
        assert eng.integration() == good, bad  # configuration and depth as they were
    assert S.load().sdrg_engine_set_integration(eng._h, None) == -1
    invalid(S, eng.integrate_device, None, out.ptr)
    invalid(S, eng.integrate_device, dev[3].data_ptr(), None)
    eng.synchronize()
    assert eng.integration() == good
    check_calls(T, eng, it, frames[3:], out=out)  # and the history: the ring goes on where it was
    eng.set_integration(mode=S.INTEGRATE_EMA, alpha=1.0, period=-3)  # EMA does not read the period
    assert eng.integration() == dict(mode=S.INTEGRATE_EMA, period=-3, alpha=1.0, depth=0)
    eng.close()
