"""CPU tests of the integration stage's NumPy restatement (tests/integrate_cases.py): hand-worked examples per mode,
the identities, and the order probes that tell the stated addition order from any other."""
import numpy as np

import integrate_cases as ic

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_period_one_and_the_first_call_return_the_inputs_bits():
    frames = ic.spread_frames(4, 2, 9, seed=1)
    frames[1, 0, 0] = np.inf
    frames[2, 1, 3] = 0.0
    frames[3, 0, 8] = f32(1e-45)  # a denormal
    for mode in (ic.MEAN, ic.MAX):
        one = ic.Integrator(mode, period=1)
        for f in frames:
            np.testing.assert_array_equal(bits(one.push(f)), bits(f))
        assert one.depth == 1
        first = ic.Integrator(mode, period=7)
        np.testing.assert_array_equal(bits(first.push(frames[0])), bits(frames[0]))
    ema = ic.Integrator(ic.EMA, alpha=0.25)
    np.testing.assert_array_equal(bits(ema.push(frames[0])), bits(frames[0]))


def test_three_frames_by_hand():
    x = [np.array([[1.0, 8.0]], np.float32), np.array([[2.0, 0.0]], np.float32), np.array([[6.0, 4.0]], np.float32)]
    mean = ic.Integrator(ic.MEAN, period=2)
    assert [mean.push(f).tolist() for f in x] == [[[1.0, 8.0]], [[1.5, 4.0]], [[4.0, 2.0]]]
    assert mean.depth == 2
    mean3 = ic.Integrator(ic.MEAN, period=3)
    got = [mean3.push(f) for f in x]
    assert got[2].tolist() == [[3.0, 4.0]] and got[2].dtype == np.float32
    peak = ic.Integrator(ic.MAX, period=2)
    assert [peak.push(f).tolist() for f in x] == [[[1.0, 8.0]], [[2.0, 8.0]], [[6.0, 4.0]]]
    ema = ic.Integrator(ic.EMA, alpha=0.25)  # y = y + 0.25 (x - y)
    assert [ema.push(f).tolist() for f in x] == [[[1.0, 8.0]], [[1.25, 6.0]], [[2.4375, 5.5]]]
    assert ema.depth == 3


def test_depth_and_reset():
    it = ic.Integrator(ic.MAX, period=3)
    assert it.depth == 0
    seen = []
    for k in range(5):
        it.push(np.full((1, 2), float(k), np.float32))
        seen.append(it.depth)
    assert seen == [1, 2, 3, 3, 3]
    it.reset()
    assert it.depth == 0
    assert it.push(np.zeros((1, 2), np.float32)).tolist() == [[0.0, 0.0]]  # the 4.0 before the reset is forgotten


def test_ema_alpha_one_is_the_input_and_a_half_is_exact_on_dyadic_inputs():
    dy = ic.dyadic_frames(6, 2, 16, seed=3)
    one = ic.Integrator(ic.EMA, alpha=1.0)
    half = ic.Integrator(ic.EMA, alpha=0.5)
    y = dy[0].astype(np.float64)
    for t, f in enumerate(dy):
        np.testing.assert_array_equal(bits(one.push(f)), bits(f))  # k / 16 < 256: every difference is exact
        if t:
            y = y + 0.5 * (f.astype(np.float64) - y)  # exact in double: at most 4 + 6 fraction bits after six frames
        got = half.push(f)
        np.testing.assert_array_equal(got.astype(np.float64), y)


def test_zero_rows_stay_zero():
    for mode, kw in ((ic.MEAN, dict(period=5)), (ic.MAX, dict(period=5)), (ic.EMA, dict(alpha=f32(0.1)))):
        it = ic.Integrator(mode, **kw)
        for _ in range(7):
            out = it.push(np.zeros((2, 5), np.float32))
            assert not bits(out).any()


def test_order_probes():
    """The values DESIGN.md §3.10 states, from NumPy's float64 and float32 additions."""
    a, b = ic.ORDER_PROBE_A, ic.ORDER_PROBE_B
    assert ic.mean_in_order(a) == f32(4194304.5) == ic.ORDER_PROBE_MEAN
    assert ic.mean_in_order(a[::-1]) == f32(4194304.0)
    assert ic.mean_in_order(a, dtype=np.float32) == f32(4194304.0)
    assert ic.mean_in_order(b) == f32(4194304.5)
    assert ic.mean_pairwise(b) == f32(4194304.0)
    for probe in (a, b):
        it = ic.Integrator(ic.MEAN, period=4)
        for v in probe:
            out = it.push(np.full((1, 1), v, np.float32))
        assert out[0, 0] == ic.ORDER_PROBE_MEAN


def test_order_probes_of_longer_periods():
    for K in (8, 16, 32, 64):
        a, b, mean = ic.order_probes(K)
        less = np.nextafter(mean, f32(0))
        assert ic.mean_in_order(a) == mean and ic.mean_in_order(b) == mean
        assert ic.mean_in_order(a[::-1]) == less and ic.mean_in_order(b[::-1]) == less
        assert ic.mean_in_order(a, dtype=np.float32) == less and ic.mean_in_order(b, dtype=np.float32) == less
        halves_swapped = np.concatenate([b[K // 2:K - 1], b[:K // 2], b[K - 1:]])  # the older values batch by batch
        assert ic.mean_in_order(halves_swapped) == less


def test_placed_probes_come_round_with_every_call_that_ends_a_period():
    for K, n in ((4, 11), (16, 5)):
        B, F = 2, 2 * K + 3
        frames = ic.place_order_probes(ic.spread_frames(F, B, n, seed=4), K)
        a, b = ic.probe_bins(n)
        assert a and b and not set(a) & set(b)
        it = ic.Integrator(ic.MEAN, period=K)
        for t in range(F):
            out = it.push(frames[t])
            if t % K == K - 1:
                assert np.all(out[:, a + b] == ic.order_probes(K)[2])


def test_spread_inputs_tell_a_float_accumulator_from_a_double():
    K, B, n = 10, 2, 512
    frames = ic.spread_frames(K, B, n, seed=5)
    it = ic.Integrator(ic.MEAN, period=K)
    for f in frames:
        want = it.push(f)
    acc = frames[0].copy()
    for f in frames[1:]:
        acc = (acc + f).astype(np.float32)
    flt = (acc.astype(np.float64) / K).astype(np.float32)
    assert np.mean(bits(flt) != bits(want)) > 0.05


def test_no_residue_of_strong_frames():
    for mode in (ic.MEAN, ic.MAX):
        K, B, n = 4, 2, 8
        frames = ic.residue_frames(K, B, n, seed=6)
        it = ic.Integrator(mode, period=K)
        outs = [it.push(f) for f in frames]
        assert np.all(np.isinf(outs[0])) and np.all(np.isinf(outs[K - 1]))
        fresh = ic.Integrator(mode, period=K)
        for f in frames[2:]:
            want = fresh.push(f)
        np.testing.assert_array_equal(bits(outs[-1]), bits(want))
        assert outs[-1].max() < 3e-20
