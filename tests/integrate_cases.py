"""The integration stage (include/sdrg.h, sdrg_engine_integrate_*) restated in NumPy, and the inputs its tests share.

Per bin, with t counting the calls since the last reset, x_t this call's value and c = min(t + 1, period):
  MEAN  S = (double)x_{t-c+1}; S = S + (double)x_i for i = t-c+2 .. t, one float64 `+` at a time in that order;
        out = (float)(S / (double)c).
  MAX   the largest of those c values.
  EMA   y = x at t = 0, else d = x - y; y = y + alpha * d in float32, one operation at a time; out = y.
Integrator holds the history (the last `period` input rows, or y) and returns each call's output.
tests/test_integrate_cases.py checks the restatement itself, tests/test_gpu_integrate.py the kernels against it."""
import numpy as np

f32 = np.float32
MEAN, MAX, EMA = 0, 1, 2
MAX_PERIOD = 64

# One bin, period 4, frames oldest -> newest.  Added in that order in double the sum is 2^24 + 1 + 2^-28 exactly and
# the mean rounds up to 4194304.5; added newest first, or in a float, or (B) pairwise, the 2^-29s are lost below the
# double's (or the float's) last place beside 2^24, the mean is the tie 4194304.25 and rounds to even, 4194304.0.
ORDER_PROBE_A = np.array([2.0 ** -29, 2.0 ** -29, 1.0, 2.0 ** 24], dtype=np.float32)
ORDER_PROBE_B = np.array([2.0 ** -29, 1.0, 2.0 ** -29, 2.0 ** 24], dtype=np.float32)
ORDER_PROBE_MEAN = f32(4194304.5)


class Integrator:
    def __init__(self, mode: int, period: int = 1, alpha: float = 0.0):
        assert mode in (MEAN, MAX, EMA)
        assert mode == EMA or 1 <= period <= MAX_PERIOD
        self.mode, self.period, self.alpha = mode, int(period), f32(alpha)
        self.reset()

    def reset(self) -> None:
        self.hist, self.y, self.t = [], None, 0

    @property
    def depth(self) -> int:
        """The number of frames the last output integrates (0 after a reset)."""
        return self.t if self.mode == EMA else min(self.t, self.period)

    def push(self, rows) -> np.ndarray:
        x = np.array(rows, dtype=np.float32, copy=True)
        self.t += 1
        if self.mode == EMA:
            if self.y is None:
                self.y = x
            else:
                d = (x - self.y).astype(np.float32)
                self.y = (self.y + (self.alpha * d).astype(np.float32)).astype(np.float32)
            return self.y.copy()
        self.hist = (self.hist + [x])[-self.period:]
        if self.mode == MAX:
            m = self.hist[0]
            for h in self.hist[1:]:
                m = np.maximum(m, h)
            return m.copy()
        with np.errstate(over="ignore", invalid="ignore"):
            s = self.hist[0].astype(np.float64)
            for h in self.hist[1:]:  # oldest first
                s = s + h.astype(np.float64)
            return (s / np.float64(len(self.hist))).astype(np.float32)


def mean_in_order(values, dtype=np.float64) -> np.float32:
    """(float)(S / c) of one bin's values added in the order given, in an accumulator of `dtype`."""
    s = dtype(values[0])
    for v in values[1:]:
        s = dtype(s + dtype(v))
    return f32(np.float64(s) / np.float64(len(values)))


def mean_pairwise(values) -> np.float32:
    """The same with the values added as a balanced tree of float64 sums."""
    v = [np.float64(x) for x in values]
    while len(v) > 1:
        v = [v[i] + v[i + 1] if i + 1 < len(v) else v[i] for i in range(0, len(v), 2)]
    return f32(v[0] / np.float64(len(values)))


def spread_frames(F: int, B: int, n: int, seed: int) -> np.ndarray:
    """[F][B][n] powers m * 2^e, m in [1, 2), e uniform in [-30, 30]: consecutive values of a bin differ by up to 2^60,
    so a float accumulator rounds the mean of many bins differently from a double one.  (Another order of the double
    additions seldom survives the rounding to float on such data: the order probes are there for that.)"""
    rng = np.random.default_rng(seed)
    m = rng.uniform(1.0, 2.0, size=(F, B, n))
    e = rng.integers(-30, 31, size=(F, B, n))
    return np.ldexp(m, e).astype(np.float32)


def order_probes(period: int):
    """(a, b, mean): two sequences of `period` values, oldest -> newest, whose mean is `mean` in the stated order and
    one float ulp less in others.  period 4: ORDER_PROBE_A and _B.  period 8, 16, 32, 64 (the tie needs a power of two):
    a is A with zeros between the 2^-29s and the 1, which the reverse order and a float accumulator get wrong; b has
    2^24 in the middle and the 1 last, which also a swap of the two halves (batches of loads added newest first) gets
    wrong."""
    assert period in (4, 8, 16, 32, 64)
    if period == 4:
        return ORDER_PROBE_A, ORDER_PROBE_B, ORDER_PROBE_MEAN
    a = np.zeros(period, np.float32)
    a[:2], a[-2], a[-1] = 2.0 ** -29, 1.0, 2.0 ** 24
    b = np.zeros(period, np.float32)
    b[:2], b[period // 2], b[-1] = 2.0 ** -29, 2.0 ** 24, 1.0
    return a, b, f32((2.0 ** 24 + 1.0 + 2.0 ** -28) / period)


def probe_bins(n: int):
    """Bins that carry probe a and probe b: the row's first and last bin and the bins on both sides of a float4
    boundary, as far as the row has them (disjoint; b may be empty for tiny rows)."""
    a = sorted({j for j in (0, 3, n - 1, n // 2) if 0 <= j < n})
    b = sorted({j for j in (4, 1, n - 2) if 0 <= j < n} - set(a))
    return a, b


def place_order_probes(frames: np.ndarray, period: int = 4) -> np.ndarray:
    """Overwrite the probe bins of every stream: frame f carries element f % period of order_probes(period), so every
    call t with t % period == period - 1 integrates exactly the probes, oldest first."""
    F, _, n = frames.shape
    pa, pb, _ = order_probes(period)
    a, b = probe_bins(n)
    for f in range(F):
        frames[f][:, a] = pa[f % period]
        frames[f][:, b] = pb[f % period]
    return frames


def residue_frames(period: int, B: int, n: int, seed: int) -> np.ndarray:
    """[period + 2][B][n]: one frame of +inf, one of 1e30f, then `period` frames of powers around 1e-20f."""
    rng = np.random.default_rng(seed)
    quiet = (rng.uniform(0.5, 2.0, size=(period, B, n)) * 1e-20).astype(np.float32)
    head = np.stack([np.full((B, n), np.inf, np.float32), np.full((B, n), f32(1e30), np.float32)])
    return np.concatenate([head, quiet])


def dyadic_frames(F: int, B: int, n: int, seed: int) -> np.ndarray:
    """[F][B][n] powers k / 16, k in [0, 4096): every EMA step with alpha = 0.5 is exact for a few frames."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 4096, size=(F, B, n)) / 16.0).astype(np.float32)
