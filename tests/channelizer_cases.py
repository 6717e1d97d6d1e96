"""NumPy restatement of the channelizer stage (include/sdrg.h, csrc/channelizer.hip): a uniform polyphase filter bank of
M channels over a stream of concatenated calls.  The stage is specified by an error bound, not by its bytes, so there are
two models on the exactly unpacked input (ddc_cases.unpack): the float32 restatement (branch sums tap by tap in float32,
a complex64 FFT) and the float64 model (float64 branch sums, np.fft), with the bound per output time

    bound[m] = (P + 2) eps sum_n |h[n]| |x[m D - n]|  +  8 log2(M) eps sqrt(M) ||u[m]||_2,     eps = 2^-24:

one rounding per product and per sum of a branch, carried through the unit-modulus DFT, plus Higham's FFT bound
(Accuracy and Stability of Numerical Algorithms, Theorem 24.2) with eta <= 8 eps, which leaves room for factored
twiddles.  The bound is derived, not tuned.  The taps are an argument: the tests pass the library's
(sdrg.channelizer_design)."""
import numpy as np

import ddc_cases as dd

CF32, CS8, CU8, CS16 = dd.CF32, dd.CS8, dd.CU8, dd.CS16
MAX_CHANNELS, MAX_TAPS_PER_CHANNEL, MAX_TAPS = 256, 32, 4096
EPS = 2.0 ** -24
CHUNK = 1 << 21  # window elements gathered at a time


def valid_config(cutoff_rel, M, P, O, first, n):
    return bool(2 <= M <= MAX_CHANNELS and M & (M - 1) == 0 and 1 <= P <= MAX_TAPS_PER_CHANNEL and M * P <= MAX_TAPS and
                O in (1, 2) and 0 < cutoff_rel <= M / 2 and n >= 1 and first >= 0 and first + n <= M)


def taps_formula(cutoff_rel, M, P):
    """The stated prototype in double: ddc_cases.taps_formula at f = cutoff_rel / M, T = L - 1, then a 0."""
    return np.concatenate([dd.taps_formula(float(M), float(cutoff_rel), M * P - 1), [0.0]])


def n_out_for(g0, n, D):
    return dd.n_out_for(g0, n, D)


def channel_of_row(k, M):
    """Row k of the fftshifted order is channel c, centred at c fs / M (c >= M / 2: negative)."""
    return (k + M // 2) % M


def _bank(e, first, n_out, m0, h, M, P, O, single):
    """e [B][L - 1 + N] complex: the samples before the frame, then the frame.  Output j in [0, n_out) has its newest
    sample at e[:, L - 1 + first + j D] and the global time m0 + j.  Returns y [B][M][n_out] in the fftshifted row order
    and, from the float64 model, bound [B][n_out]."""
    B, L, D = e.shape[0], M * P, M // O
    ctype, rtype = (np.complex64, np.float32) if single else (np.complex128, np.float64)
    hq = np.asarray(h, rtype).reshape(P, M)
    y = np.zeros((B, M, n_out), ctype)
    bound = np.zeros((B, n_out), np.float64)
    k = np.arange(M)
    c = channel_of_row(k, M)
    step = max(1, CHUNK // (B * L))
    for a in range(0, n_out, step):
        j = np.arange(a, min(a + step, n_out))
        at = (L - 1 + first + j * D)[:, None] - np.arange(L)[None, :]   # [j][n], n = p + q M
        w = e[:, at].reshape(B, j.size, P, M)
        u = np.zeros((B, j.size, M), ctype)
        for q in range(P):  # q ascending, a rounded product and a rounded sum per tap in the float32 restatement
            u = u + hq[q] * w[:, :, q, :]
        assert u.dtype == ctype
        F = np.fft.fft(u, axis=-1).astype(ctype)
        Y = F[:, :, (M - c) % M]                                        # Y_c = F[(M - c) mod M], rows in k order
        if O == 2:
            sign = 1.0 - 2.0 * ((c[None, :] * (m0 + j)[:, None]) & 1)   # (-1)^{c m}
            Y = Y * sign.astype(rtype)[None]
        y[:, :, j] = np.swapaxes(Y, 1, 2)
        if not single:
            s1 = (np.abs(w) * np.abs(hq)).sum(axis=(2, 3))
            bound[:, j] = (P + 2) * EPS * s1 + 8 * np.log2(M) * EPS * np.sqrt(M) * np.sqrt((np.abs(u) ** 2).sum(-1))
    return y, bound


def exact_samples(fmt, raw):
    """raw [B][2 N] -> the exactly unpacked float32 samples as complex64 [B][N]."""
    xr, xi = dd.unpack(fmt, np.asarray(raw).reshape(np.asarray(raw).shape[0], -1))
    return (xr + 1j * xi).astype(np.complex64)


class Bank:
    """Follows one engine's channelizer call by call: g0 and, per stream, the last L - 1 unpacked samples.  call()
    returns both models of the call's outputs: every row of the bank; the engine writes rows [first, first + n)."""

    def __init__(self, B, taps, M, P, O):
        self.B, self.M, self.P, self.O, self.D, self.L = B, M, P, O, M // O, M * P
        self.h = np.asarray(taps, np.float32).copy()
        assert self.h.size == self.L
        self.reset()

    def reset(self):
        self.g0 = 0
        self.hist = np.zeros((self.B, self.L - 1), np.complex64)

    def call(self, fmt, raw, restate=True):
        """raw [B][2 N] -> (y32 complex64 [B][M][n_out], y64 complex128 [B][M][n_out], bound [B][n_out], m0, n_out);
        y32 is None without restate (the GPU tests compare against y64 only)."""
        x = exact_samples(fmt, raw)
        n, D = x.shape[1], self.D
        e = np.concatenate([self.hist, x], axis=1)
        n_out, first, m0 = n_out_for(self.g0, n, D), (-self.g0) % D, -(-self.g0 // D)
        y32 = _bank(e, first, n_out, m0, self.h, self.M, self.P, self.O, True)[0] if restate else None
        y64, bound = _bank(e.astype(np.complex128), first, n_out, m0, self.h, self.M, self.P, self.O, False)
        self.hist = e[:, e.shape[1] - (self.L - 1):].copy()
        self.g0 += n
        return y32, y64, bound, m0, n_out


def model_f32(fmt, raw, taps, M, P, O):
    """The whole stream at once through the float32 restatement: complex64 [B][M][ceil(N / D)]."""
    return Bank(np.asarray(raw).shape[0], taps, M, P, O).call(fmt, raw)[0]


def model_f64(fmt, raw, taps, M, P, O):
    """The whole stream at once in float64: (y complex128 [B][M][ceil(N / D)], bound [B][ceil(N / D)])."""
    r = Bank(np.asarray(raw).shape[0], taps, M, P, O).call(fmt, raw)
    return r[1], r[2]


def assert_within(got, want, bound, m0, P, O, what=None):
    """|got - want| <= bound for every output (got, want [B][rows][n], bound [B][n], the outputs' global times m0 ..),
    and the input condition: over the outputs with m >= P O (windows past the zero prefix) the bound must tell the right
    value from +0, from the neighbouring row's value and from the previous output time's value in all but 1e-3 of the
    outputs, or the comparison would prove nothing."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and bound.shape == (want.shape[0], want.shape[2]), (what, got.shape, want.shape)
    bb = bound[:, None, :]
    err = np.abs(got.astype(np.complex128) - want)
    worst = float((err / np.maximum(bb, 1e-300)).max()) if err.size else 0.0
    assert np.all(err <= bb), (what, "worst error / bound", worst)
    past = (m0 + np.arange(want.shape[2])) >= P * O
    if past.sum() >= 2 and want.shape[1] >= 1:
        w, b2 = want[:, :, past], bb[:, :, past]
        assert np.mean(np.abs(w) <= b2) <= 1e-3, (what, "+0 would pass")
        if w.shape[1] > 1:
            assert np.mean(np.abs(w[:, 1:] - w[:, :-1]) <= b2) <= 1e-3, (what, "the neighbouring channel would pass")
        assert np.mean(np.abs(w[:, :, 1:] - w[:, :, :-1]) <= b2[:, :, 1:]) <= 1e-3, (what, "the previous output would pass")
    return worst
