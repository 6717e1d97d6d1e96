"""NumPy restatement of the resampler stage (include/sdrg.h, csrc/resample.hip): the polyphase FIR at the rate L / M,
the gain and the quantisation over a stream of concatenated calls, product by product and sum by sum in float32, so the
GPU tests compare bytes.  The prototype is an argument: the tests pass the library's (sdrg.resample_design), so no libm
difference enters a byte comparison; design_formula restates how the library makes it.

Also a float64 model on the same taps and the error bound the float32 sums must stay within."""
import math

import numpy as np

from ddc_cases import taps_formula
from demod_cases import quantise

OUT_S16, OUT_F32 = 0, 1
OUT_DTYPE = {OUT_S16: np.int16, OUT_F32: np.float32}
MAX_FACTOR, MAX_TAPS_PER_PHASE, MAX_TAPS, MAX_IN = 512, 64, 8192, 1 << 20
f32 = np.float32


def ceil_div(a, b):
    return -(-a // b)


def design_formula(L, M, P, cutoff_rel):
    """The stated prototype in double, [L P]: the DDC's low-pass of T = L P (less one if even) coefficients at
    f = cutoff_rel / (2 max(L, M)) cycles per upsampled sample, times L, then zeros; the caller rounds to float."""
    n = L * P
    T = n if n % 2 else n - 1
    f = cutoff_rel / (2.0 * max(L, M))
    k = np.arange(T, dtype=np.float64)
    c = k - (T - 1) // 2
    with np.errstate(invalid="ignore", divide="ignore"):
        ideal = np.where(c == 0, 2.0 * f, np.sin(2.0 * np.pi * f * c) / (np.pi * c))
    v = ideal * (0.5 - 0.5 * np.cos(2.0 * np.pi * (k + 1) / (T + 1)))
    assert np.array_equal(v / v.sum(), taps_formula(1.0, f, T))  # the DDC's formula, before the scale
    h = np.zeros(n)
    h[:T] = float(L) * v / v.sum()
    return h


def valid_config(c):
    """The rules of set_resample on a dict of sdrg_resample_config's fields."""
    L, M, P = c["interp"], c["decim"], c["taps_per_phase"]
    return bool(1 <= L <= MAX_FACTOR and 1 <= M <= MAX_FACTOR and math.gcd(L, M) == 1 and L <= 8 * M and M <= 8 * L and
                1 <= P <= MAX_TAPS_PER_PHASE and L * P <= MAX_TAPS and 0 < c["cutoff_rel"] <= 1 and
                c["components"] in (1, 2) and c["out_format"] in (OUT_S16, OUT_F32) and np.isfinite(c["gain"]) and
                1 <= c["max_in"] <= MAX_IN)


def outputs_of(g, n, L, M):
    """(m0, n_out): the outputs m with g <= floor(m M / L) < g + n are [m0, m0 + n_out)."""
    m0 = ceil_div(g * L, M)
    return m0, ceil_div((g + n) * L, M) - m0


def as_rows(x, B, components):
    """x -> float32 [B][n][components]: real rows [B][n], or complex64 rows [B][n] as (re, im)."""
    if components == 2:
        z = np.ascontiguousarray(np.asarray(x, np.complex64).reshape(B, -1))
        return z.view(np.float32).reshape(B, -1, 2)
    return np.asarray(x, np.float32).reshape(B, -1, 1)


class Resampler:
    """One engine's resampler state: g and, per stream, the last P - 1 input values."""

    def __init__(self, B, L, M, taps, gain=1.0, out_format=OUT_F32, components=1, max_in=None):
        self.B, self.L, self.M, self.out_format, self.components = B, int(L), int(M), out_format, components
        self.max_in, self.gain = max_in, f32(gain)
        self.h = np.asarray(taps, np.float32).copy()
        assert self.h.size % self.L == 0
        self.P = self.h.size // self.L
        self.reset()

    def reset(self):
        self.g = 0
        self.hist = np.zeros((self.B, self.P - 1, self.components), np.float32)

    def call(self, x):
        """x float32 [B][n] (complex64 at components 2) -> (out [B][cap] int16 or float32, [B][cap][2] at components 2,
        zeros from n_out on; n_out)."""
        B, L, M, P, H = self.B, self.L, self.M, self.P, self.P - 1
        v = as_rows(x, B, self.components)
        n = v.shape[1]
        cap = ceil_div((self.max_in if self.max_in is not None else n) * L, M)
        out = np.zeros((B, cap, self.components), OUT_DTYPE[self.out_format])
        shape = (B, cap) if self.components == 1 else (B, cap, 2)
        if n == 0:
            return out.reshape(shape), 0
        ext = np.concatenate([self.hist, v], axis=1)  # ext[:, H + t] = the value at local index t
        m0, n_out = outputs_of(self.g, n, L, M)
        if n_out > 0:
            t = (m0 + np.arange(n_out, dtype=np.int64)) * M
            q, phi = t // L - self.g, t % L
            assert q[0] >= 0 and q[-1] < n
            acc = np.zeros((B, n_out, self.components), np.float32)
            for k in range(P):
                acc = acc + self.h[phi + k * L][None, :, None] * ext[:, H + q - k]
            assert acc.dtype == np.float32
            out[:, :n_out] = quantise(acc * self.gain, self.out_format)
        if H:
            self.hist = ext[:, -H:].copy()
        self.g += n
        return out.reshape(shape), n_out


def model_f64(x, L, M, taps, gain=1.0, components=1):
    """The whole stream at once in float64 on the same float inputs and taps -> (y float64 [B][n_out][components],
    bound_sum float64 [n_out]: sum_k |h[phi + k L]| of each output)."""
    h = np.asarray(taps, np.float64)
    P = h.size // L
    B = np.asarray(x).shape[0]
    v = as_rows(x, B, components).astype(np.float64)
    n = v.shape[1]
    ext = np.concatenate([np.zeros((B, P - 1, components)), v], axis=1)
    _, n_out = outputs_of(0, n, L, M)
    t = np.arange(n_out, dtype=np.int64) * M
    q, phi = t // L, t % L
    y = np.zeros((B, n_out, components))
    s = np.zeros(n_out)
    for k in range(P):
        y += h[phi + k * L][None, :, None] * ext[:, P - 1 + q - k]
        s += np.abs(h[phi + k * L])
    return y * float(gain), s


def error_bound(P, tap_abs_sum, x_max, gain):
    """(P + 1) 2^-24 sum_k |h[phi + k L]| max|x| |gain| per output: the float32 result against model_f64 on the same
    inputs and taps, u = 2^-24.
      products  fl(h x) = h x (1 + d), |d| <= u: one rounding per term.
      sums      acc = +0 + p_0 is exact; the adds at k = 1 .. P - 1 round once each, and the term k passes through the
                adds k' >= max(k, 1): P - 1 of them for k <= 1, fewer for the later terms.
      gain      one more rounding of the whole sum.
    So every term h x carries at most 1 + (P - 1) + 1 = P + 1 factors (1 + d): to first order in u the error is at
    most (P + 1) u sum_k |h[phi + k L]| |x[q - k]| |gain|, and |x[q - k]| <= max|x|.  The second-order part,
    (P + 1) P / 2 u^2 of the same sum, is below 1.3e-4 of the bound at P = 64; the data of the tests are dense noise
    and tones, whose sum |h||x| stays below sum |h| max|x| by far more than that."""
    return (P + 1) * 2.0 ** -24 * np.asarray(tap_abs_sum, np.float64) * float(x_max) * abs(float(gain))


def response(taps, f):
    """H(f) = sum_k h[k] e^{-j 2 pi f k} in float64, f in cycles per upsampled sample."""
    h = np.asarray(taps, np.float64)
    f = np.atleast_1d(np.asarray(f, np.float64))
    k = np.arange(h.size, dtype=np.float64)
    out = np.empty(f.size, np.complex128)
    for i in range(0, f.size, 256):  # blocks: the whole matrix at once would be f.size x 8192 complex numbers
        out[i:i + 256] = np.exp(-2j * np.pi * f[i:i + 256, None] * k[None, :]) @ h
    return out


def noise(B, n, seed, components=1, amp=0.9):
    """Dense rows, each stream its own, uniform in (-amp, amp): float32 [B][n], or complex64 [B][n] at components 2."""
    rng = np.random.default_rng(seed)
    v = ((rng.random((B, components * n)) * 2 - 1) * amp).astype(np.float32)
    return v.view(np.complex64) if components == 2 else v
