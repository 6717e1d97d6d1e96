"""NumPy restatement of the demodulator stage (include/sdrg.h, csrc/demod.hip): detector, DC block, de-emphasis, FIR and
decimation, gain and quantisation over a stream of concatenated calls, operation by operation in float32, so the GPU
tests compare bytes.  kf, alpha, a and the taps are arguments: the tests pass the library's (sdrg.demod_design), so no
libm difference enters a byte comparison; design_formula restates how the library makes them.

Also a float64 model of the same pipeline (exact arctan2 and hypot, the same constants and taps) and the error budget
the float32 pipeline must stay within."""
import numpy as np

from ddc_cases import n_out_for, taps_formula

AM, FM = 0, 1
OUT_S16, OUT_F32 = 0, 1
OUT_DTYPE = {OUT_S16: np.int16, OUT_F32: np.float32}
MAX_TAPS, MAX_DECIMATION, MAX_IN = 255, 64, 1 << 20
f32 = np.float32

ATAN_C = tuple(f32(float.fromhex(c)) for c in (
    "0x1.ffffecp-1", "-0x1.554ce6p-2", "0x1.988d5p-3", "-0x1.1d09a6p-3", "0x1.8bc022p-4", "-0x1.cbe51p-5",
    "0x1.68671ep-6", "-0x1.0bce58p-8"))
PI_2, PI = f32(float.fromhex("0x1.921fb6p+0")), f32(float.fromhex("0x1.921fb6p+1"))


def atan2f(y, x):
    """sdrg_atan2f of sdrg.h: every operation in float32, in its order."""
    y, x = np.asarray(y, f32), np.asarray(x, f32)
    ax, ay = np.abs(x), np.abs(y)
    mx, mn = np.maximum(ax, ay), np.minimum(ax, ay)
    pos = mx > 0
    q = np.where(pos, mn / np.where(pos, mx, f32(1)), f32(0))
    s = q * q
    p = np.full(q.shape, ATAN_C[7], f32)
    for k in range(6, -1, -1):
        p = p * s + ATAN_C[k]
    r = p * q
    r = np.where(ay > ax, PI_2 - r, r)
    r = np.where(np.signbit(x), PI - r, r)
    r = np.copysign(r, y)
    assert r.dtype == np.float32
    return r


def design_formula(mode, fc, deviation_hz, dc_cutoff_hz, deemphasis_us, audio_cutoff_hz, T2):
    """(kf, alpha, a, taps) in double; the caller rounds to float."""
    kf = fc / (2.0 * np.pi * deviation_hz) if mode == FM else 0.0
    alpha = 1.0 - np.exp(-2.0 * np.pi * dc_cutoff_hz / fc)
    a = 1.0 - np.exp(-1.0 / (fc * deemphasis_us * 1e-6)) if deemphasis_us > 0 else 0.0
    return kf, alpha, a, taps_formula(fc, audio_cutoff_hz, T2)


def valid_config(c):
    """The rules of set_demod on a dict of sdrg_demod_config's fields."""
    fin = np.isfinite
    ok = c["mode"] in (AM, FM) and fin(c["channel_rate_hz"]) and c["channel_rate_hz"] > 0
    if ok and c["mode"] == FM:
        with np.errstate(over="ignore"):
            ok = bool(fin(c["deviation_hz"]) and c["deviation_hz"] > 0 and
                      fin(f32(c["channel_rate_hz"] / (2.0 * np.pi * c["deviation_hz"]))))
    return bool(ok and fin(c["dc_cutoff_hz"]) and c["dc_cutoff_hz"] >= 0 and fin(c["deemphasis_us"]) and
                c["deemphasis_us"] >= 0 and 1 <= c["audio_decimation"] <= MAX_DECIMATION and
                1 <= c["audio_taps"] <= MAX_TAPS and c["audio_taps"] % 2 == 1 and
                0 < c["audio_cutoff_hz"] <= c["channel_rate_hz"] / 2 and fin(c["gain"]) and
                c["out_format"] in (OUT_S16, OUT_F32) and 1 <= c["max_in"] <= MAX_IN)


def quantise(o, out_format):
    """_F32: o; _S16: (int16) rintf(min(max(o, -1), 1) * 32767.0f), ties to even."""
    o = np.asarray(o, f32)
    if out_format == OUT_F32:
        return o
    return np.rint(np.minimum(np.maximum(o, f32(-1)), f32(1)) * f32(32767)).astype(np.int16)


class Demod:
    """One engine's demodulator state: g and, per stream, w, m, s and the last T2 - 1 values of v."""

    def __init__(self, B, mode, kf, alpha, a, taps, R, gain=1.0, out_format=OUT_F32, max_in=None):
        self.B, self.mode, self.R, self.out_format, self.max_in = B, mode, int(R), out_format, max_in
        self.kf, self.alpha, self.a, self.gain = f32(kf), f32(alpha), f32(a), f32(gain)
        self.h = np.asarray(taps, np.float32).copy()
        self.T = self.h.size
        self.reset()

    def reset(self):
        B = self.B
        self.g = 0
        self.w = np.zeros(B, np.complex64)
        self.m = np.zeros(B, np.float32)
        self.s = np.zeros(B, np.float32)
        self.hist = np.zeros((B, self.T - 1), np.float32)

    def detect(self, z):
        """z complex64 [B][n] -> e float32 [B][n]; self.w becomes the call's last sample."""
        zr, zi = np.ascontiguousarray(z.real), np.ascontiguousarray(z.imag)
        if self.mode == AM:
            e = np.sqrt(zr * zr + zi * zi)
        else:
            prev = np.concatenate([self.w[:, None], z[:, :-1]], axis=1)
            wr, wi = np.ascontiguousarray(prev.real), np.ascontiguousarray(prev.imag)
            pr = zr * wr + zi * wi
            pi = zi * wr - zr * wi
            e = atan2f(pi, pr) * self.kf
            if self.g == 0:
                e[:, 0] = f32(0)
        assert e.dtype == np.float32
        self.w = z[:, -1].copy()
        return e

    def recur(self, e):
        """The DC block and the de-emphasis, sample by sample: e [B][n] -> v [B][n]."""
        if self.alpha == 0 and self.a == 0:
            return e
        v = np.empty_like(e)
        m, s, alpha, a = self.m, self.s, self.alpha, self.a
        for i in range(e.shape[1]):
            u = e[:, i]
            if alpha != 0:
                u = u - m
                m = m + alpha * u
            if a != 0:
                t = u - s
                s = s + a * t
                u = s
            v[:, i] = u
        assert m.dtype == np.float32 and s.dtype == np.float32
        self.m, self.s = m, s
        return v

    def call(self, chan):
        """chan complex64 [B][n] -> (out [B][cap] int16 or float32, zeros from n_out on; n_out)."""
        B, R, T, H = self.B, self.R, self.T, self.T - 1
        z = np.asarray(chan, np.complex64).reshape(B, -1)
        n = z.shape[1]
        cap = -(-(self.max_in if self.max_in is not None else n) // R)
        out = np.zeros((B, cap), OUT_DTYPE[self.out_format])
        if n == 0:
            return out, 0
        v = self.recur(self.detect(z))
        ext = np.concatenate([self.hist, v], axis=1)  # ext[:, H + t] = v at local index t
        n_out = n_out_for(self.g, n, R)
        first = (-self.g) % R
        if n_out > 0:
            at = H + first + R * np.arange(n_out)
            acc = np.zeros((B, n_out), np.float32)
            for k in range(T):
                acc = acc + self.h[k] * ext[:, at - k]
            assert acc.dtype == np.float32
            out[:, :n_out] = quantise(acc * self.gain, self.out_format)
        if H:
            self.hist = ext[:, -H:].copy()
        self.g += n
        return out, n_out


def model_f64(mode, chan, kf, alpha, a, taps, R, gain=1.0):
    """The whole stream at once in float64 on the same CF32 samples: exact hypot / arctan2, the same (float) constants
    and taps, direct convolution.  -> (audio float64 [B][ceil(n / R)], e float64 [B][n])."""
    z = np.asarray(chan, np.complex64).astype(np.complex128)
    B, n = z.shape
    if mode == AM:
        e = np.abs(z)
    else:
        p = z * np.conj(np.concatenate([np.zeros((B, 1), np.complex128), z[:, :-1]], axis=1))
        e = np.arctan2(p.imag, p.real) * float(kf)
        e[:, 0] = 0.0
    v = e.copy()
    alpha, a = float(alpha), float(a)
    if alpha != 0 or a != 0:
        m, s = np.zeros(B), np.zeros(B)
        for i in range(n):
            u = e[:, i]
            if alpha != 0:
                u = u - m
                m = m + alpha * u
            if a != 0:
                s = s + a * (u - s)
                u = s
            v[:, i] = u
    h = np.asarray(taps, np.float64)
    T = h.size
    ext = np.concatenate([np.zeros((B, T - 1)), v], axis=1)
    at = T - 1 + R * np.arange(-(-n // R))
    y = np.zeros((B, at.size))
    for k in range(T):
        y += h[k] * ext[:, at - k]
    return y * float(gain), e


def error_bound(alpha, a, taps, gain, kf, E):
    """The FM pipeline in float32 against model_f64 on the same samples, |z| the same at both ends of a step; u = 2^-24,
    E >= max |e|.
      detector  pr and pi: two rounded products and a rounded sum each, 3 u |z||w| per component, an angle of at most
                sqrt(2) 3 u < 4.3 u; sdrg_atan2f within 5e-7 rad of arctan2 on floats (tests/test_demod_cases.py); the
                product with kf u |e| <= pi u kf: d_e = kf (5e-7 + 8 u).
      DC block  u = e - m has gain 1 + sum alpha (1 - alpha)^k = 2 on an input error; per step the product and the sum
                put at most u (2 alpha E + E) into m, which forgets at the rate alpha: u E (2 + 1 / alpha), and the
                subtraction rounds by u 2 E: d_u = 2 d_e + u E (4 + 1 / alpha), |u| <= U = 2 E.
      de-emph   gain 1; per step the subtraction (scaled by a), the product and the sum put at most u U (4 a + 1) into
                s, which forgets at the rate a: d_v = d_u + u U (4 + 1 / a), |v| <= U.
      FIR       one rounding per product and per sum: d_y = sum|h| (d_v + (T2 + 1) u U)  (U = E without the DC block).
      gain      d_o = |gain| d_y (1 + u) + u |gain| U sum|h|."""
    u = 2.0 ** -24
    alpha, a, gain, kf, E = float(alpha), float(a), abs(float(gain)), float(kf), float(E)
    sh = float(np.abs(np.asarray(taps, np.float64)).sum())
    d = kf * (5e-7 + 8 * u)
    U = E
    if alpha != 0:
        d = 2 * d + u * E * (4 + 1 / alpha)
        U = 2 * E
    if a != 0:
        d = d + u * U * (4 + 1 / a)
    d = sh * (d + (len(taps) + 1) * u * U)
    return gain * d * (1 + u) + u * gain * U * sh


def fm_tone(B, n, fc, f_mod, beta, amp=0.5, carrier_hz=0.0):
    """phi[i] = 2 pi carrier i / fc + beta_b sin(2 pi f_mod i / fc) in float64 (the phase integral of a frequency
    carrier + beta f_mod cos(2 pi f_mod t)), z = amp e^{j phi} rounded to CF32; beta_b = beta (b + 1) / B."""
    i = np.arange(n, dtype=np.float64)
    betas = beta * (np.arange(B) + 1.0) / B
    phi = 2.0 * np.pi * carrier_hz * i / fc + betas[:, None] * np.sin(2.0 * np.pi * f_mod * i / fc)
    return (amp * np.exp(1j * phi)).astype(np.complex64)


def noise(B, n, seed, amp=0.9):
    """Dense CF32 rows, each stream its own: components uniform in (-amp, amp)."""
    rng = np.random.default_rng(seed)
    v = ((rng.random((B, 2 * n)) * 2 - 1) * amp).astype(np.float32)
    return v.view(np.complex64)
