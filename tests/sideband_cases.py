"""NumPy restatement of the sideband stage (include/sdrg.h, csrc/sideband.hip): the two real sums per output, the
sideband's difference or sum, decimation, gain and quantisation over a stream of concatenated calls, operation by
operation in float32, so the GPU tests compare bytes.  cr and ci are arguments: the tests pass the library's
(sdrg.sideband_design), so no libm difference enters a byte comparison; design_formula restates how the library makes
them.

Also a float64 model of the same pipeline (the same float taps, direct convolution) and the error budget the float32
pipeline must stay within."""
import numpy as np

from ddc_cases import n_out_for, taps_formula

UPPER, LOWER, BOTH = 0, 1, 2
OUT_S16, OUT_F32 = 0, 1
OUT_DTYPE = {OUT_S16: np.int16, OUT_F32: np.float32}
MAX_TAPS, MAX_DECIMATION, MAX_IN = 511, 64, 1 << 20
f32 = np.float32


def design_formula(fc, low_hz, high_hz, T):
    """(cr, ci) in double; the caller rounds to float.  p is the DDC's prototype at f = (high - low) / (2 fc), which
    taps_formula takes as cutoff / rate; theta_k = 2 pi fm (k - (T - 1) / 2) / fc at the band's middle fm."""
    p = taps_formula(fc, (float(high_hz) - float(low_hz)) / 2.0, T)
    fm = (float(low_hz) + float(high_hz)) / 2.0
    theta = 2.0 * np.pi * fm * (np.arange(T, dtype=np.float64) - (T - 1) // 2) / float(fc)
    return p * np.cos(theta), p * np.sin(theta)


def valid_config(c):
    """The rules of set_sideband on a dict of sdrg_sideband_config's fields."""
    fin = np.isfinite
    return bool(fin(c["channel_rate_hz"]) and c["channel_rate_hz"] > 0 and fin(c["low_hz"]) and fin(c["high_hz"]) and
                0 <= c["low_hz"] < c["high_hz"] <= c["channel_rate_hz"] / 2 and c["mode"] in (UPPER, LOWER, BOTH) and
                1 <= c["audio_decimation"] <= MAX_DECIMATION and 1 <= c["taps"] <= MAX_TAPS and c["taps"] % 2 == 1 and
                c["out_format"] in (OUT_S16, OUT_F32) and 1 <= c["max_in"] <= MAX_IN and fin(c["gain"]))


def quantise(o, out_format):
    """_F32: o; _S16: (int16) rintf(min(max(o, -1), 1) * 32767.0f), ties to even."""
    o = np.asarray(o, f32)
    if out_format == OUT_F32:
        return o
    return np.rint(np.minimum(np.maximum(o, f32(-1)), f32(1)) * f32(32767)).astype(np.int16)


class Sideband:
    """One engine's sideband state: g and, per stream, the last T - 1 samples."""

    def __init__(self, B, cr, ci, R, mode=UPPER, gain=1.0, out_format=OUT_F32, max_in=None):
        self.B, self.R, self.mode, self.out_format, self.max_in = B, int(R), mode, out_format, max_in
        self.gain = f32(gain)
        self.cr, self.ci = np.asarray(cr, np.float32).copy(), np.asarray(ci, np.float32).copy()
        assert self.cr.shape == self.ci.shape and self.cr.ndim == 1
        self.T = self.cr.size
        self.reset()

    def reset(self):
        self.g = 0
        self.hr = np.zeros((self.B, self.T - 1), np.float32)
        self.hi = np.zeros((self.B, self.T - 1), np.float32)

    def call(self, chan):
        """chan complex64 [B][n] -> (out [B][cap] int16 or float32, [B][cap][2] at BOTH, zeros from n_out on; n_out)."""
        B, R, T, H = self.B, self.R, self.T, self.T - 1
        z = np.asarray(chan, np.complex64).reshape(B, -1)
        n = z.shape[1]
        cap = -(-(self.max_in if self.max_in is not None else n) // R)
        out = np.zeros((B, cap, 2) if self.mode == BOTH else (B, cap), OUT_DTYPE[self.out_format])
        if n == 0:
            return out, 0
        er = np.concatenate([self.hr, np.ascontiguousarray(z.real)], axis=1)  # er[:, H + t] = zr at local index t
        ei = np.concatenate([self.hi, np.ascontiguousarray(z.imag)], axis=1)
        n_out = n_out_for(self.g, n, R)
        first = (-self.g) % R
        if n_out > 0:
            at = H + first + R * np.arange(n_out)
            ax = np.zeros((B, n_out), np.float32)
            ay = np.zeros((B, n_out), np.float32)
            for k in range(T):
                ax = ax + self.cr[k] * er[:, at - k]
                ay = ay + self.ci[k] * ei[:, at - k]
            u, lo = ax - ay, ax + ay
            assert u.dtype == np.float32 and lo.dtype == np.float32
            if self.mode == BOTH:
                out[:, :n_out, 0] = quantise(u * self.gain, self.out_format)
                out[:, :n_out, 1] = quantise(lo * self.gain, self.out_format)
            else:
                out[:, :n_out] = quantise((u if self.mode == UPPER else lo) * self.gain, self.out_format)
        if H:
            self.hr, self.hi = er[:, -H:].copy(), ei[:, -H:].copy()
        self.g += n
        return out, n_out


def model_f64(chan, cr, ci, R, gain=1.0):
    """The whole stream at once in float64 on the same CF32 samples and float taps, direct convolution:
    -> float64 [B][ceil(n / R)][2], the columns (u gain, l gain)."""
    z = np.asarray(chan, np.complex64).astype(np.complex128)
    B, n = z.shape
    cr, ci = np.asarray(cr, np.float64), np.asarray(ci, np.float64)
    T = cr.size
    ext = np.concatenate([np.zeros((B, T - 1), np.complex128), z], axis=1)
    at = T - 1 + R * np.arange(-(-n // R))
    a, bm = np.zeros((B, at.size)), np.zeros((B, at.size))
    for k in range(T):
        a += cr[k] * ext[:, at - k].real
        bm += ci[k] * ext[:, at - k].imag
    return np.stack([a - bm, a + bm], axis=-1) * float(gain)


def error_bound(T, max_abs_z, cr, ci, gain=1.0):
    """The float32 pipeline against model_f64 on the same samples and taps, per output; u = 2^-24, M >= max(|zr|, |zi|),
    S = sum|cr| + sum|ci|.
      sums      each of the T terms of acc.x is rounded once as a product and at most T - 1 times more in the sums
                behind it (the first sum, +0 + x, is exact): |d acc.x| <= T u M sum|cr| to first order, and the same for
                acc.y with ci.
      sideband  acc.x -+ acc.y rounds by u |acc.x -+ acc.y| <= u M S: |d u|, |d l| <= (T + 1) u M S.
      gain      the product rounds by u |o| <= u |gain| M S: |d o| <= (T + 2) u |gain| M S.
      the rest  the terms of second order are (1 + u)^(T + 2) - 1 - (T + 2) u < u for T <= 511 (513^2 u < 1/60), which
                the bound takes whole: (T + 3) u |gain| M S.
    A product below the smallest normal float is rounded by at most 2^-150 absolutely in place of u relatively: 2 T of
    them, and the last product, add (2 T + 1) 2^-150 max(1, |gain|)."""
    u = 2.0 ** -24
    S = float(np.abs(np.asarray(cr, np.float64)).sum() + np.abs(np.asarray(ci, np.float64)).sum())
    g = abs(float(gain))
    return (T + 3) * u * float(max_abs_z) * S * g + (2 * T + 1) * 2.0 ** -150 * max(1.0, g)


def response(cr, ci, f_rel):
    """C(f) of c = cr + j ci at f_rel cycles per input sample, in double: the upper sideband's gain at +f_rel."""
    c = np.asarray(cr, np.float64) + 1j * np.asarray(ci, np.float64)
    return np.sum(c * np.exp(-2j * np.pi * f_rel * np.arange(c.size)))


def tone(B, n, f_rel, amp=0.5, phase=0.0):
    """A complex tone at f_rel cycles per sample, in double, rounded to CF32: [B][n] (the same on every stream)."""
    t = np.arange(n, dtype=np.float64)
    z = (amp * np.exp(2j * np.pi * f_rel * t + 1j * phase)).astype(np.complex64)
    return np.ascontiguousarray(np.broadcast_to(z, (B, n)))


# ---- the behavioural case: two CS8 tones of amplitude 50 at +251.0 kHz and +248.5 kHz, fs 2 MHz; DDC at +250 kHz,
# D = 41, T = 255, cutoff 4 kHz: the tones sit at +1000 Hz and -1500 Hz of a channel at 2 MHz / 41.  Sideband BOTH,
# 300 - 2700 Hz, T = 511, R = 1.

TWO_TONE_FS, TWO_TONE_N, TWO_TONE_FRAMES, TWO_TONE_SETTLED = 2_000_000, 16384, 12, 4096
TWO_TONE_DDC = dict(offset_hz=250_000.0, cutoff_hz=4000.0, decimation=41, taps=255)
TWO_TONE_SIDEBAND = dict(channel_rate_hz=TWO_TONE_FS / 41, low_hz=300.0, high_hz=2700.0, mode=BOTH, audio_decimation=1,
                         taps=511, out_format=OUT_F32, max_in=400, gain=1.0)


def two_tone_raw(B=1):
    """CS8 [B][2 N frames]: 50 e^{j 2 pi 251 kHz t} + 50 e^{j 2 pi 248.5 kHz t}, in LSB, rounded."""
    t = np.arange(TWO_TONE_N * TWO_TONE_FRAMES, dtype=np.float64) / TWO_TONE_FS
    z = 50.0 * np.exp(2j * np.pi * 251_000.0 * t) + 50.0 * np.exp(2j * np.pi * 248_500.0 * t + 0.4j)
    raw = np.empty(2 * t.size, np.int8)
    raw[0::2], raw[1::2] = np.round(z.real).astype(np.int8), np.round(z.imag).astype(np.int8)
    return np.ascontiguousarray(np.broadcast_to(raw, (B, raw.size)))


def two_tone_separation_db(column):
    """Over the last 4096 outputs of a column under a Hann window: (the strongest bin, the 1 kHz bin, the 1.5 kHz bin,
    the 1 kHz bin's level over the 1.5 kHz bin's in dB)."""
    y = np.asarray(column, np.float64)[-TWO_TONE_SETTLED:]
    assert y.size == TWO_TONE_SETTLED
    spec = np.abs(np.fft.rfft(y * np.hanning(y.size)))
    fc = TWO_TONE_FS / 41
    k1, k15 = int(round(1000.0 / fc * y.size)), int(round(1500.0 / fc * y.size))
    return int(np.argmax(spec)), k1, k15, 20.0 * np.log10(spec[k1] / spec[k15])


def noise(B, n, seed, amp=0.9):
    """Dense CF32 rows, each stream its own: components uniform in (-amp, amp)."""
    rng = np.random.default_rng(seed)
    v = ((rng.random((B, 2 * n)) * 2 - 1) * amp).astype(np.float32)
    return v.view(np.complex64)
