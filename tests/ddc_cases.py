"""NumPy restatement of the DDC stage (include/sdrg.h, csrc/ddc.hip): unpack, NCO mix, FIR and decimation over a stream
of concatenated calls, operation by operation in float32, so the GPU tests compare bytes.  The taps and the phasor tables
are arguments: the tests pass the library's (sdrg.ddc_design, sdrg.nco_tables), so no libm difference enters a byte
comparison; taps_formula and tables_formula restate how the library makes them, for the tests of the design itself.

Also a float64 model (exact e^{-j theta}, the same taps, direct convolution) for the accuracy bound."""
import numpy as np

CF32, CS8, CU8, CS16 = 0, 1, 2, 3
RAW_DTYPE = {CF32: np.float32, CS8: np.int8, CU8: np.uint8, CS16: np.int16}
MAX_TAPS, MAX_DECIMATION = 511, 512
f32 = np.float32


def nco_increment(hz, fs):
    """round(frac(hz / fs) * 2^32) mod 2^32 (design.cpp nco_increment)."""
    turns = float(hz) / float(fs)
    frac = turns - np.floor(turns)
    return int(np.floor(frac * 4294967296.0 + 0.5)) & 0xFFFFFFFF


def taps_formula(fs, cutoff_hz, T):
    """The stated design in double; the caller rounds to float."""
    k = np.arange(T, dtype=np.float64)
    c = k - (T - 1) // 2
    f = float(cutoff_hz) / float(fs)
    with np.errstate(invalid="ignore", divide="ignore"):
        ideal = np.where(c == 0, 2.0 * f, np.sin(2.0 * np.pi * f * c) / (np.pi * c))
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * (k + 1) / (T + 1))
    v = ideal * w
    return v / v.sum()


def tables_formula():
    """hi[a] = e^{-j 2 pi a / 2^10}, lo[b] = e^{-j 2 pi b / 2^20} in double: [2][1024][2]."""
    a = np.arange(1024, dtype=np.float64)
    tab = np.empty((2, 1024, 2), np.float64)
    for i, div in enumerate((1024.0, 1048576.0)):
        t = 2.0 * np.pi * a / div
        tab[i, :, 0] = np.cos(t)
        tab[i, :, 1] = -np.sin(t)
    return tab


def valid_config(fs, offset_hz, cutoff_hz, D, T):
    return bool(np.isfinite(offset_hz) and 1 <= D <= MAX_DECIMATION and 1 <= T <= MAX_TAPS and T % 2 == 1 and
                0 < cutoff_hz <= fs / 2)


def unpack(fmt, raw):
    """raw [..., 2 N] of RAW_DTYPE[fmt] -> (xr, xi) float32 [..., N]: load_i1 / load_q1 of ssb_common.h."""
    raw = np.asarray(raw, RAW_DTYPE[fmt])
    v = raw.astype(np.float32)
    if fmt == CS8:
        v = v * f32(1.0 / 128.0)
    elif fmt == CU8:
        v = (v - f32(127.4)) * f32(1.0 / 128.0)
    elif fmt == CS16:
        v = v * f32(1.0 / 32768.0)
    return np.ascontiguousarray(v[..., 0::2]), np.ascontiguousarray(v[..., 1::2])


def mix(tab, inc, g0, xr, xi):
    """(xr + j xi) * hi[ph >> 22] * lo[(ph >> 12) & 1023], ph = (uint32)(inc * (g0 + t)): every product and sum rounded
    to float32 on its own, in nco_mix's order."""
    tab = np.asarray(tab, np.float32).reshape(2, 1024, 2)
    n = xr.shape[-1]
    g = (np.uint64(g0 & 0xFFFFFFFF) + np.arange(n, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)
    ph = (np.uint64(inc) * g) & np.uint64(0xFFFFFFFF)
    H = tab[0][(ph >> np.uint64(22)).astype(np.int64)]
    L = tab[1][((ph >> np.uint64(12)) & np.uint64(1023)).astype(np.int64)]
    wr = H[:, 0] * L[:, 0] - H[:, 1] * L[:, 1]
    wi = H[:, 0] * L[:, 1] + H[:, 1] * L[:, 0]
    vr = xr * wr - xi * wi
    vi = xr * wi + xi * wr
    assert vr.dtype == np.float32 and vi.dtype == np.float32
    return vr, vi


def n_out_for(g0, n, D):
    return -(-(g0 + n) // D) - (-(-g0 // D))


class Ddc:
    """One engine's DDC state: g0 and, per stream, the last T - 1 mixed samples."""

    def __init__(self, B, taps, tab, inc, D):
        self.B, self.D, self.inc = B, int(D), int(inc)
        self.h = np.asarray(taps, np.float32).copy()
        self.T = self.h.size
        self.tab = np.asarray(tab, np.float32).copy()
        self.reset()

    def reset(self):
        self.g0 = 0
        self.hr = np.zeros((self.B, self.T - 1), np.float32)
        self.hi = np.zeros((self.B, self.T - 1), np.float32)

    def call(self, fmt, raw):
        """raw [B][2 N] -> (out complex64 [B][cap], zeros from n_out on; n_out)."""
        B, D, T, H = self.B, self.D, self.T, self.T - 1
        xr, xi = unpack(fmt, np.asarray(raw).reshape(B, -1))
        n = xr.shape[1]
        vr, vi = mix(self.tab, self.inc, self.g0, xr, xi)
        er = np.concatenate([self.hr, vr], axis=1)  # er[:, H + t] = v at local index t
        ei = np.concatenate([self.hi, vi], axis=1)
        cap = -(-n // D)
        n_out = n_out_for(self.g0, n, D)
        first = (-self.g0) % D
        out = np.zeros((B, cap, 2), np.float32)
        if n_out > 0:
            at = H + first + D * np.arange(n_out)
            ar = np.zeros((B, n_out), np.float32)
            ai = np.zeros((B, n_out), np.float32)
            for k in range(T):
                ar = ar + self.h[k] * er[:, at - k]
                ai = ai + self.h[k] * ei[:, at - k]
            assert ar.dtype == np.float32
            out[:, :n_out, 0] = ar
            out[:, :n_out, 1] = ai
        if H:
            self.hr, self.hi = er[:, -H:].copy(), ei[:, -H:].copy()
        self.g0 += n
        return out.view(np.complex64)[..., 0], n_out


def model_f64(fmt, raw, taps, inc, D):
    """The whole stream at once in float64: exact unpack, exact e^{-j 2 pi inc g / 2^32}, the same taps, direct
    convolution.  raw [B][2 N] -> complex128 [B][ceil(N / D)]."""
    raw = np.asarray(raw, RAW_DTYPE[fmt]).astype(np.float64)
    if fmt == CS8:
        raw = raw / 128.0
    elif fmt == CU8:
        raw = (raw - np.float64(f32(127.4))) / 128.0
    elif fmt == CS16:
        raw = raw / 32768.0
    x = raw[:, 0::2] + 1j * raw[:, 1::2]
    n = x.shape[1]
    ph = (int(inc) * np.arange(n, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)  # inc * g < 2^64 for g < 2^32
    v = x * np.exp(-2j * np.pi * ph.astype(np.float64) / 4294967296.0)
    h = np.asarray(taps, np.float64)
    T = h.size
    e = np.concatenate([np.zeros((x.shape[0], T - 1), np.complex128), v], axis=1)
    at = T - 1 + D * np.arange(-(-n // D))
    y = np.zeros((x.shape[0], at.size), np.complex128)
    for k in range(T):
        y += h[k] * e[:, at - k]
    return y


def error_bound(T, max_abs_x, taps):
    """|err| per component <= (1.3e-5 + (T + 3) 2^-24) max|x| sum|h|: the phasor's 1.2e-5 plus the mix's
    roundings, and one rounding per product and per sum of the FIR."""
    return (1.3e-5 + (T + 3) * 2.0 ** -24) * float(max_abs_x) * float(np.abs(np.asarray(taps, np.float64)).sum())


def response(taps, f_rel):
    """H(f) of the taps at f_rel cycles per input sample, in double."""
    h = np.asarray(taps, np.float64)
    return np.sum(h * np.exp(-2j * np.pi * f_rel * np.arange(h.size)))


def noise(fmt, B, n, seed, amp=0.9):
    """Dense raw input [B][2 n] of the format: every value class appears (full range integers, floats in (-amp, amp))."""
    rng = np.random.default_rng(seed)
    if fmt == CF32:
        return ((rng.random((B, 2 * n)) * 2 - 1) * amp).astype(np.float32)
    info = np.iinfo(RAW_DTYPE[fmt])
    return rng.integers(info.min, info.max + 1, (B, 2 * n)).astype(RAW_DTYPE[fmt])


def tone(fmt, B, n, f_rel, amp=0.5, phase=0.0):
    """A complex tone at f_rel cycles per sample, quantised to the format: [B][2 n] (the same on every stream)."""
    t = np.arange(n, dtype=np.float64)
    z = amp * np.exp(2j * np.pi * f_rel * t + 1j * phase)
    iq = np.empty(2 * n, np.float64)
    iq[0::2], iq[1::2] = z.real, z.imag
    if fmt == CF32:
        raw = iq.astype(np.float32)
    elif fmt == CS8:
        raw = np.round(iq * 128.0).clip(-128, 127).astype(np.int8)
    elif fmt == CU8:
        raw = np.round(iq * 128.0 + 127.4).clip(0, 255).astype(np.uint8)
    else:
        raw = np.round(iq * 32768.0).clip(-32768, 32767).astype(np.int16)
    return np.ascontiguousarray(np.broadcast_to(raw, (B, 2 * n)))
