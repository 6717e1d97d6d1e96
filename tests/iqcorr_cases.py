"""NumPy restatement of the IQ correction stage (include/sdrg.h, csrc/iqcorr.hip): the samples' scaling, the block moments
by the adjacent-pair tree, the DC and balance step, the ramped output and the records, over a stream of concatenated
calls, operation by operation in float32, so the GPU tests compare bytes; one function per paragraph of the header's
semantics.  beta_dc, beta_bal and floor_thr are arguments: the tests pass the library's (sdrg.iqcorr_design), so no libm
difference enters a byte comparison; design_formula restates how the library makes them.  model64 is the same law in
float64, and receiver() the impaired test signal of the selectivity cases."""
import numpy as np

import display_cases as dc

f32 = np.float32
DC, BALANCE = 1, 2
MIN_BLOCK, MAX_BLOCK, MAX_IN = 64, 1024, 1 << 20
CF32, CS8, CU8, CS16 = 0, 1, 2, 3  # SDRG_IQ_*
RAW_DTYPE = {CS8: np.int8, CU8: np.uint8, CS16: np.int16, CF32: np.float32}
RECORD = np.dtype([("dc_re", "<f4"), ("dc_im", "<f4"), ("w_re", "<f4"), ("w_im", "<f4"), ("power", "<f4"),
                   ("image_db", "<f4"), ("held_blocks", "<i4"), ("seeded", "<i4")])
QUIET = dict(invalid="ignore", over="ignore", under="ignore", divide="ignore")


# ---- design

def design_formula(dc_tau_blocks, balance_tau_blocks, floor_db):
    """(beta_dc, beta_bal, floor_thr) in double; the caller rounds to float.  A beta is exactly 1 at tau = 0."""
    beta = lambda tau: 1.0 - np.exp(-1.0 / tau) if tau > 0 else 1.0  # noqa: E731
    return beta(dc_tau_blocks), beta(balance_tau_blocks), 10.0 ** (floor_db / 10.0)


def valid_config(c):
    """The rules of set_iqcorr on a dict of sdrg_iqcorr_config's fields."""
    fin = np.isfinite
    ok = fin(c["dc_tau_blocks"]) and c["dc_tau_blocks"] >= 0 and fin(c["balance_tau_blocks"]) and \
        c["balance_tau_blocks"] >= 0 and fin(c["floor_db"]) and c["mode"] in (DC, BALANCE, DC | BALANCE) and \
        MIN_BLOCK <= c["block"] <= MAX_BLOCK and c["block"] & (c["block"] - 1) == 0 and 1 <= c["max_in"] <= MAX_IN
    if ok:
        with np.errstate(over="ignore", under="ignore"):
            thr = f32(10.0 ** (c["floor_db"] / 10.0)) if c["floor_db"] < 3000 else f32(np.inf)
        ok = bool(fin(thr) and thr > 0)
    return bool(ok)


# ---- sample

def sample(raw, fmt):
    """raw [..., 2 n] in the type of fmt -> (zr, zi) float32 [..., n]: the format's scaled value, as the DDC reads it."""
    raw = np.asarray(raw, RAW_DTYPE[fmt])
    v = raw.astype(np.float32)
    if fmt == CS8:
        v = v * f32(1.0 / 128.0)
    elif fmt == CU8:
        v = (v - f32(127.4)) * f32(1.0 / 128.0)
    elif fmt == CS16:
        v = v * f32(1.0 / 32768.0)
    assert v.dtype == np.float32
    return np.ascontiguousarray(v[..., 0::2]), np.ascontiguousarray(v[..., 1::2])


# ---- block moments

def tree_sum(q):
    """The adjacent-pair tree over the last axis (a power of two long): q'[i] = q[2 i] + q[2 i + 1] until one is left."""
    q = np.asarray(q, f32)
    while q.shape[-1] > 1:
        q = q[..., 0::2] + q[..., 1::2]
    assert q.dtype == np.float32
    return q[..., 0]


def running_sum(q):
    """What the tree is not: the values added one after the other in float32."""
    acc = f32(0)
    for v in np.asarray(q, f32):
        acc = f32(acc + v)
    return acc


def block_moments(zr, zi):
    """zr, zi float32 [..., S], whole blocks -> (mr, mi, a, b, p) float32 [...]: the means and the centred moments."""
    S = zr.shape[-1]
    r = f32(1.0) / f32(S)
    with np.errstate(**QUIET):
        q1, q2 = zr * zr, zi * zi
        e, s, c = q1 - q2, q1 + q2, zr * zi
        mr, mi = tree_sum(zr) * r, tree_sum(zi) * r
        E, W, C = tree_sum(e) * r, tree_sum(s) * r, tree_sum(c) * r
        rr, ii = mr * mr, mi * mi
        a = E - (rr - ii)
        b = C - mr * mi
        p = W - (rr + ii)
    for v in (mr, mi, a, b, p):
        assert v.dtype == np.float32
    return mr, mi, a, b, p


# ---- step

class State:
    """dr, di, wr, wi, A, B, P, seeded of B streams, all zero after a restart, and theta after the block before."""

    def __init__(self, B):
        z = lambda: np.zeros(B, np.float32)  # noqa: E731
        self.dr, self.di, self.wr, self.wi, self.A, self.B, self.P = z(), z(), z(), z(), z(), z(), z()
        self.seeded = np.zeros(B, np.int32)
        self.prev = np.zeros((B, 4), np.float32)

    def theta(self):
        return np.stack([self.dr, self.di, self.wr, self.wi], axis=-1)


def step(st, mode, beta_dc, beta_bal, floor_thr, mr, mi, a, b, p):
    """One completed block's moments [B] into st; returns which streams held it (int32 [B])."""
    st.prev = st.theta()
    held = np.zeros(mr.shape, np.int32)
    with np.errstate(**QUIET):
        if mode & DC:
            if beta_dc == 1:
                st.dr, st.di = mr.copy(), mi.copy()
            else:
                st.dr = st.dr + beta_dc * (mr - st.dr)
                st.di = st.di + beta_dc * (mi - st.di)
        if mode & BALANCE:
            low = p < floor_thr
            seed = ~low & (st.seeded == 0)
            move = ~low & (st.seeded != 0)
            A = np.where(seed, a, np.where(move, st.A + beta_bal * (a - st.A), st.A))
            Bm = np.where(seed, b, np.where(move, st.B + beta_bal * (b - st.B), st.B))
            P = np.where(seed, p, np.where(move, st.P + beta_bal * (p - st.P), st.P))
            st.A, st.B, st.P = A.astype(np.float32), Bm.astype(np.float32), P.astype(np.float32)
            st.seeded = np.where(low, st.seeded, 1).astype(np.int32)
            cr, ci = st.A / st.P, (f32(2.0) * st.B) / st.P
            m = cr * cr + ci * ci
            fit = ~low & (m <= f32(0.25))
            d = f32(1.0) + np.sqrt(f32(1.0) - m)
            st.wr = np.where(fit, cr / d, st.wr).astype(np.float32)
            st.wi = np.where(fit, ci / d, st.wi).astype(np.float32)
            held = (~fit).astype(np.int32)
    for v in (st.dr, st.di, st.wr, st.wi, st.A, st.B, st.P):
        assert v.dtype == np.float32
    return held


# ---- output

def output(zr, zi, i, t0, t1, S):
    """The samples zr, zi [B][m] at the in-block indices i [m] under the ramp from t0 to t1 ([B][m][4] or [B][1][4]:
    theta after the blocks k - 2 and k - 1) -> complex64 [B][m]."""
    r = f32(1.0) / f32(S)
    t = ((np.asarray(i) + 1).astype(np.float32) * r).astype(np.float32)
    with np.errstate(**QUIET):
        par = t0 + (t1 - t0) * t[None, :, None]
        dr, di, wr, wi = par[..., 0], par[..., 1], par[..., 2], par[..., 3]
        ur, ui = zr - dr, zi - di
        yr = ur - (wr * ur + wi * ui)
        yi = ui - (wi * ur - wr * ui)
    assert yr.dtype == np.float32 and yi.dtype == np.float32
    return np.ascontiguousarray(np.stack([yr, yi], axis=-1)).view(np.complex64)[..., 0]


# ---- record

def record(st, held):
    rec = np.zeros(st.dr.shape[0], RECORD)
    rec["dc_re"], rec["dc_im"], rec["w_re"], rec["w_im"], rec["power"] = st.dr, st.di, st.wr, st.wi, st.P
    with np.errstate(**QUIET):
        rec["image_db"] = dc.db((st.wr * st.wr + st.wi * st.wi).astype(np.float32))
    rec["held_blocks"], rec["seeded"] = held, st.seeded
    return rec


class Iqcorr:
    """One engine's stage: g and, per stream, the scaled samples of the block in progress and the State."""

    def __init__(self, B, beta_dc, beta_bal, floor_thr, mode, S):
        self.B, self.S, self.mode = B, int(S), int(mode)
        self.beta_dc, self.beta_bal, self.floor_thr = f32(beta_dc), f32(beta_bal), f32(floor_thr)
        self.reset()

    def reset(self):
        self.g = 0
        self.pend_r = np.zeros((self.B, 0), np.float32)
        self.pend_i = np.zeros((self.B, 0), np.float32)
        self.st = State(self.B)

    def call(self, raw, fmt=CF32, in_stride=None):
        """raw [B][2 n] in the type of fmt (complex [B][n] at CF32 too) -> (out complex64 [B][in_stride], zeros from n
        on; records [B]; n_blocks)."""
        B, S = self.B, self.S
        raw = np.asarray(raw)
        if fmt == CF32 and np.iscomplexobj(raw):
            raw = np.ascontiguousarray(raw, np.complex64).view(np.float32)
        zr, zi = sample(raw.reshape(B, raw.size // B), fmt)
        n = zr.shape[1]
        off = self.g % S
        assert off == self.pend_r.shape[1]
        ar, ai = np.concatenate([self.pend_r, zr], axis=1), np.concatenate([self.pend_i, zi], axis=1)
        nb = (off + n) // S
        th = [self.st.prev, self.st.theta()]  # theta after the blocks -2 and -1, counted from the call's first
        held = np.zeros(B, np.int32)
        if nb:
            mom = block_moments(ar[:, :nb * S].reshape(B, nb, S), ai[:, :nb * S].reshape(B, nb, S))
            for k in range(nb):
                held += step(self.st, self.mode, self.beta_dc, self.beta_bal, self.floor_thr, *(m[:, k] for m in mom))
                th.append(self.st.theta())
        th = np.stack(th, axis=1)  # [B][nb + 2][4]
        out = np.zeros((B, n if in_stride is None else in_stride), np.complex64)
        if n:
            u = off + np.arange(n)
            k = u // S
            out[:, :n] = output(zr, zi, u % S, th[:, k], th[:, k + 1], S)
        self.pend_r, self.pend_i = ar[:, nb * S:].copy(), ai[:, nb * S:].copy()
        self.g += n
        return out, record(self.st, held), nb


def one_call(raw, fmt, beta_dc, beta_bal, floor_thr, mode, S):
    raw = np.asarray(raw)
    raw = raw.reshape(1, -1) if raw.ndim == 1 else raw
    return Iqcorr(raw.shape[0], beta_dc, beta_bal, floor_thr, mode, S).call(raw, fmt)


def in_calls(raw, fmt, cuts, beta_dc, beta_bal, floor_thr, mode, S):
    """The stream raw [B][2 n] cut at the sample indices `cuts`: (the outs concatenated, the last records, the blocks in
    all, the held blocks in all)."""
    raw = np.asarray(raw)
    if fmt == CF32 and np.iscomplexobj(raw):
        raw = np.ascontiguousarray(raw, np.complex64).view(np.float32)
    q = Iqcorr(raw.shape[0], beta_dc, beta_bal, floor_thr, mode, S)
    edges = [0] + list(cuts) + [raw.shape[1] // 2]
    outs, blocks, held, rec = [], 0, 0, None
    for a, b in zip(edges[:-1], edges[1:]):
        o, rec, nb = q.call(raw[:, 2 * a:2 * b], fmt)
        outs.append(o)
        blocks += nb
        held = held + rec["held_blocks"]
    return np.concatenate(outs, axis=1), rec, blocks, held


# ---- the same law in float64

def model64(z, beta_dc, beta_bal, floor_thr, mode, S):
    """z complex [n] (one stream, already scaled) -> (y complex128 [n], theta after the last block [4])."""
    z = np.asarray(z, np.complex128)
    n = len(z)
    nb = n // S
    dr = di = wr = wi = A = Bm = P = 0.0
    seeded = False
    th = [np.zeros(4), np.zeros(4)]
    for k in range(nb):
        x = z[k * S:(k + 1) * S]
        m = x.mean()
        a = np.mean(x.real ** 2 - x.imag ** 2) - (m.real ** 2 - m.imag ** 2)
        b = np.mean(x.real * x.imag) - m.real * m.imag
        p = np.mean(np.abs(x) ** 2) - abs(m) ** 2
        if mode & DC:
            dr, di = dr + beta_dc * (m.real - dr), di + beta_dc * (m.imag - di)
        if mode & BALANCE and p >= floor_thr:
            if not seeded:
                A, Bm, P, seeded = a, b, p, True
            else:
                A, Bm, P = A + beta_bal * (a - A), Bm + beta_bal * (b - Bm), P + beta_bal * (p - P)
            cr, ci = A / P, 2 * Bm / P
            mm = cr * cr + ci * ci
            if mm <= 0.25:
                d = 1 + np.sqrt(1 - mm)
                wr, wi = cr / d, ci / d
        th.append(np.array([dr, di, wr, wi]))
    th = np.stack(th)
    u = np.arange(n)
    k = u // S
    t = ((u % S) + 1) / S
    par = th[k] + (th[k + 1] - th[k]) * t[:, None]
    x = z - (par[:, 0] + 1j * par[:, 1])
    return x - (par[:, 2] + 1j * par[:, 3]) * np.conj(x), th[-1]


# ---- test signals

def noise(B, n, seed, amp=1.0):
    rng = np.random.default_rng(seed)
    return (amp * (rng.standard_normal((B, n)) + 1j * rng.standard_normal((B, n))) / np.sqrt(2.0)).astype(np.complex64)


def impaired(z, gain=1.05, phase_deg=3.0, dc=0j):
    """An ideal baseband through a mixer with a Q gain and phase error and an offset: Q' = gain (Q cos + I sin)."""
    ph = np.deg2rad(phase_deg)
    return z.real + 1j * gain * (z.imag * np.cos(ph) + z.real * np.sin(ph)) + dc


def to_raw(z, fmt, scale=None):
    """complex [B][n] -> raw [B][2 n] in the type of fmt; the integer formats round scale * z (CU8 around 127.4)."""
    z = np.asarray(z)
    v = np.stack([z.real, z.imag], axis=-1).reshape(z.shape[:-1] + (-1,))
    if fmt == CF32:
        return v.astype(np.float32)
    if fmt == CU8:
        return np.clip(np.rint(v * scale + 127.4), 0, 255).astype(np.uint8)
    lim = 127 if fmt == CS8 else 32767
    return np.clip(np.rint(v * scale), -lim - 1, lim).astype(RAW_DTYPE[fmt])


FS, N_SEL, TONE_HZ, WEAK_HZ = 2_000_000, 1 << 18, 250_037.0, -411_000.0
# format -> (the integer scale, the offset of I and of Q in the units the issue states them in)
SEL_FORMATS = {CU8: (100.0, (3.0, -2.0)), CS16: (20000.0, (300.0, -150.0)), CF32: (1.0, (0.02, -0.01))}


def receiver(fmt, seed=7):
    """The selectivity input: a tone of 0.5 at +250 037 Hz, one of 0.05 at -411 kHz, noise of sigma 0.01 per component,
    Q' = 1.05 (Q cos 3 + I sin 3), the format's offsets, quantised: raw [1][2 N_SEL]."""
    rng = np.random.default_rng(seed)
    t = np.arange(N_SEL) / FS
    z = 0.5 * np.exp(2j * np.pi * TONE_HZ * t) + 0.05 * np.exp(2j * np.pi * WEAK_HZ * t)
    z = z + 0.01 * (rng.standard_normal(N_SEL) + 1j * rng.standard_normal(N_SEL))
    scale, (oi, oq) = SEL_FORMATS[fmt]
    x = impaired(z, dc=(oi + 1j * oq) / scale)
    return to_raw(x[None, :], fmt, scale)


def levels_db(y, last=65536):
    """(image under tone, DC under tone) in dB on the last `last` samples under a Blackman window, the largest of +-3
    bins around each."""
    y = np.asarray(y, np.complex128)[-last:]
    sp = np.abs(np.fft.fft(y * np.blackman(last))) ** 2
    peak = lambda hz: max(sp[(int(round(hz * last / FS)) + d) % last] for d in range(-3, 4))  # noqa: E731
    tone = peak(TONE_HZ)
    return 10 * np.log10(tone / peak(-TONE_HZ)), 10 * np.log10(tone / peak(0.0))
