"""NumPy restatement of the noise blanker stage (include/sdrg.h, csrc/blanker.hip): the samples' scaling and powers, the
block floor by the sub-blocks' adjacent-pair trees, the level step, the hits, the windowed and delayed output and the
records, over a stream of concatenated calls, operation by operation in float32, so the GPU tests compare bytes; one
function per paragraph of the header's semantics.  beta, ratio and floor_thr are arguments: the tests pass the library's
(sdrg.blanker_design), so no libm difference enters a byte comparison; design_formula restates how the library makes
them.  whole_stream is the same law written a second time, over the concatenated stream block by block and with one
cumsum over its hit flags, and pulsed() the test signal of the benefit case."""
import numpy as np

import display_cases as dc
import iqcorr_cases as iq
from iqcorr_cases import CF32, CS8, CS16, CU8, RAW_DTYPE, sample, to_raw, tree_sum  # noqa: F401  (the tests' names)

f32 = np.float32
MIN_BLOCK, MAX_BLOCK, MAX_IN, MAX_LEAD, MAX_TAIL, SUB = 64, 1024, 1 << 20, 16, 64, 16
RECORD = np.dtype([("level", "<f4"), ("level_db", "<f4"), ("hits", "<i4"), ("blanked", "<i4")])
QUIET = iq.QUIET


# ---- design

def design_formula(tau_blocks, threshold_db, floor_db):
    """(beta, ratio, floor_thr) in double; the caller rounds to float.  beta is exactly 1 at tau = 0."""
    beta = 1.0 - np.exp(-1.0 / tau_blocks) if tau_blocks > 0 else 1.0
    return beta, 10.0 ** (threshold_db / 10.0), 10.0 ** (floor_db / 10.0)


def valid_config(c):
    """The rules of set_blanker on a dict of sdrg_blanker_config's fields."""
    fin = np.isfinite
    ok = fin(c["tau_blocks"]) and c["tau_blocks"] >= 0 and fin(c["threshold_db"]) and fin(c["floor_db"]) and \
        MIN_BLOCK <= c["block"] <= MAX_BLOCK and c["block"] & (c["block"] - 1) == 0 and \
        0 <= c["lead"] <= MAX_LEAD and 0 <= c["tail"] <= MAX_TAIL and 1 <= c["max_in"] <= MAX_IN
    for k in ("threshold_db", "floor_db"):
        if ok:
            with np.errstate(over="ignore", under="ignore"):
                v = f32(10.0 ** (c[k] / 10.0)) if c[k] < 3000 else f32(np.inf)
            ok = bool(fin(v) and v > 0)
    return bool(ok)


# ---- sample

def power(zr, zi):
    """q = zr zr + zi zi: two products and one sum."""
    with np.errstate(**QUIET):
        a, b = zr * zr, zi * zi
        q = a + b
    assert q.dtype == np.float32
    return q


# ---- floor

def block_floor(q):
    """q float32 [..., S], whole blocks -> F float32 [...]: the least of the sub-blocks' pair trees, times 0.0625f."""
    S = q.shape[-1]
    with np.errstate(**QUIET):
        f = tree_sum(q.reshape(q.shape[:-1] + (S // SUB, SUB)))
        F = f.min(axis=-1) * f32(0.0625)
    assert F.dtype == np.float32
    return F


# ---- step

def step(L, seeded, F, beta, ratio, floor_thr):
    """One completed block's F [B] -> (L, seeded, thr after the block)."""
    with np.errstate(**QUIET):
        L = np.where(seeded != 0, L + beta * (F - L), F).astype(np.float32)
        thr = np.maximum(L, floor_thr) * ratio
    assert thr.dtype == np.float32
    return L, np.ones_like(seeded), thr


# ---- hit

def hits_of(q, thr_before):
    """q [B][n] against the thresholds after the block before each sample's own, [B][n]."""
    return q > thr_before


# ---- output

def output(z_ext, hit_ext, n, lead, tail, first_live):
    """z_ext complex64 [B][lead + n]: the inputs from `lead` before the call's first on; hit_ext bool [B][lead + tail +
    n]: the hit flags from lead + tail before it on.  Output j carries z_ext[j] unless a flag in hit_ext[j .. j + lead +
    tail] is set, or j < first_live (its input lies before the stream).  -> (out complex64 [B][n], blanked [B])."""
    W = lead + tail
    c = np.concatenate([np.zeros((hit_ext.shape[0], 1), np.int64), np.cumsum(hit_ext, axis=1)], axis=1)
    any_hit = (c[:, W + 1:W + 1 + n] - c[:, :n]) > 0
    live = np.arange(n)[None, :] >= first_live
    out = np.where(live & ~any_hit, z_ext[:, :n], np.complex64(0)).astype(np.complex64)
    return out, (live & any_hit).sum(axis=1).astype(np.int32)


# ---- record

def record(L, hits, blanked):
    rec = np.zeros(L.shape[0], RECORD)
    rec["level"] = L
    with np.errstate(**QUIET):
        rec["level_db"] = dc.db(L)
    rec["hits"], rec["blanked"] = hits, blanked
    return rec


class Blanker:
    """One engine's stage: g and, per stream, the powers of the block in progress, L, seeded, the threshold in force, the
    last lead + tail hit flags and the last lead scaled samples."""

    def __init__(self, B, beta, ratio, floor_thr, S, lead, tail):
        self.B, self.S, self.lead, self.tail = B, int(S), int(lead), int(tail)
        self.beta, self.ratio, self.floor_thr = f32(beta), f32(ratio), f32(floor_thr)
        self.reset()

    def reset(self):
        B = self.B
        self.g = 0
        self.pend = np.zeros((B, 0), np.float32)
        self.L = np.zeros(B, np.float32)
        self.seeded = np.zeros(B, np.int32)
        self.thr = np.full(B, np.inf, np.float32)
        self.flags = np.zeros((B, self.lead + self.tail), bool)
        self.last = np.zeros((B, self.lead), np.complex64)

    def call(self, raw, fmt=CF32, in_stride=None):
        """raw [B][2 n] in the type of fmt (complex [B][n] at CF32 too) -> (out complex64 [B][in_stride], zeros from n
        on; records [B]; n_blocks)."""
        B, S, lead, tail = self.B, self.S, self.lead, self.tail
        raw = np.asarray(raw)
        if fmt == CF32 and np.iscomplexobj(raw):
            raw = np.ascontiguousarray(raw, np.complex64).view(np.float32)
        zr, zi = sample(raw.reshape(B, raw.size // B), fmt)
        n = zr.shape[1]
        q = power(zr, zi)
        off = self.g % S
        assert off == self.pend.shape[1]
        allq = np.concatenate([self.pend, q], axis=1)
        nb = (off + n) // S
        thrs = [self.thr]  # in force for the call's blocks 0, 1, ...
        if nb:
            F = block_floor(allq[:, :nb * S].reshape(B, nb, S))
            for k in range(nb):
                self.L, self.seeded, thr = step(self.L, self.seeded, F[:, k], self.beta, self.ratio, self.floor_thr)
                thrs.append(thr)
        thrs = np.stack(thrs, axis=1)  # [B][nb + 1]
        k = (off + np.arange(n)) // S
        hit = hits_of(q, thrs[:, k]) if n else np.zeros((B, 0), bool)
        z = np.ascontiguousarray(np.stack([zr, zi], axis=-1)).view(np.complex64)[..., 0]
        z_ext, hit_ext = np.concatenate([self.last, z], axis=1), np.concatenate([self.flags, hit], axis=1)
        out = np.zeros((B, n if in_stride is None else in_stride), np.complex64)
        out[:, :n], blanked = output(z_ext, hit_ext, n, lead, tail, max(lead - self.g, 0))
        if n:
            self.pend, self.thr = allq[:, nb * S:].copy(), thrs[:, -1].copy()
            self.flags = hit_ext[:, hit_ext.shape[1] - (lead + tail):].copy()
            self.last = z_ext[:, z_ext.shape[1] - lead:].copy()
        self.g += n
        return out, record(self.L, hit.sum(axis=1), blanked), nb


def one_call(raw, fmt, beta, ratio, floor_thr, S, lead, tail):
    raw = np.asarray(raw)
    raw = raw.reshape(1, -1) if raw.ndim == 1 else raw
    return Blanker(raw.shape[0], beta, ratio, floor_thr, S, lead, tail).call(raw, fmt)


def in_calls(raw, fmt, cuts, beta, ratio, floor_thr, S, lead, tail):
    """The stream raw [B][2 n] cut at the sample indices `cuts`: (the outs concatenated, the last records, the blocks in
    all, the hits in all, the blanked outputs in all)."""
    raw = np.asarray(raw)
    if fmt == CF32 and np.iscomplexobj(raw):
        raw = np.ascontiguousarray(raw, np.complex64).view(np.float32)
    m = Blanker(raw.shape[0], beta, ratio, floor_thr, S, lead, tail)
    edges = [0] + list(cuts) + [raw.shape[1] // 2]
    outs, blocks, hits, blanked, rec = [], 0, 0, 0, None
    for a, b in zip(edges[:-1], edges[1:]):
        o, rec, nb = m.call(raw[:, 2 * a:2 * b], fmt)
        outs.append(o)
        blocks += nb
        hits, blanked = hits + rec["hits"], blanked + rec["blanked"]
    return np.concatenate(outs, axis=1), rec, blocks, hits, blanked


# ---- the same law a second time: one stream, block by block, one cumsum over the whole stream's hit flags

def whole_stream(z, beta, ratio, floor_thr, S, lead, tail):
    """z complex64 [n] (one stream, already scaled) -> (out complex64 [n], L, hits, blanked)."""
    z = np.asarray(z, np.complex64)
    n = len(z)
    beta, ratio, floor_thr = f32(beta), f32(ratio), f32(floor_thr)
    re, im = z.real.astype(np.float32), z.imag.astype(np.float32)
    hit = np.zeros(n, bool)
    L, thr, seeded = f32(0), f32(np.inf), False
    with np.errstate(**QUIET):
        for k in range((n + S - 1) // S):
            a, b = k * S, min((k + 1) * S, n)
            q = re[a:b] * re[a:b] + im[a:b] * im[a:b]
            hit[a:b] = q > thr
            if b - a < S:
                break
            f = []
            for j in range(S // 16):
                v = q[16 * j:16 * j + 16]
                v = v[0::2] + v[1::2]  # 8
                v = v[0::2] + v[1::2]  # 4
                v = v[0::2] + v[1::2]  # 2
                f.append(f32(v[0] + v[1]))
            F = f32(min(f) * f32(0.0625))
            L = f32(L + beta * f32(F - L)) if seeded else F
            seeded = True
            thr = f32(max(L, floor_thr) * ratio)
    c = np.concatenate([[0], np.cumsum(hit)])
    j = np.arange(n)
    lo, hi = np.maximum(j - lead - tail, 0), j + 1  # the window [max(i - tail, 0), i + lead] of i = j - lead
    gone = (c[hi] - c[lo]) > 0
    live = j >= lead
    out = np.zeros(n, np.complex64)
    keep = live & ~gone
    out[keep] = z[j[keep] - lead]
    return out, L, int(hit.sum()), int((live & gone).sum())


# ---- test signals

FS, N_BEN, TONE_HZ = 2_000_000, 1 << 18, 250_037.0
PULSE = (1.0, 0.5, 0.25, 0.12, 0.06)
BENEFIT = dict(tau_blocks=16.0, threshold_db=13.0, floor_db=-100.0, lead=2, tail=8)


def pulsed(seed=7, pulses=True, n=N_BEN):
    """The benefit case's input, complex128 [n]: noise of sigma 0.01 per component, a tone of 0.1 at +250 037 Hz and, with
    `pulses`, one pulse per 1000 samples at a jittered position with a random phase, amplitudes PULSE over five
    consecutive samples.  The noise and the tone are the same with and without the pulses."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / FS
    z = 0.1 * np.exp(2j * np.pi * TONE_HZ * t) + 0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    at = np.arange(0, n - 1000, 1000) + rng.integers(100, 900, len(range(0, n - 1000, 1000)))
    ph = np.exp(2j * np.pi * rng.random(len(at)))
    if pulses:
        for d, a in enumerate(PULSE):
            z[at + d] += a * ph
    return z


def spectrum_levels(y, last=65536):
    """(the median bin, the tone's peak) in dB over the last `last` samples under a Blackman window."""
    y = np.asarray(y, np.complex128)[-last:]
    sp = np.abs(np.fft.fft(y * np.blackman(last))) ** 2
    k = int(round(TONE_HZ * last / FS))
    return 10 * np.log10(np.median(sp)), 10 * np.log10(max(sp[(k + d) % last] for d in range(-3, 4)))


def gaussian(B, n, seed, sigma=1.0):
    """Complex Gaussian noise of mean power sigma^2, complex64 [B][n]."""
    return iq.noise(B, n, seed, sigma)
