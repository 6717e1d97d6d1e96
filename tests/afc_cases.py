"""NumPy restatement of the AFC stage (include/sdrg.h, csrc/afc.hip): the lag-1 products, the block sums by the
adjacent-pair tree, the step (smoothed sums, coherence, lock, increment), the running phase, the NCO mix and the records,
over a stream of concatenated calls, operation by operation in float32, so the GPU tests compare bytes; one function per
paragraph of the header's semantics.  The design values and the NCO tables are arguments: the tests pass the library's
(sdrg.afc_design, sdrg.nco_tables), so no libm difference enters a byte comparison; design_formula restates how the
library makes the former.  model64 is the same law in float64 with an exact phasor, error_bound what separates the two,
and carrier() / fm() the test signals."""
import numpy as np

import display_cases as dc
from demod_cases import atan2f

f32 = np.float32
TRACK, MEASURE = 1, 2
LOCKED, SEEDED = 1, 2
MIN_BLOCK, MAX_BLOCK, MAX_IN = 16, 1024, 1 << 20
RECORD = np.dtype([("offset_hz", "<f4"), ("step", "<f4"), ("inc", "<i4"), ("coherence", "<f4"), ("level", "<f4"),
                   ("level_db", "<f4"), ("held_blocks", "<i4"), ("flags", "<i4")])
DESIGN = ("beta", "floor_thr", "lock_thr", "max_s", "K", "hz_per_inc", "rad_per_inc")
QUIET = dict(invalid="ignore", over="ignore", under="ignore", divide="ignore")
M32 = np.uint64(0xFFFFFFFF)


# ---- design

def design_formula(channel_rate, max_offset_hz, tau_blocks, floor_db, lock_threshold):
    """The seven values in double, in DESIGN's order; the caller rounds to float.  beta is exactly 1 at tau = 0."""
    beta = 1.0 - np.exp(-1.0 / tau_blocks) if tau_blocks > 0 else 1.0
    return (beta, 10.0 ** (floor_db / 10.0), lock_threshold, 2.0 ** 32 * max_offset_hz / channel_rate, 2.0 ** 31 / np.pi,
            channel_rate / 2.0 ** 32, np.pi / 2.0 ** 31)


def valid_config(c):
    """The rules of set_afc on a dict of sdrg_afc_config's fields."""
    fin = np.isfinite
    ok = fin(c["channel_rate"]) and c["channel_rate"] > 0 and 0 < c["max_offset_hz"] <= c["channel_rate"] / 4 and \
        fin(c["tau_blocks"]) and c["tau_blocks"] >= 0 and fin(c["floor_db"]) and 0 <= c["lock_threshold"] <= 1 and \
        c["mode"] in (TRACK, MEASURE) and MIN_BLOCK <= c["block"] <= MAX_BLOCK and c["block"] & (c["block"] - 1) == 0 and \
        1 <= c["max_in"] <= MAX_IN
    if ok:
        with np.errstate(over="ignore", under="ignore"):
            thr = f32(10.0 ** (c["floor_db"] / 10.0)) if c["floor_db"] < 3000 else f32(np.inf)
        ok = bool(fin(thr) and thr > 0)
    return bool(ok)


# ---- products

def products(zr, zi):
    """zr, zi float32 [..., S], whole blocks -> (pr, pi, q) float32 [..., S]: the sample times the conjugate of the one
    before it in its block (+0 at the block's first), and its power."""
    with np.errstate(**QUIET):
        pr, pi = np.zeros_like(zr), np.zeros_like(zr)
        pr[..., 1:] = zr[..., 1:] * zr[..., :-1] + zi[..., 1:] * zi[..., :-1]
        pi[..., 1:] = zi[..., 1:] * zr[..., :-1] - zr[..., 1:] * zi[..., :-1]
        q = zr * zr + zi * zi
    for v in (pr, pi, q):
        assert v.dtype == np.float32
    return pr, pi, q


# ---- block

def tree_sum(q):
    """The adjacent-pair tree over the last axis (a power of two long): q'[i] = q[2 i] + q[2 i + 1] until one is left."""
    q = np.asarray(q, f32)
    with np.errstate(**QUIET):
        while q.shape[-1] > 1:
            q = q[..., 0::2] + q[..., 1::2]
    assert q.dtype == np.float32
    return q[..., 0]


def block_sums(zr, zi):
    """zr, zi float32 [..., S] -> (Rr, Ri, W) float32 [...]."""
    r = f32(1.0) / f32(zr.shape[-1])
    with np.errstate(**QUIET):
        Rr, Ri, W = (tree_sum(v) * r for v in products(zr, zi))
    return Rr, Ri, W


# ---- step

class State:
    """A, B, P, coh, inc, Phi (of the first sample of the block in progress) and the flags of B streams: all zero after a
    restart."""

    def __init__(self, B):
        z = lambda: np.zeros(B, np.float32)  # noqa: E731
        self.A, self.B, self.P, self.coh = z(), z(), z(), z()
        self.inc = np.zeros(B, np.int32)
        self.phi = np.zeros(B, np.uint32)
        self.flags = np.zeros(B, np.int32)


def step(st, d, Rr, Ri, W):
    """One completed block's sums [B] into st (d: the design, a dict of float32); returns which streams held it."""
    with np.errstate(**QUIET):
        low = W < d["floor_thr"]
        seed = ~low & ((st.flags & SEEDED) == 0)
        move = ~low & ((st.flags & SEEDED) != 0)
        beta = d["beta"]
        A = np.where(seed, Rr, np.where(move, st.A + beta * (Rr - st.A), st.A))
        Bm = np.where(seed, Ri, np.where(move, st.B + beta * (Ri - st.B), st.B))
        P = np.where(seed, W, np.where(move, st.P + beta * (W - st.P), st.P))
        st.A, st.B, st.P = A.astype(np.float32), Bm.astype(np.float32), P.astype(np.float32)
        coh = np.sqrt(st.A * st.A + st.B * st.B) / st.P
        st.coh = np.where(low, st.coh, coh).astype(np.float32)
        locked = ~low & (coh >= d["lock_thr"])
        s = atan2f(st.B, st.A) * d["K"]
        s = np.minimum(np.maximum(s, -d["max_s"]), d["max_s"])
        assert s.dtype == np.float32
        inc = np.rint(np.where(locked, s, f32(0))).astype(np.int32)  # ties to even
        st.inc = np.where(locked, inc, st.inc).astype(np.int32)
        st.flags = np.where(low, st.flags, SEEDED | np.where(locked, LOCKED, 0)).astype(np.int32)
    for v in (st.A, st.B, st.P, st.coh):
        assert v.dtype == np.float32
    return low.astype(np.int32)


# ---- phase

def next_phase(phi, inc, S):
    """Phi_(k+1) = (uint32)(Phi_k + (uint32) inc_(k-1) * S), [B]."""
    return ((phi.astype(np.uint64) + (inc.astype(np.int64) & 0xFFFFFFFF).astype(np.uint64) * np.uint64(S)) & M32).astype(np.uint32)


def sample_phase(phi, inc, i):
    """ph = (uint32)(Phi_k + (uint32) inc_(k-1) * i): phi, inc, i of one shape, or broadcast."""
    inc = (np.asarray(inc).astype(np.int64) & 0xFFFFFFFF).astype(np.uint64)
    return ((np.asarray(phi).astype(np.uint64) + inc * np.asarray(i).astype(np.uint64)) & M32).astype(np.uint32)


# ---- output

def output(tab, zr, zi, ph):
    """z * hi[ph >> 22] * lo[(ph >> 12) & 1023]: every product and sum rounded on its own, in the order of the DDC's
    mix (ddc_cases.mix) -> complex64."""
    tab = np.asarray(tab, np.float32).reshape(2, 1024, 2)
    H, L = tab[0][(ph >> 22).astype(np.int64)], tab[1][((ph >> 12) & 1023).astype(np.int64)]
    with np.errstate(**QUIET):
        wr = H[..., 0] * L[..., 0] - H[..., 1] * L[..., 1]
        wi = H[..., 0] * L[..., 1] + H[..., 1] * L[..., 0]
        yr = zr * wr - zi * wi
        yi = zr * wi + zi * wr
    assert yr.dtype == np.float32 and yi.dtype == np.float32
    return np.ascontiguousarray(np.stack([yr, yi], axis=-1)).view(np.complex64)[..., 0]


# ---- records

def record(st, d, held):
    rec = np.zeros(st.A.shape[0], RECORD)
    with np.errstate(**QUIET):
        rec["offset_hz"] = st.inc.astype(np.float32) * d["hz_per_inc"]
        rec["step"] = st.inc.astype(np.float32) * d["rad_per_inc"]
        rec["level_db"] = dc.db(st.P)
    rec["inc"], rec["coherence"], rec["level"], rec["held_blocks"], rec["flags"] = st.inc, st.coh, st.P, held, st.flags
    return rec


class Afc:
    """One engine's stage: g and, per stream, the samples of the block in progress and the State.  `trace` collects
    (inc, coh, flags, held) after every completed block, each [B]."""

    def __init__(self, B, design, S, tab, mode=TRACK):
        self.B, self.S, self.mode = B, int(S), int(mode)
        self.d = {k: f32(design[k]) for k in DESIGN}
        self.tab = np.asarray(tab, np.float32).reshape(2, 1024, 2)
        self.reset()

    def reset(self):
        self.g = 0
        self.pend_r = np.zeros((self.B, 0), np.float32)
        self.pend_i = np.zeros((self.B, 0), np.float32)
        self.st = State(self.B)
        self.trace = []

    def call(self, chan, in_stride=None):
        """chan complex64 [B][n] -> (out complex64 [B][in_stride], zeros from n on, or None when measuring; records [B];
        n_blocks)."""
        B, S, st = self.B, self.S, self.st
        chan = np.ascontiguousarray(chan, np.complex64).reshape(B, -1)
        zr, zi = np.ascontiguousarray(chan.real), np.ascontiguousarray(chan.imag)
        n = zr.shape[1]
        off = self.g % S
        assert off == self.pend_r.shape[1]
        ar, ai = np.concatenate([self.pend_r, zr], axis=1), np.concatenate([self.pend_i, zi], axis=1)
        nb = (off + n) // S
        phis, incs = [st.phi], [st.inc]  # of the call's blocks 0 .. nb: the last is the one left in progress
        held = np.zeros(B, np.int32)
        if nb:
            Rr, Ri, W = block_sums(ar[:, :nb * S].reshape(B, nb, S), ai[:, :nb * S].reshape(B, nb, S))
            for k in range(nb):
                st.phi = next_phase(st.phi, st.inc, S)  # the block was mixed by the increment before its own step
                h = step(st, self.d, Rr[:, k], Ri[:, k], W[:, k])
                held += h
                phis.append(st.phi)
                incs.append(st.inc)
                self.trace.append((st.inc.copy(), st.coh.copy(), st.flags.copy(), h))
        out = None
        if self.mode == TRACK:
            out = np.zeros((B, n if in_stride is None else in_stride), np.complex64)
            if n:
                u = off + np.arange(n)
                k = u // S
                phis, incs = np.stack(phis, axis=1), np.stack(incs, axis=1)  # [B][nb + 1]
                out[:, :n] = output(self.tab, zr, zi, sample_phase(phis[:, k], incs[:, k], (u % S)[None, :]))
        self.pend_r, self.pend_i = ar[:, nb * S:].copy(), ai[:, nb * S:].copy()
        self.g += n
        return out, record(st, self.d, held), nb

    def traced(self, name):
        """The trace's inc, coh, flags or held as [blocks][B]."""
        return np.stack([t[("inc", "coh", "flags", "held").index(name)] for t in self.trace])


def one_call(chan, design, S, tab, mode=TRACK):
    chan = np.asarray(chan)
    chan = chan.reshape(1, -1) if chan.ndim == 1 else chan
    q = Afc(chan.shape[0], design, S, tab, mode)
    return q.call(chan) + (q,)


def in_calls(chan, cuts, design, S, tab, mode=TRACK):
    """The stream chan [B][n] cut at the sample indices `cuts`: (the outs concatenated, the last records, the blocks in
    all, the held blocks in all)."""
    chan = np.asarray(chan)
    q = Afc(chan.shape[0], design, S, tab, mode)
    edges = [0] + list(cuts) + [chan.shape[1]]
    outs, blocks, held, rec = [], 0, 0, None
    for a, b in zip(edges[:-1], edges[1:]):
        o, rec, nb = q.call(chan[:, a:b])
        outs.append(o)
        blocks += nb
        held = held + rec["held_blocks"]
    return (np.concatenate(outs, axis=1) if mode == TRACK else None), rec, blocks, held


# ---- the same law in float64

def model64(z, design, S):
    """z complex [n] (one stream) -> (y complex128 [n], inc after every block as float64 [n // S], coh likewise): the
    law in float64, the angle by arctan2, the increment not rounded to an integer's float but to the integer, and the
    phasor e^{-j 2 pi ph / 2^32} exact."""
    z = np.asarray(z, np.complex128)
    d = {k: float(design[k]) for k in DESIGN}
    n, nb = len(z), len(z) // S
    A = Bm = P = 0.0
    seeded, inc, phi = False, 0, 0
    incs, cohs, phis = [0], [], [0]
    for k in range(nb):
        x = z[k * S:(k + 1) * S]
        R = np.sum(x[1:] * np.conj(x[:-1])) / S
        W = np.mean(np.abs(x) ** 2)
        phi = (phi + inc * S) % (1 << 32)
        coh = cohs[-1] if cohs else 0.0
        if W >= d["floor_thr"]:
            if not seeded:
                A, Bm, P, seeded = R.real, R.imag, W, True
            else:
                A, Bm, P = A + d["beta"] * (R.real - A), Bm + d["beta"] * (R.imag - Bm), P + d["beta"] * (W - P)
            coh = np.hypot(A, Bm) / P
            if coh >= d["lock_thr"]:
                inc = int(np.rint(min(max(np.arctan2(Bm, A) * 2.0 ** 31 / np.pi, -d["max_s"]), d["max_s"])))
        incs.append(inc)
        phis.append(phi)
        cohs.append(coh)
    u = np.arange(n)
    k = u // S
    ph = (np.array(phis, np.int64)[k] + np.array(incs, np.int64)[k] * (u % S)) % (1 << 32)
    return z * np.exp(-2j * np.pi * ph / 2.0 ** 32), np.array(incs[1:], np.float64), np.array(cohs)


def error_bound(S, beta, coh_min, max_abs_s, n, amp):
    """(the most |inc32 - inc64| of a block, the most |y32 - y64| over n samples of magnitude <= amp), for a stream whose
    decisions (floor, lock, clamp) fall the same way in both, u = 2^-24:
      sums      a product carries u, the tree log2 S levels of u each, the scale by 1 / S one more, all relative to the
                sum of magnitudes, which for pr and pi is at most the block's W (Cauchy-Schwarz): (log2 S + 3) u W.
      smoothing X + beta (Y - X) rounds three times, 3 u of the magnitude, and an error decays by (1 - beta) a block:
                3 u / beta in all.  Together e = (log2 S + 3 + 3 / beta) u, relative to P.
      angle     an error e P in (A, B) turns a vector of length coh P by at most e / coh; sdrg_atan2f is within 3.6e-7.
      inc       K times that, the product phi K rounded (|s| u), and the two roundings to an integer (1).
      phase     the increments' errors add up sample by sample: 2 pi d_inc n / 2^32 radians at the stream's end.
      output    the phasor's table keeps 20 bits of the phase (2 pi / 2^20), its entries and the four products and two
                sums of each complex product carry a few u: 8 u in all."""
    u = 2.0 ** -24
    e = (np.log2(S) + 3 + 3 / beta) * u
    d_inc = 2.0 ** 31 / np.pi * (e / coh_min + 3.6e-7) + max_abs_s * u + 1
    d_phase = 2 * np.pi * d_inc * n / 2.0 ** 32
    return d_inc, amp * (d_phase + 2 * np.pi / 2.0 ** 20 + 8 * u)


# ---- test signals

def white(rng, n, power):
    """Complex white noise of mean power `power`: the real parts drawn first, then the imaginary."""
    s = np.sqrt(power / 2.0)
    return s * rng.standard_normal(n) + 1j * s * rng.standard_normal(n)


def carrier(n, hz, rate, amp=0.5, snr_db=None, rng=None, phase=0.0):
    """A carrier of `amp` at hz in a channel of `rate`, with white noise snr_db under it: complex64 [n]."""
    z = amp * np.exp(1j * (2 * np.pi * hz * np.arange(n) / rate + phase))
    if snr_db is not None:
        z = z + white(rng, n, amp * amp / 10.0 ** (snr_db / 10.0))
    return z.astype(np.complex64)


def fm(n, carrier_hz, rate, tone_hz=1000.0, deviation_hz=3000.0, amp=0.5, snr_db=None, rng=None):
    """FM of a tone_hz tone with deviation_hz around carrier_hz, with white noise snr_db under it: complex64 [n]."""
    t = np.arange(n) / rate
    z = amp * np.exp(1j * (2 * np.pi * carrier_hz * t + deviation_hz / tone_hz * np.sin(2 * np.pi * tone_hz * t)))
    if snr_db is not None:
        z = z + white(rng, n, amp * amp / 10.0 ** (snr_db / 10.0))
    return z.astype(np.complex64)


def lag_offset_hz(y, rate):
    """The offset of y by the angle of its lag-1 product sum, in Hz."""
    y = np.asarray(y, np.complex128)
    return float(np.angle(np.sum(y[1:] * np.conj(y[:-1]))) * rate / (2 * np.pi))


def mean_step_hz(y, rate):
    """The mean phase step of y, sample to sample, in Hz."""
    y = np.asarray(y, np.complex128)
    return float(np.mean(np.angle(y[1:] * np.conj(y[:-1]))) * rate / (2 * np.pi))
