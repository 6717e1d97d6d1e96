"""NumPy restatement of the tone detector stage (include/sdrg.h, csrc/tones.hip): the products against the design's
table, the adjacent-pair tree over each sub-block of 64, the block's accumulators, the powers, the candidate and the
latch, and the records, over a stream of concatenated calls, operation by operation in float32, so the GPU tests compare
bytes.  The design (table, wf and the five scalars) is an argument: the tests pass the library's (sdrg.tones_design), so
no libm difference enters a byte comparison; design_formula restates how the library makes it.  The records' dB is the
display stage's (display_cases.db)."""
import numpy as np

import display_cases as dc
from squelch_cases import running_sum, tree_sum  # noqa: F401  (the tests tell the tree from the running sum)

f32 = np.float32
SUB, MAX_TONES, MAX_SUB_BLOCKS, MAX_IN = 64, 64, 256, 65536
RECT, HANN = 0, 1
RECORD = np.dtype([("tone", "<i4"), ("candidate", "<i4"), ("power", "<f4"), ("power_db", "<f4"), ("share", "<f4"),
                   ("tone_blocks", "<i4"), ("changes", "<i4"), ("run", "<i4")])
SCALARS = ("pnorm", "enorm", "min_power", "dom", "share_thr")
# the 50 standard CTCSS tones, Hz
CTCSS = (67.0, 69.3, 71.9, 74.4, 77.0, 79.7, 82.5, 85.4, 88.5, 91.5, 94.8, 97.4, 100.0, 103.5, 107.2, 110.9, 114.8, 118.8,
         123.0, 127.3, 131.8, 136.5, 141.3, 146.2, 151.4, 156.7, 159.8, 162.2, 165.5, 167.9, 171.3, 173.8, 177.3, 179.9,
         183.5, 186.2, 189.9, 192.8, 196.6, 199.5, 203.5, 206.5, 210.7, 218.1, 225.7, 229.1, 233.6, 241.8, 250.3, 254.1)


def design_formula(rate_hz, freq_hz, sub_blocks, window, components, min_db, dominance_db, share):
    """The design in double; the caller rounds to float: (c [K][S], s [K][S], w [S], and the five scalars as a dict)."""
    S = SUB * sub_blocks
    i = np.arange(S, dtype=np.float64)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * (i + 1.0) / (S + 1.0)) if window == HANN else np.ones(S)
    t = np.asarray(freq_hz, np.float64)[:, None] * i[None, :] / float(rate_hz)
    theta = 2.0 * np.pi * (t - np.floor(t))
    W1, W2 = w.sum(), (w * w).sum()
    two = 2.0 if components == 1 else 1.0
    sc = dict(pnorm=two * two / (W1 * W1), enorm=two / W2, min_power=10.0 ** (min_db / 10.0),
              dom=10.0 ** (dominance_db / 10.0), share_thr=float(share))
    return w[None, :] * np.cos(theta), w[None, :] * np.sin(theta), w, sc


def formula_design(**cfg):
    """What sdrg.tones_design returns, from design_formula: for the tests that need no library."""
    c, s, w, sc = design_formula(cfg["rate_hz"], cfg["freq_hz"], cfg["sub_blocks"], cfg.get("window", RECT),
                                 cfg.get("components", 1), cfg.get("min_db", 0.0), cfg.get("dominance_db", 0.0),
                                 cfg.get("share", 0.0))
    d = {k: f32(v) for k, v in sc.items()}
    d["table"] = np.stack([c, s], axis=-1).astype(np.float32)
    d["wf"] = w.astype(np.float32)
    return d


def valid_config(c):
    """The rules of set_tones on a dict of sdrg_tones_config's fields (freq_hz: the first n_tones count)."""
    fin = np.isfinite
    fa, K = c["rate_hz"], c["n_tones"]
    ok = fin(fa) and fa > 0 and c["components"] in (1, 2) and 1 <= K <= MAX_TONES and \
        1 <= c["sub_blocks"] <= MAX_SUB_BLOCKS and c["window"] in (RECT, HANN) and fin(c["min_db"]) and \
        fin(c["dominance_db"]) and c["dominance_db"] >= 0 and 0 <= c["share"] <= 1 and \
        1 <= c["confirm_blocks"] <= 255 and 0 <= c["release_blocks"] <= 255 and 1 <= c["max_in"] <= MAX_IN
    if ok:
        for f in list(c["freq_hz"])[:K]:
            ok = ok and fin(f) and (0 < f < fa / 2 if c["components"] == 1 else abs(f) <= fa / 2)
        ok = ok and len(list(c["freq_hz"])) >= K
    return bool(ok)


def latch_step(state, cand, confirm, release):
    """The latch on plain ints: state = (tone, last, run, miss) and a block's candidate -> the state after it."""
    tone, last, run, miss = state
    if cand >= 0 and cand == last:
        run = min(run + 1, 65535)
    else:
        run = 1 if cand >= 0 else 0
    last = cand
    if cand >= 0 and run >= confirm:
        tone, miss = cand, 0
    elif tone >= 0:
        if cand == tone:
            miss = 0
        else:
            miss += 1
            if miss > release:
                tone, miss = -1, 0
    return tone, last, run, miss


class Tones:
    """One engine's tone detector state: g and, per stream, the values of the sub-block in progress, the 2 K + 1
    accumulators, the latch and what the record repeats.  d is the design (table, wf and the scalars)."""

    def __init__(self, B, d, components, sub_blocks, confirm, release, max_in):
        self.B, self.comp, self.Q = B, int(components), int(sub_blocks)
        self.S = SUB * self.Q
        self.c = np.ascontiguousarray(d["table"][:, :, 0], np.float32)
        self.s = np.ascontiguousarray(d["table"][:, :, 1], np.float32)
        self.wf = np.asarray(d["wf"], np.float32)
        self.K = self.c.shape[0]
        assert self.c.shape == (self.K, self.S) and self.wf.shape == (self.S,)
        for k in SCALARS:
            setattr(self, k, f32(d[k]))
        self.confirm, self.release = int(confirm), int(release)
        self.cap_blocks = (int(max_in) + self.S - 1) // self.S
        self.reset()

    def reset(self):
        B, K = self.B, self.K
        self.g = 0
        self.vals = np.zeros((B, SUB), np.float32 if self.comp == 1 else np.complex64)
        self.C, self.Sn, self.E = np.zeros((B, K), np.float32), np.zeros((B, K), np.float32), np.zeros(B, np.float32)
        self.tone, self.last = np.full(B, -1, np.int32), np.full(B, -1, np.int32)
        self.run, self.miss = np.zeros(B, np.int32), np.zeros(B, np.int32)
        self.power, self.share = np.zeros(B, np.float32), np.zeros(B, np.float32)

    def sub_sums(self, x, q):
        """The sums of sub-block q of a block over its 64 values x [B][64]: (C [B][K], S [B][K], E [B])."""
        at = slice(SUB * q, SUB * q + SUB)
        c, s, wf = self.c[None, :, at], self.s[None, :, at], self.wf[None, at]
        with np.errstate(all="ignore"):
            if self.comp == 1:
                xr = np.asarray(x, np.float32)
                Ci, Si = xr[:, None, :] * c, xr[:, None, :] * s
                a = xr * wf
                e = a * a
            else:
                xr, xi = np.ascontiguousarray(x.real)[:, None, :], np.ascontiguousarray(x.imag)[:, None, :]
                Ci = xr * c + xi * s
                Si = xi * c - xr * s
                a, b = xr[:, 0] * wf, xi[:, 0] * wf
                e = a * a + b * b
            assert Ci.dtype == Si.dtype == e.dtype == np.float32
            return tree_sum(Ci), tree_sum(Si), tree_sum(e)

    def block_end(self):
        """The powers P [B][K] of the block the accumulators hold, and the candidate and the latch from them."""
        B, K = self.B, self.K
        with np.errstate(all="ignore"):
            P = (self.C * self.C + self.Sn * self.Sn) * self.pnorm
            Et = self.E * self.enorm
            best = np.argmax(P, axis=1)  # the first of the largest
            rows = np.arange(B)
            Pb = P[rows, best]
            if K == 1:
                P2 = np.zeros(B, np.float32)
            else:
                rest = P.copy()
                rest[rows, best] = f32(-1)
                P2 = rest.max(axis=1)
            share = Pb / np.maximum(Et, f32(1e-30))
            ok = (Pb >= self.min_power) & (Pb >= self.share_thr * Et) & (Pb >= self.dom * P2)
        assert P.dtype == share.dtype == np.float32
        cand = np.where(ok, best, -1).astype(np.int32)
        for b in range(B):
            st = latch_step((int(self.tone[b]), int(self.last[b]), int(self.run[b]), int(self.miss[b])), int(cand[b]),
                            self.confirm, self.release)
            self.tone[b], self.last[b], self.run[b], self.miss[b] = st
        self.power, self.share = Pb.astype(np.float32), share
        self.C[:], self.Sn[:], self.E[:] = 0, 0, 0
        return P

    def call(self, x):
        """x [B][n] (float32, or complex64 at components 2) -> (powers float32 [B][cap_blocks][K], +0 from n_blocks on;
        records [B]; n_blocks)."""
        B, S = self.B, self.S
        x = np.asarray(x, self.vals.dtype).reshape(B, -1)
        n = x.shape[1]
        powers = np.zeros((B, self.cap_blocks, self.K), np.float32)
        tone_blocks, changes = np.zeros(B, np.int32), np.zeros(B, np.int32)
        n_blocks, i = 0, 0
        while i < n:
            fill = (self.g + i) % SUB
            m = min(SUB - fill, n - i)
            self.vals[:, fill:fill + m] = x[:, i:i + m]
            i += m
            if fill + m == SUB:
                q = ((self.g + i - SUB) % S) // SUB
                c, s, e = self.sub_sums(self.vals, q)
                with np.errstate(all="ignore"):
                    self.C, self.Sn, self.E = self.C + c, self.Sn + s, self.E + e
                if q == self.Q - 1:
                    before = self.tone.copy()
                    powers[:, n_blocks] = self.block_end()
                    tone_blocks += self.tone >= 0
                    changes += self.tone != before
                    n_blocks += 1
        self.g += n
        rec = np.zeros(B, RECORD)
        rec["tone"], rec["candidate"], rec["power"], rec["share"] = self.tone, self.last, self.power, self.share
        with np.errstate(all="ignore"):
            rec["power_db"] = dc.db(self.power)
        rec["tone_blocks"], rec["changes"], rec["run"] = tone_blocks, changes, self.run
        return powers, rec, n_blocks


def model(B, d, **cfg):
    """A Tones for a configuration's fields (as sdrg's set_tones takes them) and its design d."""
    return Tones(B, d, cfg.get("components", 1), cfg["sub_blocks"], cfg["confirm_blocks"], cfg.get("release_blocks", 0),
                 cfg["max_in"])


def in_calls(m, x, cuts):
    """The stream x [B][n] cut at the indices `cuts` through the model m: (the completed blocks' powers concatenated
    [B][blocks][K], the last records, every call's records)."""
    edges = [0] + list(cuts) + [x.shape[1]]
    rows, recs = [], []
    for a, b in zip(edges[:-1], edges[1:]):
        p, rec, nb = m.call(x[:, a:b])
        rows.append(p[:, :nb])
        recs.append(rec)
    return np.concatenate(rows, axis=1), recs[-1], recs


def tone(n, f, fa, amp=1.0, phase=0.0, complex_=False):
    t = np.arange(n, dtype=np.float64)
    z = amp * np.exp(1j * (2.0 * np.pi * f * t / fa + phase))
    return z.astype(np.complex64) if complex_ else z.real.astype(np.float32)


def uniform_noise(B, n, seed, sd):
    """Uniform noise of standard deviation sd: amplitude sd sqrt(3)."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1.0, 1.0, (B, n)) * sd * np.sqrt(3.0)).astype(np.float32)
