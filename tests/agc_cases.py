"""NumPy restatement of the AGC stage (include/sdrg.h, csrc/agc.hip): the block statistic (the squelch's adjacent-pair
tree times 1 / S, or the peak power), the attack / hang / decay law, the two-block ramp and the records, over a stream of
concatenated calls, operation by operation in float32, so the GPU tests compare bytes.  The design values are arguments:
the tests pass the library's (sdrg.agc_design), so no libm difference enters a byte comparison; design_formula restates
how the library makes them.  The records' dB is glibc's log10f (stats_np.log10f, as display_cases.db).  model_f64 is the
same law in float64, and error_bound what separates a settled float32 output's block RMS from the target."""
import math

import numpy as np

import display_cases as dc
import squelch_cases as sq
import stats_np

f32 = np.float32
MIN_BLOCK, MAX_BLOCK, MAX_HANG, MAX_IN = 16, 1024, 65535, 1 << 20
MEAN, PEAK = 0, 1
RECORD = np.dtype([("gain", "<f4"), ("gain_db", "<f4"), ("level_db", "<f4"), ("attacks", "<i4")])
DESIGN = ("max_gain", "init_gain", "floor_thr", "alpha_a", "alpha_d")


def design_formula(max_gain_db, initial_gain_db, floor_db, attack_blocks, decay_blocks):
    """(max_gain, init_gain, floor_thr, alpha_a, alpha_d) in double; the caller rounds to float.  An alpha is exactly 1
    at 0 blocks, floor_thr exactly 0 at -inf dB."""
    alpha = lambda x: 1.0 - math.exp(-1.0 / x) if x > 0 else 1.0  # noqa: E731
    floor = 0.0 if floor_db == -math.inf else 10.0 ** (floor_db / 10.0)
    return 10.0 ** (max_gain_db / 20.0), 10.0 ** (initial_gain_db / 20.0), floor, alpha(attack_blocks), alpha(decay_blocks)


def valid_config(c):
    """The rules of set_agc on a dict of sdrg_agc_config's fields."""
    fin = np.isfinite
    with np.errstate(over="ignore", under="ignore"):
        t = f32(c["target"]) if fin(c["target"]) else f32(np.nan)
        ok = bool(fin(t) and t > 0) and fin(c["max_gain_db"]) and fin(c["initial_gain_db"]) and \
            (fin(c["floor_db"]) or c["floor_db"] == -math.inf) and fin(c["attack_blocks"]) and c["attack_blocks"] >= 0 and \
            fin(c["decay_blocks"]) and c["decay_blocks"] >= 0 and c["detector"] in (MEAN, PEAK) and \
            MIN_BLOCK <= c["block"] <= MAX_BLOCK and c["block"] & (c["block"] - 1) == 0 and \
            0 <= c["hang_blocks"] <= MAX_HANG and 1 <= c["max_in"] <= MAX_IN
        if ok:
            big = lambda db, per: f32(10.0 ** (db / per)) if db < 3000 else f32(np.inf)  # noqa: E731
            mx, init, floor = big(c["max_gain_db"], 20.0), big(c["initial_gain_db"], 20.0), big(c["floor_db"], 10.0)
            ok = bool(fin(mx) and mx > 0 and fin(init) and init > 0 and init <= mx and fin(floor))
    return bool(ok)


def peak(q):
    return np.asarray(q, f32).max(axis=-1)


class Agc:
    """One engine's AGC state: g and, per stream, the powers of the block in progress, G = gain[last], G_prev, the hang
    counter and P_last."""

    def __init__(self, B, target, design, S, H, detector=MEAN):
        self.B, self.S, self.H, self.detector = B, int(S), int(H), detector
        self.target = f32(target)
        self.max_gain, self.init_gain, self.floor_thr, self.alpha_a, self.alpha_d = (f32(design[k]) for k in DESIGN)
        self.r = f32(1.0) / f32(self.S)
        self.reset()

    def reset(self):
        B = self.B
        self.g = 0
        self.pw = np.zeros((B, self.S), np.float32)
        self.G = np.full(B, self.init_gain, np.float32)
        self.Gp = self.G.copy()
        self.hang = np.zeros(B, np.int32)
        self.Pl = np.zeros(B, np.float32)
        self.gains = []  # gain[k] of every block completed since the reset, for the tests that look at the law

    def statistic(self):
        return sq.tree_sum(self.pw) * self.r if self.detector == MEAN else peak(self.pw)

    def step(self, P):
        """One completed block of statistics P [B]; returns which streams took the attack branch."""
        G, hang = self.G, self.hang
        with np.errstate(all="ignore"):
            a = np.sqrt(P)
            want = np.minimum(self.target / a, self.max_gain)
            d = want - G
            up = want if self.alpha_a == 1 else G + self.alpha_a * d
            down = want if self.alpha_d == 1 else G + self.alpha_d * d
        assert a.dtype == want.dtype == d.dtype == up.dtype == down.dtype == np.float32
        live = ~(P < self.floor_thr)
        attack = live & (want < G)
        count = live & ~attack & (hang > 0)
        decay = live & ~attack & (hang == 0)
        self.Gp = G
        self.G = np.where(attack, up, np.where(decay, down, G)).astype(np.float32)
        self.hang = np.where(attack, self.H, np.where(count, hang - 1, hang)).astype(np.int32)
        self.Pl = P.astype(np.float32)
        self.gains.append(self.G.copy())
        return attack

    def weights(self, first, m):
        """w [B][m] of the in-block indices first .. first + m - 1 under the ramp from G_prev to G."""
        t = ((first + np.arange(m) + 1).astype(np.float32) * self.r).astype(np.float32)
        with np.errstate(all="ignore"):
            d = self.G - self.Gp
            w = self.Gp[:, None] + d[:, None] * t[None, :]
        assert w.dtype == np.float32
        return w

    def apply(self, z, first):
        w = self.weights(first, z.shape[1])
        zr, zi = np.ascontiguousarray(z.real), np.ascontiguousarray(z.imag)
        with np.errstate(all="ignore"):
            out = np.stack([zr * w, zi * w], axis=-1)
        assert out.dtype == np.float32
        return np.ascontiguousarray(out).view(np.complex64)[..., 0]

    def call(self, chan, in_stride=None):
        """chan complex64 [B][n] -> (out complex64 [B][in_stride], zeros from n on; records [B]; n_blocks)."""
        B, S = self.B, self.S
        z = np.asarray(chan, np.complex64).reshape(B, -1)
        n = z.shape[1]
        out = np.zeros((B, n if in_stride is None else in_stride), np.complex64)
        attacks = np.zeros(B, np.int32)
        n_blocks, i = 0, 0
        while i < n:
            fill = (self.g + i) % S
            m = min(S - fill, n - i)
            seg = z[:, i:i + m]
            self.pw[:, fill:fill + m] = sq.powers(seg)
            out[:, i:i + m] = self.apply(seg, fill)
            i += m
            if fill + m == S:
                attacks += self.step(self.statistic())
                n_blocks += 1
        self.g += n
        rec = np.zeros(B, RECORD)
        with np.errstate(all="ignore"):
            rec["gain"], rec["gain_db"] = self.G, (f32(20.0) * stats_np.log10f(self.G)).astype(np.float32)
        rec["level_db"], rec["attacks"] = dc.db(self.Pl), attacks
        return out, rec, n_blocks


def one_call(chan, target, design, S, H, detector=MEAN):
    z = np.asarray(chan, np.complex64)
    z = z.reshape(1, -1) if z.ndim == 1 else z
    return Agc(z.shape[0], target, design, S, H, detector).call(z)


def in_calls(chan, cuts, target, design, S, H, detector=MEAN):
    """The stream chan [B][n] cut at the indices `cuts`: (the outs concatenated, the last records, the blocks in all,
    the attacks in all)."""
    z = np.asarray(chan, np.complex64)
    agc = Agc(z.shape[0], target, design, S, H, detector)
    edges = [0] + list(cuts) + [z.shape[1]]
    outs, blocks, rec, attacks = [], 0, None, np.zeros(z.shape[0], np.int64)
    for a, b in zip(edges[:-1], edges[1:]):
        o, rec, nb = agc.call(z[:, a:b])
        outs.append(o)
        blocks += nb
        attacks += rec["attacks"]
    return np.concatenate(outs, axis=1), rec, blocks, attacks


def model_f64(chan, target, design, S, H, detector=MEAN):
    """The same law in float64 on whole blocks (chan [B][K S]): (out complex128 [B][K S], gain [K][B])."""
    z = np.asarray(chan, np.complex128)
    B, n = z.shape
    assert n % S == 0
    mx, init, floor, aa, ad = (float(design[k]) for k in DESIGN)
    G, Gp, hang = np.full(B, init), np.full(B, init), np.zeros(B, np.int64)
    t = (np.arange(S) + 1.0) / S
    out, gains = np.empty_like(z), []
    for k in range(n // S):
        blk = z[:, k * S:(k + 1) * S]
        out[:, k * S:(k + 1) * S] = blk * (Gp[:, None] + (G - Gp)[:, None] * t[None, :])
        p = blk.real ** 2 + blk.imag ** 2
        P = p.mean(axis=1) if detector == MEAN else p.max(axis=1)
        with np.errstate(all="ignore"):
            want = np.minimum(float(target) / np.sqrt(P), mx)
        live = ~(P < floor)
        attack = live & (want < G)
        count, decay = live & ~attack & (hang > 0), live & ~attack & (hang == 0)
        Gp, G = G, np.where(attack, G + aa * (want - G), np.where(decay, G + ad * (want - G), G))
        hang = np.where(attack, H, np.where(count, hang - 1, hang))
        gains.append(G.copy())
    return out, np.array(gains)


def block_rms(out, S):
    o = np.asarray(out, np.complex128)
    p = (o.real ** 2 + o.imag ** 2).reshape(o.shape[0], -1, S)
    return np.sqrt(p.mean(axis=2))


def settling_blocks(design, want, tol):
    """The first global block whose output is settled for a stream of constant block statistic, whose wanted gain is
    `want` (below max_gain): every step moves G towards `want` by at least alpha = min(alpha_a, alpha_d) of the distance,
    whichever branch it takes (hang_blocks = 0), so |gain[k] - want| <= (1 - alpha)^(k + 1) |init_gain - want|, which is
    tol * want from k = K on; block b is multiplied by gain[b - 2] .. gain[b - 1], hence K + 2."""
    alpha = min(float(design["alpha_a"]), float(design["alpha_d"]))
    dist = abs(float(design["init_gain"]) - want)
    if dist <= tol * want:
        return 2
    if alpha >= 1.0:
        return 3
    K = math.ceil(math.log(dist / (tol * want)) / -math.log1p(-alpha)) - 1
    return max(K, 0) + 2


def error_bound(target, S, design, tol):
    """How far a settled output block's RMS may be from the target, for a stream whose blocks all have the same mean
    power in exact arithmetic (a carrier whose modulation has a whole number of periods per block), detector MEAN,
    hang_blocks = 0; u = 2^-24, alpha = min(alpha_a, alpha_d), relative to the target:
      law       the float64 model of the same law is within tol of its fixed point after settling_blocks: tol.
      input     the samples are rounded to CF32, u each, 2 u on a power; a power is two rounded products and a rounded
                sum, 2 u; the tree adds log2 S roundings and the product with 1 / S two more (1 / S is exact, the product
                is not below the normal range): P is within e_P = (log2 S + 6) u of the exact mean power.
      want      sqrtf halves e_P and rounds, the quotient rounds: e_w = e_P / 2 + 2 u.  `want` moves by that much from
                block to block, and so, at either side of it, does the branch.
      gain      d, the product and the sum round, 3 u |G| at most per step, and the fixed point moves by e_w; the
                recurrence forgets at the rate alpha: e_G = (e_w + 3 u) / alpha.
      ramp      g1 - g0, the product with t and the sum: 3 u on w, on top of e_G for g0 and g1 each; the products with zr
                and zi round, u; the RMS of the block then has the relative error of w: e_G + 4 u."""
    u = 2.0 ** -24
    alpha = min(float(design["alpha_a"]), float(design["alpha_d"]))
    e_p = (math.log2(S) + 6) * u
    e_w = e_p / 2 + 2 * u
    e_g = (e_w + 3 * u) / alpha
    return float(target) * (tol + e_g + 4 * u)


def am_carriers(B, n, S, amps, depth=0.5, periods=4, f_rel=0.013):
    """B AM channels, complex64 [B][n]: stream b has the carrier amplitude amps[b], a modulation of `depth` with
    `periods` whole periods in every block of S (so every block has the mean power amps[b]^2 (1 + depth^2 / 2) exactly,
    before the rounding to float) and a carrier offset of f_rel (b + 1) cycles per sample."""
    i = np.arange(n, dtype=np.float64)
    z = np.empty((B, n), np.complex128)
    for b in range(B):
        env = 1.0 + depth * np.cos(2 * np.pi * periods * i / S + 0.3 * b)
        z[b] = amps[b] * env * np.exp(2j * np.pi * f_rel * (b + 1) * i)
    return z.astype(np.complex64)


def levels(B, n, seed, S, pattern, loud=1.0, quiet=0.01):
    """squelch_cases.keyed: noise whose rms changes block by block (each stream at its own blocks), so that the law
    attacks, hangs and decays in every stream."""
    return sq.keyed(B, n, seed, S, pattern, loud, quiet)


# the behavioural case: two AM channels 30 dB apart, 2 x 64 blocks of S = 64, settled to within tol of the law's fixed point
AM = dict(B=2, S=64, blocks=64, amps=(1.0, 10.0 ** -1.5), target=0.25, tol=1e-3,
          cfg=dict(target=0.25, max_gain_db=60.0, initial_gain_db=0.0, floor_db=-math.inf, attack_blocks=2.0,
                   decay_blocks=4.0, detector=MEAN, block=64, hang_blocks=0, max_in=64 * 64))


def am_case(S):
    """(z, design, the first settled block, the bound) of the behavioural case, which the CPU and the GPU test share; S is
    the sdrg module, whose design the restatement is fed."""
    d = S.agc_design(**AM["cfg"])
    z = am_carriers(AM["B"], AM["S"] * AM["blocks"], AM["S"], AM["amps"])
    wants = [AM["target"] / (a * math.sqrt(1 + 0.5 ** 2 / 2)) for a in AM["amps"]]
    first = max(settling_blocks(d, w, AM["tol"]) for w in wants)
    return z, d, first, error_bound(AM["target"], AM["S"], d, AM["tol"])
