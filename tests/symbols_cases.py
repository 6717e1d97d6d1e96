"""NumPy restatement of the symbol stage (include/sdrg.h, csrc/symbols.hip): the clock, the products, the block sums by
the adjacent-pair tree, the step (smoothed sums, coherence, lock, tau, slips, levels), the symbol (interpolation and
decision) and the records, over a stream of concatenated calls, operation by operation in float32, so the GPU tests
compare bytes; one function per paragraph of the header's semantics.  The design values and the table are arguments: the
tests pass the library's (sdrg.symbols_design), so no libm difference enters a byte comparison; design_formula restates
how the library makes them.  model64 is the same law in float64, and signal() the behaviour tests' transmitter."""
import numpy as np

from afc_cases import tree_sum
from demod_cases import atan2f

f32 = np.float32
LEVEL_TRACK, LEVEL_FIXED = 1, 2
HARD, SOFT = 1, 2
LOCKED, SEEDED = 1, 2
UNLOCKED = 0x80
MIN_BLOCK, MAX_BLOCK, MAX_IN, HISTORY, TABLE = 64, 1024, 1 << 20, 66, 1024
RECORD = np.dtype([("tau_frac", "<f4"), ("tau", "<u4"), ("coherence", "<f4"), ("centre", "<f4"), ("threshold", "<f4"),
                   ("slips", "<i4"), ("held_blocks", "<i4"), ("flags", "<i4")])
DESIGN = ("trim", "inc", "rinc", "beta", "beta_level", "floor_thr", "lock_thr", "K", "rs", "scale", "centre", "threshold")
QUIET = dict(invalid="ignore", over="ignore", under="ignore", divide="ignore")
M32 = (1 << 32) - 1
BASE = dict(sample_rate=48000.0, symbol_rate=4800.0, tau_blocks=8.0, tau_level_blocks=8.0, floor_db=-60.0,
            lock_threshold=0.1, phase_trim=0.0, level_scale=1.0, fixed_centre=0.0, fixed_threshold=1.0, levels=2,
            block=1024, level_mode=LEVEL_TRACK, format=HARD, max_in=4096)


# ---- design

def design_formula(c):
    """The design of a configuration (a dict of sdrg_symbols_config's fields) in double and Python integers, each
    rounded once, and the table in double; the caller compares."""
    beta = lambda tau: 1.0 - np.exp(-1.0 / tau) if tau > 0 else 1.0  # noqa: E731
    inc = int(np.rint(2.0 ** 32 * c["symbol_rate"] / c["sample_rate"]))
    k = np.arange(TABLE)
    w = 2.0 * np.pi * (k + 0.5) / TABLE
    return dict(trim=int(np.rint(c["phase_trim"] * 2.0 ** 32)), inc=inc, rinc=f32(1.0 / inc), beta=f32(beta(c["tau_blocks"])),
                beta_level=f32(beta(c["tau_level_blocks"])), floor_thr=f32(10.0 ** (c["floor_db"] / 10.0)),
                lock_thr=f32(c["lock_threshold"]), K=f32(2.0 ** 31 / np.pi), rs=f32(1.0 / c["block"]),
                scale=f32(c["level_scale"]), centre=f32(c["fixed_centre"]), threshold=f32(c["fixed_threshold"]),
                table=np.stack([np.cos(w), np.sin(w)], axis=1))


def valid_config(c):
    """The rules of set_symbols on a dict of sdrg_symbols_config's fields."""
    fin = np.isfinite
    ok = fin(c["sample_rate"]) and c["sample_rate"] > 0 and fin(c["symbol_rate"]) and c["symbol_rate"] > 0
    ok = ok and 2 <= c["sample_rate"] / c["symbol_rate"] <= 64 and c["levels"] in (2, 4)
    ok = ok and MIN_BLOCK <= c["block"] <= MAX_BLOCK and c["block"] & (c["block"] - 1) == 0
    ok = ok and fin(c["tau_blocks"]) and c["tau_blocks"] >= 0 and fin(c["tau_level_blocks"]) and c["tau_level_blocks"] >= 0
    ok = ok and fin(c["floor_db"]) and 0 <= c["lock_threshold"] <= 1 and -0.5 <= c["phase_trim"] <= 0.5
    ok = ok and c["level_mode"] in (LEVEL_TRACK, LEVEL_FIXED) and fin(c["level_scale"]) and c["level_scale"] > 0
    ok = ok and fin(c["fixed_centre"]) and fin(c["fixed_threshold"]) and c["fixed_threshold"] > 0
    ok = ok and c["format"] in (HARD, SOFT) and 1 <= c["max_in"] <= MAX_IN
    if ok:
        ok = (1 << 26) <= int(np.rint(2.0 ** 32 * c["symbol_rate"] / c["sample_rate"])) <= (1 << 31)
    if ok:
        with np.errstate(over="ignore", under="ignore"):
            thr = f32(10.0 ** (c["floor_db"] / 10.0)) if c["floor_db"] < 3000 else f32(np.inf)
        ok = bool(fin(thr) and thr > 0)
    return bool(ok)


# ---- clock

def clock(inc, i):
    """c_i = (uint32)(inc i) for the global indices i (an array of Python-sized integers as uint64, or an int)."""
    i = np.asarray(i, np.uint64) & np.uint64(M32)  # inc (i mod 2^32) stays under 2^63
    return ((np.uint64(inc) * i) & np.uint64(M32)).astype(np.uint32)


def emits(inc, g, n):
    """Which of the call's values [g, g + n) emit: i >= 1 and c_i < inc; bool [n]."""
    i = np.arange(g, g + n, dtype=np.uint64)
    return (clock(inc, i) < np.uint32(inc)) & (i >= 1)


def count(inc, g):
    """K(g) = floor(inc (g - 1) / 2^32) for g >= 1, K(0) = 0, in Python integers."""
    return (inc * (g - 1)) >> 32 if g >= 1 else 0


def cap(inc, max_in):
    return ((inc * max_in) >> 32) + 1


# ---- products

def products(x, c, tab):
    """x float32 [..., S], whole blocks, c uint32 [..., S] their clock, tab float32 [TABLE][2] -> (a, b, u, q) float32
    [..., S]: the squared difference to the value before it in its block (+0 at the block's first), that against the
    clock's phasor, and the square."""
    with np.errstate(**QUIET):
        u = np.zeros_like(x)
        dx = x[..., 1:] - x[..., :-1]
        u[..., 1:] = dx * dx
        t = tab[(c >> np.uint32(22)).astype(np.int64)]
        a, b = u * t[..., 0], u * t[..., 1]
        a[..., 0], b[..., 0] = 0, 0
        q = x * x
    for v in (a, b, u, q):
        assert v.dtype == np.float32
    return a, b, u, q


# ---- block

def block_sums(x, c, tab, rs):
    """x float32 [..., S], c uint32 [..., S] or [S] -> (Ab, Bb, Ub, Mb, Qb) float32 [...]."""
    a, b, u, q = products(x, np.broadcast_to(c, x.shape), tab)
    with np.errstate(**QUIET):
        return tuple(tree_sum(v) * rs for v in (a, b, u, x, q))


# ---- step

def slipped(tau, nxt):
    """The slip rule on uint32 arrays: the sampling point went round the cell's edge."""
    tau, nxt = np.asarray(tau, np.uint32), np.asarray(nxt, np.uint32)
    d = (nxt - tau).astype(np.int32)
    return ((d >= 0) & (nxt < tau)) | ((d < 0) & (nxt > tau))


class State:
    """The step's words of B streams after a restart."""

    def __init__(self, B, d, track):
        z = lambda: np.zeros(B, np.float32)  # noqa: E731
        self.A, self.B, self.U, self.M, self.Q, self.coh = z(), z(), z(), z(), z(), z()
        self.tau = np.full(B, ((1 << 31) + d["trim"]) & M32, np.uint32)
        self.flags = np.zeros(B, np.int32)
        self.slips = np.zeros(B, np.int32)
        self.centre = np.full(B, 0.0 if track else d["centre"], np.float32)
        self.thr = np.full(B, 1.0 if track else d["threshold"], np.float32)


def step(st, d, track, Ab, Bb, Ub, Mb, Qb):
    """One completed block's sums [B] into st (d: the design); returns which streams held it."""
    with np.errstate(**QUIET):
        low = Qb < d["floor_thr"]
        seed = ~low & ((st.flags & SEEDED) == 0)
        move = ~low & ((st.flags & SEEDED) != 0)

        def smooth(X, Xb, beta):
            return np.where(seed, Xb, np.where(move, X + beta * (Xb - X), X)).astype(np.float32)

        st.A, st.B, st.U = smooth(st.A, Ab, d["beta"]), smooth(st.B, Bb, d["beta"]), smooth(st.U, Ub, d["beta"])
        st.M, st.Q = smooth(st.M, Mb, d["beta_level"]), smooth(st.Q, Qb, d["beta_level"])
        coh = np.where(st.U == 0, f32(0), np.sqrt(st.A * st.A + st.B * st.B) / st.U).astype(np.float32)
        st.coh = np.where(low, st.coh, coh).astype(np.float32)
        locked = ~low & (coh >= d["lock_thr"])
        s = np.rint(atan2f(st.B, st.A) * d["K"])
        assert s.dtype == np.float32
        ang = np.where(locked, s, f32(0)).astype(np.int64)
        nxt = ((ang - (d["inc"] >> 1) + (1 << 31) + d["trim"]) & M32).astype(np.uint32)
        st.slips = (st.slips + (locked & slipped(st.tau, nxt))).astype(np.int32)
        st.tau = np.where(locked, nxt, st.tau).astype(np.uint32)
        st.flags = np.where(low, st.flags, SEEDED | np.where(locked, LOCKED, 0)).astype(np.int32)
        if track:
            w = st.Q - st.M * st.M
            thr = d["scale"] * np.sqrt(np.maximum(w, f32(0)))
            st.centre = np.where(low, st.centre, st.M).astype(np.float32)
            st.thr = np.where(low, st.thr, thr).astype(np.float32)
    for v in (st.A, st.B, st.U, st.M, st.Q, st.coh, st.centre, st.thr):
        assert v.dtype == np.float32
    return low.astype(np.int32)


# ---- symbol

def sample(d, c, tau, x_at):
    """For emitting samples with the clock c (uint32) and their blocks' tau (uint32), of one shape: (qd, nu), then y from
    x_at(back), the values `back` samples before each: y = x0 - nu (x0 - x1)."""
    num = c.astype(np.uint64) + (np.uint64(1 << 32) - tau.astype(np.uint64))
    qd = num // np.uint64(d["inc"])
    r = (num - qd * np.uint64(d["inc"])).astype(np.uint32)
    assert qd.size == 0 or qd.max() <= HISTORY - 1
    with np.errstate(**QUIET):
        nu = r.astype(np.float32) * d["rinc"]
        x0, x1 = x_at(qd.astype(np.int64)), x_at(qd.astype(np.int64) + 1)
        y = x0 - nu * (x0 - x1)
    assert y.dtype == np.float32
    return y, qd, nu


def decide(v, thr, locked, levels):
    """SDRG_SYM_HARD: the byte of v under thr."""
    with np.errstate(**QUIET):
        if levels == 2:
            s = (v >= 0).astype(np.uint8)
        else:
            s = np.where(v < -thr, 0, np.where(v < 0, 1, np.where(v < thr, 2, 3))).astype(np.uint8)
    return s | np.where(locked, 0, UNLOCKED).astype(np.uint8)


def soft(v, thr):
    """SDRG_SYM_SOFT: thr > 0 ? v / thr : +0."""
    with np.errstate(**QUIET):
        out = np.where(thr > 0, v / thr, f32(0)).astype(np.float32)
    return out


# ---- records

def record(st, held):
    rec = np.zeros(st.A.shape[0], RECORD)
    rec["tau_frac"] = st.tau.astype(np.float32) * f32(2.0 ** -32)
    rec["tau"], rec["coherence"], rec["centre"], rec["threshold"] = st.tau, st.coh, st.centre, st.thr
    rec["slips"], rec["held_blocks"], rec["flags"] = st.slips, held, st.flags
    return rec


class Symbols:
    """One engine's stage: g and, per stream, the HISTORY values before the block in progress, that block's values and
    the State.  `trace` collects (tau, coh, flags, held) after every completed block, each [B]; `marks` the global index
    of every emitting sample and `points` [B][symbols] the sampling instants i - qd - nu, as float64."""

    def __init__(self, B, design, table, block, levels=2, level_mode=LEVEL_TRACK, format=HARD, max_in=MAX_IN):
        self.B, self.S, self.levels, self.track, self.fmt = B, int(block), int(levels), level_mode == LEVEL_TRACK, format
        self.d = {k: (int(design[k]) if k in ("trim", "inc") else f32(design[k])) for k in DESIGN}
        self.tab = np.asarray(table, np.float32).reshape(TABLE, 2)
        self.cap = cap(self.d["inc"], max_in)
        self.reset()

    def reset(self):
        self.g = 0
        self.hist = np.zeros((self.B, HISTORY), np.float32)
        self.pend = np.zeros((self.B, 0), np.float32)
        self.st = State(self.B, self.d, self.track)
        self.trace, self.marks, self.points = [], [], []

    def call(self, x):
        """x float32 [B][n] -> (symbols [B][cap] uint8 or float32, zeros from n_sym on; records [B]; n_sym)."""
        B, S, st, d = self.B, self.S, self.st, self.d
        x = np.ascontiguousarray(x, np.float32).reshape(B, -1)
        n = x.shape[1]
        off = self.g % S
        assert off == self.pend.shape[1]
        ar = np.concatenate([self.hist, self.pend, x], axis=1)  # position u at HISTORY + u
        nb = (off + n) // S
        per = [(st.tau, st.centre, st.thr, (st.flags & LOCKED) != 0)]  # of the call's blocks 0 .. nb
        held = np.zeros(B, np.int32)
        if nb:
            c = clock(d["inc"], np.arange(self.g - off, self.g - off + nb * S, dtype=np.uint64)).reshape(nb, S)
            sums = block_sums(ar[:, HISTORY:HISTORY + nb * S].reshape(B, nb, S), c[None], self.tab, d["rs"])
            for k in range(nb):
                h = step(st, d, self.track, *(v[:, k] for v in sums))
                held += h
                per.append((st.tau, st.centre, st.thr, (st.flags & LOCKED) != 0))
                self.trace.append((st.tau.copy(), st.coh.copy(), st.flags.copy(), h))
        t = np.flatnonzero(emits(d["inc"], self.g, n))
        n_sym = len(t)
        out = np.zeros((B, self.cap), np.float32 if self.fmt == SOFT else np.uint8)
        if n_sym:
            u = off + t
            k = u // S
            tau, centre, thr, locked = (np.stack(v, axis=1)[:, k] for v in zip(*per))  # [B][n_sym]
            c = np.broadcast_to(clock(d["inc"], self.g + t.astype(np.uint64)), tau.shape)
            x_at = lambda back: np.take_along_axis(ar, HISTORY + u[None, :] - back, axis=1)  # noqa: E731
            y, qd, nu = sample(d, c, tau, x_at)
            with np.errstate(**QUIET):
                v = y - centre
            out[:, :n_sym] = soft(v, thr) if self.fmt == SOFT else decide(v, thr, locked, self.levels)
            self.marks.append(self.g + t)
            self.points.append((self.g + t)[None, :] - qd.astype(np.float64) - nu.astype(np.float64))
        keep = HISTORY + nb * S
        self.hist, self.pend = ar[:, keep - HISTORY:keep].copy(), ar[:, keep:].copy()
        self.g += n
        return out, record(st, held), n_sym

    def traced(self, name):
        """The trace's tau, coh, flags or held as [blocks][B]."""
        return np.stack([t[("tau", "coh", "flags", "held").index(name)] for t in self.trace])


def make(B, design, cfg):
    """The restatement for a configuration (a dict with block, levels, level_mode, format, max_in) and its design."""
    return Symbols(B, design, design["table"], cfg["block"], cfg["levels"], cfg["level_mode"], cfg["format"], cfg["max_in"])


def in_calls(q, x, cuts):
    """The stream x [B][n] through q cut at the sample indices `cuts`: (the symbols of all calls concatenated, the last
    records, the held blocks in all)."""
    edges = [0] + list(cuts) + [x.shape[1]]
    outs, held, rec = [], 0, None
    for a, b in zip(edges[:-1], edges[1:]):
        o, rec, ns = q.call(x[:, a:b])
        assert not o[:, ns:].view(np.uint8).any()
        outs.append(o[:, :ns])
        held = held + rec["held_blocks"]
    return np.concatenate(outs, axis=1), rec, held


# ---- the same law in float64

def model64(x, design, S, levels=2):
    """x [n] (one stream) -> (symbols int [K], locked bool [K], sampling instants float64 [K], coh after every block):
    the law in float64, TRACK levels, the angle by arctan2 and the clock's phasor exact."""
    x = np.asarray(x, np.float64)
    d = {k: (int(design[k]) if k in ("trim", "inc") else float(design[k])) for k in DESIGN}
    inc, n, nb = d["inc"], len(x), len(x) // S
    i = np.arange(n)
    c = (inc * i) % (1 << 32)
    u = np.zeros(n)
    u[1:] = (x[1:] - x[:-1]) ** 2
    u[::S] = 0
    ph = np.exp(2j * np.pi * ((c >> 22) + 0.5) / TABLE)
    A = B = U = M = Q = 0.0
    seeded, locked, tau, centre, thr = False, False, ((1 << 31) + d["trim"]) % (1 << 32), 0.0, 1.0
    per, cohs, coh = [(tau, centre, thr, locked)], [], 0.0
    for k in range(nb):
        sl = slice(k * S, (k + 1) * S)
        R, Ub, Mb, Qb = np.sum(u[sl] * ph[sl]) / S, np.sum(u[sl]) / S, np.mean(x[sl]), np.mean(x[sl] ** 2)
        if Qb >= d["floor_thr"]:
            if not seeded:
                A, B, U, M, Q, seeded = R.real, R.imag, Ub, Mb, Qb, True
            else:
                A, B, U = A + d["beta"] * (R.real - A), B + d["beta"] * (R.imag - B), U + d["beta"] * (Ub - U)
                M, Q = M + d["beta_level"] * (Mb - M), Q + d["beta_level"] * (Qb - Q)
            coh = np.hypot(A, B) / U if U else 0.0
            locked = coh >= d["lock_thr"]
            if locked:
                tau = (int(np.rint(np.arctan2(B, A) * 2.0 ** 31 / np.pi)) - (inc >> 1) + (1 << 31) + d["trim"]) % (1 << 32)
            centre, thr = M, d["scale"] * np.sqrt(max(Q - M * M, 0.0))
        per.append((tau, centre, thr, locked))
        cohs.append(coh)
    t = np.flatnonzero((c < inc) & (i >= 1))
    syms, lock, inst = [], [], []
    xp = np.concatenate([np.zeros(HISTORY + 1), x])
    for e in t:
        tau, centre, thr, lk = per[e // S]
        num = int(c[e]) + (1 << 32) - tau
        qd, r = divmod(num, inc)
        nu = r / inc
        x0, x1 = xp[HISTORY + 1 + e - qd], xp[HISTORY + e - qd]
        v = x0 - nu * (x0 - x1) - centre
        syms.append(int(v >= 0) if levels == 2 else (0 if v < -thr else 1 if v < 0 else 2 if v < thr else 3))
        lock.append(lk)
        inst.append(e - qd - nu)
    return np.array(syms), np.array(lock, bool), np.array(inst), np.array(cohs)


# ---- the behaviour tests' transmitter

def signal(levels, T, snr_db, n_symbols=40000, seed=1, dc=0.7, start=0.37):
    """n_symbols random symbols of `levels` levels (+-1, or +-1 and +-3) as rectangular cells of T samples (T need not
    be an integer) from start T on, through a Hann window of round(0.6 T) points of unit sum, white noise snr_db under
    the signal's mean square, and a DC offset -> (x float32 [n], the symbols, the cells' first edge in samples)."""
    rng = np.random.default_rng(seed)
    sym = rng.integers(0, levels, n_symbols)
    lev = (2 * sym - (levels - 1)).astype(np.float64)
    n = int(np.floor((n_symbols + start) * T))
    cell = np.floor((np.arange(n) - start * T) / T).astype(np.int64)
    s = np.where(cell >= 0, lev[np.clip(cell, 0, n_symbols - 1)], 0.0)
    N = int(round(0.6 * T))
    w = np.hanning(N + 2)[1:-1]  # N points, none of them zero
    s = np.convolve(s, w / w.sum(), mode="same")  # out[i] = sum_j w[j] s[i + (N - 1) // 2 - j]
    if snr_db is not None:
        s = s + rng.standard_normal(n) * np.sqrt(np.mean(s * s) / 10.0 ** (snr_db / 10.0))
    # the cells' first edge as the filtered signal shows it: an even window delays by half a sample
    return (s + dc).astype(np.float32), sym, start * T + (N - 1) / 2 - (N - 1) // 2


def noise(n, seed, dc=0.7):
    return (np.random.default_rng(seed).standard_normal(n) + dc).astype(np.float32)


def score(q, out, sym, T, edge, first_block=24):
    """q has taken a whole signal() in as stream 0 and `out` [K] are the bytes it wrote: those from block first_block on
    that were sampled while locked, against the transmitter's cell that holds each sampling instant -> (errors, scored,
    the instants' fractions of their cells, the steps from cell to cell that are not 1: symbols doubled or missed)."""
    marks, points = np.concatenate(q.marks), np.concatenate(q.points, axis=1)[0]
    assert len(marks) == len(out)
    at = (points - edge) / T
    cell = np.floor(at).astype(np.int64)
    use = (marks // q.S >= first_block) & ((out & UNLOCKED) == 0) & (cell >= 0) & (cell < len(sym))
    errors = int(np.count_nonzero((out[use] & 3) != sym[cell[use]]))
    return errors, int(np.count_nonzero(use)), (at - cell)[use], int(np.count_nonzero(np.diff(cell[use]) != 1))
