"""NumPy restatement of the squelch stage (include/sdrg.h, csrc/squelch.hip): block powers by the adjacent-pair tree, the
smoothed level, the hysteresis gate with its hang time, the ramps and the records, over a stream of concatenated calls,
operation by operation in float32, so the GPU tests compare bytes.  open_thr, close_thr and beta are arguments: the tests
pass the library's (sdrg.squelch_design), so no libm difference enters a byte comparison; design_formula restates how
the library makes them.  The records' dB is the display stage's (display_cases.db)."""
import numpy as np

import display_cases as dc

f32 = np.float32
MIN_BLOCK, MAX_BLOCK, MAX_HANG, MAX_IN = 16, 1024, 65535, 1 << 20
RECORD = np.dtype([("level", "<f4"), ("level_db", "<f4"), ("open", "<i4"), ("open_blocks", "<i4")])
CLOSED, RAMP_UP, RAMP_DOWN, OPEN = 0, 1, 2, 3


def design_formula(open_db, close_db, tau_blocks):
    """(open_thr, close_thr, beta) in double; the caller rounds to float.  beta is exactly 1 at tau_blocks = 0."""
    beta = 1.0 - np.exp(-1.0 / tau_blocks) if tau_blocks > 0 else 1.0
    return 10.0 ** (open_db / 10.0), 10.0 ** (close_db / 10.0), beta


def valid_config(c):
    """The rules of set_squelch on a dict of sdrg_squelch_config's fields."""
    fin = np.isfinite
    ok = fin(c["open_db"]) and fin(c["close_db"]) and c["close_db"] <= c["open_db"] and fin(c["tau_blocks"]) and \
        c["tau_blocks"] >= 0 and MIN_BLOCK <= c["block"] <= MAX_BLOCK and c["block"] & (c["block"] - 1) == 0 and \
        0 <= c["hang_blocks"] <= MAX_HANG and 1 <= c["max_in"] <= MAX_IN
    if ok:
        with np.errstate(over="ignore", under="ignore"):
            for db in (c["open_db"], c["close_db"]):
                thr = f32(10.0 ** (db / 10.0)) if db < 3000 else f32(np.inf)
                ok = ok and bool(fin(thr) and thr > 0)
    return bool(ok)


def tree_sum(q):
    """The adjacent-pair tree over the last axis (a power of two long): q'[i] = q[2 i] + q[2 i + 1] until one is left."""
    q = np.asarray(q, f32)
    while q.shape[-1] > 1:
        q = q[..., 0::2] + q[..., 1::2]
    assert q.dtype == np.float32
    return q[..., 0]


def running_sum(q):
    """What the tree is not: the powers added one after the other in float32."""
    acc = f32(0)
    for v in np.asarray(q, f32):
        acc = f32(acc + v)
    return acc


def powers(z):
    """p = zr zr + zi zi of complex64 samples: two rounded products, one rounded sum."""
    z = np.asarray(z, np.complex64)
    zr, zi = np.ascontiguousarray(z.real), np.ascontiguousarray(z.imag)
    p = zr * zr + zi * zi
    assert p.dtype == np.float32
    return p


class Squelch:
    """One engine's squelch state: g and, per stream, the powers of the block in progress, L, open, hang and the
    current block's code."""

    def __init__(self, B, open_thr, close_thr, beta, S, H):
        self.B, self.S, self.H = B, int(S), int(H)
        self.open_thr, self.close_thr, self.beta = f32(open_thr), f32(close_thr), f32(beta)
        self.r = f32(1.0) / f32(self.S)
        self.reset()

    def reset(self):
        B = self.B
        self.g = 0
        self.pw = np.zeros((B, self.S), np.float32)
        self.L = np.zeros(B, np.float32)
        self.open = np.zeros(B, np.int32)
        self.hang = np.zeros(B, np.int32)
        self.code = np.zeros(B, np.int32)

    def step(self, P):
        """One completed block of mean powers P [B]: the level, the gate, the next block's code."""
        with np.errstate(invalid="ignore", over="ignore"):
            if self.beta == 1:
                L = P.copy()
            else:
                d = P - self.L
                L = self.L + self.beta * d
        assert L.dtype == np.float32
        was, hang = self.open, self.hang
        is_open = was == 1
        hold = is_open & (L >= self.close_thr)
        count = is_open & ~hold & (hang > 0)
        shut = is_open & ~hold & (hang == 0)
        opens = ~is_open & (L >= self.open_thr)
        self.hang = np.where(hold | opens, self.H, np.where(count, hang - 1, hang)).astype(np.int32)
        self.open = np.where(shut, 0, np.where(opens, 1, was)).astype(np.int32)
        self.code = (2 * was + self.open).astype(np.int32)
        self.L = L

    def gate(self, z, first):
        """z complex64 [B][m], the samples at the in-block indices first .. first + m - 1, under self.code."""
        S, r = self.S, self.r
        i = first + np.arange(z.shape[1])
        up = ((i + 1).astype(np.float32) * r).astype(np.float32)
        down = ((S - 1 - i).astype(np.float32) * r).astype(np.float32)
        code = self.code[:, None]
        w = np.where(code == RAMP_UP, up[None, :], down[None, :]).astype(np.float32)
        zr, zi = np.ascontiguousarray(z.real), np.ascontiguousarray(z.imag)
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            ramp = np.stack([zr * w, zi * w], axis=-1)
        assert ramp.dtype == np.float32
        whole = np.stack([zr, zi], axis=-1)
        out = np.where((code == OPEN)[..., None], whole, np.where((code == CLOSED)[..., None], f32(0), ramp))
        return np.ascontiguousarray(out, np.float32).view(np.complex64)[..., 0]

    def call(self, chan, in_stride=None):
        """chan complex64 [B][n] -> (out complex64 [B][in_stride], zeros from n on; records [B]; n_blocks)."""
        B, S = self.B, self.S
        z = np.asarray(chan, np.complex64).reshape(B, -1)
        n = z.shape[1]
        out = np.zeros((B, n if in_stride is None else in_stride), np.complex64)
        open_blocks = np.zeros(B, np.int32)
        n_blocks, i = 0, 0
        while i < n:
            fill = (self.g + i) % S
            m = min(S - fill, n - i)
            seg = z[:, i:i + m]
            self.pw[:, fill:fill + m] = powers(seg)
            out[:, i:i + m] = self.gate(seg, fill)
            i += m
            if fill + m == S:
                self.step(tree_sum(self.pw) * self.r)
                open_blocks += self.open
                n_blocks += 1
        self.g += n
        rec = np.zeros(B, RECORD)
        rec["level"], rec["level_db"], rec["open"], rec["open_blocks"] = self.L, dc.db(self.L), self.open, open_blocks
        return out, rec, n_blocks


def one_call(chan, open_thr, close_thr, beta, S, H):
    z = np.asarray(chan, np.complex64)
    z = z.reshape(1, -1) if z.ndim == 1 else z
    return Squelch(z.shape[0], open_thr, close_thr, beta, S, H).call(z)


def in_calls(chan, cuts, open_thr, close_thr, beta, S, H):
    """The stream chan [B][n] cut at the indices `cuts`: (the outs concatenated, the last records, the blocks in all)."""
    z = np.asarray(chan, np.complex64)
    sq = Squelch(z.shape[0], open_thr, close_thr, beta, S, H)
    edges = [0] + list(cuts) + [z.shape[1]]
    outs, blocks, rec = [], 0, None
    for a, b in zip(edges[:-1], edges[1:]):
        o, rec, nb = sq.call(z[:, a:b])
        outs.append(o)
        blocks += nb
    return np.concatenate(outs, axis=1), rec, blocks


def noise(B, n, seed, amp=1.0):
    rng = np.random.default_rng(seed)
    return (amp * (rng.standard_normal((B, n)) + 1j * rng.standard_normal((B, n))) / np.sqrt(2.0)).astype(np.complex64)


def keyed(B, n, seed, S, pattern, loud=1.0, quiet=0.01):
    """Noise whose rms is `loud` in the blocks of S where pattern (cycled, shifted by the stream's index) is 1, `quiet`
    where it is 0: every stream opens and closes at its own blocks."""
    z = noise(B, n, seed)
    blocks = np.arange(n) // S
    for b in range(B):
        on = np.asarray(pattern)[(blocks + b) % len(pattern)] != 0
        z[b] *= np.where(on, f32(loud), f32(quiet)).astype(np.float32)
    return z
