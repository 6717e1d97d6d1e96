"""CPU tests of the symbol stage: its NumPy restatement (tests/symbols_cases.py) on a hand-worked signal and on the
rules of its step, its continuity over calls of any length, its behaviour on 2- and 4-level signals, a clock offset and
noise (the figures of the stage's design note, each with its condition), the library's host-only functions (the design,
its refusals, the symbol count) and the boundary (the header declares the entry points, the library and sdrg.EXPORTS
carry them).  No device is touched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import symbols_cases as sc

f32 = np.float32
NEW_SYMBOLS = ("sdrg_symbols_design", "sdrg_symbols_geometry", "sdrg_symbols_count", "sdrg_engine_set_symbols",
               "sdrg_engine_get_symbols", "sdrg_engine_symbols_reset", "sdrg_engine_symbols_max_out",
               "sdrg_engine_symbols_device", "sdrg_engine_symbols_host", "sdrg_engine_listen_symbols_host")
OK = sc.BASE
INC10 = 429496730  # 4800 symbols/s at 48 kHz: rint(2^32 / 10)


@pytest.fixture(scope="module")
def S():
    import sdrg
    return sdrg


def test_header_library_and_mirror_carry_the_stage(S):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sdrg.h")).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", S.lib_path()], capture_output=True, text=True, check=True).stdout
    L = S.load()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert re.search(r"\bT %s$" % s, nm, flags=re.M), s
        assert s in S.EXPORTS and hasattr(L, s)
    for s in ("sdrg_symbols_config", "sdrg_symbols_record", "sdrg_symbols_design_values", "#define SDRG_SYM_LEVEL_TRACK 1",
              "#define SDRG_SYM_LEVEL_FIXED 2", "#define SDRG_SYM_HARD 1", "#define SDRG_SYM_SOFT 2",
              "#define SDRG_SYM_MIN_BLOCK 64", "#define SDRG_SYM_MAX_BLOCK 1024", "#define SDRG_SYM_HISTORY 66"):
        assert s in text
    assert ctypes.sizeof(S.SymbolsConfig) == 104 and ctypes.sizeof(S.SymbolsDesign) == 56
    assert S.SymbolsRecord == sc.RECORD and S.SymbolsRecord.itemsize == 32
    assert (S.SYM_LEVEL_TRACK, S.SYM_LEVEL_FIXED, S.SYM_HARD, S.SYM_SOFT) == (sc.LEVEL_TRACK, sc.LEVEL_FIXED, sc.HARD, sc.SOFT)
    assert (S.SYM_LOCKED, S.SYM_SEEDED, S.SYM_UNLOCKED, S.SYM_HISTORY, S.SYM_TABLE) == \
        (sc.LOCKED, sc.SEEDED, sc.UNLOCKED, sc.HISTORY, sc.TABLE)
    assert tuple(k for k, _ in S.SymbolsDesign._fields_) == sc.DESIGN
    for block in (64, 128, 256, 512, 1024):
        assert S.symbols_geometry(block) == (max(512, block), 256)
    t = ctypes.c_int32()
    for bad in (0, 16, 32, 96, 2048, -64):
        assert L.sdrg_symbols_geometry(bad, ctypes.byref(t), None) == -1


BAD = [("sample_rate", 0.0), ("sample_rate", -48000.0), ("sample_rate", np.inf), ("sample_rate", np.nan),
       ("symbol_rate", 0.0), ("symbol_rate", np.nan), ("symbol_rate", np.inf), ("symbol_rate", 48000.0 / 1.99),
       ("symbol_rate", 48000.0 / 64.01), ("levels", 0), ("levels", 3), ("levels", 8), ("block", 32), ("block", 96),
       ("block", 2048), ("block", 0), ("tau_blocks", -1.0), ("tau_blocks", np.inf), ("tau_blocks", np.nan),
       ("tau_level_blocks", -0.5), ("tau_level_blocks", np.inf), ("floor_db", np.nan), ("floor_db", np.inf),
       ("floor_db", 400.0), ("floor_db", -500.0), ("lock_threshold", -0.01), ("lock_threshold", 1.01),
       ("lock_threshold", np.nan), ("phase_trim", -0.51), ("phase_trim", 0.51), ("phase_trim", np.nan),
       ("level_mode", 0), ("level_mode", 3), ("level_scale", 0.0), ("level_scale", -1.0), ("level_scale", np.inf),
       ("fixed_centre", np.nan), ("fixed_centre", np.inf), ("fixed_threshold", 0.0), ("fixed_threshold", np.inf),
       ("format", 0), ("format", 3), ("max_in", 0), ("max_in", (1 << 20) + 1)]


@pytest.mark.parametrize("field,value", BAD)
def test_each_bad_field_is_refused_on_its_own(S, field, value):
    """Every other field is valid: the one field refuses the design (and, by the same check, set_symbols)."""
    S.symbols_design(**OK)
    assert sc.valid_config(OK)
    cfg = dict(OK, **{field: value})
    assert not sc.valid_config(cfg)
    with pytest.raises(S.SdrgError) as ei:
        S.symbols_design(**cfg)
    assert "SDRG_E_INVALID" in str(ei.value)


def test_the_limits_are_accepted(S):
    for cfg in (dict(OK, symbol_rate=24000.0), dict(OK, symbol_rate=750.0), dict(OK, block=64), dict(OK, tau_blocks=0.0),
                dict(OK, tau_level_blocks=0.0), dict(OK, lock_threshold=0.0), dict(OK, lock_threshold=1.0),
                dict(OK, phase_trim=-0.5), dict(OK, phase_trim=0.5), dict(OK, levels=4, format=sc.SOFT),
                dict(OK, level_mode=sc.LEVEL_FIXED, fixed_centre=-3.0), dict(OK, max_in=1), dict(OK, max_in=1 << 20),
                dict(OK, floor_db=-440.0)):
        assert sc.valid_config(cfg), cfg
        S.symbols_design(**cfg)


def test_design_agrees_with_the_formulas(S):
    for cfg in (OK, dict(OK, tau_blocks=0.0, tau_level_blocks=0.0), dict(OK, symbol_rate=24000.0),
                dict(OK, symbol_rate=750.0, block=64), dict(OK, sample_rate=50000.0, phase_trim=-0.5),
                dict(OK, symbol_rate=1200.0, phase_trim=0.123, floor_db=-120.0, lock_threshold=1.0, level_scale=2 / np.sqrt(5),
                     fixed_centre=-0.7, fixed_threshold=1e-3, tau_level_blocks=1e6), dict(OK, floor_db=-440.0)):
        got, want = S.symbols_design(**cfg), sc.design_formula(cfg)
        assert tuple(got) == sc.DESIGN + ("table",)
        assert got["inc"] == want["inc"] and got["trim"] == want["trim"]
        for name in sc.DESIGN[2:]:
            assert got[name].dtype == np.float32
            assert got[name].tobytes() == want[name].tobytes() or \
                abs(float(got[name]) - float(want[name])) <= float(np.spacing(want[name])), (cfg, name)
        assert got["table"].dtype == np.float32 and got["table"].shape == (sc.TABLE, 2)
        assert np.all(np.abs(got["table"] - want["table"]) <= np.spacing(np.abs(want["table"]).astype(np.float32)))
    d = S.symbols_design(**dict(OK, tau_blocks=0.0, tau_level_blocks=0.0))
    assert d["beta"].tobytes() == f32(1.0).tobytes() and d["beta_level"].tobytes() == f32(1.0).tobytes()
    assert S.symbols_design(**OK)["inc"] == INC10 and S.symbols_design(**OK)["rs"] == f32(2.0 ** -10)
    assert S.symbols_design(**dict(OK, symbol_rate=24000.0))["inc"] == 1 << 31
    assert S.symbols_design(**dict(OK, symbol_rate=750.0))["inc"] == 1 << 26
    assert S.symbols_design(**dict(OK, phase_trim=0.5))["trim"] == 1 << 31
    # the table's two halves mirror each other exactly: the hand-worked signal below leans on it
    t = S.symbols_design(**OK)["table"]
    assert np.array_equal(t[512:], -t[:512])


@pytest.mark.parametrize("inc", [1 << 26, 1 << 31, 894784853])
def test_count_agrees_with_a_scan_of_the_clock(S, inc):
    """sdrg_symbols_count against the emitting samples counted one by one in Python integers."""
    def scan(g, n):
        return sum(1 for i in range(g, g + n) if i >= 1 and (inc * i) & sc.M32 < inc)
    near = (1 << 32) // inc
    for g in (0, 1, near - 1, near, near + 1, 2 * near + 1, (1 << 40) + 3):
        for n in (0, 1, 2, near - 1, near, near + 1, 777):
            assert S.symbols_count(inc, g, n) == scan(g, n) == sc.count(inc, g + n) - sc.count(inc, g), (g, n)
            assert int(np.count_nonzero(sc.emits(inc, g, n))) == scan(g, n)
    assert S.load().sdrg_symbols_count((1 << 26) - 1, 0, 10) == -1 and S.load().sdrg_symbols_count((1 << 31) + 1, 0, 10) == -1


def test_counts_of_every_cut_add_up(S):
    rng = np.random.default_rng(7)
    for inc in (1 << 26, INC10, 894784853, 1 << 31):
        for g0 in (0, 5, (1 << 40) + 3):
            n = 3000
            whole = S.symbols_count(inc, g0, n)
            for cut in list(range(0, 70)) + list(rng.integers(0, n + 1, 20)):
                assert S.symbols_count(inc, g0, cut) + S.symbols_count(inc, g0 + cut, n - cut) == whole
            assert whole <= sc.cap(inc, n)
            edges = np.concatenate([[0], np.sort(rng.integers(0, n + 1, 9)), [n]])
            assert sum(S.symbols_count(inc, g0 + int(a), int(b - a)) for a, b in zip(edges[:-1], edges[1:])) == whole


def square(n):
    return np.tile(np.array([1, 1, -1, -1], np.float32), n // 4 + 1)[:n]


@pytest.mark.parametrize("trim,want_y", [(0.25, 1.0), (-0.25, -1.0), (0.0, None)])
def test_a_signal_worked_by_hand(S, trim, want_y):
    """inc = 2^30: cells of 4 samples, c_i = (i mod 4) 2^30, and i emits when i mod 4 = 0 (i >= 4).  x = +1 +1 -1 -1
    repeated has dx = +2 at i mod 4 = 0 and -2 at i mod 4 = 2, so u = 4 there and 0 elsewhere, against tab[0] = (c, s) =
    (cos, sin)(pi / 1024) and tab[512] = (-c, -s).  In a block of S = 64 the first position (i mod 4 = 0) has u = +0, so
    the sums keep 15 edges at phase 0 and 16 at phase 1 / 2: every level of the tree is exact (integers times c or s),
    T(a) = -4 c, T(b) = -4 s, T(u) = 4 * 31, T(x) = 0, T(q) = 64.  The first block seeds: A = -4 c / 64, B = -4 s / 64,
    U = 124 / 64, M = 0, Q = 1; coh is about (4 / 64) / (124 / 64) = 1 / 31, over the threshold 0.01: locked.  The angle
    is -pi + pi / 1024 within sdrg_atan2f's 3.6e-7, so ang = -2^31 + 2^21 within 3.6e-7 K + 256 < 512, and
      tau = ang - 2^29 + 2^31 + trim = 2^32 - 2^29 + 2^21 + trim 2^32 (mod 2^32):
    the surviving edge (between i mod 4 = 1 and 2, half a sample before i mod 4 = 2: 1.5), half a cell on (3.5 of 4 =
    0.875 = 1 - 2^29 / 2^32), plus the table's half entry 2^21 / 2^32.  TRACK levels: centre = +0, thr = sqrtf(1 - 0) = 1.
    Before: tau = 2^31 + trim, unlocked, centre = +0, thr = 1: the first 15 symbols (i = 4 .. 60) carry 0x80.
    From block 1 on, with c_i = 0 at an emitting i, num = 2^32 - tau:
      trim = +0.25  tau = 2^29 + 2^21 + e; num = 7 2^29 - 2^21 - e, qd = 3, 0 < r < 2^30: between x[i - 3] = +1 and
                    x[i - 4] = +1 (i mod 4 = 0): y = 1 - nu 0 = +1 exactly, the middle of the +1 +1 run: bit 1.
      trim = -0.25  tau = 5 2^29 + 2^21 + e; num = 3 2^29 - 2^21 - e, qd = 1: between x[i - 1] = -1 and x[i - 2] = -1:
                    y = -1 exactly: bit 0.
      trim = 0      num = 2^29 - 2^21 - e, qd = 0, r = num: between x[i] = +1 and x[i - 1] = -1, at nu = (float) r *
                    2^-30 (exact: rinc is a power of two): y = 1 - 2 nu = 2^-8 + 2^-29 e', every step exact for the r at
                    hand: bit 1, from the table's half entry alone; asserted from the tau that was found.
    Before the lock (block 0): trim = +0.25: tau = 3 2^30, num = 2^30: qd = 1, r = 0: y = x[i - 1] = -1: 0x80 | 0;
    trim = -0.25: tau = 2^30, num = 3 2^30: qd = 3: y = x[i - 3] = +1: 0x80 | 1; trim = 0: num = 2^31: qd = 2: y = x[i -
    2] = -1: 0x80 | 0."""
    cfg = dict(OK, sample_rate=48000.0, symbol_rate=12000.0, block=64, lock_threshold=0.01, phase_trim=trim, max_in=4096)
    des = S.symbols_design(**cfg)
    assert des["inc"] == 1 << 30 and des["rinc"] == f32(2.0 ** -30)
    q = sc.make(1, des, cfg)
    n = 64 * 5
    out, rec, n_sym = q.call(square(n)[None])
    assert n_sym == n // 4 - 1 == S.symbols_count(1 << 30, 0, n)
    tau = int(rec["tau"][0])
    expect = ((1 << 32) - (1 << 29) + (1 << 21) + int(trim * 2 ** 32)) & sc.M32
    assert abs(tau - expect) < 512 and rec["flags"][0] == 3 and rec["slips"][0] <= 1 and rec["held_blocks"][0] == 0
    assert np.all(q.traced("tau") == tau)  # every block is the first again: the smoothed sums never move
    assert rec["centre"][0].tobytes() == f32(0).tobytes() and rec["threshold"][0] == f32(1)
    assert abs(float(rec["coherence"][0]) - 1 / 31) < 1e-6
    assert rec["tau_frac"][0] == f32(tau) * f32(2.0 ** -32)
    before = {0.25: 0x80, -0.25: 0x81, 0.0: 0x80}[trim]
    assert np.all(out[0, :15] == before)
    y = 1.0 - 2.0 * float(f32((1 << 32) - tau) * f32(2.0 ** -30)) if want_y is None else want_y
    assert np.all(out[0, 15:n_sym] == (1 if y >= 0 else 0)) and not out[0, n_sym:].any()
    # the same stream in SOFT: v / thr = y, bit for bit
    qs = sc.make(1, des, dict(cfg, format=sc.SOFT))
    soft, _, _ = qs.call(square(n)[None])
    assert soft.dtype == np.float32 and np.all(soft[0, 15:n_sym].view(np.uint32) == f32(y).view(np.uint32))
    assert np.all(soft[0, :15] == {0.25: -1.0, -0.25: 1.0, 0.0: -1.0}[trim])
    if want_y is None:
        assert abs(y - 2.0 ** -8) < 1e-5


def test_the_slip_rule():
    H = 1 << 31
    table = [(10, 20, False), (20, 10, False), (0xFFFFFF00, 0x10, True), (0x10, 0xFFFFFF00, True), (5, 5, False),
             (0, H - 1, False), (0, H, True), (0, H + 1, True), (H, 0, False), (H + 1, 0, True), (H - 1, 0, False),
             (0x40000000, 0xC0000000, True), (0xC0000000, 0x40000000, False), (0xC0000001, 0x40000000, True),
             (0xFFFFFFFF, 0, True), (0, 0xFFFFFFFF, True), (1, 0xFFFFFFFF, True), (0xFFFFFFFF, 0xFFFFFFFE, False)]
    for tau, nxt, want in table:
        d = ((nxt - tau + H) % (1 << 32)) - H  # the int32 of the difference
        assert ((d >= 0 and nxt < tau) or (d < 0 and nxt > tau)) == want, (tau, nxt)
        assert bool(sc.slipped(np.uint32(tau), np.uint32(nxt))) == want, (tau, nxt)


def stream(B, n, seed, T=10.0, levels=2, snr_db=20.0):
    return np.stack([sc.signal(levels, T, snr_db, n_symbols=int(n / T) + 2, seed=seed + b, start=0.37 + 0.05 * b)[0][:n]
                     for b in range(B)])


def test_floor_seed_and_beta_one(S):
    cfg = dict(OK, block=64, floor_db=-20.0, tau_blocks=0.0, tau_level_blocks=0.0)
    des = S.symbols_design(**cfg)
    assert des["beta"] == 1 and des["beta_level"] == 1
    x = stream(2, 64 * 8, 3)
    x[0, 64:192] = 0  # blocks 1 and 2 of stream 0 lie under the floor; so does its block 0, scaled down
    x[0, :64] *= f32(1e-3)
    q = sc.make(2, des, cfg)
    out, rec, _ = q.call(x)
    held, flags = q.traced("held"), q.traced("flags")
    assert held[:, 0].tolist() == [1, 1, 1, 0, 0, 0, 0, 0] and not held[:, 1].any() and rec["held_blocks"].tolist() == [3, 0]
    assert flags[:3, 0].tolist() == [0, 0, 0] and (flags[3:, 0] & sc.SEEDED).all() and (flags[:, 1] & sc.SEEDED).all()
    assert np.all(q.traced("coh")[:3, 0] == 0) and np.all(q.traced("tau")[:3, 0] == 1 << 31)
    # while held and unseeded the levels stay a restart's: centre +0, thr 1, and every symbol carries 0x80
    t = np.flatnonzero(sc.emits(des["inc"], 0, 64 * 8))
    first = np.searchsorted(t, 4 * 64)  # block 4 is the first sampled after a step that was not held
    assert np.all(out[0, :first] & 0x80)
    # beta = 1: after each block the state is the block's own sums, so the record is the last block's alone
    c = sc.clock(des["inc"], np.arange(7 * 64, 8 * 64, dtype=np.uint64))
    Ab, Bb, Ub, Mb, Qb = sc.block_sums(x[:, 7 * 64:], c[None], q.tab, des["rs"])
    assert q.st.A.tobytes() == Ab.tobytes() and q.st.B.tobytes() == Bb.tobytes() and q.st.U.tobytes() == Ub.tobytes()
    assert q.st.M.tobytes() == Mb.tobytes() and q.st.Q.tobytes() == Qb.tobytes() and rec["centre"].tobytes() == Mb.tobytes()
    # the seed is the first block over the floor whatever beta: a slow stage's state after it is that block's sums
    slow = S.symbols_design(**dict(cfg, tau_blocks=50.0, tau_level_blocks=50.0))
    q2 = sc.make(2, slow, cfg)
    q2.call(x[:, :64 * 4])
    c = sc.clock(des["inc"], np.arange(3 * 64, 4 * 64, dtype=np.uint64))
    assert q2.st.A[0].tobytes() == sc.block_sums(x[:1, 3 * 64:4 * 64], c[None], q.tab, des["rs"])[0].tobytes()


def test_soft_with_a_zero_threshold_and_the_flag_before_lock(S):
    cfg = dict(OK, block=64, format=sc.SOFT, max_in=1024)
    des = S.symbols_design(**cfg)
    q = sc.make(1, des, cfg)
    x = np.full((1, 640), 0.25, np.float32)  # a constant: Q - M M = 0 exactly, so thr = +0 after the first block
    out, rec, n_sym = q.call(x)
    assert rec["threshold"][0].tobytes() == f32(0).tobytes() and rec["centre"][0] == f32(0.25)
    t = np.flatnonzero(sc.emits(des["inc"], 0, 640))
    late = t >= 64
    assert np.all(out[0, :n_sym][late].view(np.uint32) == 0) and np.any(out[0, :n_sym][~late] != 0)
    # HARD: U = 0 gives coh = +0, never locked: every byte carries 0x80; with lock_threshold 0 it locks at once
    for thr, want in ((0.1, 0x80), (0.0, 0)):
        c2 = dict(cfg, format=sc.HARD, lock_threshold=thr)
        q = sc.make(1, S.symbols_design(**c2), c2)
        out, rec, n_sym = q.call(x)
        assert rec["coherence"][0].tobytes() == f32(0).tobytes()
        assert np.all(out[0, :n_sym][late] & 0x80 == want) and np.all(out[0, :n_sym][~late] & 0x80 == 0x80)


@pytest.mark.parametrize("levels,fmt,mode", [(2, sc.HARD, sc.LEVEL_TRACK), (4, sc.SOFT, sc.LEVEL_TRACK),
                                             (4, sc.HARD, sc.LEVEL_FIXED)])
def test_every_cut_of_a_stream_gives_the_bytes_of_one_call(S, levels, fmt, mode):
    """n = 0 and n = 1, cuts inside a block, and cuts that leave the symbol's 66 values of history across the seam: at
    64 samples per symbol a symbol reaches back 65 values, over a whole block of 64 and the call before it."""
    for rate, block, n in ((4800.0, 64, 700), (750.0, 64, 1500), (4800.0 * 10 / 10.4167, 256, 1100)):
        cfg = dict(OK, symbol_rate=rate, levels=levels, format=fmt, level_mode=mode, block=block, lock_threshold=0.05,
                   tau_blocks=2.0, fixed_centre=0.7, fixed_threshold=2.0, level_scale=2 / np.sqrt(5) if levels == 4 else 1.0,
                   max_in=2048)
        des = S.symbols_design(**cfg)
        x = stream(2, n, 11, T=48000.0 / rate, levels=levels)
        whole, rec, n_sym = sc.make(2, des, cfg).call(x)
        assert n_sym == sc.count(des["inc"], n) and (whole[:, :n_sym] != 0).any()
        cuts = [[c] for c in list(range(0, 70)) + [block - 1, block, block + 1, 2 * block, n - 1, n]]
        cuts += [[0, 0, 1, 2], [1, 1, 65, 66, 67, 133], [block - 1, block, block + 1], [63, 64, 64, 65, 130, 131, 200],
                 list(range(5, n, 37)), list(range(1, 300))]
        for cut in cuts:
            got, r, _ = sc.in_calls(sc.make(2, des, cfg), x, cut)
            assert got.tobytes() == whole[:, :n_sym].tobytes(), (rate, cut)
            for k in ("tau", "coherence", "centre", "threshold", "slips", "flags", "tau_frac"):
                assert r[k].tobytes() == rec[k].tobytes(), (rate, cut, k)


# ---- behaviour: the readings of the restatement beside each condition (a float64 prototype's readings in DESIGN §3.24)

def behave(S, fs, rate, levels, snr_db, ppm=0.0):
    cfg = dict(OK, sample_rate=fs, symbol_rate=rate, levels=levels, level_scale=1.0 if levels == 2 else 2 / np.sqrt(5),
               max_in=1 << 20)
    des = S.symbols_design(**cfg)
    T = fs / rate * (1 + ppm * 1e-6)
    x, sym, edge = sc.signal(levels, T, snr_db)
    q = sc.make(1, des, cfg)
    outs = []
    for a in range(0, len(x), 1 << 20):
        o, rec, ns = q.call(x[None, a:a + (1 << 20)])
        outs.append(o[0, :ns])
    errors, scored, frac, jumps = sc.score(q, np.concatenate(outs), sym, T, edge)
    print(fs, rate, levels, snr_db, ppm, "errors", errors, "of", scored, "instant", frac.mean() if scored else None,
          "jumps", jumps, "slips", rec["slips"][0], "coherence", rec["coherence"][0])
    return errors, scored, frac, jumps, rec, q


def test_two_levels_at_20_db(S):
    errors, scored, frac, jumps, rec, _ = behave(S, 48000.0, 4800.0, 2, 20.0)
    assert errors == 0 and scored > 37000  # reads 0 of 37 543
    assert abs(frac.mean() - 0.5) < 0.05 and jumps == 0 and rec["slips"][0] == 0  # reads 0.4801, spread 0.0009


def test_four_levels_at_20_db(S):
    errors, scored, frac, jumps, rec, _ = behave(S, 48000.0, 4800.0, 4, 20.0)
    assert scored > 37000 and errors / scored < 1e-3  # reads 0 of 37 543
    assert abs(frac.mean() - 0.5) < 0.05 and jumps == 0  # reads 0.4802


def test_four_levels_at_12_db(S):
    errors, scored, frac, _, _, _ = behave(S, 48000.0, 4800.0, 4, 12.0)
    assert scored > 37000 and 0.01 < errors / scored < 0.08  # reads 1468 of 37 543: 3.9 %
    assert abs(frac.mean() - 0.5) < 0.05  # reads 0.4801


@pytest.mark.parametrize("ppm", [-50.0, 50.0])
def test_a_clock_offset_slips(S, ppm):
    """50 ppm of 40 000 symbols is two cells: the sampling point goes round the cell's edge twice, each time one
    transmitter symbol is sampled twice (or not at all), counted by `slips`, and every scored symbol is still right."""
    errors, scored, frac, jumps, rec, _ = behave(S, 50000.0, 4800.0, 4, 25.0, ppm)
    assert errors == 0 and scored > 37000  # reads 0 of 37 639 (-50 ppm), 0 of 37 643 (+50 ppm)
    assert 2 <= rec["slips"][0] <= 4 and jumps == 2  # reads 2 and 2, both ways
    assert abs(frac.mean() - 0.5) < 0.05  # reads 0.5409 and 0.4589: the smoothed estimate trails the drift


def test_forty_samples_per_symbol(S):
    errors, scored, frac, _, rec, _ = behave(S, 48000.0, 1200.0, 2, 30.0)
    assert errors == 0 and scored > 39000  # reads 0 of 39 386
    assert abs(frac.mean() - 0.5) < 0.05  # reads 0.4926
    # at 10 dB the squared difference of 40 samples per symbol drowns: never locked (coherence reads 0.013)
    _, scored, _, _, rec, q = behave(S, 48000.0, 1200.0, 2, 10.0)
    assert scored == 0 and not (q.traced("flags") & sc.LOCKED).any() and rec["coherence"][0] < 0.1


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_noise_does_not_lock(S, seed):
    des = S.symbols_design(**OK)
    q = sc.make(1, des, dict(OK, max_in=1 << 20))
    out, rec, n_sym = q.call(sc.noise(400000, seed)[None])
    print("noise", seed, "coherence max", q.traced("coh").max(), "last", rec["coherence"][0])
    assert not (q.traced("flags") & sc.LOCKED).any() and np.all(out[0, :n_sym] & 0x80)  # reads at most 0.077, last 0.01


def test_restatement_follows_the_float64_model(S):
    """The decisions of the float32 restatement against the same law in float64 on a clean signal: every symbol, the
    lock of every block and the sampling instants within 1e-3 of a sample (tau differs by the angle's 3.6e-7 K / 2^32
    of a cell and the sums' rounding, far under that)."""
    cfg = dict(OK, block=256, levels=4, level_scale=2 / np.sqrt(5), max_in=1 << 16)
    des = S.symbols_design(**cfg)
    x, _, _ = sc.signal(4, 10.0, 30.0, n_symbols=3000, seed=5)
    q = sc.make(1, des, cfg)
    out, _, n_sym = q.call(x[None])
    sym, lock, inst, coh = sc.model64(x, des, 256, levels=4)
    assert n_sym == len(sym) and np.array_equal((out[0, :n_sym] & 0x80) == 0, lock)
    assert np.array_equal(out[0, :n_sym] & 3, sym)
    assert np.max(np.abs(np.concatenate(q.points, axis=1)[0] - inst)) < 1e-3
    assert np.max(np.abs(q.traced("coh")[:, 0] - coh)) < 1e-4
