"""CPU tests of the tone detector stage: its NumPy restatement (tests/tones_cases.py) on hand-worked streams, the tree
against a running sum and rounded products against fused ones, its continuity over calls of any length, the tie rule, the
latch table, the three signal cases of the stage's purpose (a CTCSS tone in noise, a keyed tone, the sign of a complex
tone), the host-side design and its refusals, and the boundary (the header declares the entry points, the library and
sdrg.EXPORTS carry them).  No device is touched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import tones_cases as tc

f32 = np.float32
NEW_SYMBOLS = ("sdrg_tones_design", "sdrg_tones_geometry", "sdrg_engine_set_tones", "sdrg_engine_get_tones",
               "sdrg_engine_tones_reset", "sdrg_engine_tones_max_blocks", "sdrg_engine_tones_device",
               "sdrg_engine_tones_host", "sdrg_engine_listen_tones_host")
OK = dict(rate_hz=8000.0, components=1, freq_hz=(1000.0, 1750.0), sub_blocks=2, window=tc.RECT, min_db=-40.0,
          dominance_db=6.0, share=0.25, confirm_blocks=2, release_blocks=1, max_in=4096)
FA_CTCSS = 2_000_000 / 41 / 4


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
    for s in ("sdrg_tones_config", "sdrg_tones_record", "sdrg_tones_scalars", "#define SDRG_TONES_MAX_TONES 64",
              "#define SDRG_TONES_MAX_SUB_BLOCKS 256", "#define SDRG_TONES_MAX_IN 65536", "#define SDRG_TONES_RECT 0",
              "#define SDRG_TONES_HANN 1"):
        assert s in text
    assert ctypes.sizeof(S.TonesConfig) == 8 + 64 * 8 + 3 * 8 + 8 * 4 and ctypes.sizeof(S.TonesScalars) == 20
    assert S.TonesRecord == tc.RECORD and S.TonesRecord.itemsize == 32
    assert (S.TONES_MAX_TONES, S.TONES_MAX_SUB_BLOCKS, S.TONES_MAX_IN) == (tc.MAX_TONES, tc.MAX_SUB_BLOCKS, tc.MAX_IN)
    assert (S.TONES_RECT, S.TONES_HANN) == (tc.RECT, tc.HANN)
    assert S.tones_geometry() >= 1
    assert L.sdrg_tones_geometry(None) == -1


@pytest.mark.parametrize("cfg", [
    OK, dict(OK, window=tc.HANN, sub_blocks=3), dict(OK, components=2, freq_hz=(-4000.0, 0.0, 425.0, 4000.0)),
    dict(OK, rate_hz=FA_CTCSS, freq_hz=tc.CTCSS, sub_blocks=128, window=tc.HANN, min_db=-30.0, dominance_db=10.0,
         share=0.05, max_in=16384),
    dict(OK, freq_hz=(3999.9,), sub_blocks=256, window=tc.HANN, min_db=-200.0, dominance_db=0.0, share=1.0, max_in=65536)])
def test_design_agrees_with_the_formulas(S, cfg):
    got = S.tones_design(**cfg)
    c, s, w, sc = tc.design_formula(cfg["rate_hz"], cfg["freq_hz"], cfg["sub_blocks"], cfg["window"], cfg["components"],
                                    cfg["min_db"], cfg["dominance_db"], cfg["share"])
    K, n = len(cfg["freq_hz"]), 64 * cfg["sub_blocks"]
    assert got["table"].shape == (K, n, 2) and got["table"].dtype == np.float32 and got["wf"].shape == (n,)

    def close(g, want, what):
        err = np.abs(g.astype(np.float64) - want)
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        # cos and sin of an angle that is itself rounded: its double rounding error (2^-50 at most), on top of the ulp
        assert np.all(err <= ulp + 2.0 ** -50), (what, float(err.max()))

    close(got["table"][:, :, 0], c, "c")
    close(got["table"][:, :, 1], s, "s")
    close(got["wf"], w, "wf")
    for k in tc.SCALARS:
        assert got[k].dtype == np.float32
        assert abs(float(got[k]) - sc[k]) <= float(np.spacing(f32(abs(sc[k])))), (k, got[k], sc[k])
    assert got["share_thr"] == f32(cfg["share"])
    assert tc.valid_config(dict(cfg, n_tones=K))


@pytest.mark.parametrize("bad", [
    dict(rate_hz=0.0), dict(rate_hz=-8000.0), dict(rate_hz=float("inf")), dict(rate_hz=float("nan")), dict(components=0),
    dict(components=3), dict(n_tones=0), dict(n_tones=65), dict(n_tones=-1), dict(freq_hz=(1000.0, 0.0)),
    dict(freq_hz=(1000.0, 4000.0)), dict(freq_hz=(-1000.0, 1750.0)), dict(freq_hz=(float("nan"), 1750.0)),
    dict(freq_hz=(1000.0, float("inf"))), dict(components=2, freq_hz=(4000.1,)), dict(components=2, freq_hz=(-4000.1,)),
    dict(sub_blocks=0), dict(sub_blocks=257), dict(window=2), dict(window=-1), dict(min_db=float("nan")),
    dict(min_db=float("inf")), dict(dominance_db=-0.5), dict(dominance_db=float("nan")), dict(dominance_db=float("inf")),
    dict(share=-0.01), dict(share=1.01), dict(share=float("nan")), dict(confirm_blocks=0), dict(confirm_blocks=256),
    dict(release_blocks=-1), dict(release_blocks=256), dict(max_in=0), dict(max_in=65537)])
def test_each_bad_field_is_refused_on_its_own(S, bad):
    cfg = dict(OK, **bad)
    full = dict(cfg)
    full.setdefault("n_tones", len(cfg["freq_hz"]))
    assert not tc.valid_config(full), bad
    with pytest.raises(S.SdrgError) as ei:
        S.tones_design(**cfg)
    assert "SDRG_E_INVALID" in str(ei.value)
    S.tones_design(**OK)  # and the good one passes
    assert S.load().sdrg_tones_design(None, None, None, None) == -1


def test_equal_and_edge_frequencies_are_accepted(S):
    S.tones_design(**dict(OK, freq_hz=(1000.0, 1000.0)))
    S.tones_design(**dict(OK, components=2, freq_hz=(4000.0, -4000.0, 0.0)))
    S.tones_design(**dict(OK, freq_hz=(1e-3, 3999.999), dominance_db=0.0, share=0.0, release_blocks=0))


def test_a_cosine_worked_by_hand():
    """K = 1, Q = 1, RECT, fa = 4 f: x = A (1, 0, -1, 0, ...) exactly.  c is (1, ~0, -1, ~0, ...), so C = 32 A; s is (0, 1, ~0,
    -1, ...) against zeros and the tiny sines of pi and 2 pi, so |S| < 1e-14; E = 32 A^2; pnorm = 4 / 64^2 and enorm = 2 /
    64: P = A^2 and Et = A^2, bit for bit at A = 0.5, and the share is 1."""
    cfg = dict(rate_hz=4000.0, freq_hz=(1000.0,), sub_blocks=1, confirm_blocks=1, max_in=64, min_db=-20.0, share=0.5)
    d = tc.formula_design(**cfg)
    assert d["pnorm"] == f32(4 / 4096) and d["enorm"] == f32(2 / 64)
    m = tc.model(1, d, **cfg)
    x = (f32(0.5) * np.tile(np.array([1, 0, -1, 0], np.float32), 16))[None, :]
    C, Sn, E = m.sub_sums(x, 0)
    assert C[0, 0] == f32(16.0) and abs(float(Sn[0, 0])) < 1e-14 and E[0] == f32(8.0)
    powers, rec, nb = m.call(x)
    assert nb == 1 and powers.shape == (1, 1, 1) and powers[0, 0, 0] == f32(0.25)
    r = rec[0]
    assert (r["tone"], r["candidate"], r["tone_blocks"], r["changes"], r["run"]) == (0, 0, 1, 1, 1)
    assert r["power"] == f32(0.25) and r["share"] == f32(1.0) and abs(float(r["power_db"]) + 6.0206) < 1e-3


def test_the_tree_is_not_a_running_sum_and_the_products_are_not_fused():
    cfg = dict(rate_hz=8000.0, freq_hz=(1000.0,), sub_blocks=1, confirm_blocks=1, max_in=64)
    m = tc.model(1, tc.formula_design(**cfg), **cfg)
    x = np.ones((1, 64), np.float32)
    x[0, 0] = 4096.0  # e = (2^24, 1, 1, ...): the tree keeps the pairs of ones, a running sum drops every one
    E = m.sub_sums(x, 0)[2][0]
    assert E == f32(2 ** 24 + 62) and tc.running_sum(x[0] * x[0]) == f32(2 ** 24)
    c2 = dict(cfg, components=2, freq_hz=(1234.5,))
    d2 = tc.formula_design(**c2)
    m2 = tc.model(1, d2, **c2)
    rng = np.random.default_rng(5)
    z = (rng.standard_normal((1, 64)) + 1j * rng.standard_normal((1, 64))).astype(np.complex64)
    c, s = d2["table"][0, :, 0].astype(np.float64), d2["table"][0, :, 1].astype(np.float64)
    xr, xi = z[0].real.astype(np.float64), z[0].imag.astype(np.float64)
    rounded = (xr * c).astype(np.float32) + (xi * s).astype(np.float32)
    fused = (xr * c + (xi * s).astype(np.float32).astype(np.float64)).astype(np.float32)  # fma(xr, c, xi s)
    assert np.any(rounded != fused)
    assert m2.sub_sums(z, 0)[0][0, 0] == tc.tree_sum(rounded) != tc.tree_sum(fused)


@pytest.mark.parametrize("components", [1, 2])
def test_any_cut_of_a_stream_gives_the_whole_streams_bytes(components):
    cfg = dict(OK, components=components, window=tc.HANN, freq_hz=(700.0, 1000.0, 1750.0), max_in=1024)
    d = tc.formula_design(**cfg)
    S_, B, n = 128, 2, 5 * 128 + 37
    rng = np.random.default_rng(11)
    x = tc.tone(n, 1000.0, 8000.0, 0.5, complex_=components == 2)[None, :] + \
        (0.05 * rng.standard_normal((B, n))).astype(np.float32)
    whole, rec, _ = tc.in_calls(tc.model(B, d, **cfg), x, [])
    assert whole.shape == (B, 5, 3) and np.all(rec["tone"] == 1)
    for piece in (0, 1, 63, 64, 65, S_ - 1, S_ + 1):
        cuts = list(range(piece, n, piece)) if piece else [0, 0, 200, 200]
        got, got_rec, recs = tc.in_calls(tc.model(B, d, **cfg), x, cuts)
        assert got.tobytes() == whole.tobytes(), piece
        for k in ("tone", "candidate", "power", "power_db", "share", "run"):
            assert got_rec[k].tobytes() == rec[k].tobytes(), (piece, k)
        assert sum(int(r["changes"][0]) for r in recs) == 1 and sum(int(r["tone_blocks"][0]) for r in recs) == 4


def test_two_equal_frequencies_tie_and_the_first_wins():
    cfg = dict(OK, freq_hz=(1750.0, 1000.0, 1000.0), dominance_db=0.0, confirm_blocks=1, max_in=256)
    d = tc.formula_design(**cfg)
    powers, rec, nb = tc.model(1, d, **cfg).call(tc.tone(256, 1000.0, 8000.0, 0.7)[None, :])
    assert nb == 2 and np.all(powers[0, :, 1] == powers[0, :, 2]) and np.all(powers[0, :, 1] > powers[0, :, 0])
    assert rec["tone"][0] == 1 and rec["candidate"][0] == 1
    # with any dominance over 0 dB the twin denies the candidate: P2 = P_k*
    cfg = dict(cfg, dominance_db=0.1)
    _, rec, _ = tc.model(1, tc.formula_design(**cfg), **cfg).call(tc.tone(256, 1000.0, 8000.0, 0.7)[None, :])
    assert rec["tone"][0] == -1 and rec["candidate"][0] == -1 and rec["power"][0] > 0.4


LATCH_TABLE = [
    # confirm, release, the blocks' candidates, the tone after each block
    (1, 0, [0, 0, -1, 1, 1, -1, -1], [0, 0, -1, 1, 1, -1, -1]),
    (1, 2, [0, -1, -1, 0, -1, -1, -1, 0], [0, 0, 0, 0, 0, 0, -1, 0]),
    (3, 0, [0, 0, 0, 0, -1, 0, 0, 0], [-1, -1, 0, 0, -1, -1, -1, 0]),
    (3, 2, [0, 0, 1, 1, 1, -1, 0, -1, -1, -1], [-1, -1, -1, -1, 1, 1, 1, -1, -1, -1]),  # the candidate changes mid-run
    (3, 2, [0, 0, 0, 1, 1, 0, 1, 1, 1], [-1, -1, 0, 0, 0, 0, 0, 0, 1]),  # another tone is a miss until it is confirmed
    (2, 1, [1, 1, 0, 1, 0, 0], [-1, 1, 1, 1, 1, 0]),
]


@pytest.mark.parametrize("confirm, release, cands, tones", LATCH_TABLE)
def test_the_latch_table(confirm, release, cands, tones):
    st, got = (-1, -1, 0, 0), []
    for c in cands:
        st = tc.latch_step(st, c, confirm, release)
        got.append(st[0])
    assert got == tones


def test_the_latch_through_the_stage():
    """The fourth row of the table as signals: tone 0, tone 1 and silence by the block."""
    cfg = dict(OK, sub_blocks=1, confirm_blocks=3, release_blocks=2, max_in=640)
    d = tc.formula_design(**cfg)
    cands = LATCH_TABLE[3][2]
    x = np.concatenate([tc.tone(64, cfg["freq_hz"][c], 8000.0, 0.5) if c >= 0 else np.zeros(64, np.float32) for c in cands])
    m = tc.model(1, d, **cfg)
    got = []
    for b in range(len(cands)):
        _, rec, nb = m.call(x[None, 64 * b:64 * b + 64])
        assert nb == 1 and rec["candidate"][0] == cands[b]
        got.append(int(rec["tone"][0]))
    assert got == LATCH_TABLE[3][3]
    _, rec, _ = tc.model(1, d, **cfg).call(x[None, :])
    assert (rec["tone"][0], rec["tone_blocks"][0], rec["changes"][0]) == (-1, 3, 2)


# ---- the signal cases -----------------------------------------------------------------------------------------------

CTCSS_CFG = dict(rate_hz=FA_CTCSS, components=1, freq_hz=tc.CTCSS, sub_blocks=128, window=tc.HANN, min_db=-30.0,
                 dominance_db=10.0, share=0.05, confirm_blocks=2, release_blocks=1, max_in=8192)


def db10(a, b):
    return 10.0 * np.log10(float(a) / float(b))


def test_a_ctcss_tone_in_noise_latches_after_the_second_block_and_noise_alone_never():
    d = tc.formula_design(**CTCSS_CFG)
    S_, k100 = 8192, tc.CTCSS.index(100.0)
    x = tc.tone(10 * S_, 100.0, FA_CTCSS, 0.15)[None, :] + tc.uniform_noise(1, 10 * S_, 21, 0.3)
    m = tc.model(1, d, **CTCSS_CFG)
    for b in range(10):
        powers, rec, nb = m.call(x[:, S_ * b:S_ * (b + 1)])
        P = powers[0, 0]
        others = np.delete(P, [k100 - 1, k100, k100 + 1]).max()
        print("block", b, "P100", P[k100], "share", rec["share"][0], "neighbours dB", db10(P[k100 - 1], P[k100]),
              db10(P[k100 + 1], P[k100]), "others dB", db10(others, P[k100]), "tone", rec["tone"][0])
        assert nb == 1 and rec["candidate"][0] == k100
        # The noise in a tone's bin is 4 sd^2 W2 / W1^2 = 6.6e-5 on average, 25.3 dB under A^2 = 0.0225, and
        # exponentially distributed; it moves the tone's own reading by 0.054 A rms in amplitude, under a third in power
        # at five sigma (and 0.5 dB at the 1.1 sigma allowed for below).
        assert abs(float(P[k100]) - 0.0225) < 0.0225 / 3
        assert 0.07 < rec["share"][0] < 0.16
        # The 47 tones outside the main lobe read noise alone: the largest of 10 x 47 readings passes 12 times the mean
        # (10.8 dB over it) with a chance of 470 e^-12 = 0.3 %, so with the 0.5 dB it stays 14 dB under the tone.
        assert db10(others, P[k100]) < -14
        # The two neighbours add the tone's leakage to their noise, in amplitude: 0.062 A at 97.4 Hz (1.75 bins off, 24.1
        # dB down) and 0.027 A at 103.5 Hz; the noise of one of 20 readings passes 7.6 times the mean, 0.15 A, with a
        # chance of 1 %, so a neighbour stays under 0.21 A, 13.5 dB down, 13 with the 0.5 dB.
        assert db10(P[k100 - 1], P[k100]) < -13 and db10(P[k100 + 1], P[k100]) < -13
        assert rec["tone"][0] == (k100 if b >= 1 else -1)
    m = tc.model(1, d, **CTCSS_CFG)
    noise = tc.uniform_noise(1, 20 * S_, 22, 0.3)
    for b in range(20):
        _, rec, _ = m.call(noise[:, S_ * b:S_ * (b + 1)])
        print("noise block", b, "power", rec["power"][0], "share", rec["share"][0])
        assert rec["candidate"][0] == -1 and rec["tone"][0] == -1 and rec["run"][0] == 0


def test_a_keyed_tone_is_followed_block_by_block():
    cfg = dict(rate_hz=8000.0, components=1, freq_hz=(700.0,), sub_blocks=2, window=tc.RECT, min_db=-20.0,
               dominance_db=0.0, share=0.5, confirm_blocks=1, release_blocks=0, max_in=128 * 18)
    d = tc.formula_design(**cfg)
    blocks = 18
    on = (np.arange(blocks) // 3) % 2 == 0
    x = tc.tone(128 * blocks, 700.0, 8000.0, 0.5) * np.repeat(on, 128) + tc.uniform_noise(1, 128 * blocks, 4, 0.003)[0]
    m = tc.model(1, d, **cfg)
    for b in range(blocks):
        _, rec, nb = m.call(x[None, 128 * b:128 * b + 128].astype(np.float32))
        print("block", b, "on", bool(on[b]), "power", rec["power"][0], "share", rec["share"][0], "tone", rec["tone"][0])
        assert nb == 1 and rec["tone"][0] == (0 if on[b] else -1)
    _, rec, nb = tc.model(1, d, **cfg).call(x[None, :].astype(np.float32))
    edges = 1 + int(np.count_nonzero(on[1:] != on[:-1]))
    print("changes", rec["changes"][0], "edges", edges)
    assert nb == blocks and rec["changes"][0] == edges == 6 and rec["tone_blocks"][0] == int(on.sum())


@pytest.mark.parametrize("sign, want", [(+1, 0), (-1, 1)])
def test_the_sign_of_a_complex_tone(sign, want):
    cfg = dict(rate_hz=8000.0, components=2, freq_hz=(425.0, -425.0), sub_blocks=16, window=tc.HANN, min_db=-20.0,
               dominance_db=20.0, share=0.5, confirm_blocks=1, release_blocks=0, max_in=2048)
    d = tc.formula_design(**cfg)
    z = tc.tone(2048, sign * 425.0, 8000.0, 0.5, complex_=True)[None, :]
    powers, rec, nb = tc.model(1, d, **cfg).call(z)
    for b in range(nb):
        down = db10(powers[0, b, 1 - want], powers[0, b, want])
        print("block", b, "P", powers[0, b], "other tone dB", down)
        assert down <= -60.0
        assert abs(float(powers[0, b, want]) - 0.25) < 0.01
    assert nb == 2 and rec["tone"][0] == want and abs(float(rec["share"][0]) - 1.0) < 0.01
