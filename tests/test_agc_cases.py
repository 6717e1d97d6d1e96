"""CPU tests of the AGC stage: its NumPy restatement (tests/agc_cases.py) on hand-worked streams for each branch of the
gain law, the ramp's weights, both detectors, its continuity over calls of any length, the host-side design and its
refusals, the boundary (the header declares the entry points, the library and sdrg.EXPORTS carry them), and the settled
level of two AM channels 30 dB apart against agc_cases.error_bound.  No device is touched."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import agc_cases as ag
import squelch_cases as sq

f32 = np.float32
NEW_SYMBOLS = ("sdrg_agc_design", "sdrg_agc_geometry", "sdrg_engine_set_agc", "sdrg_engine_get_agc",
               "sdrg_engine_agc_reset", "sdrg_engine_agc_device", "sdrg_engine_agc_host", "sdrg_engine_listen_host")
OK = dict(target=0.25, max_gain_db=60.0, initial_gain_db=0.0, floor_db=-math.inf, attack_blocks=0.0, decay_blocks=0.0,
          detector=ag.MEAN, block=16, hang_blocks=2, max_in=4096)
S16 = 16


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
    for s in ("sdrg_agc_config", "sdrg_agc_record", "#define SDRG_AGC_MIN_BLOCK 16", "#define SDRG_AGC_MAX_BLOCK 1024",
              "#define SDRG_AGC_MAX_HANG 65535", "#define SDRG_AGC_DET_MEAN 0", "#define SDRG_AGC_DET_PEAK 1",
              "#define SDRG_LISTEN_SQUELCH 1", "#define SDRG_LISTEN_AGC 2", "#define SDRG_LISTEN_RESAMPLE 4"):
        assert s in text
    assert ctypes.sizeof(S.AgcConfig) == 64
    assert S.AGC_RECORD_DTYPE == ag.RECORD and S.AGC_RECORD_DTYPE.itemsize == 16
    assert (S.LISTEN_SQUELCH, S.LISTEN_AGC, S.LISTEN_RESAMPLE) == (1, 2, 4)
    assert (S.AGC_DET_MEAN, S.AGC_DET_PEAK) == (ag.MEAN, ag.PEAK) and S.AGC_DESIGN_FIELDS == ag.DESIGN
    for block in (16, 32, 64, 128, 256, 512, 1024):
        assert S.agc_geometry(block) == max(512, block)
    t = ctypes.c_int32()
    for bad in (0, 8, 24, 2048, -16):
        assert L.sdrg_agc_geometry(bad, ctypes.byref(t)) == -1
    assert L.sdrg_agc_geometry(64, None) == -1


def test_design_agrees_with_the_formulas(S):
    for cfg in (OK, dict(OK, max_gain_db=0.0), dict(OK, max_gain_db=37.5, initial_gain_db=-20.0, floor_db=-60.0),
                dict(OK, attack_blocks=0.5, decay_blocks=25.0), dict(OK, attack_blocks=1e6, decay_blocks=1e-3),
                dict(OK, floor_db=-440.0), dict(OK, initial_gain_db=-600.0, max_gain_db=-590.0),  # denormal, positive
                dict(OK, target=1e-30, floor_db=30.0)):
        got = S.agc_design(**cfg)
        want = ag.design_formula(cfg["max_gain_db"], cfg["initial_gain_db"], cfg["floor_db"], cfg["attack_blocks"],
                                 cfg["decay_blocks"])
        for name, w in zip(ag.DESIGN, want):
            assert got[name].dtype == np.float32
            assert abs(float(got[name]) - w) <= float(np.spacing(f32(abs(w)))), (cfg, name, got[name], w)
        assert got["init_gain"] <= got["max_gain"] and ag.valid_config(cfg)
    d = S.agc_design(**OK)
    assert d["init_gain"] == f32(1.0) and d["max_gain"] == f32(1000.0)
    assert d["floor_thr"].tobytes() == f32(0.0).tobytes()  # -inf dB is +0: no block is under the floor
    for name in ("alpha_a", "alpha_d"):
        assert d[name].tobytes() == f32(1.0).tobytes()  # exactly 1 at 0 blocks
    d = S.agc_design(**dict(OK, attack_blocks=1.0, decay_blocks=4.0))
    assert 0 < d["alpha_d"] < d["alpha_a"] < 1
    # any pointer may be NULL
    c, v = S.AgcConfig(**OK), ctypes.c_float()
    assert S.load().sdrg_agc_design(ctypes.byref(c), None, None, None, None, None) == 0
    assert S.load().sdrg_agc_design(ctypes.byref(c), None, None, None, None, ctypes.byref(v)) == 0 and v.value == 1.0
    assert S.load().sdrg_agc_design(None, None, None, None, None, None) == -1


@pytest.mark.parametrize("bad", [
    dict(target=0.0), dict(target=-1.0), dict(target=float("nan")), dict(target=float("inf")), dict(target=1e39),
    dict(target=1e-60), dict(max_gain_db=float("nan")), dict(max_gain_db=float("inf")), dict(max_gain_db=800.0),
    dict(max_gain_db=-1.0), dict(initial_gain_db=60.5), dict(initial_gain_db=-1000.0),
    dict(initial_gain_db=float("-inf")), dict(floor_db=float("nan")), dict(floor_db=float("inf")), dict(floor_db=400.0),
    dict(attack_blocks=-1.0), dict(attack_blocks=float("inf")), dict(attack_blocks=float("nan")),
    dict(decay_blocks=-0.5), dict(decay_blocks=float("inf")), dict(decay_blocks=float("nan")), dict(detector=2),
    dict(detector=-1), dict(block=48), dict(block=8), dict(block=2048), dict(block=0), dict(hang_blocks=-1),
    dict(hang_blocks=65536), dict(max_in=0), dict(max_in=(1 << 20) + 1)], ids=lambda d: "%s=%s" % next(iter(d.items())))
def test_each_bad_field_is_refused_on_its_own(S, bad):
    S.agc_design(**OK)
    assert ag.valid_config(OK) and not ag.valid_config(dict(OK, **bad))
    with pytest.raises(S.SdrgError) as ei:
        S.agc_design(**dict(OK, **bad))
    assert "SDRG_E_INVALID" in str(ei.value)


def test_the_limits_themselves_are_accepted(S):
    for edge in (dict(block=1024), dict(hang_blocks=65535), dict(hang_blocks=0), dict(max_in=1), dict(max_in=1 << 20),
                 dict(initial_gain_db=60.0), dict(max_gain_db=0.0), dict(floor_db=-1000.0), dict(floor_db=380.0),
                 dict(attack_blocks=1e300), dict(detector=ag.PEAK), dict(target=1e-44)):
        S.agc_design(**dict(OK, **edge))
        assert ag.valid_config(dict(OK, **edge))


# ---- hand-worked streams: S = 16, target 0.25; a block of amplitude a (a power of two) has P = a a and want = 0.25 / a


def blocks_of(amps):
    """One stream whose block j is S16 samples of (amps[j], 0): its mean and its peak power are amps[j]^2, exactly for
    powers of two."""
    return np.repeat(np.asarray(amps, np.float32), S16).astype(np.complex64)[None, :]


def design(S, **over):
    return S.agc_design(**dict(OK, **over))


def run(S, amps, H=0, detector=ag.MEAN, **over):
    """(the model after one call of blocks_of(amps), out [n], records, n_blocks)."""
    m = ag.Agc(1, OK["target"], design(S, **over), S16, H, detector)
    out, rec, nb = m.call(blocks_of(amps))
    return m, out[0], rec, nb


def gains_of(m):
    return [float(g[0]) for g in m.gains]


@pytest.mark.parametrize("H", [0, 1, 2, 5])
def test_attack_then_the_hang_held_exactly_h_blocks_then_decay(S, H):
    # 1.0 wants 0.25 (an attack from 1); 0.25 wants 1.0: H blocks hold 0.25, the next decays to 1.0 at alpha_d = 1
    m, out, rec, nb = run(S, [1.0] + [0.25] * (H + 2), H)
    assert gains_of(m) == [0.25] + [0.25] * H + [1.0, 1.0]
    assert nb == H + 3 and rec["attacks"][0] == 1 and rec["gain"][0] == f32(1.0) and rec["gain_db"][0] == 0.0
    assert abs(rec["level_db"][0] - 10 * math.log10(0.0625)) < 1e-5 and m.hang[0] == 0


def test_an_attack_reloads_the_hang_and_an_equal_level_does_not(S):
    # want == G is no attack: the hang counts down through blocks that want what they have
    m, _, rec, _ = run(S, [1.0, 1.0, 1.0, 0.5, 1.0, 0.5, 0.5, 0.5], H=2)
    #            attack  h2->1  h1->0 decay  attack h2->1 h1->0 decay
    assert gains_of(m) == [0.25, 0.25, 0.25, 0.5, 0.25, 0.25, 0.25, 0.5] and rec["attacks"][0] == 2


def test_attack_and_decay_are_smoothed_operation_by_operation(S):
    d = design(S, attack_blocks=1.0, decay_blocks=3.0)
    aa, ad = d["alpha_a"], d["alpha_d"]
    amps = [2.0, 2.0, 0.125, 0.125, 0.125, 4.0]
    m, _, rec, _ = run(S, amps, H=1, attack_blocks=1.0, decay_blocks=3.0)
    G, hang, want_gains, attacks = f32(1.0), 0, [], 0
    for a in amps:
        want = f32(f32(0.25) / f32(a))
        dd = f32(want - G)
        if want < G:
            G, hang, attacks = f32(G + f32(aa * dd)), 1, attacks + 1
        elif hang > 0:
            hang -= 1
        else:
            G = f32(G + f32(ad * dd))
        want_gains.append(float(G))
    assert gains_of(m) == want_gains and rec["attacks"][0] == attacks == 3 and rec["gain"][0] == f32(want_gains[-1])
    assert abs(rec["gain_db"][0] - 20 * math.log10(want_gains[-1])) < 1e-5


def test_a_block_under_the_floor_changes_nothing(S):
    # floor 10^-3.3 = 5.0e-4: the blocks of amplitude 2^-6 (P = 2.4e-4) and 0 are held, 2^-5 (P = 9.8e-4) is not
    over = dict(floor_db=-33.0)
    m, _, rec, _ = run(S, [1.0, 2.0 ** -6, 0.0, 2.0 ** -6, 2.0 ** -5, 2.0 ** -5], H=1, **over)
    assert gains_of(m) == [0.25, 0.25, 0.25, 0.25, 0.25, 8.0]  # the held blocks leave the hang at 1 for block 4
    assert rec["attacks"][0] == 1
    # P_last is the last block's statistic whether or not it was held
    m, _, rec, _ = run(S, [1.0, 0.0], H=0, **over)
    assert gains_of(m) == [0.25, 0.25] and abs(rec["level_db"][0] + 200.0) < 1e-3 and m.Gp[0] == f32(0.25)
    # without a floor the same zeros run the gain up to max_gain
    m, _, _, _ = run(S, [1.0, 0.0], H=0)
    assert gains_of(m) == [0.25, 1000.0]


def test_a_zero_block_and_a_faint_one_give_max_gain(S):
    m, _, rec, _ = run(S, [0.0], max_gain_db=20.0)
    assert gains_of(m) == [10.0] and rec["gain"][0] == f32(10.0) and abs(rec["gain_db"][0] - 20.0) < 2e-6
    m, _, _, _ = run(S, [2.0 ** -10, 2.0 ** -4], max_gain_db=20.0)  # wants 256 and 4
    assert gains_of(m) == [10.0, 4.0]


def test_every_ramp_weight_of_one_block_and_blocks_0_and_1(S):
    z = np.repeat(np.array([1, 3 - 5j, -3 + 5j, 2j], np.complex64), S16)[None, :]  # powers 1, 34, 34, 4
    d = design(S, initial_gain_db=6.0)
    m = ag.Agc(1, 0.25, d, S16, 0)
    out, rec, nb = m.call(z)
    g = [d["init_gain"], d["init_gain"]] + [x[0] for x in m.gains]  # gain[-2], gain[-1], gain[0] ..
    assert g[2] == f32(0.25) and g[3] == f32(f32(0.25) / np.sqrt(f32(34.0)))
    r = f32(1.0) / f32(S16)
    for b in range(4):
        g0, g1 = g[b], g[b + 1]
        for i in range(S16):
            t = f32(f32(i + 1) * r)
            w = f32(g0 + f32(f32(g1 - g0) * t))
            zin, o = z[0, b * S16 + i], out[0, b * S16 + i]
            assert o.real.tobytes() == f32(zin.real * w).tobytes() and o.imag.tobytes() == f32(zin.imag * w).tobytes()
    # block 0 runs at init_gain (no decision yet: g0 = g1, so d = 0 and w = g0 whatever t is); block 1 ramps from
    # init_gain to gain[0], block 0's decision, from its first sample on, and block 2 goes on from where block 1 ended
    init = d["init_gain"]
    assert out[0, :S16].tobytes() == (z[0, :S16] * init).astype(np.complex64).tobytes()
    assert abs(out[0, S16]) < abs(np.complex64(z[0, S16] * init))
    end1 = f32(init + f32(f32(0.25) - init))  # t = 1
    assert out[0, 2 * S16 - 1].real == f32(f32(3.0) * end1) and abs(end1 - f32(0.25)) <= np.spacing(init)
    assert nb == 4 and rec["attacks"][0] == 2  # 1 -> 0.25 -> 0.25 / sqrt(34); then 34 again (equal: no attack), then 4


def test_the_mean_is_the_squelchs_tree_not_a_running_sum(S):
    """The squelch test's constructed block: one sample of power 1, then fifteen of power 2^-24."""
    amps = np.full(S16, 2.0 ** -12, np.float32)
    amps[0] = 1.0
    p = sq.powers(amps.astype(np.complex64))
    tree = sq.tree_sum(p)
    assert sq.running_sum(p) == f32(1.0) and tree == f32(1.0 + 14 * 2.0 ** -24)
    d = design(S)
    m = ag.Agc(1, 0.25, d, S16, 0)
    _, rec, nb = m.call(amps.astype(np.complex64)[None, :])
    P = f32(tree * f32(1.0 / 16))
    assert nb == 1 and m.Pl[0] == P and P != f32(1.0 / 16)
    assert m.G[0] == f32(f32(0.25) / np.sqrt(P)) and m.G[0] != f32(f32(0.25) / np.sqrt(f32(1.0 / 16)))


def test_the_peak_detector(S):
    z = np.full((1, 2 * S16), 0.125 + 0j, np.complex64)
    z[0, 5] = 0.5j  # one sample of power 0.25 among powers of 2^-6
    z[0, S16 + 15] = -2.0
    m = ag.Agc(1, 0.25, design(S), S16, 0, ag.PEAK)
    _, rec, _ = m.call(z)
    assert gains_of(m) == [0.5, 0.125] and m.Pl[0] == f32(4.0) and rec["attacks"][0] == 2
    mean = ag.Agc(1, 0.25, design(S), S16, 0, ag.MEAN)
    mean.call(z)
    assert gains_of(mean)[0] > 1.0  # the mean of that block is small: the two detectors decide differently
    # the maximum does not depend on where in the block it stands
    for at in range(S16):
        z = np.full((1, S16), 0.125 + 0j, np.complex64)
        z[0, at] = 1.0
        m = ag.Agc(1, 0.25, design(S), S16, 0, ag.PEAK)
        m.call(z)
        assert gains_of(m) == [0.25]


@pytest.mark.parametrize("S_,H,att,dec,det", [(16, 1, 0.0, 0.0, ag.MEAN), (16, 0, 0.7, 2.0, ag.PEAK),
                                              (64, 2, 0.0, 1.5, ag.MEAN)])
def test_any_cut_of_a_stream_gives_the_bytes_of_one_call(S, S_, H, att, dec, det):
    B, n = 3, 11 * S_ + 5
    d = design(S, attack_blocks=att, decay_blocks=dec, floor_db=-30.0)
    z = ag.levels(B, n, 5, S_, (1, 1, 0, 0, 0, 1, 0), quiet=0.02)
    z[:, 4 * S_:5 * S_] = 0  # a block under the floor
    want, want_rec, want_nb = ag.one_call(z, 0.25, d, S_, H, det)
    assert want_rec["attacks"].min() > 0
    rng = np.random.default_rng(17)
    cut_sets = [[], [0], [n], [1], [0, 0, 1, 2, 2], [S_ - 1], [S_], [S_ + 1],
                [3 * S_ + 2, 3 * S_ + 5, 3 * S_ + 9, 3 * S_ + 9],  # three calls, and one without samples, inside one block
                list(range(1, n)),  # every call a single sample
                list(range(S_, n, S_)), sorted(rng.integers(0, n + 1, 9).tolist()),
                sorted(rng.integers(0, n + 1, 40).tolist())]
    for cuts in cut_sets:
        got, rec, nb, attacks = ag.in_calls(z, cuts, 0.25, d, S_, H, det)
        assert got.tobytes() == want.tobytes(), cuts
        assert nb == want_nb == n // S_
        for k in ("gain", "gain_db", "level_db"):
            assert rec[k].tobytes() == want_rec[k].tobytes(), (cuts, k)
        assert attacks.tolist() == want_rec["attacks"].tolist(), cuts  # a call counts its own blocks


def test_a_call_without_samples_reports_and_changes_nothing(S):
    d = design(S, initial_gain_db=-6.0)
    model = ag.Agc(2, 0.25, d, S16, 1)
    out, rec, nb = model.call(np.zeros((2, 0), np.complex64), in_stride=7)
    assert out.shape == (2, 7) and not out.view(np.uint32).any() and nb == 0 and model.g == 0
    assert np.all(rec["gain"] == d["init_gain"]) and np.all(np.abs(rec["level_db"] + 200.0) < 1e-3)
    assert np.all(np.abs(rec["gain_db"] + 6.0) < 1e-5)
    out, rec, nb = model.call(sq.noise(2, 1, 2))  # n = 1
    assert nb == 0 and out.shape == (2, 1) and np.all(rec["gain"] == d["init_gain"])
    _, before, _ = model.call(sq.noise(2, 40, 3))
    _, after, nb = model.call(np.zeros((2, 0), np.complex64))
    assert nb == 0 and model.g == 41 and after["attacks"].tolist() == [0, 0]
    for k in ("gain", "gain_db", "level_db"):
        assert after[k].tobytes() == before[k].tobytes()


# ---- the behavioural case: two AM channels 30 dB apart settle on the target

def test_two_am_channels_30_db_apart_settle_within_the_bound(S):
    z, d, first, bound = ag.am_case(S)
    assert 10 < first < ag.AM["blocks"] - 8 and bound < 1.1e-3 * ag.AM["target"]
    out, rec, nb = ag.one_call(z, ag.AM["target"], d, ag.AM["S"], 0)
    rms_in = ag.block_rms(z, ag.AM["S"])
    assert 29.9 < 20 * np.log10(rms_in[0, -1] / rms_in[1, -1]) < 30.1
    rms = ag.block_rms(out, ag.AM["S"])
    dist = np.abs(rms[:, first:] - ag.AM["target"]).max()
    print("settled from block", first, "distance", dist, "bound", bound)
    assert dist <= bound, (dist, bound)
    assert np.abs(rms[:, 2] - ag.AM["target"]).max() > 100 * bound  # not yet at block 2: the bound says something
    # against the float64 model of the same law: its own distance is the law's (tol), the difference the rounding's
    out64, gains64 = ag.model_f64(z, ag.AM["target"], d, ag.AM["S"], 0)
    rms64 = ag.block_rms(out64, ag.AM["S"])
    assert np.abs(rms64[:, first:] - ag.AM["target"]).max() <= ag.AM["tol"] * ag.AM["target"]
    assert np.abs(rms[:, first:] - rms64[:, first:]).max() <= bound - ag.AM["tol"] * ag.AM["target"]
    assert nb == ag.AM["blocks"] and np.all(np.abs(rec["gain_db"] - 20 * np.log10(gains64[-1])) < 1e-3)
