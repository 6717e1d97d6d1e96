"""CPU tests of the AFC stage: its NumPy restatement (tests/afc_cases.py) on hand-worked blocks, its continuity over
calls of any length, the restatement against the same law in float64 within a derived bound, its behaviour on carriers,
FM and noise (the figures of the stage's design note, each with its margin), the host-side design and its refusals, and
the boundary (the header declares the entry points, the library and sdrg.EXPORTS carry them).  No device is touched."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import afc_cases as af

f32 = np.float32
NEW_SYMBOLS = ("sdrg_afc_design", "sdrg_afc_geometry", "sdrg_afc_offset_hz", "sdrg_engine_set_afc", "sdrg_engine_get_afc",
               "sdrg_engine_afc_reset", "sdrg_engine_afc_device", "sdrg_engine_afc_host", "sdrg_engine_listen_afc_host")
RATE = 48000.0
OK = dict(channel_rate=RATE, max_offset_hz=5000.0, tau_blocks=16.0, floor_db=-60.0, lock_threshold=0.25, mode=af.TRACK,
          block=256, max_in=4096)
BLOCKS, SKIP, SB = 400, 200, 256  # the behaviour cases: 400 blocks of 256, the first 200 discarded


@pytest.fixture(scope="module")
def S():
    import sdrg
    return sdrg


@pytest.fixture(scope="module")
def tab(S):
    return S.nco_tables()


def test_header_library_and_mirror_carry_the_stage(S):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sdrg.h")).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", S.lib_path()], capture_output=True, text=True, check=True).stdout
    L = S.load()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert re.search(r"\bT %s$" % s, nm, flags=re.M), s
        assert s in S.EXPORTS and hasattr(L, s)
    for s in ("sdrg_afc_config", "sdrg_afc_record", "sdrg_afc_design_values", "#define SDRG_AFC_TRACK 1",
              "#define SDRG_AFC_MEASURE 2", "#define SDRG_AFC_MIN_BLOCK 16", "#define SDRG_AFC_MAX_BLOCK 1024"):
        assert s in text
    assert ctypes.sizeof(S.AfcConfig) == 56 and ctypes.sizeof(S.AfcDesign) == 28
    assert S.AfcRecord == af.RECORD and S.AfcRecord.itemsize == 32
    assert (S.AFC_TRACK, S.AFC_MEASURE, S.AFC_LOCKED, S.AFC_SEEDED) == (af.TRACK, af.MEASURE, af.LOCKED, af.SEEDED)
    assert tuple(k for k, _ in S.AfcDesign._fields_) == af.DESIGN
    for block in (16, 32, 64, 128, 256, 512, 1024):
        assert S.afc_geometry(block) == max(512, block)
    t = ctypes.c_int32()
    for bad in (0, 8, 48, 2048, -64):
        assert L.sdrg_afc_geometry(bad, ctypes.byref(t)) == -1
    assert L.sdrg_afc_geometry(64, None) == -1


def test_design_agrees_with_the_formulas(S):
    for cfg in (OK, dict(OK, tau_blocks=0.0), dict(OK, tau_blocks=0.25, floor_db=30.0, lock_threshold=1.0),
                dict(OK, channel_rate=2_000_000.0 / 41, max_offset_hz=1.0, lock_threshold=0.0),
                dict(OK, tau_blocks=1e6, floor_db=-120.0), dict(OK, floor_db=-440.0)):  # a denormal floor
        got = S.afc_design(**cfg)
        want = af.design_formula(cfg["channel_rate"], cfg["max_offset_hz"], cfg["tau_blocks"], cfg["floor_db"],
                                 cfg["lock_threshold"])
        assert tuple(got) == af.DESIGN
        for name, w in zip(af.DESIGN, want):
            assert got[name].dtype == np.float32
            assert abs(float(got[name]) - w) <= float(np.spacing(f32(abs(w)))), (cfg, name, got[name], w)
        assert af.valid_config(cfg)
    assert S.afc_design(**dict(OK, tau_blocks=0.0))["beta"].tobytes() == f32(1.0).tobytes()
    assert S.afc_design(**dict(OK, floor_db=0.0))["floor_thr"] == f32(1.0)
    assert S.afc_design(**dict(OK, max_offset_hz=RATE / 4))["max_s"] == f32(2.0 ** 30)  # the most: inc fits an int32
    assert S.afc_design(**OK)["lock_thr"] == f32(0.25)


def test_offset_hz_is_the_increment_in_double(S):
    assert S.afc_offset_hz(1 << 30, RATE) == RATE / 4 and S.afc_offset_hz(-(1 << 30), RATE) == -RATE / 4
    assert S.afc_offset_hz(0, RATE) == 0.0
    assert S.afc_offset_hz(110458576, RATE) == 110458576 * RATE / 2.0 ** 32
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert math.isnan(S.afc_offset_hz(5, bad))


@pytest.mark.parametrize("bad", [
    dict(channel_rate=0.0), dict(channel_rate=-48000.0), dict(channel_rate=float("inf")), dict(channel_rate=float("nan")),
    dict(max_offset_hz=0.0), dict(max_offset_hz=-1.0), dict(max_offset_hz=12000.5), dict(max_offset_hz=float("nan")),
    dict(max_offset_hz=float("inf")), dict(tau_blocks=-1.0), dict(tau_blocks=float("inf")), dict(tau_blocks=float("nan")),
    dict(floor_db=float("nan")), dict(floor_db=float("-inf")), dict(floor_db=float("inf")), dict(floor_db=400.0),
    dict(floor_db=-500.0), dict(lock_threshold=-0.01), dict(lock_threshold=1.01), dict(lock_threshold=float("nan")),
    dict(mode=0), dict(mode=3), dict(mode=4), dict(mode=-1), dict(block=8), dict(block=48), dict(block=2048),
    dict(block=0), dict(max_in=0), dict(max_in=(1 << 20) + 1)], ids=lambda d: "%s=%s" % next(iter(d.items())))
def test_each_bad_field_is_refused_on_its_own(S, bad):
    S.afc_design(**OK)
    assert af.valid_config(OK) and not af.valid_config(dict(OK, **bad))
    with pytest.raises(S.SdrgError) as ei:
        S.afc_design(**dict(OK, **bad))
    assert "SDRG_E_INVALID" in str(ei.value)


def test_the_limits_themselves_are_accepted(S):
    for edge in (dict(block=1024), dict(block=16), dict(mode=af.MEASURE), dict(max_in=1), dict(max_in=1 << 20),
                 dict(floor_db=380.0), dict(tau_blocks=1e300), dict(max_offset_hz=RATE / 4), dict(lock_threshold=0.0),
                 dict(lock_threshold=1.0), dict(max_offset_hz=1e-300)):
        S.afc_design(**dict(OK, **edge))
        assert af.valid_config(dict(OK, **edge))


# ---- hand-worked blocks: S = 16, beta 1


def quarter_turns(n, amp=1.0):
    """z[i] = amp j^i: a carrier at a quarter of the rate, every sample exact."""
    return (amp * np.array([1, 1j, -1, -1j] * (n // 4))).astype(np.complex64)


def test_a_quarter_rate_carrier_by_hand(S, tab):
    """z[i] = j^i: z[i] conj(z[i - 1]) = j for the 15 products of a block of 16, so Rr = 0, Ri = 15 / 16 and W = 1: the
    seam costs one product in S.  coh = 15 / 16, phi = pi / 2, s = phi K rounds to 2^30 (the clamp at a quarter of the
    rate), and from block 1 on every sample is turned back by a quarter turn more than the one before it."""
    d = S.afc_design(**dict(OK, tau_blocks=0.0, max_offset_hz=RATE / 4, block=16))
    z = quarter_turns(64)[None, :]
    pr, pi, q = af.products(z.real.reshape(1, 4, 16).copy(), z.imag.reshape(1, 4, 16).copy())
    assert np.array_equal(pr, np.zeros_like(pr)) and np.all(pi[..., 0] == 0) and np.all(pi[..., 1:] == 1) and np.all(q == 1)
    out, rec, nb, q = af.one_call(z, d, 16, tab)
    r = rec[0]
    assert nb == 4 and r["inc"] == 1 << 30 and r["flags"] == af.LOCKED | af.SEEDED and r["held_blocks"] == 0
    assert r["coherence"] == f32(15 / 16) and r["level"] == f32(1.0) and r["level_db"] == f32(0.0)
    assert r["offset_hz"] == f32(RATE / 4) and abs(r["step"] - np.pi / 2) < 1e-7
    assert np.array_equal(out[0, :16], z[0, :16])  # block 0 is mixed by inc_-1 = 0: hi[0] lo[0] = 1
    assert np.abs(out[0, 16:] - 1.0).max() < 1e-6  # Phi_1 = 0, then a quarter turn a sample: the carrier stands still
    assert np.array_equal(q.traced("inc")[:, 0], np.full(4, 1 << 30))


def test_the_sums_are_pair_trees_not_running_sums(S, tab):
    """Powers 1, then 2^-24 fifteen times: a running sum loses every one of them, the tree only the one paired with
    the 1."""
    z = np.full(16, 2.0 ** -12, np.float32).astype(np.complex64)
    z[0] = 1.0
    d = S.afc_design(**dict(OK, tau_blocks=0.0, block=16))
    _, rec, _, _ = af.one_call(z[None, :], d, 16, tab)
    assert rec["level"][0] == f32(1.0 + 14 * 2.0 ** -24) * f32(1 / 16) and rec["level"][0] != f32(1 / 16)


def test_products_are_rounded_before_they_are_added(S, tab):
    """zr = 1 + 2^-12, zi = 2^-12: zr zr rounds to 1 + 2^-11, and adding zi zi = 2^-24 rounds back to it; fused into one
    rounding the power would be 1 + 2^-11 + 2^-23."""
    zr, zi = 1.0 + 2.0 ** -12, 2.0 ** -12
    z = np.full((1, 16), zr + 1j * zi, np.complex64)
    d = S.afc_design(**dict(OK, tau_blocks=0.0, block=16))
    _, rec, _, _ = af.one_call(z, d, 16, tab)
    fused = f32(zr * zr + zi * zi)
    assert fused == f32(1.0 + 2.0 ** -11 + 2.0 ** -23)
    assert rec["level"][0] == f32(1.0 + 2.0 ** -11) and rec["level"][0] != fused


def test_any_cut_of_a_stream_equals_one_call(S, tab):
    B, n, Sb = 3, 1000, 64
    rng = np.random.default_rng(11)
    z = np.stack([af.carrier(n, 700.0 * (b + 1), RATE, 0.5, 15.0, rng) for b in range(B)])
    for mode in (af.TRACK, af.MEASURE):
        d = S.afc_design(**dict(OK, tau_blocks=3.0, block=Sb, mode=mode))
        whole, rec, nb, _ = af.one_call(z, d, Sb, tab, mode)
        assert nb == n // Sb and np.all(rec["flags"] == 3) and (whole is None) == (mode == af.MEASURE)
        for cuts in ([1], [0, 0, 1, 2], [63, 64, 65], [64, 128, 128, 129], [999], [n], [500], list(range(7, n, 37)),
                     [31, 32, 33, 640, 641]):
            out, r, blocks, held = af.in_calls(z, cuts, d, Sb, tab, mode)
            if mode == af.TRACK:
                assert out.tobytes() == whole.tobytes(), cuts
            assert blocks == nb and np.array_equal(held, rec["held_blocks"])
            for k in ("offset_hz", "step", "inc", "coherence", "level", "level_db", "flags"):
                assert r[k].tobytes() == rec[k].tobytes(), (cuts, k)


def test_the_restatement_against_float64(S, tab):
    """A clean carrier, far from every decision (the floor, the lock threshold, the clamp): block by block the increment
    within error_bound's first figure of the float64 law's, and every output sample within its second."""
    Sb, n, amp, hz = 256, 64 * 256, 0.5, 1234.5
    cfg = dict(OK, block=Sb)
    d = S.afc_design(**cfg)
    z = af.carrier(n, hz, RATE, amp, 40.0, np.random.default_rng(3))
    out, rec, nb, q = af.one_call(z, d, Sb, tab)
    y64, inc64, coh64 = af.model64(z, d, Sb)
    assert coh64.min() > 0.9 and np.abs(inc64).max() < 0.5 * float(d["max_s"])
    d_inc, d_y = af.error_bound(Sb, float(d["beta"]), coh64.min(), np.abs(inc64).max(), n, np.abs(z).max())
    inc32 = q.traced("inc")[:, 0].astype(np.float64)
    print("inc: %.1f apart at most (bound %.1f); out: %.3g apart at most (bound %.3g)"
          % (np.abs(inc32 - inc64).max(), d_inc, np.abs(out[0] - y64).max(), d_y))
    assert nb == 64 and np.abs(inc32 - inc64).max() <= d_inc
    assert np.abs(out[0] - y64).max() <= d_y
    assert abs(q.traced("coh")[-1, 0] - coh64[-1]) < 1e-5


# ---- behaviour: S = 256, 48 kHz, tau 16 blocks, floor -60 dB, lock 0.25, clamp 5 kHz, 400 blocks, default_rng(1)


def behaviour(S, tab, z):
    d = S.afc_design(**OK)
    out, rec, nb, q = af.one_call(z, d, SB, tab)
    assert nb == BLOCKS
    hz = q.traced("inc")[SKIP:, 0].astype(np.float32) * d["hz_per_inc"]
    return out[0], rec[0], q, hz


def test_a_carrier_at_40_db_is_found_within_half_a_hertz(S, tab):
    z = af.carrier(BLOCKS * SB, 1234.5, RATE, 0.5, 40.0, np.random.default_rng(1))
    _, rec, _, hz = behaviour(S, tab, z)
    print("offset_hz - 1234.5: %+.2f ... %+.2f" % ((hz - 1234.5).min(), (hz - 1234.5).max()))
    assert np.abs(hz - 1234.5).max() <= 0.5 and rec["flags"] == 3


def test_a_carrier_at_20_db_is_found_within_five_hertz_and_removed(S, tab):
    z = af.carrier(BLOCKS * SB, 1234.5, RATE, 0.5, 20.0, np.random.default_rng(1))
    out, _, _, hz = behaviour(S, tab, z)
    resid = af.lag_offset_hz(out[SKIP * SB:], RATE)
    print("offset_hz - 1234.5: %+.2f ... %+.2f; residual %.3f Hz" % ((hz - 1234.5).min(), (hz - 1234.5).max(), resid))
    assert np.abs(hz - 1234.5).max() <= 5.0 and abs(resid) < 1.0
    assert abs(af.lag_offset_hz(z[SKIP * SB:], RATE) - 1234.5) < 1.0  # what went in


def test_fm_is_centred_on_its_carrier(S, tab):
    z = af.fm(BLOCKS * SB, 1500.0, RATE, 1000.0, 3000.0, 0.5, 20.0, np.random.default_rng(1))
    out, _, _, hz = behaviour(S, tab, z)
    step_in, step_out = af.mean_step_hz(z[SKIP * SB:], RATE), af.mean_step_hz(out[SKIP * SB:], RATE)
    print("offset_hz: mean %.2f, %+.1f ... %+.1f around 1500; mean phase step %.1f -> %.2f Hz"
          % (hz.mean(), (hz - 1500).min(), (hz - 1500).max(), step_in, step_out))
    assert abs(hz.mean() - 1500.0) <= 2.0 and np.abs(hz - 1500.0).max() <= 25.0
    assert abs(step_out) < 5.0 and abs(step_in - 1500.0) < 5.0


def test_noise_alone_never_locks_and_passes_in_bytes(S, tab):
    z = af.white(np.random.default_rng(1), BLOCKS * SB, 0.25).astype(np.complex64)
    out, rec, q, _ = behaviour(S, tab, z)
    coh = q.traced("coh")[:, 0]
    print("coherence at most %.3f" % coh.max())
    assert coh.max() < 0.25 and not q.traced("inc").any() and not (q.traced("flags") & af.LOCKED).any()
    assert out.tobytes() == z.tobytes() and rec["flags"] == af.SEEDED and rec["inc"] == 0  # hi[0] lo[0] = 1


def test_a_signal_under_the_floor_holds_every_block(S, tab):
    z = af.fm(BLOCKS * SB, 1500.0, RATE, 1000.0, 3000.0, 0.5, 20.0, np.random.default_rng(1)) * f32(1e-5)
    out, rec, q, _ = behaviour(S, tab, z)
    assert q.traced("held").all() and rec["held_blocks"] == BLOCKS and rec["flags"] == 0 and rec["inc"] == 0
    assert rec["coherence"].tobytes() == rec["level"].tobytes() == bytes(4) and out.tobytes() == z.tobytes()


def test_a_carrier_beyond_the_clamp_gives_the_clamp(S, tab):
    z = af.carrier(BLOCKS * SB, 6000.0, RATE, 0.5, 20.0, np.random.default_rng(1))
    _, rec, q, _ = behaviour(S, tab, z)
    max_s = S.afc_design(**OK)["max_s"]
    assert np.all(q.traced("inc")[SKIP:, 0] == int(np.rint(max_s))) and rec["inc"] == int(np.rint(max_s))
    assert rec["offset_hz"] == f32(np.rint(max_s)) * S.afc_design(**OK)["hz_per_inc"]


def test_a_negative_offset_mirrors_the_estimate(S, tab):
    """The conjugate signal is the carrier at -1234.5 Hz: Ri changes its sign and nothing else, sdrg_atan2f is odd, the
    clamp and the rounding are symmetric: every increment is the other's negative, bit for bit.  The outputs mirror
    each other only as far as the tables do: the phases ph and 2^32 - ph are cut to 20 bits one step apart (2 pi / 2^20
    radians, times a sample of at most 1)."""
    z = af.carrier(BLOCKS * SB, 1234.5, RATE, 0.5, 20.0, np.random.default_rng(1))
    out, rec, q, hz = behaviour(S, tab, z)
    out_m, rec_m, q_m, hz_m = behaviour(S, tab, np.conj(z))
    assert np.array_equal(q_m.traced("inc"), -q.traced("inc")) and rec_m["inc"] == -rec["inc"] < 0
    assert np.abs(hz_m + 1234.5).max() <= 5.0 and np.abs(z).max() <= 1.0
    assert np.abs(out_m - np.conj(out)).max() <= 2 * np.pi / 2.0 ** 20 + 1e-6
    assert rec_m["coherence"] == rec["coherence"] and rec_m["offset_hz"] == -rec["offset_hz"]


def test_the_lock_holds_the_increment_while_it_is_lost(S, tab):
    """A carrier, then noise alone at the same power until the smoothed coherence has fallen under the threshold, then
    the carrier again: inc stays where the last locked block left it while unlocked, and moves again afterwards; a
    block under the floor in between moves nothing at all."""
    Sb, rng = 64, np.random.default_rng(5)
    d = S.afc_design(**dict(OK, tau_blocks=2.0, block=Sb, lock_threshold=0.5))
    parts = [af.carrier(8 * Sb, 2000.0, RATE, 0.5, 30.0, rng), af.white(rng, 24 * Sb, 0.25).astype(np.complex64),
             np.zeros(Sb, np.complex64), af.carrier(8 * Sb, -3000.0, RATE, 0.5, 30.0, rng)]
    _, rec, nb, q = af.one_call(np.concatenate(parts), d, Sb, tab)
    inc, locked, held = q.traced("inc")[:, 0], q.traced("flags")[:, 0] & af.LOCKED, q.traced("held")[:, 0]
    assert nb == 41 and locked[:8].all() and abs(inc[7] * float(d["hz_per_inc"]) - 2000.0) < 20.0
    lost = np.flatnonzero(locked == 0)
    assert lost.size >= 8 and lost[0] >= 8 and lost[-1] < 40
    for k in lost:  # unlocked: the increment of the block before
        assert inc[k] == inc[k - 1]
    assert held.sum() == 1 and held[32] == 1 and inc[32] == inc[31] and q.traced("coh")[32, 0] == q.traced("coh")[31, 0]
    assert locked[-1] and abs(inc[-1] * float(d["hz_per_inc"]) + 3000.0) < 100.0 and rec["held_blocks"][0] == 1
