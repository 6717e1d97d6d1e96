"""CPU tests of the IQ correction stage: its NumPy restatement (tests/iqcorr_cases.py) on hand-worked blocks, its
continuity over calls of any length, the adjacent-pair tree against a running sum, rounded products against fused ones,
the holds, its selectivity on an impaired receiver's signal, the host-side design and its refusals, and the boundary (the
header declares the entry points, the library and sdrg.EXPORTS carry them).  No device is touched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import iqcorr_cases as iq

f32 = np.float32
NEW_SYMBOLS = ("sdrg_iqcorr_design", "sdrg_iqcorr_geometry", "sdrg_engine_set_iqcorr", "sdrg_engine_get_iqcorr",
               "sdrg_engine_iqcorr_reset", "sdrg_engine_iqcorr_device", "sdrg_engine_iqcorr_host",
               "sdrg_engine_iqcorr_process_host")
OK = dict(dc_tau_blocks=0.0, balance_tau_blocks=0.0, floor_db=-60.0, mode=3, block=64, max_in=4096)
S64 = 64


@pytest.fixture(scope="module")
def S():
    import sdrg
    return sdrg


def design(S, **over):
    d = S.iqcorr_design(**dict(OK, **over))
    return d["beta_dc"], d["beta_bal"], d["floor_thr"]


def test_header_library_and_mirror_carry_the_stage(S):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sdrg.h")).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", S.lib_path()], capture_output=True, text=True, check=True).stdout
    L = S.load()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert re.search(r"\bT %s$" % s, nm, flags=re.M), s
        assert s in S.EXPORTS and hasattr(L, s)
    for s in ("sdrg_iqcorr_config", "sdrg_iqcorr_record", "#define SDRG_IQCORR_DC 1", "#define SDRG_IQCORR_BALANCE 2",
              "#define SDRG_IQCORR_MIN_BLOCK 64", "#define SDRG_IQCORR_MAX_BLOCK 1024"):
        assert s in text
    assert ctypes.sizeof(S.IqcorrConfig) == 40
    assert S.IqcorrRecord == iq.RECORD and S.IqcorrRecord.itemsize == 32
    assert (S.IQCORR_DC, S.IQCORR_BALANCE) == (iq.DC, iq.BALANCE)
    assert (S.CF32, S.CS8, S.CU8, S.CS16) == (iq.CF32, iq.CS8, iq.CU8, iq.CS16)
    for block in (64, 128, 256, 512, 1024):
        assert S.iqcorr_geometry(block) == max(512, block)
    t = ctypes.c_int32()
    for bad in (0, 16, 32, 96, 2048, -64):
        assert L.sdrg_iqcorr_geometry(bad, ctypes.byref(t)) == -1
    assert L.sdrg_iqcorr_geometry(64, None) == -1


def test_design_agrees_with_the_formulas(S):
    for cfg in (OK, dict(OK, dc_tau_blocks=16.0, balance_tau_blocks=16.0), dict(OK, dc_tau_blocks=0.25, floor_db=30.0),
                dict(OK, balance_tau_blocks=1e6, floor_db=-120.0), dict(OK, floor_db=-440.0)):  # a denormal floor
        got = S.iqcorr_design(**cfg)
        want = iq.design_formula(cfg["dc_tau_blocks"], cfg["balance_tau_blocks"], cfg["floor_db"])
        for name, w in zip(("beta_dc", "beta_bal", "floor_thr"), want):
            assert got[name].dtype == np.float32
            assert abs(float(got[name]) - w) <= float(np.spacing(f32(abs(w)))), (cfg, name, got[name], w)
        assert iq.valid_config(cfg)
    d = S.iqcorr_design(**OK)
    assert d["beta_dc"].tobytes() == f32(1.0).tobytes() and d["beta_bal"].tobytes() == f32(1.0).tobytes()
    assert S.iqcorr_design(**dict(OK, floor_db=0.0))["floor_thr"] == f32(1.0)
    assert 0 < S.iqcorr_design(**dict(OK, dc_tau_blocks=4.0))["beta_dc"] < 1


@pytest.mark.parametrize("bad", [
    dict(block=48), dict(block=32), dict(block=2048), dict(block=0), dict(mode=0), dict(mode=4), dict(mode=7),
    dict(mode=-1), dict(dc_tau_blocks=-1.0), dict(dc_tau_blocks=float("inf")), dict(dc_tau_blocks=float("nan")),
    dict(balance_tau_blocks=-1.0), dict(balance_tau_blocks=float("inf")), dict(balance_tau_blocks=float("nan")),
    dict(floor_db=float("nan")), dict(floor_db=float("-inf")), dict(floor_db=float("inf")), dict(floor_db=400.0),
    dict(floor_db=-500.0), dict(max_in=0), dict(max_in=(1 << 20) + 1)], ids=lambda d: "%s=%s" % next(iter(d.items())))
def test_each_bad_field_is_refused_on_its_own(S, bad):
    S.iqcorr_design(**OK)
    assert iq.valid_config(OK) and not iq.valid_config(dict(OK, **bad))
    with pytest.raises(S.SdrgError) as ei:
        S.iqcorr_design(**dict(OK, **bad))
    assert "SDRG_E_INVALID" in str(ei.value)


def test_the_limits_themselves_are_accepted(S):
    for edge in (dict(block=1024), dict(block=64), dict(mode=1), dict(mode=2), dict(max_in=1), dict(max_in=1 << 20),
                 dict(floor_db=380.0), dict(dc_tau_blocks=1e300)):
        S.iqcorr_design(**dict(OK, **edge))
        assert iq.valid_config(dict(OK, **edge))


# ---- hand-worked blocks: S = 64, both betas 1, floor 1e-6


def test_a_constant_input_is_an_offset_and_nothing_else(S):
    """(0.5, -0.25) for four blocks: every block's mean is the sample, its centred power 0, so the balance holds; block 0
    passes whole, block 1 ramps the offset in, and from block 2 on the output is (+0, +0)."""
    z = np.full((1, 4 * S64), 0.5 - 0.25j, np.complex64)
    out, rec, nb = iq.one_call(z, iq.CF32, *design(S), 3, S64)
    assert nb == 4
    t = (np.arange(S64) + 1).astype(np.float32) * f32(1.0 / S64)
    assert np.array_equal(out[0, :S64], z[0, :S64])
    assert np.array_equal(out[0, S64:2 * S64].real, f32(0.5) - f32(0.5) * t)
    assert np.array_equal(out[0, S64:2 * S64].imag, f32(-0.25) - f32(-0.25) * t)
    assert out[0, 2 * S64 - 1] == 0 and out[0, 2 * S64:].tobytes() == bytes(8 * 2 * S64)
    r = rec[0]
    assert (r["dc_re"], r["dc_im"], r["held_blocks"], r["seeded"]) == (f32(0.5), f32(-0.25), 4, 0)
    assert r["w_re"].tobytes() == r["w_im"].tobytes() == r["power"].tobytes() == bytes(4)
    assert r["image_db"] == f32(-200.0)


def test_a_gain_error_alone_has_a_closed_form(S):
    """(1.1 cos, sin) = 1.05 e^{j phi} + 0.05 e^{-j phi}: w = K2 / K1 = 1 / 21, and y = (1.05 - 0.05 / 21) e^{j phi}."""
    phi = 2 * np.pi * 4 * np.arange(4 * S64) / S64  # four cycles a block
    x = (1.1 * np.cos(phi) + 1j * np.sin(phi)).astype(np.complex64)[None, :]
    out, rec, nb = iq.one_call(x, iq.CF32, *design(S, mode=2), 2, S64)
    r = rec[0]
    assert nb == 4 and r["held_blocks"] == 0 and r["seeded"] == 1
    assert abs(r["w_re"] - 1 / 21) < 2e-7 and abs(r["w_im"]) < 1e-7
    assert abs(r["power"] - 1.105) < 1e-6 and abs(r["image_db"] - 20 * np.log10(1 / 21)) < 1e-4
    assert r["dc_re"].tobytes() == r["dc_im"].tobytes() == bytes(4)  # BALANCE alone: the offset stays +0
    assert np.array_equal(out[:, :S64], x[:, :S64])  # block 0 passes whole
    want = (1.05 - 0.05 / 21) * np.exp(1j * phi[2 * S64:])
    assert np.abs(out[0, 2 * S64:] - want).max() < 1e-6
    y64, th = iq.model64(x[0], 1.0, 1.0, 1e-6, 2, S64)
    assert np.abs(out[0] - y64).max() < 1e-6 and abs(th[2] - 1 / 21) < 1e-7


def test_the_means_are_pair_trees_not_running_sums(S):
    zr = np.full(S64, 2.0 ** -24, np.float32)
    zr[0] = 1.0
    tree, run = iq.tree_sum(zr), iq.running_sum(zr)
    # the running sum loses every 2^-24; the tree loses only the one paired with the 1
    assert run == f32(1.0) and tree == f32(1.0 + 62 * 2.0 ** -24) and tree != run
    _, rec, _ = iq.one_call(zr.astype(np.complex64)[None, :], iq.CF32, *design(S, mode=1), 1, S64)
    assert rec["dc_re"][0] == tree * f32(1.0 / S64) and rec["dc_re"][0] != run * f32(1.0 / S64)


def test_products_are_rounded_before_they_are_added(S):
    """zr = 1 + 2^-12, zi = 2^-12 with alternating signs (a block of mean 0): zr zr rounds to 1 + 2^-11, and adding
    zi zi = 2^-24 rounds back to it; zr zr + zi zi fused into one rounding is 1 + 2^-11 + 2^-23."""
    zr, zi = 1.0 + 2.0 ** -12, 2.0 ** -12
    sign = np.where(np.arange(S64) % 2 == 0, 1.0, -1.0)
    z = (sign * (zr + 1j * zi)).astype(np.complex64)[None, :]
    assert z[0, 0].real == zr and z[0, 0].imag == zi  # representable
    _, rec, _ = iq.one_call(z, iq.CF32, *design(S, mode=2), 2, S64)
    fused = f32(zr * zr + zi * zi)  # exact in double: one rounding
    assert fused == f32(1.0 + 2.0 ** -11 + 2.0 ** -23)
    assert rec["power"][0] == f32(1.0 + 2.0 ** -11) and rec["power"][0] != fused and rec["seeded"][0] == 1


@pytest.mark.parametrize("fmt", [iq.CS8, iq.CU8, iq.CS16, iq.CF32])
def test_any_cut_of_a_stream_equals_one_call(S, fmt):
    B, n, Sb = 3, 1000, 64
    z = iq.impaired(iq.noise(B, n, 11, 0.3), dc=0.05 - 0.02j)
    raw = iq.to_raw(z, fmt, {iq.CS8: 100.0, iq.CU8: 100.0, iq.CS16: 20000.0, iq.CF32: 1.0}[fmt])
    d = design(S, dc_tau_blocks=3.0, balance_tau_blocks=2.0)
    whole, rec, nb = iq.one_call(raw, fmt, *d, 3, Sb)
    assert nb == n // Sb and rec["seeded"].all()
    for cuts in ([1], [0, 0, 1, 2], [63, 64, 65], [64, 128, 128, 129], [999], [n], [500], list(range(7, n, 37)),
                 [31, 32, 33, 640, 641]):
        out, r, blocks, held = iq.in_calls(raw, fmt, cuts, *d, 3, Sb)
        assert out.tobytes() == whole.tobytes(), cuts
        assert blocks == nb and np.array_equal(held, rec["held_blocks"])
        for k in ("dc_re", "dc_im", "w_re", "w_im", "power", "image_db", "seeded"):
            assert r[k].tobytes() == rec[k].tobytes(), (cuts, k)


def test_dc_only_leaves_the_balance_at_plus_zero(S):
    raw = iq.to_raw(iq.impaired(iq.noise(2, 512, 3, 0.3), dc=-0.1 + 0.2j), iq.CF32)
    out, rec, _ = iq.one_call(raw, iq.CF32, *design(S, dc_tau_blocks=2.0), 1, S64)
    for k in ("w_re", "w_im", "power"):
        assert rec[k].tobytes() == bytes(8), k
    assert not rec["seeded"].any() and not rec["held_blocks"].any() and np.all(rec["image_db"] == f32(-200.0))
    assert np.all(np.abs(rec["dc_re"] + 0.1) < 0.05) and np.all(np.abs(rec["dc_im"] - 0.2) < 0.05)


def test_a_block_under_the_floor_holds_and_so_does_one_too_lopsided(S):
    d = design(S, floor_db=-20.0)  # 0.01
    loud = iq.impaired(iq.noise(1, S64, 5, 0.5))
    quiet = iq.noise(1, S64, 6, 0.01)  # mean power 1e-4
    real = np.cos(2 * np.pi * 5 * np.arange(S64) / S64)[None, :].astype(np.complex64)  # a = p: cr = 1, m = 1
    q = iq.Iqcorr(1, *d, 2, S64)
    _, r0, _ = q.call(quiet)
    assert (r0["held_blocks"][0], r0["seeded"][0]) == (1, 0) and r0["w_re"].tobytes() == bytes(4)
    _, r1, _ = q.call(loud)
    assert (r1["held_blocks"][0], r1["seeded"][0]) == (0, 1) and r1["w_re"][0] != 0
    _, r2, _ = q.call(quiet)  # under the floor: nothing of the balance moves
    assert r2["held_blocks"][0] == 1
    for k in ("w_re", "w_im", "power"):
        assert r2[k].tobytes() == r1[k].tobytes(), k
    _, r3, _ = q.call(real)  # above the floor, m > 0.25: A, B, P move, w stays
    assert r3["held_blocks"][0] == 1 and r3["power"][0] != r1["power"][0]
    assert r3["w_re"].tobytes() == r1["w_re"].tobytes() and r3["w_im"].tobytes() == r1["w_im"].tobytes()


# ---- selectivity: the image and the offset of an impaired receiver, at least 60 dB under the tone


@pytest.fixture(scope="module")
def receivers():
    return {fmt: iq.receiver(fmt) for fmt in iq.SEL_FORMATS}


@pytest.mark.parametrize("Sb", [256, 1024])
@pytest.mark.parametrize("fmt", list(iq.SEL_FORMATS), ids=["cu8", "cs16", "cf32"])
def test_selectivity_of_the_restatement(S, receivers, fmt, Sb):
    raw = receivers[fmt]
    zr, zi = iq.sample(raw, fmt)
    image_in, dc_in = iq.levels_db(zr[0] + 1j * zi[0])
    assert image_in < 30 and dc_in < 31  # what the receiver delivers
    d = design(S, dc_tau_blocks=16.0, balance_tau_blocks=16.0, block=Sb)
    out, rec, nb = iq.one_call(raw, fmt, *d, 3, Sb)
    image, dc = iq.levels_db(out[0])
    print("fmt %d S %d: image %.1f dB and DC %.1f dB under the tone (input %.1f, %.1f)" % (fmt, Sb, image, dc, image_in, dc_in))
    assert nb == iq.N_SEL // Sb and rec["held_blocks"][0] == 0
    assert image >= 60.0 and dc >= 60.0
    assert abs(rec["w_re"][0] / -0.0245 - 1) <= 0.02 and abs(rec["w_im"][0] / 0.0262 - 1) <= 0.02
