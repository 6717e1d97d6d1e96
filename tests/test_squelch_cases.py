"""CPU tests of the squelch stage: its NumPy restatement (tests/squelch_cases.py) on hand-worked streams for each gate
code, its continuity over calls of any length, the adjacent-pair tree against a running sum, the host-side design and
its refusals, and the boundary (the header declares the entry points, the library and sdrg.EXPORTS carry them).  No
device is touched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import squelch_cases as sq

f32 = np.float32
NEW_SYMBOLS = ("sdrg_squelch_design", "sdrg_squelch_geometry", "sdrg_engine_set_squelch", "sdrg_engine_get_squelch",
               "sdrg_engine_squelch_reset", "sdrg_engine_squelch_device", "sdrg_engine_squelch_host",
               "sdrg_engine_ddc_squelch_demod_host", "sdrg_engine_ddc_squelch_demod_resample_host")
OK = dict(open_db=-3.0, close_db=-10.0, tau_blocks=0.0, block=16, hang_blocks=2, max_in=4096)
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
    for s in ("sdrg_squelch_config", "sdrg_squelch_record", "#define SDRG_SQUELCH_MIN_BLOCK 16",
              "#define SDRG_SQUELCH_MAX_BLOCK 1024", "#define SDRG_SQUELCH_MAX_HANG 65535",
              "#define SDRG_SQUELCH_MAX_IN 1048576"):
        assert s in text
    assert ctypes.sizeof(S.SquelchConfig) == 40
    assert S.SquelchRecord == sq.RECORD and S.SquelchRecord.itemsize == 16
    for block in (16, 32, 64, 128, 256, 512, 1024):
        assert S.squelch_geometry(block) == max(512, block)
    t = ctypes.c_int32()
    for bad in (0, 8, 24, 2048, -16):
        assert L.sdrg_squelch_geometry(bad, ctypes.byref(t)) == -1
    assert L.sdrg_squelch_geometry(64, None) == -1


def test_design_agrees_with_the_formulas(S):
    for cfg in (OK, dict(OK, open_db=0.0, close_db=0.0), dict(OK, open_db=-40.0, close_db=-47.5, tau_blocks=8.0),
                dict(OK, open_db=30.0, close_db=-120.0, tau_blocks=0.25), dict(OK, tau_blocks=1e6),
                dict(OK, open_db=-440.0, close_db=-449.0)):  # thresholds that are denormal floats, still positive
        got = S.squelch_design(**cfg)
        want = sq.design_formula(cfg["open_db"], cfg["close_db"], cfg["tau_blocks"])
        for name, w in zip(("open_thr", "close_thr", "beta"), want):
            assert got[name].dtype == np.float32
            assert abs(float(got[name]) - w) <= float(np.spacing(f32(abs(w)))), (cfg, name, got[name], w)
        assert got["close_thr"] <= got["open_thr"] and sq.valid_config(cfg)
    assert S.squelch_design(**dict(OK, open_db=0.0))["open_thr"] == f32(1.0)  # 0 dB is a mean power of 1
    beta = S.squelch_design(**dict(OK, tau_blocks=0.0))["beta"]
    assert beta.tobytes() == f32(1.0).tobytes()
    assert 0 < S.squelch_design(**dict(OK, tau_blocks=4.0))["beta"] < 1


@pytest.mark.parametrize("bad", [
    dict(block=48), dict(block=8), dict(block=2048), dict(block=0), dict(close_db=-2.0), dict(open_db=400.0),
    dict(close_db=-500.0), dict(open_db=float("nan")), dict(close_db=float("-inf")), dict(tau_blocks=-1.0),
    dict(tau_blocks=float("inf")), dict(tau_blocks=float("nan")), dict(hang_blocks=-1), dict(hang_blocks=65536),
    dict(max_in=0), dict(max_in=(1 << 20) + 1)], ids=lambda d: "%s=%s" % next(iter(d.items())))
def test_each_bad_field_is_refused_on_its_own(S, bad):
    S.squelch_design(**OK)
    assert sq.valid_config(OK) and not sq.valid_config(dict(OK, **bad))
    with pytest.raises(S.SdrgError) as ei:
        S.squelch_design(**dict(OK, **bad))
    assert "SDRG_E_INVALID" in str(ei.value)


def test_the_limits_themselves_are_accepted(S):
    for edge in (dict(block=1024), dict(hang_blocks=65535), dict(hang_blocks=0), dict(max_in=1), dict(max_in=1 << 20),
                 dict(open_db=-10.0), dict(open_db=380.0), dict(tau_blocks=1e300)):
        S.squelch_design(**dict(OK, **edge))
        assert sq.valid_config(dict(OK, **edge))


# ---- hand-worked streams: S = 16, beta = 1, thresholds 10^-0.3 = 0.501 and 0.1; a block of amplitude a has P = a a


def blocks_of(amps):
    """One stream whose block j is S16 samples of (amps[j], 0): its mean power is amps[j]^2, exactly for powers of two."""
    return np.repeat(np.asarray(amps, np.float32), S16).astype(np.complex64)[None, :]


def codes_of(out, z, S=S16):
    """The code of every block, read from the first and the last weight out / z of the block."""
    w = (out.real / z.real).reshape(-1, S)
    table = {(0.0, 0.0): sq.CLOSED, (1.0, 1.0): sq.OPEN, (1.0 / S, 1.0): sq.RAMP_UP, ((S - 1.0) / S, 0.0): sq.RAMP_DOWN}
    return [table[(float(r[0]), float(r[-1]))] for r in w]


def design(S, **over):
    d = S.squelch_design(**dict(OK, **over))
    return d["open_thr"], d["close_thr"], d["beta"]


LOW = 2.0 ** -4  # P = 2^-8, below the close threshold


@pytest.mark.parametrize("H", [0, 1, 2, 5])
def test_the_hang_holds_exactly_h_blocks(S, H):
    z = blocks_of([1.0] + [LOW] * (H + 4))
    out, rec, nb = sq.one_call(z, *design(S), S16, H)
    # block 0 opens the gate for block 1; block 1 is the first below close_thr: H further blocks pass whole, then the ramp
    assert codes_of(out[0], z[0]) == [sq.CLOSED, sq.RAMP_UP] + [sq.OPEN] * H + [sq.RAMP_DOWN, sq.CLOSED, sq.CLOSED]
    assert nb == H + 5 and rec["open"][0] == 0 and rec["open_blocks"][0] == H + 1
    assert rec["level"][0] == f32(LOW * LOW)


def test_a_level_above_close_thr_reloads_the_hang(S):
    mid = 0.5  # P = 0.25: between the thresholds
    z = blocks_of([1.0, LOW, mid, LOW, LOW, LOW, LOW])
    out, rec, _ = sq.one_call(z, *design(S), S16, 1)
    # block 1 counts the hang down to 0, block 2 reloads it, blocks 3 and 4 use it up and close
    assert codes_of(out[0], z[0]) == [sq.CLOSED, sq.RAMP_UP, sq.OPEN, sq.OPEN, sq.OPEN, sq.RAMP_DOWN, sq.CLOSED]


def test_a_level_between_the_thresholds_keeps_the_state_it_found(S):
    mid = 0.5
    closed = blocks_of([mid] * 5)
    out, rec, _ = sq.one_call(closed, *design(S), S16, 0)
    assert codes_of(out[0], closed[0]) == [sq.CLOSED] * 5 and rec["open"][0] == 0 and rec["level"][0] == f32(0.25)
    assert not out.view(np.uint32).any()
    opened = blocks_of([1.0] + [mid] * 5)
    out, rec, _ = sq.one_call(opened, *design(S), S16, 0)
    assert codes_of(out[0], opened[0]) == [sq.CLOSED, sq.RAMP_UP] + [sq.OPEN] * 4
    assert rec["open"][0] == 1 and rec["open_blocks"][0] == 6
    assert out[0, 2 * S16:].tobytes() == opened[0, 2 * S16:].tobytes()  # code 3: the input's bytes


def test_equal_thresholds(S):
    o, c, beta = design(S, open_db=-6.0, close_db=-6.0)
    assert o == c and f32(0.25) < o < f32(0.2512)
    z = blocks_of([1.0, 0.5, 1.0, 1.0, 0.5, 0.5, 1.0])  # P = 0.25 is just below 10^-0.6
    out, rec, _ = sq.one_call(z, o, c, beta, S16, 0)
    assert codes_of(out[0], z[0]) == [sq.CLOSED, sq.RAMP_UP, sq.RAMP_DOWN, sq.RAMP_UP, sq.OPEN, sq.RAMP_DOWN, sq.CLOSED]
    # a level equal to the threshold opens, and holds
    z = blocks_of([1.0, 1.0, 1.0])
    out, rec, _ = sq.one_call(z, f32(1.0), f32(1.0), beta, S16, 0)
    assert codes_of(out[0], z[0]) == [sq.CLOSED, sq.RAMP_UP, sq.OPEN] and rec["open"][0] == 1


def test_the_ramps_first_and_last_weights(S):
    # powers 64, 34, 34, 34 against the thresholds 50 and 40: block 0 opens, block 1 closes, the rest stay closed
    z = np.repeat(np.array([8, 3 - 5j, -3 + 5j, -3 + 5j], np.complex64), S16)[None, :]
    out, rec, _ = sq.one_call(z, f32(50.0), f32(40.0), f32(1.0), S16, 0)
    r = f32(1.0) / f32(S16)
    up, down = out[0, S16:2 * S16], out[0, 2 * S16:3 * S16]
    zin = z[0, S16]
    assert up[0] == np.complex64(complex(zin.real * r, zin.imag * r)) and up[-1].tobytes() == zin.tobytes()
    for i in range(S16):
        w = f32(i + 1) * r
        assert up[i].real == f32(zin.real * w) and up[i].imag == f32(zin.imag * w)
        w = f32(S16 - 1 - i) * r
        assert down[i].real == f32(f32(-3.0) * w) and down[i].imag == f32(f32(5.0) * w)
    assert down[0] == np.complex64(complex(-3 * 15 / 16, 5 * 15 / 16))
    # the last weight of a ramp down is 0: the products' zeros keep the input's signs
    assert down[-1].tobytes() == np.complex64(complex(-0.0, 0.0)).tobytes()
    assert not out[0, :S16].view(np.uint32).any() and not out[0, 3 * S16:].view(np.uint32).any()


def test_block_0_is_closed_even_under_a_strong_input(S):
    z = blocks_of([1000.0, 1000.0])
    out, rec, nb = sq.one_call(z, *design(S), S16, 3)
    assert not out[0, :S16].view(np.uint32).any() and codes_of(out[0], z[0]) == [sq.CLOSED, sq.RAMP_UP]
    assert nb == 2 and rec["open"][0] == 1 and rec["level"][0] == f32(1e6) and abs(rec["level_db"][0] - 60.0) < 1e-4
    # a first call that ends inside block 0: no block completed, no level yet
    out, rec, nb = sq.one_call(z[:, :S16 - 1], *design(S), S16, 3)
    assert nb == 0 and not out.view(np.uint32).any() and rec["level"].tobytes() == f32(0).tobytes()
    assert rec["open"][0] == 0 and abs(rec["level_db"][0] + 200.0) < 1e-3


def test_the_level_is_smoothed_operation_by_operation(S):
    o, c, beta = design(S, tau_blocks=3.0)
    amps = [1.0, 0.5, 2.0, 0.25, 0.25]
    L = f32(0)
    for j in range(len(amps)):
        _, rec, _ = sq.one_call(blocks_of(amps[:j + 1]), o, c, beta, S16, 0)
        d = f32(f32(amps[j] * amps[j]) - L)
        L = f32(L + f32(beta * d))
        assert rec["level"][0].tobytes() == L.tobytes(), j


def test_the_tree_is_not_a_running_sum(S):
    """One sample of power 1, then fifteen of power 2^-24: added one after the other each of them is half an ulp of the
    sum and rounds away; paired first, they reach 14 * 2^-24."""
    amps = np.full(S16, 2.0 ** -12, np.float32)
    amps[0] = 1.0
    p = sq.powers(amps.astype(np.complex64))
    assert sq.running_sum(p) == f32(1.0)
    tree = sq.tree_sum(p)
    assert tree == f32(1.0 + 14 * 2.0 ** -24) and tree != sq.running_sum(p)
    _, rec, nb = sq.one_call(amps.astype(np.complex64)[None, :], f32(0.5), f32(0.1), f32(1.0), S16, 0)
    assert nb == 1 and rec["level"][0] == f32(tree * f32(1.0 / 16)) and rec["level"][0] != f32(1.0 / 16)
    # and the pairs are those of the in-block index: the same powers one place on give another sum
    q = np.zeros(S16, np.float32)
    q[0], q[1], q[2] = 1.0, 2.0 ** -24, 2.0 ** -24
    assert sq.tree_sum(q) == f32(1.0) and sq.tree_sum(np.roll(q, 1)) == f32(1.0 + 2.0 ** -23)


@pytest.mark.parametrize("S_,H,tau", [(16, 1, 0.0), (16, 0, 2.0), (64, 2, 1.5)])
def test_any_cut_of_a_stream_gives_the_bytes_of_one_call(S, S_, H, tau):
    B, n = 3, 11 * S_ + 5
    o, c, beta = design(S, open_db=-3.0, close_db=-9.0, tau_blocks=tau)
    z = sq.keyed(B, n, 5, S_, (1, 1, 0, 0, 0, 1, 0))
    want, want_rec, want_nb = sq.one_call(z, o, c, beta, S_, H)
    assert set(np.unique(want_rec["open"])) <= {0, 1} and want_rec["open_blocks"].min() > 0
    rng = np.random.default_rng(17)
    cut_sets = [[], [0], [n], [1], [0, 0, 1, 2, 2], [S_ - 1], [S_], [S_ + 1],
                [3 * S_ + 2, 3 * S_ + 5, 3 * S_ + 9, 3 * S_ + 9],  # three calls, and one without samples, inside one block
                list(range(1, n)),  # every call a single sample
                list(range(S_, n, S_)), sorted(rng.integers(0, n + 1, 9).tolist()),
                sorted(rng.integers(0, n + 1, 40).tolist())]
    for cuts in cut_sets:
        got, rec, nb = sq.in_calls(z, cuts, o, c, beta, S_, H)
        assert got.tobytes() == want.tobytes(), cuts
        assert nb == want_nb == n // S_
        for k in ("level", "level_db", "open"):
            assert rec[k].tobytes() == want_rec[k].tobytes(), (cuts, k)
    # open_blocks counts the call's own blocks: over the calls they add up to the one call's
    model = sq.Squelch(B, o, c, beta, S_, H)
    total = sum(model.call(part)[1]["open_blocks"] for part in np.array_split(z, 7, axis=1))
    assert total.tolist() == want_rec["open_blocks"].tolist()


def test_a_call_without_samples_reports_and_changes_nothing(S):
    o, c, beta = design(S)
    model = sq.Squelch(2, o, c, beta, S16, 1)
    out, rec, nb = model.call(np.zeros((2, 0), np.complex64), in_stride=7)
    assert out.shape == (2, 7) and not out.view(np.uint32).any() and nb == 0 and model.g == 0
    assert np.all(np.abs(rec["level_db"] + 200.0) < 1e-3)
    _, before, _ = model.call(sq.noise(2, 40, 3))
    _, after, nb = model.call(np.zeros((2, 0), np.complex64))
    assert nb == 0 and model.g == 40 and after["open_blocks"].tolist() == [0, 0]
    for k in ("level", "level_db", "open"):
        assert after[k].tobytes() == before[k].tobytes()
