"""CPU tests of the noise blanker stage: its NumPy restatement (tests/blanker_cases.py) on hand-worked streams, its
continuity over calls of any length against the whole-stream model, the sum-then-min tree against a plain sum and a plain
minimum, its benefit on a pulsed signal, the host-side design and its refusals, and the boundary (the header declares the
entry points, the library and sdrg.EXPORTS carry them).  No device is touched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import blanker_cases as bk

f32 = np.float32
NEW_SYMBOLS = ("sdrg_blanker_design", "sdrg_blanker_geometry", "sdrg_engine_set_blanker", "sdrg_engine_get_blanker",
               "sdrg_engine_blanker_reset", "sdrg_engine_blanker_device", "sdrg_engine_blanker_host",
               "sdrg_engine_clean_process_host")
OK = dict(tau_blocks=0.0, threshold_db=10.0, floor_db=-60.0, block=64, lead=2, tail=3, max_in=4096)
S64 = 64


@pytest.fixture(scope="module")
def S():
    import sdrg
    return sdrg


def design(S, **over):
    d = S.blanker_design(**dict(OK, **over))
    return d["beta"], d["ratio"], d["floor_thr"]


def test_header_library_and_mirror_carry_the_stage(S):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sdrg.h")).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", S.lib_path()], capture_output=True, text=True, check=True).stdout
    L = S.load()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert re.search(r"\bT %s$" % s, nm, flags=re.M), s
        assert s in S.EXPORTS and hasattr(L, s)
    for s in ("sdrg_blanker_config", "sdrg_blanker_record", "#define SDRG_BLANKER_MIN_BLOCK 64",
              "#define SDRG_BLANKER_MAX_BLOCK 1024", "#define SDRG_BLANKER_MAX_LEAD 16", "#define SDRG_BLANKER_MAX_TAIL 64",
              "#define SDRG_CLEAN_IQCORR 1"):
        assert s in text
    assert ctypes.sizeof(S.BlankerConfig) == 40
    assert S.BlankerRecord == bk.RECORD and S.BlankerRecord.itemsize == 16
    assert (S.BLANKER_MAX_LEAD, S.BLANKER_MAX_TAIL, S.CLEAN_IQCORR) == (bk.MAX_LEAD, bk.MAX_TAIL, 1)
    for block in (64, 128, 256, 512, 1024):
        assert S.blanker_geometry(block) == (max(512, block), 512)
    a, b = ctypes.c_int32(), ctypes.c_int32()
    for bad in (0, 16, 32, 96, 2048, -64):
        assert L.sdrg_blanker_geometry(bad, ctypes.byref(a), ctypes.byref(b)) == -1
    assert L.sdrg_blanker_geometry(64, None, None) == -1
    assert L.sdrg_blanker_geometry(1024, None, ctypes.byref(b)) == 0 and b.value == 512
    assert L.sdrg_blanker_geometry(1024, ctypes.byref(a), None) == 0 and a.value == 1024


def test_design_agrees_with_the_formulas(S):
    for cfg in (OK, dict(OK, tau_blocks=16.0, threshold_db=13.0), dict(OK, tau_blocks=0.25, floor_db=30.0),
                dict(OK, tau_blocks=1e6, floor_db=-120.0, threshold_db=-3.0), dict(OK, floor_db=-440.0),  # a denormal floor
                dict(OK, threshold_db=60.0)):
        got = S.blanker_design(**cfg)
        want = bk.design_formula(cfg["tau_blocks"], cfg["threshold_db"], cfg["floor_db"])
        for name, w in zip(("beta", "ratio", "floor_thr"), want):
            assert got[name].dtype == np.float32
            assert abs(float(got[name]) - w) <= float(np.spacing(f32(abs(w)))), (cfg, name, got[name], w)
        assert bk.valid_config(cfg)
    assert S.blanker_design(**OK)["beta"].tobytes() == f32(1.0).tobytes()  # tau 0
    assert S.blanker_design(**OK)["ratio"] == f32(10.0) and S.blanker_design(**dict(OK, floor_db=0.0))["floor_thr"] == f32(1.0)
    assert 0 < S.blanker_design(**dict(OK, tau_blocks=4.0))["beta"] < 1


@pytest.mark.parametrize("bad", [
    dict(block=48), dict(block=32), dict(block=2048), dict(block=0), dict(lead=-1), dict(lead=17), dict(tail=-1),
    dict(tail=65), dict(tau_blocks=-1.0), dict(tau_blocks=float("inf")), dict(tau_blocks=float("nan")),
    dict(threshold_db=float("nan")), dict(threshold_db=float("inf")), dict(threshold_db=float("-inf")),
    dict(threshold_db=400.0), dict(threshold_db=-500.0), dict(floor_db=float("nan")), dict(floor_db=float("-inf")),
    dict(floor_db=float("inf")), dict(floor_db=400.0), dict(floor_db=-500.0), dict(max_in=0),
    dict(max_in=(1 << 20) + 1)], ids=lambda d: "%s=%s" % next(iter(d.items())))
def test_each_bad_field_is_refused_on_its_own(S, bad):
    S.blanker_design(**OK)
    assert bk.valid_config(OK) and not bk.valid_config(dict(OK, **bad))
    with pytest.raises(S.SdrgError) as ei:
        S.blanker_design(**dict(OK, **bad))
    assert "SDRG_E_INVALID" in str(ei.value)


def test_the_limits_and_null_pointers(S):
    for edge in (dict(block=1024), dict(block=64), dict(lead=0), dict(lead=16), dict(tail=0), dict(tail=64),
                 dict(max_in=1), dict(max_in=1 << 20), dict(floor_db=380.0), dict(threshold_db=-440.0),
                 dict(tau_blocks=1e300)):
        S.blanker_design(**dict(OK, **edge))
        assert bk.valid_config(dict(OK, **edge))
    L = S.load()
    c = S.BlankerConfig(**OK)
    assert L.sdrg_blanker_design(None, None, None, None) == -1
    assert L.sdrg_blanker_design(ctypes.byref(c), None, None, None) == 0  # any of the three may be null
    r = ctypes.c_float()
    assert L.sdrg_blanker_design(ctypes.byref(c), None, ctypes.byref(r), None) == 0 and r.value == 10.0
    for fn in (L.sdrg_engine_blanker_reset,):
        assert fn(None) == -1
    assert L.sdrg_engine_set_blanker(None, ctypes.byref(c)) == -1
    assert L.sdrg_engine_get_blanker(None, None, None, None, None, None) == -1
    n = ctypes.c_int32(-7)
    assert L.sdrg_engine_blanker_device(None, None, 1, 64, 64, None, None, ctypes.byref(n)) == -1
    assert L.sdrg_engine_blanker_host(None, None, 1, 64, 64, None, None, ctypes.byref(n)) == -1
    assert L.sdrg_engine_clean_process_host(None, None, 1, 0, 1, None, None, None, 0, None, None) == -1
    assert n.value == -7


# ---- hand-worked streams


def planted(n, at, lead, tail):
    """The output paragraph alone on the samples 1, 2, ... n with hits planted at the global indices `at`, the stream
    starting with the call: (out [n], blanked)."""
    z = np.concatenate([np.zeros(lead), np.arange(1, n + 1)]).astype(np.complex64)[None, :]
    hit = np.zeros((1, lead + tail + n), bool)
    hit[0, lead + tail + np.asarray(at, int)] = True
    out, blanked = bk.output(z, hit, n, lead, tail, lead)
    return out[0].real.astype(int).tolist(), int(blanked[0])


def test_the_window_of_a_single_hit():
    # lead 2, tail 3: a hit at v zeroes the inputs v - 2 .. v + 3, which leave at the outputs v .. v + 5
    assert planted(12, [5], 2, 3) == ([0, 0, 1, 2, 3, 0, 0, 0, 0, 0, 0, 10], 6)
    # at index 0 the lead reaches before the stream: the outputs 0 and 1 carry nothing, and are not counted
    assert planted(8, [0], 2, 3) == ([0, 0, 0, 0, 0, 0, 5, 6], 4)
    # at lead - 1 = 1: output 1 carries nothing (not counted); the outputs 2 .. 6 carry the inputs 0 .. 4, all blanked
    assert planted(9, [1], 2, 3) == ([0, 0, 0, 0, 0, 0, 0, 6, 7], 5)
    # lead = tail = 0: the hit alone, and no delay
    assert planted(5, [0, 3], 0, 0) == ([0, 2, 3, 0, 5], 2)
    # two hits whose windows merge (5 and 9: inputs 3 .. 12), and two whose windows do not (5 and 12)
    assert planted(16, [5, 9], 2, 3) == ([0, 0, 1, 2, 3] + [0] * 10 + [14], 10)
    assert planted(20, [5, 12], 2, 3) == ([0, 0, 1, 2, 3] + [0] * 6 + [10] + [0] * 6 + [17, 18], 12)


def quiet_with(loud_at, n=4 * S64, amp=0.1):
    """One stream of n samples (amp, 0) with (1, 0) at the indices loud_at."""
    z = np.full((1, n), amp, np.complex64)
    z[0, list(loud_at)] = 1.0
    return z


def test_nothing_is_a_hit_before_the_first_block_completes(S):
    z = quiet_with([0, 1, 63])
    out, rec, nb = bk.one_call(z, bk.CF32, *design(S), S64, 2, 3)
    assert nb == 4 and rec["hits"][0] == 0 and rec["blanked"][0] == 0
    assert np.array_equal(out[0, 2:], z[0, :-2]) and out[0, :2].tobytes() == bytes(16)
    # the sub-blocks with the loud samples do not move the floor: F = 16 q 0.0625 of a quiet one
    q = f32(0.1) * f32(0.1)
    assert rec["level"][0] == bk.tree_sum(np.full(16, q, np.float32)) * f32(0.0625)


def test_a_hit_at_a_blocks_last_and_first_sample(S):
    """thr after block 0 is 10 q: the loud sample at 127, the last of block 1, is judged by block 0, the one at 128 by
    block 1, whose floor is the same; lead 2, tail 3."""
    for at in (127, 128, 2 * S64 + 5):
        z = quiet_with([at])
        out, rec, nb = bk.one_call(z, bk.CF32, *design(S), S64, 2, 3)
        want = np.concatenate([np.zeros(2, np.complex64), z[0, :-2]])
        want[at:at + 6] = 0
        assert out[0].tobytes() == want.tobytes(), at
        assert (rec["hits"][0], rec["blanked"][0]) == (1, 6)
        w, L, hits, blanked = bk.whole_stream(z[0], *design(S), S64, 2, 3)
        assert w.tobytes() == out[0].tobytes() and (hits, blanked) == (1, 6) and L == rec["level"][0]


def test_the_decision_never_reaches_into_its_own_block(S):
    """A block that is loud throughout raises the level only for the block after it: with beta 1 its own samples are
    hits (judged by the quiet block before), and the quiet block after it has none although the level is high."""
    z = quiet_with(range(S64, 2 * S64))
    out, rec, _ = bk.one_call(z, bk.CF32, *design(S, lead=0, tail=0), S64, 0, 0)
    assert rec["hits"][0] == S64 and rec["blanked"][0] == S64
    assert not out[0, S64:2 * S64].any() and np.array_equal(out[0, 2 * S64:], z[0, 2 * S64:])


def test_the_floor_is_a_minimum_of_sums(S):
    """A block of q = 2 but for a sub-block of fifteen 1 and one 3: F = 18 / 16, neither the block's mean power nor its
    least power; and a sub-block of 1 and fifteen 2^-24 adds as a pair tree, not one after the other."""
    q = np.full(S64, 2.0, np.float32)
    q[16:32] = 1.0
    q[20] = 3.0
    assert bk.block_floor(q) == f32(18.0 / 16.0)
    assert bk.block_floor(q) != q.min() and bk.block_floor(q) != bk.tree_sum(q) * f32(1.0 / S64)
    z = np.sqrt(q).astype(np.complex64)[None, :]
    z[0, 20], z[0, 16:20], z[0, 21:32] = np.sqrt(f32(3.0)), 1.0, 1.0
    _, rec, _ = bk.one_call(z, bk.CF32, *design(S), S64, 0, 0)
    zr, zi = bk.sample(z.view(np.float32), bk.CF32)
    assert rec["level"][0] == bk.block_floor(bk.power(zr, zi))[0]
    assert abs(rec["level"][0] - 18.0 / 16.0) < 1e-6
    q = np.full(S64, 4.0, np.float32)
    q[:16] = 2.0 ** -24
    q[0] = 1.0
    assert bk.block_floor(q) == f32((1.0 + 14 * 2.0 ** -24) * 0.0625)  # running: 1 / 16


@pytest.mark.parametrize("fmt", [bk.CS8, bk.CU8, bk.CS16, bk.CF32])
def test_any_cut_of_a_stream_equals_one_call(S, fmt):
    B, n, Sb, lead, tail = 3, 1000, 64, 3, 7
    rng = np.random.default_rng(5)
    z = bk.gaussian(B, n, 11, 0.1).astype(np.complex128)
    for b in range(B):  # pulses, single and in runs, at block seams among them
        at = np.concatenate([rng.integers(64, n, 12), [127, 128, 191, 640, 641, 642, n - 1]])
        z[b, at] += 0.9
    raw = bk.to_raw(z, fmt, {bk.CS8: 100.0, bk.CU8: 100.0, bk.CS16: 20000.0, bk.CF32: 1.0}[fmt])
    d = design(S, tau_blocks=3.0)
    whole, rec, nb = bk.one_call(raw, fmt, *d, Sb, lead, tail)
    assert nb == n // Sb and (rec["hits"] >= 15).all() and (rec["blanked"] > rec["hits"]).all()
    zr, zi = bk.sample(raw, fmt)
    for b in range(B):  # the law written a second time
        w, L, hits, blanked = bk.whole_stream(zr[b] + 1j * zi[b], *d, Sb, lead, tail)
        assert w.tobytes() == whole[b].tobytes()
        assert (L, hits, blanked) == (rec["level"][b], rec["hits"][b], rec["blanked"][b])
    for cuts in ([1], [0, 0, 1, 2], [63, 64, 65], [64, 128, 128, 129], [999], [n], [500], list(range(7, n, 37)),
                 [31, 32, 33, 640, 641], [126, 127, 128, 129, 130], list(range(600, 700))):  # 100 calls of one sample
        out, r, blocks, hits, blanked = bk.in_calls(raw, fmt, cuts, *d, Sb, lead, tail)
        assert out.tobytes() == whole.tobytes(), cuts
        assert blocks == nb and np.array_equal(hits, rec["hits"]) and np.array_equal(blanked, rec["blanked"]), cuts
        for k in ("level", "level_db"):
            assert r[k].tobytes() == rec[k].tobytes(), (cuts, k)


def test_a_call_without_samples_leaves_the_stream_where_it_is(S):
    m = bk.Blanker(2, *design(S), S64, 2, 3)
    z = bk.gaussian(2, 200, 3, 0.1)
    a, ra, _ = m.call(z[:, :100])
    out, r0, nb = m.call(z[:, :0], in_stride=5)
    assert nb == 0 and out.shape == (2, 5) and not out.view(np.uint32).any() and m.g == 100
    assert r0["level"].tobytes() == ra["level"].tobytes() and not r0["hits"].any() and not r0["blanked"].any()
    b, _, _ = m.call(z[:, 100:])
    whole, _, _ = bk.one_call(z, bk.CF32, *design(S), S64, 2, 3)
    assert np.concatenate([a, b], axis=1).tobytes() == whole.tobytes()


# ---- the benefit: a pulsed signal's spectrum floor comes back down, the tone stays


@pytest.fixture(scope="module")
def signals():
    return bk.pulsed(pulses=False), bk.pulsed()


@pytest.mark.parametrize("Sb", [64, 256, 1024])
@pytest.mark.parametrize("fmt", [bk.CF32, bk.CS16], ids=["cf32", "cs16"])
def test_benefit_of_the_restatement(S, signals, fmt, Sb):
    scale = 20000.0 if fmt == bk.CS16 else 1.0
    clean, dirty = (bk.to_raw(z[None, :], fmt, scale) for z in signals)
    as_z = lambda raw: np.add(*(c * k for c, k in zip(bk.sample(raw, fmt), (1, 1j))))[0]  # noqa: E731
    med_c, pk_c = bk.spectrum_levels(as_z(clean))
    med_d, _ = bk.spectrum_levels(as_z(dirty))
    d = S.blanker_design(block=Sb, max_in=bk.N_BEN, **bk.BENEFIT)
    args = (d["beta"], d["ratio"], d["floor_thr"], Sb, bk.BENEFIT["lead"], bk.BENEFIT["tail"])
    out, rec, nb = bk.one_call(dirty, fmt, *args)
    med, pk = bk.spectrum_levels(out[0])
    _, rec_c, _ = bk.one_call(clean, fmt, *args)
    print("fmt %d S %d: input %.2f dB over the clean median, output %.2f dB, tone %+.2f dB, %d hits, %d blanked" % (
        fmt, Sb, med_d - med_c, med - med_c, pk - pk_c, rec["hits"][0], rec["blanked"][0]))
    assert nb == bk.N_BEN // Sb
    assert med_d - med_c >= 6.0
    assert med - med_c <= 1.5
    assert abs(pk - pk_c) <= 0.3
    assert rec_c["hits"][0] == 0 and rec_c["blanked"][0] == 0
    d60 = S.blanker_design(block=Sb, max_in=bk.N_BEN, **dict(bk.BENEFIT, threshold_db=60.0))
    out60, rec60, _ = bk.one_call(dirty, fmt, d60["beta"], d60["ratio"], d60["floor_thr"], *args[3:])
    z = as_z(dirty).astype(np.complex64)
    assert rec60["hits"][0] == 0
    assert out60[0].tobytes() == np.concatenate([np.zeros(2, np.complex64), z[:-2]]).tobytes()
