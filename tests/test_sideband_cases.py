"""CPU tests of the sideband stage: its NumPy restatement (tests/sideband_cases.py) on hand-worked streams, its
continuity over calls of any length, BOTH against UPPER and LOWER, the mirror law, the int16 quantisation, the
restatement against a float64 model within a derived error budget, the selectivity of the stated band-pass, the
host-side design and the boundary (the header declares the entry points, the library and sdrg.EXPORTS carry them).  No
device is touched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import ddc_cases as dd
import sideband_cases as sb

f32 = np.float32
NEW_SYMBOLS = ("sdrg_sideband_design", "sdrg_sideband_geometry", "sdrg_engine_set_sideband", "sdrg_engine_get_sideband",
               "sdrg_engine_sideband_reset", "sdrg_engine_sideband_max_out", "sdrg_engine_sideband_device",
               "sdrg_engine_sideband_host", "sdrg_engine_listen_sideband_host")
FC = 2_000_000 / 41
OK = dict(channel_rate_hz=FC, low_hz=300.0, high_hz=2700.0, mode=sb.UPPER, audio_decimation=4, taps=255,
          out_format=sb.OUT_F32, max_in=4096, gain=0.5)


@pytest.fixture(scope="module")
def S():
    import sdrg
    return sdrg


def c64(*z):
    return np.array([z], np.complex64)


def test_header_library_and_mirror_carry_the_stage(S):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sdrg.h")).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", S.lib_path()], capture_output=True, text=True, check=True).stdout
    L = S.load()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert re.search(r"\bT %s$" % s, nm, flags=re.M), s
        assert s in S.EXPORTS and hasattr(L, s)
    for s in ("sdrg_sideband_config", "#define SDRG_SIDEBAND_UPPER 0", "#define SDRG_SIDEBAND_LOWER 1",
              "#define SDRG_SIDEBAND_BOTH 2", "#define SDRG_SIDEBAND_OUT_S16 0", "#define SDRG_SIDEBAND_OUT_F32 1",
              "#define SDRG_SIDEBAND_MAX_TAPS 511", "#define SDRG_SIDEBAND_MAX_DECIMATION 64",
              "#define SDRG_SIDEBAND_MAX_IN 1048576"):
        assert s in text
    assert L.sdrg_abi_version() == 1
    assert ctypes.sizeof(S.SidebandConfig) == 48
    assert (S.SIDEBAND_UPPER, S.SIDEBAND_LOWER, S.SIDEBAND_BOTH) == (sb.UPPER, sb.LOWER, sb.BOTH)
    assert (S.SIDEBAND_OUT_S16, S.SIDEBAND_OUT_F32) == (sb.OUT_S16, sb.OUT_F32)
    assert (S.SIDEBAND_MAX_TAPS, S.SIDEBAND_MAX_DECIMATION, S.SIDEBAND_MAX_IN) == (sb.MAX_TAPS, sb.MAX_DECIMATION, sb.MAX_IN)
    # the geometry: a tile of at least one output and at most a workgroup's lanes, whose window fits the LDS samples
    for R in (1, 3, 4, 16, 64):
        for T in (1, 3, 127, 255, 511):
            tile = S.sideband_geometry(R, T)
            assert 1 <= tile <= 256 and (tile - 1) * R + T <= 3072, (R, T, tile)
    assert S.sideband_geometry(64, 511) == 40 and S.sideband_geometry(1, 1) == 256
    t = ctypes.c_int32()
    assert L.sdrg_sideband_geometry(0, 3, ctypes.byref(t)) == -1
    assert L.sdrg_sideband_geometry(65, 3, ctypes.byref(t)) == -1
    assert L.sdrg_sideband_geometry(4, 4, ctypes.byref(t)) == -1
    assert L.sdrg_sideband_geometry(4, 513, ctypes.byref(t)) == -1
    assert L.sdrg_sideband_geometry(4, 3, None) == -1


def test_design_agrees_with_the_formulas(S):
    cases = [OK, dict(OK, taps=1), dict(OK, low_hz=0.0, high_hz=3000.0, taps=511),
             dict(OK, channel_rate_hz=48_000.0, low_hz=600.0, high_hz=800.0, taps=127),
             dict(OK, low_hz=0.0, high_hz=FC / 2, taps=3)]
    for cfg in cases:
        got = S.sideband_design(**cfg)
        cr, ci = sb.design_formula(cfg["channel_rate_hz"], cfg["low_hz"], cfg["high_hz"], cfg["taps"])
        for name, want in (("cr", cr), ("ci", ci)):
            g = got[name]
            assert g.dtype == np.float32 and g.shape == (cfg["taps"],)
            # one float ulp of the formula: libm's sin and cos against NumPy's, in double, ahead of the one rounding
            assert np.all(np.abs(g.astype(np.float64) - want) <= np.spacing(np.abs(want).astype(f32))), (name, cfg)
        # the filter is Hermitian about its middle: cr even, ci odd
        assert np.array_equal(got["cr"], got["cr"][::-1]) and np.array_equal(got["ci"], -got["ci"][::-1])
    one = S.sideband_design(**dict(OK, taps=1))
    assert one["cr"].tolist() == [1.0] and one["ci"].tolist() == [0.0]
    L = S.load()
    c = S.SidebandConfig(**OK)
    assert L.sdrg_sideband_design(None, None, None) == -1
    assert L.sdrg_sideband_design(ctypes.byref(c), None, None) == 0  # either result pointer may be NULL


def test_design_refuses_each_bad_field_on_its_own(S):
    S.sideband_design(**OK)
    assert sb.valid_config(OK)
    nan, inf = float("nan"), float("inf")
    bad = [dict(mode=3), dict(mode=-1), dict(low_hz=-1.0), dict(low_hz=2700.0), dict(low_hz=3000.0),
           dict(high_hz=FC / 2 + 1.0), dict(low_hz=nan), dict(high_hz=nan), dict(high_hz=inf), dict(channel_rate_hz=nan),
           dict(channel_rate_hz=0.0), dict(channel_rate_hz=-1.0), dict(channel_rate_hz=inf), dict(audio_decimation=0),
           dict(audio_decimation=65), dict(taps=0), dict(taps=254), dict(taps=513), dict(taps=-1), dict(max_in=0),
           dict(max_in=(1 << 20) + 1), dict(gain=inf), dict(gain=nan), dict(out_format=2), dict(out_format=-1)]
    for b in bad:
        cfg = dict(OK, **b)
        assert not sb.valid_config(cfg), b
        with pytest.raises(S.SdrgError) as ei:
            S.sideband_design(**cfg)
        assert "SDRG_E_INVALID" in str(ei.value), b
    # the limits themselves
    S.sideband_design(**dict(OK, audio_decimation=64, taps=511, low_hz=0.0, high_hz=FC / 2, max_in=1 << 20))
    S.sideband_design(**dict(OK, audio_decimation=1, taps=1, max_in=1, gain=-3.0, mode=sb.BOTH, out_format=sb.OUT_S16))


# ---- the law -----------------------------------------------------------------------------------------------------------

def test_hand_worked_stream():
    """T = 3, R = 2, taps chosen so every product and sum is exact: cr = (1, 2, 4), ci = (8, 16, 32)."""
    cr, ci = [1.0, 2.0, 4.0], [8.0, 16.0, 32.0]
    z = c64(1 + 1j, 2 - 1j, -3 + 2j, 0.5 + 0j, 1 - 2j)
    # outputs at the global indices 0, 2, 4; z[j] = 0 for j < 0
    ax = [1 * 1, 1 * -3 + 2 * 2 + 4 * 1, 1 * 1 + 2 * 0.5 + 4 * -3]
    ay = [8 * 1, 8 * 2 + 16 * -1 + 32 * 1, 8 * -2 + 16 * 0 + 32 * 2]
    up = [a - b for a, b in zip(ax, ay)]
    lo = [a + b for a, b in zip(ax, ay)]
    for mode, want in ((sb.UPPER, up), (sb.LOWER, lo)):
        out, n_out = sb.Sideband(1, cr, ci, 2, mode, gain=0.5).call(z)
        assert n_out == 3 and out.shape == (1, 3) and out[0].tolist() == [0.5 * w for w in want]
    out, n_out = sb.Sideband(1, cr, ci, 2, sb.BOTH, gain=2.0, max_in=9).call(z)
    assert n_out == 3 and out.shape == (1, 5, 2) and not out[:, 3:].any()
    assert out[0, :3, 0].tolist() == [2 * w for w in up] and out[0, :3, 1].tolist() == [2 * w for w in lo]
    # a second call continues the stream: global indices 5 .. 8, outputs at 6 and 8
    m = sb.Sideband(1, cr, ci, 2, sb.UPPER)
    m.call(z)
    out, n_out = m.call(c64(1j, 2 + 0j, 0j, -1 - 1j))
    # index 6: z6 = 2, z5 = j, z4 = 1 - 2j; index 8: z8 = -1 - j, z7 = 0, z6 = 2
    assert n_out == 2 and m.g == 9
    assert out[0].tolist() == [(1 * 2 + 2 * 0 + 4 * 1) - (8 * 0 + 16 * 1 + 32 * -2),
                               (1 * -1 + 2 * 0 + 4 * 2) - (8 * -1 + 16 * 0 + 32 * 0)]
    # a call without samples: out written, the state where it was
    out, n_out = m.call(np.zeros((1, 0), np.complex64))
    assert n_out == 0 and out.shape == (1, 0) and m.g == 9


def test_every_sum_is_rounded_on_its_own():
    """1 + 2^-24 + 2^-24 in this order is 1 in float32 (each half ulp rounds to even); a fused or reordered sum gives
    1 + 2^-23."""
    e = 2.0 ** -24
    out, _ = sb.Sideband(1, [e, e, 1.0], [0.0, 0.0, 0.0], 1, sb.UPPER).call(c64(1 + 0j, 1 + 0j, 1 + 0j))
    assert out[0, 2] == f32(1.0 + 2 * e) and f32(f32(f32(1.0) + f32(e)) + f32(e)) == f32(1.0)
    # k ascending: cr[0] z[m] first.  At m = 2: ((e * 1 + e * 1) + 1 * 1) = 1 + 2^-23 exactly
    out, _ = sb.Sideband(1, [1.0, e, e], [0.0, 0.0, 0.0], 1, sb.UPPER).call(c64(1 + 0j, 1 + 0j, 1 + 0j))
    assert out[0, 2] == f32(1.0)  # (1 + e) + e, each rounded to even: 1


@pytest.mark.parametrize("mode", [sb.UPPER, sb.LOWER, sb.BOTH])
@pytest.mark.parametrize("R,T", [(1, 1), (1, 31), (3, 15), (7, 63), (64, 9)])
def test_any_cut_of_a_stream_gives_the_bytes_of_one_call(S, mode, R, T):
    B, n = 3, 700
    des = S.sideband_design(**dict(OK, audio_decimation=R, taps=T))
    chan = sb.noise(B, n, seed=R * 100 + T)
    whole, n_whole = sb.Sideband(B, des["cr"], des["ci"], R, mode, 0.7).call(chan)
    assert n_whole == -(-n // R)
    rng = np.random.default_rng(T)
    for cuts in ([0, 1, 1, 2, 0, 63, 64, 65, 0], list(rng.integers(0, 90, 12)), [1] * 70, [n]):
        m = sb.Sideband(B, des["cr"], des["ci"], R, mode, 0.7)
        parts, at = [], 0
        for c in list(cuts) + [n]:
            c = min(int(c), n - at)
            out, n_out = m.call(chan[:, at:at + c])
            assert out.shape[1] == -(-c // R) and not out[:, n_out:].any()
            parts.append(out[:, :n_out])
            at += c
        assert at == n and m.g == n
        assert np.concatenate(parts, axis=1).tobytes() == whole.tobytes(), cuts


def test_both_is_upper_and_lower_and_lower_of_the_conjugate_is_upper(S):
    B, n = 4, 900
    for fmt in (sb.OUT_F32, sb.OUT_S16):
        des = S.sideband_design(**dict(OK, taps=127))
        chan = sb.noise(B, n, seed=5)
        outs = {m: sb.Sideband(B, des["cr"], des["ci"], 3, m, 1.3, fmt).call(chan)[0] for m in (sb.UPPER, sb.LOWER, sb.BOTH)}
        assert outs[sb.BOTH][..., 0].tobytes() == outs[sb.UPPER].tobytes()
        assert outs[sb.BOTH][..., 1].tobytes() == outs[sb.LOWER].tobytes()
        assert outs[sb.UPPER].tobytes() != outs[sb.LOWER].tobytes()
        # conj(z) negates every zi, so every product ci zi and every partial sum of acc.y: x - (-y) = x + y in bytes
        mirrored = sb.Sideband(B, des["cr"], des["ci"], 3, sb.LOWER, 1.3, fmt).call(np.conj(chan))[0]
        assert mirrored.tobytes() == outs[sb.UPPER].tobytes()


def test_int16_clamps_and_rounds_ties_to_even():
    # T = 1, cr = 1, ci = 0: u = zr.  o = zr gain
    m = sb.Sideband(1, [1.0], [0.0], 1, sb.UPPER, 1.0, sb.OUT_S16)
    half = lambda k: (k + 0.5) / 32767.0  # noqa: E731
    z = c64(2.0, -2.0, 1.0, -1.0, 0.0, 0.5, 1e-9, float(f32(half(0))), float(f32(half(1))), float(f32(half(2))))
    out, _ = m.call(z)
    assert out.dtype == np.int16
    want = np.rint(np.clip(z.real.astype(f32), -1, 1) * f32(32767)).astype(np.int16)
    assert out[0, :7].tolist() == [32767, -32767, 32767, -32767, 0, 16384, 0] and np.array_equal(out, want)
    # exact ties: o * 32767 = k + 1/2 in float32 arithmetic goes to the even neighbour
    prod = (z.real[0, 7:].astype(f32) * f32(32767)).astype(np.float64)
    for p, o in zip(prod, out[0, 7:]):
        if p % 1.0 == 0.5:
            assert int(o) % 2 == 0 and abs(int(o) - p) == 0.5
    assert sb.quantise(f32([0.5 / 32767 * 1.0000001, 1.5 / 32767, 2.5 / 32767]), sb.OUT_S16).dtype == np.int16
    assert np.rint(f32([0.5, 1.5, 2.5, -0.5, -1.5])).tolist() == [0.0, 2.0, 2.0, -0.0, -2.0]
    both, _ = sb.Sideband(1, [1.0], [1.0], 1, sb.BOTH, 1.0, sb.OUT_S16).call(c64(0.75 + 0.5j, -0.75 - 0.5j))
    assert both[0].tolist() == [[8192, 32767], [-8192, -32767]]  # u = 0.25, l = 1.25 clamped


@pytest.mark.parametrize("R,T", [(1, 511), (4, 255), (1, 1), (64, 127)])
def test_restatement_agrees_with_the_float64_model(S, R, T):
    """Measured worst |err| against the bound: 2.7e-7 of 5.2e-5 at (1, 511), 1.6e-7 of 2.2e-5 at (4, 255), 9.4e-8 of
    9.3e-6 at (64, 127) and 2.8e-8 of 1.7e-7 at (1, 1) (the bound is a worst case over signs; random roundings add as
    their root sum of squares)."""
    B, n = 4, 3000
    des = S.sideband_design(**dict(OK, audio_decimation=R, taps=T))
    chan = sb.noise(B, n, seed=9 + T)
    gain = 0.8
    got, n_out = sb.Sideband(B, des["cr"], des["ci"], R, sb.BOTH, gain).call(chan)
    want = sb.model_f64(chan, des["cr"], des["ci"], R, f32(gain))
    assert n_out == want.shape[1] and got.shape == want.shape
    bound = sb.error_bound(T, 0.9, des["cr"], des["ci"], gain)
    err = np.abs(got.astype(np.float64) - want).max()
    print(f"sideband f32 vs f64 (R={R}, T={T}): worst err {err:.3e}, bound {bound:.3e}, ratio {err / bound:.4f}")
    assert err <= bound
    assert np.abs(want).max() > 0.01


# ---- selectivity: fc = 2 MHz / 41, 300 - 2700 Hz, T = 511, R = 1 --------------------------------------------------------

@pytest.fixture(scope="module")
def voice_filter(S):
    return S.sideband_design(**dict(OK, taps=511, audio_decimation=1))


def rms(x):
    return float(np.sqrt(np.mean(np.asarray(x, np.float64) ** 2)))


@pytest.mark.parametrize("sign", [+1, -1])
def test_a_tone_comes_out_of_its_own_sideband_only(voice_filter, sign):
    """A tone of amplitude 0.5 at +1000 Hz: UPPER passes it at 0.5 / sqrt 2 RMS within 0.1 % (the float taps' gain there
    is -0.0005 dB), LOWER holds it at least 80 dB below (the taps give 101.7 dB; the float32 sums' worst case,
    (T + 3) 2^-24 sum|c| 0.5 with sum|c| = 2.37, is 80 dB below 0.5 / sqrt 2).  At -1000 Hz the two swap."""
    cr, ci = voice_filter["cr"], voice_filter["ci"]
    n, T = 511 + 4096, 511
    z = sb.tone(1, n, sign * 1000.0 / FC, amp=0.5)
    both, n_out = sb.Sideband(1, cr, ci, 1, sb.BOTH).call(z)
    assert n_out == n
    up, lo = both[0, T:, 0], both[0, T:, 1]  # settled: every tap on the tone
    passed, stopped = (up, lo) if sign > 0 else (lo, up)
    want = 0.5 / np.sqrt(2.0)
    assert abs(rms(passed) / want - 1.0) < 1e-3, rms(passed)
    assert 20 * np.log10(rms(stopped) / rms(passed)) <= -80.0, rms(stopped)
    # what the issue states about the taps themselves
    c_abs = float(np.abs(cr.astype(np.float64)).sum() + np.abs(ci.astype(np.float64)).sum())
    gain_db = 20 * np.log10(abs(sb.response(cr, ci, 1000.0 / FC)))
    image_db = 20 * np.log10(abs(sb.response(cr, ci, -1000.0 / FC)))
    assert abs(gain_db) < 0.001 and image_db < -100.0 and 2.3 < c_abs < 2.45, (gain_db, image_db, c_abs)


def test_two_tones_come_out_of_a_sideband_each_in_the_restatements_chained(S):
    """The behavioural case of tests/test_gpu_sideband.py on the restatements alone (the DDC's from the formulas of its
    design): the upper column peaks at the 1 kHz bin with the 1.5 kHz bin at least 60 dB below it, the lower column
    the reverse.  Measured: 80.3 dB and 75.0 dB (CS8 rounding of the tones included)."""
    fs, n = sb.TWO_TONE_FS, sb.TWO_TONE_N
    raw = sb.two_tone_raw()
    cfg = sb.TWO_TONE_DDC
    taps = dd.taps_formula(fs, cfg["cutoff_hz"], cfg["taps"]).astype(f32)
    ddc = dd.Ddc(1, taps, dd.tables_formula().astype(f32), dd.nco_increment(cfg["offset_hz"], fs), cfg["decimation"])
    des = S.sideband_design(**sb.TWO_TONE_SIDEBAND)
    band = sb.Sideband(1, des["cr"], des["ci"], 1, sb.BOTH, 1.0, sb.OUT_F32, 400)
    cols = []
    for f in range(sb.TWO_TONE_FRAMES):
        chan, n_chan = ddc.call(dd.CS8, raw[:, 2 * n * f:2 * n * (f + 1)])
        out, n_out = band.call(chan[:, :n_chan])
        cols.append(out[0, :n_out])
    cols = np.concatenate(cols)
    assert cols.shape[0] >= sb.TWO_TONE_SETTLED + 511 + 7
    peak, k1, k15, up_db = sb.two_tone_separation_db(cols[:, 0])
    assert peak == k1 and up_db >= 60.0, (peak, k1, up_db)
    peak, k1, k15, lo_db = sb.two_tone_separation_db(cols[:, 1])
    print(f"two tones: upper 1 kHz over 1.5 kHz {up_db:.1f} dB, lower 1.5 kHz over 1 kHz {-lo_db:.1f} dB")
    assert peak == k15 and -lo_db >= 60.0, (peak, k15, lo_db)
