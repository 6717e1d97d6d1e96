"""CPU tests of the demodulator stage: its NumPy restatement (tests/demod_cases.py) on hand-worked streams, its
continuity over calls of any length, sdrg_atan2f against arctan2, the FM pipeline against a float64 model within a
derived error budget, AM, the int16 quantisation, the host-side design and the boundary (the header declares the entry
points, the library and sdrg.EXPORTS carry them).  No device is touched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import demod_cases as dm

f32 = np.float32
NEW_SYMBOLS = ("sdrg_demod_design", "sdrg_demod_geometry", "sdrg_engine_set_demod", "sdrg_engine_get_demod",
               "sdrg_engine_demod_reset", "sdrg_engine_demod_max_out", "sdrg_engine_demod_device",
               "sdrg_engine_demod_host", "sdrg_engine_ddc_demod_host")
OK = dict(mode=dm.FM, channel_rate_hz=200_000.0, deviation_hz=75_000.0, dc_cutoff_hz=20.0, deemphasis_us=75.0,
          audio_decimation=4, audio_taps=127, audio_cutoff_hz=15_000.0, gain=0.5, out_format=dm.OUT_F32, max_in=4096)


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
    for s in ("sdrg_demod_config", "#define SDRG_DEMOD_AM 0", "#define SDRG_DEMOD_FM 1", "#define SDRG_DEMOD_OUT_S16 0",
              "#define SDRG_DEMOD_OUT_F32 1", "#define SDRG_DEMOD_MAX_TAPS 255", "#define SDRG_DEMOD_MAX_DECIMATION 64",
              "#define SDRG_DEMOD_MAX_IN 1048576"):
        assert s in text
    assert L.sdrg_abi_version() == 1
    assert ctypes.sizeof(S.DemodConfig) == 64
    assert (S.DEMOD_AM, S.DEMOD_FM, S.DEMOD_OUT_S16, S.DEMOD_OUT_F32) == (dm.AM, dm.FM, dm.OUT_S16, dm.OUT_F32)
    assert (S.DEMOD_MAX_TAPS, S.DEMOD_MAX_DECIMATION, S.DEMOD_MAX_IN) == (dm.MAX_TAPS, dm.MAX_DECIMATION, dm.MAX_IN)
    # the geometry: a tile of at least one output and at most a workgroup's lanes, whose window fits the LDS samples
    for R in (1, 3, 16, 64):
        for T2 in (1, 3, 127, 255):
            tile, chunk = S.demod_geometry(R, T2)
            assert 1 <= tile <= 256 and (tile - 1) * R + T2 <= 6144 and chunk == 64
    t = ctypes.c_int32()
    assert L.sdrg_demod_geometry(0, 3, ctypes.byref(t), ctypes.byref(t)) == -1
    assert L.sdrg_demod_geometry(65, 3, ctypes.byref(t), ctypes.byref(t)) == -1
    assert L.sdrg_demod_geometry(4, 4, ctypes.byref(t), ctypes.byref(t)) == -1
    assert L.sdrg_demod_geometry(4, 257, ctypes.byref(t), ctypes.byref(t)) == -1
    assert L.sdrg_demod_geometry(4, 3, None, ctypes.byref(t)) == -1


def test_design_agrees_with_the_formulas(S):
    cases = [OK, dict(OK, mode=dm.AM, deviation_hz=0.0), dict(OK, channel_rate_hz=2_000_000 / 41, deviation_hz=5000.0,
                                                              audio_cutoff_hz=3000.0, audio_taps=1),
             dict(OK, dc_cutoff_hz=0.0, deemphasis_us=0.0, audio_taps=255, audio_cutoff_hz=100_000.0),
             dict(OK, deemphasis_us=50.0, dc_cutoff_hz=300.0, audio_taps=3)]
    for cfg in cases:
        got = S.demod_design(**cfg)
        kf, alpha, a, taps = dm.design_formula(cfg["mode"], cfg["channel_rate_hz"], cfg["deviation_hz"],
                                               cfg["dc_cutoff_hz"], cfg["deemphasis_us"], cfg["audio_cutoff_hz"],
                                               cfg["audio_taps"])
        assert got["taps"].dtype == np.float32 and got["taps"].shape == (cfg["audio_taps"],)
        assert got["taps"].tobytes() == taps.astype(np.float32).tobytes()
        for name, want in (("kf", kf), ("alpha", alpha), ("a", a)):
            assert abs(float(got[name]) - want) <= float(np.spacing(f32(abs(want)))), (name, got[name], want)
        assert (got["alpha"] == 0) == (cfg["dc_cutoff_hz"] == 0) and (got["a"] == 0) == (cfg["deemphasis_us"] == 0)
        if cfg["mode"] == dm.AM:
            assert got["kf"] == 0
    assert S.demod_design(**dict(OK, audio_taps=1))["taps"].tolist() == [1.0]
    L = S.load()
    c = S.DemodConfig(**OK)
    assert L.sdrg_demod_design(None, None, None, None, None) == -1
    assert L.sdrg_demod_design(ctypes.byref(c), None, None, None, None) == 0  # every result pointer may be NULL


def test_design_refuses_each_bad_field_on_its_own(S):
    S.demod_design(**OK)
    assert dm.valid_config(OK)
    nan, inf = float("nan"), float("inf")
    bad = [dict(mode=2), dict(mode=-1), dict(channel_rate_hz=0.0), dict(channel_rate_hz=-1.0), dict(channel_rate_hz=nan),
           dict(channel_rate_hz=inf), dict(deviation_hz=0.0), dict(deviation_hz=-5.0), dict(deviation_hz=nan),
           dict(deviation_hz=inf), dict(deviation_hz=1e-40), dict(dc_cutoff_hz=-1.0), dict(dc_cutoff_hz=nan),
           dict(dc_cutoff_hz=inf), dict(deemphasis_us=-1.0), dict(deemphasis_us=nan), dict(deemphasis_us=inf),
           dict(audio_decimation=0), dict(audio_decimation=65), dict(audio_decimation=-2), dict(audio_taps=0),
           dict(audio_taps=2), dict(audio_taps=257), dict(audio_taps=-1), dict(audio_cutoff_hz=0.0),
           dict(audio_cutoff_hz=-1.0), dict(audio_cutoff_hz=100_001.0), dict(audio_cutoff_hz=nan), dict(gain=nan),
           dict(gain=inf), dict(out_format=2), dict(out_format=-1), dict(max_in=0), dict(max_in=(1 << 20) + 1),
           dict(max_in=-1)]
    for b in bad:
        cfg = dict(OK, **b)
        assert not dm.valid_config(cfg), b
        with pytest.raises(S.SdrgError) as ei:
            S.demod_design(**cfg)
        assert "SDRG_E_INVALID" in str(ei.value), b
    # the limits themselves, and AM whatever deviation_hz holds
    S.demod_design(**dict(OK, audio_decimation=64, audio_taps=255, audio_cutoff_hz=100_000.0, max_in=1 << 20))
    S.demod_design(**dict(OK, audio_decimation=1, audio_taps=1, max_in=1, gain=-3.0, dc_cutoff_hz=0.0, deemphasis_us=0.0))
    S.demod_design(**dict(OK, mode=dm.AM, deviation_hz=nan))


def test_atan2f_stays_within_5e7_of_arctan2():
    """4e6 points: angle uniform in (-pi, pi), radius exp(U(-20, 5)), both coordinates rounded to float.  The worst
    error of exactly these float32 steps is 3.52e-7 rad; the margin to 5e-7 is for a differently built NumPy."""
    rng = np.random.default_rng(1)
    n = 4_000_000
    ang = rng.uniform(-np.pi, np.pi, n)
    rad = np.exp(rng.uniform(-20.0, 5.0, n))
    x, y = (rad * np.cos(ang)).astype(np.float32), (rad * np.sin(ang)).astype(np.float32)
    got = dm.atan2f(y, x)
    err = np.abs(got.astype(np.float64) - np.arctan2(y.astype(np.float64), x.astype(np.float64)))
    err = np.minimum(err, 2 * np.pi - err)  # +pi and -pi are the same direction
    print(f"sdrg_atan2f: worst error {err.max():.3e} rad")
    assert err.max() <= 5e-7


def test_atan2f_exact_values():
    h = float.fromhex
    c0, pi_2, pi = h("0x1.ffffecp-1"), h("0x1.921fb6p+0"), h("0x1.921fb6p+1")
    # q = 1 on the diagonals: p = the float32 Horner sum of the coefficients, r = p
    p = dm.ATAN_C[7]
    for k in range(6, -1, -1):
        p = f32(f32(p * f32(1)) + dm.ATAN_C[k])
    d = float(p)
    assert abs(d - np.pi / 4) < 4e-7
    want = {(0, 1): 0.0, (1, 1): d, (1, 0): pi_2, (1, -1): float(f32(pi) - f32(d)), (0, -1): pi,
            (-1, -1): -float(f32(pi) - f32(d)), (-1, 0): -pi_2, (-1, 1): -d}
    for (y, x), w in want.items():
        for scale in (1.0, 3.0, 2.0 ** -140, 2.0 ** 100):
            got = dm.atan2f(f32(y * scale), f32(x * scale))
            assert got.dtype == np.float32 and float(got) == w, (y, x, scale, got, w)
    assert c0 < 1.0
    # (+-0, +-0): q = 0, the sign bit of x chooses 0 or pi and y gives the sign
    z, nz = f32(0.0), f32(-0.0)
    for y, x, w in ((z, z, 0.0), (nz, z, -0.0), (z, nz, pi), (nz, nz, -pi)):
        got = dm.atan2f(y, x)
        assert float(got) == w and np.signbit(got) == np.signbit(f32(w)), (y, x, got)
    # x = -0 beside a y: the sign bit, not a comparison, folds the angle
    assert float(dm.atan2f(f32(1), nz)) == float(f32(pi) - f32(pi_2))


def test_hand_worked_detectors():
    """AM: |3+4j| = 5, |0| = 0, |-5-12j| = 13.  FM, kf = 2: 1, j, -1, -j, 1 are four steps of +pi/2: p = z conj(w) = j,
    q = 0 / 1, r = 0 folded to pi/2 (ay > ax); the first sample of the stream has no predecessor: +0.  A second call
    continues from the stored sample: 1 -> -1 is p = -1: r = pi - 0, the sign of pi = +0: +pi; -1 -> -1 is p = 1: 0."""
    d = dm.Demod(1, dm.AM, 0, 0, 0, [1.0], 1)
    out, n = d.call(c64(3 + 4j, 0, -5 - 12j))
    assert n == 3 and out.dtype == np.float32 and out[0].tolist() == [5.0, 0.0, 13.0]
    d = dm.Demod(1, dm.FM, 2.0, 0, 0, [1.0], 1)
    out, n = d.call(c64(1, 1j, -1, -1j, 1))
    half = float(dm.PI_2 * f32(2))
    assert out[0].tolist() == [0.0, half, half, half, half] and not np.signbit(out[0, 0])
    out, n = d.call(c64(-1, -1))
    assert out[0].tolist() == [float(dm.PI * f32(2)), 0.0] and d.g == 7 and d.w[0] == -1
    # clockwise: -pi/2 steps
    out, n = dm.Demod(1, dm.FM, 1.0, 0, 0, [1.0], 1).call(c64(1, -1j, -1))
    assert out[0].tolist() == [0.0, -float(dm.PI_2), -float(dm.PI_2)]


def test_hand_worked_recurrences():
    """alpha = 1/2 on e = 1, 1, 1 (|z| = 1): u = 1, 1/2, 1/4 with m = 1/2, 3/4, 7/8.  a = 1/2 on u = 1, 1, 1:
    s = 1/2, 3/4, 7/8.  Both: u = 1, 1/2, 1/4 -> s = 1/2, 1/2, 3/8."""
    z = c64(1, 1j, -1)
    d = dm.Demod(1, dm.AM, 0, 0.5, 0, [1.0], 1)
    assert d.call(z)[0][0].tolist() == [1.0, 0.5, 0.25] and d.m[0] == 0.875 and d.s[0] == 0
    d = dm.Demod(1, dm.AM, 0, 0, 0.5, [1.0], 1)
    assert d.call(z)[0][0].tolist() == [0.5, 0.75, 0.875] and d.s[0] == 0.875 and d.m[0] == 0
    d = dm.Demod(1, dm.AM, 0, 0.5, 0.5, [1.0], 1)
    assert d.call(z)[0][0].tolist() == [0.5, 0.5, 0.375]
    # the state carries over: one more sample of each
    assert d.call(c64(1))[0][0].tolist() == [0.25]  # u = 1 - 7/8 = 1/8, s = 3/8 + (1/8 - 3/8) / 2


def test_hand_worked_fir_and_decimation():
    """T2 = 3, R = 2, h = [1, 2, 3], gain 2, AM of 1, 3, 2, 4, 5 | 1, 2, 2 (real, positive: e = the sample).
    y[0] = h0 v0 = 1; y[1] = h0 v2 + h1 v1 + h2 v0 = 2 + 6 + 3 = 11; y[2] = h0 v4 + h1 v3 + h2 v2 = 5 + 8 + 6 = 19;
    second call (g = 5, n = 3: only m = 3 has 5 <= 2 m < 8): y[3] = h0 v6 + h1 v5 + h2 v4 = 2 + 2 + 15 = 19.
    max_in = 5: cap = 3, and the second call leaves two zero entries."""
    d = dm.Demod(1, dm.AM, 0, 0, 0, [1, 2, 3], 2, gain=2.0, max_in=5)
    out, n = d.call(c64(1, 3, 2, 4, 5))
    assert n == 3 and out[0].tolist() == [2.0, 22.0, 38.0]
    out, n = d.call(c64(1, 2, 2))
    assert n == 1 and out.shape == (1, 3) and out[0].tolist() == [38.0, 0.0, 0.0]
    assert d.g == 8 and d.hist[0].tolist() == [2.0, 2.0]
    # n = 0: no outputs, nothing moves
    out, n = d.call(np.zeros((1, 0), np.complex64))
    assert n == 0 and out.shape == (1, 3) and not out.any() and d.g == 8 and d.hist[0].tolist() == [2.0, 2.0]


def test_s16_clamps_and_rounds_ties_to_even():
    q = lambda v: dm.quantise(np.array(v, np.float32), dm.OUT_S16).tolist()  # noqa: E731
    assert q([2.0, 1.0, -1.0, -7.5, 0.0, -0.0, 1e-30]) == [32767, 32767, -32767, -32767, 0, 0, 0]
    # 0.5 * 32767 = 16383.5 exactly: the tie goes to the even 16384, and so does its negative
    assert q([0.5, -0.5]) == [16384, -16384]
    # every float whose product with 32767.0f is a tie k + 1/2: k even stays, k odd goes up
    o = (np.arange(1, 1 << 16, dtype=np.float32) / f32(1 << 16))
    prod = o * f32(32767)
    ties = prod[(prod - np.floor(prod)) == 0.5]
    even = np.floor(ties) % 2 == 0
    assert even.any() and (~even).any()
    got = dm.quantise(o, dm.OUT_S16)[(prod - np.floor(prod)) == 0.5]
    assert np.array_equal(got, np.where(even, np.floor(ties), np.floor(ties) + 1).astype(np.int16))
    assert np.array_equal(got, np.array([round(float(t)) for t in ties], np.int16))  # Python's round is ties-to-even
    d = dm.Demod(1, dm.AM, 0, 0, 0, [1.0], 1, gain=0.5, out_format=dm.OUT_S16)
    out, n = d.call(c64(1, 3, 0.5, 4j))
    assert out.dtype == np.int16 and out[0].tolist() == [16384, 32767, 8192, 32767]
    assert dm.quantise(np.array([0.3], np.float32), dm.OUT_F32).dtype == np.float32


@pytest.mark.parametrize("mode,out_format", [(dm.FM, dm.OUT_F32), (dm.AM, dm.OUT_F32), (dm.FM, dm.OUT_S16)])
def test_continuity_over_any_cut(S, mode, out_format):
    """One call of 1000 samples equals calls of 1, 0, 7, 250, 1, 0 and 741, byte for byte, and n_out follows
    ceil((g + n) / R) - ceil(g / R)."""
    B, R, T2 = 3, 8, 63
    cfg = dict(OK, mode=mode, audio_decimation=R, audio_taps=T2, out_format=out_format, gain=0.3)
    des = S.demod_design(**cfg)
    chan = dm.noise(B, 1000, seed=5)
    make = lambda: dm.Demod(B, mode, des["kf"], des["alpha"], des["a"], des["taps"], R, cfg["gain"], out_format)  # noqa
    whole, n_whole = make().call(chan)
    assert n_whole == 125 and whole.dtype == dm.OUT_DTYPE[out_format] and np.abs(whole.astype(np.float64)).max() > 0
    d = make()
    parts, at = [], 0
    for n in (1, 0, 7, 250, 1, 0, 741):
        out, n_out = d.call(chan[:, at:at + n])
        assert n_out == -(-(at + n) // R) - -(-at // R) and out.shape == (B, -(-n // R))
        assert not out[:, n_out:].any()
        parts.append(out[:, :n_out])
        at += n
    assert at == 1000 and d.g == 1000
    assert np.concatenate(parts, axis=1).tobytes() == whole.tobytes()


@pytest.mark.parametrize("fc,dev,f_mod,beta,dc,de,R,T2", [
    (200_000.0, 75_000.0, 1000.0, 2.0, 20.0, 75.0, 4, 127),       # broadcast FM behind D = 10
    (2_000_000 / 41, 5000.0, 1000.0, 5.0, 300.0, 0.0, 1, 1),      # narrow-band FM behind D = 41
    (2_000_000 / 41, 5000.0, 400.0, 7.5, 0.0, 50.0, 6, 63)])
def test_fm_tone_within_the_error_budget(S, fc, dev, f_mod, beta, dc, de, R, T2):
    """A tone of modulation index beta <= pi fc / (4 deviation), its phase integrated in float64 and the samples rounded
    to CF32; the float audio against the float64 model of the same pipeline on the same samples, within
    demod_cases.error_bound."""
    assert beta <= np.pi * fc / (4 * dev)
    B, n, gain = 4, 6000, 0.8
    cfg = dict(OK, channel_rate_hz=fc, deviation_hz=dev, dc_cutoff_hz=dc, deemphasis_us=de, audio_decimation=R,
               audio_taps=T2, audio_cutoff_hz=min(fc / 2, 0.4 * fc / R), gain=gain)
    des = S.demod_design(**cfg)
    chan = dm.fm_tone(B, n, fc, f_mod, beta, amp=0.5, carrier_hz=0.01 * fc)
    d = dm.Demod(B, dm.FM, des["kf"], des["alpha"], des["a"], des["taps"], R, gain)
    parts, at = [], 0
    for m in (2500, 3500):
        out, n_out = d.call(chan[:, at:at + m])
        parts.append(out[:, :n_out])
        at += m
    got = np.concatenate(parts, axis=1).astype(np.float64)
    want, e = dm.model_f64(dm.FM, chan, des["kf"], des["alpha"], des["a"], des["taps"], R, gain)
    assert got.shape == want.shape and np.abs(want).max() > 0.01
    bound = dm.error_bound(des["alpha"], des["a"], des["taps"], gain, des["kf"], np.abs(e).max() * 1.001)
    err = np.abs(got - want).max()
    print(f"fc {fc:.0f} dev {dev:.0f} R {R} T2 {T2}: max error {err:.3g}, bound {bound:.3g}, max |audio| "
          f"{np.abs(want).max():.3g}")
    assert err <= bound
    # what comes out is the tone: past the transients the strongest bin of stream B - 1's audio is f_mod's
    y = got[-1, -(1024 // R):]
    spec = np.abs(np.fft.rfft((y - y.mean()) * np.hanning(y.size)))
    assert abs(int(np.argmax(spec)) - f_mod / (fc / R) * y.size) <= 1


def test_am_envelope_and_dc_block(S):
    """A carrier 0.4 (1 + 0.5 cos(2 pi 500 t)) e^{j theta}, theta a 3 kHz rotation, at fc = 48 kHz.  Without the DC
    block e is the envelope: hypot of the two float components within 2.5 ulp (two products, a sum, a root: half an
    ulp each, the first three halved by the root).  With it (200 Hz: alpha = 0.0258, forgetting 2000 samples to
    0.974^2000 < 1e-22) u over whole periods of the modulation has the mean (m_end - m_start) / (alpha n), zero for a
    periodic m up to the roundings of m, u E (2 + 1 / alpha) of demod_cases.error_bound, so |mean| <= 1e-5 E."""
    fc, n = 48_000.0, 6000
    i = np.arange(n, dtype=np.float64)
    env = 0.4 * (1 + 0.5 * np.cos(2 * np.pi * 500.0 * i / fc))
    chan = (env * np.exp(2j * np.pi * 3000.0 * i / fc))[None, :].astype(np.complex64)
    cfg = dict(OK, mode=dm.AM, channel_rate_hz=fc, dc_cutoff_hz=0.0, deemphasis_us=0.0, audio_decimation=1, audio_taps=1,
               audio_cutoff_hz=fc / 2, gain=1.0)
    des = S.demod_design(**cfg)
    out, n_out = dm.Demod(1, dm.AM, des["kf"], des["alpha"], des["a"], des["taps"], 1).call(chan)
    exact = np.hypot(chan.real.astype(np.float64), chan.imag.astype(np.float64))
    assert n_out == n and np.all(np.abs(out - exact) <= 2.5 * np.spacing(exact.astype(np.float32)))
    assert np.abs(out[0] - env).max() <= 4 * 2.0 ** -24 * 0.6 + 2.5 * 2.0 ** -24  # the components' own rounding
    des = S.demod_design(**dict(cfg, dc_cutoff_hz=200.0))
    assert des["alpha"] != 0
    u, _ = dm.Demod(1, dm.AM, des["kf"], des["alpha"], des["a"], des["taps"], 1).call(chan)
    settled = u[0, 2016:5952].astype(np.float64)  # 41 periods of 96 samples
    assert abs(settled.mean()) <= 1e-5 * 0.6 and abs(out[0, 2016:5952].mean() - 0.4) < 1e-5
    assert np.ptp(settled) > 0.3  # the modulation itself passes
