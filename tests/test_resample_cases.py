"""CPU tests of the resampler stage: its NumPy restatement (tests/resample_cases.py) on hand-worked streams, its
continuity over calls of any length, the float32 sums against a float64 model within the derived error bound, a tone
through 123 / 125 against the ideal delayed tone, the int16 quantisation, the host-side design, sdrg_resample_ratio and
the boundary (the header declares the entry points, the library and sdrg.EXPORTS carry them).  No device is touched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import resample_cases as rs

f32 = np.float32
NEW_SYMBOLS = ("sdrg_resample_design", "sdrg_resample_tile_outputs", "sdrg_resample_ratio", "sdrg_engine_set_resample",
               "sdrg_engine_get_resample", "sdrg_engine_resample_reset", "sdrg_engine_resample_max_out",
               "sdrg_engine_resample_device", "sdrg_engine_resample_host", "sdrg_engine_ddc_demod_resample_host")
OK = dict(interp=123, decim=125, taps_per_phase=16, cutoff_rel=0.9, components=1, out_format=rs.OUT_F32, gain=0.5,
          max_in=1639)


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
    for s in ("sdrg_resample_config", "#define SDRG_RESAMPLE_OUT_S16 0", "#define SDRG_RESAMPLE_OUT_F32 1",
              "#define SDRG_RESAMPLE_MAX_FACTOR 512", "#define SDRG_RESAMPLE_MAX_TAPS_PER_PHASE 64",
              "#define SDRG_RESAMPLE_MAX_TAPS 8192", "#define SDRG_RESAMPLE_MAX_IN 1048576"):
        assert s in text
    assert L.sdrg_abi_version() == 1
    assert ctypes.sizeof(S.ResampleConfig) == 40
    assert (S.RESAMPLE_OUT_S16, S.RESAMPLE_OUT_F32) == (rs.OUT_S16, rs.OUT_F32)
    assert (S.RESAMPLE_MAX_FACTOR, S.RESAMPLE_MAX_TAPS_PER_PHASE, S.RESAMPLE_MAX_TAPS, S.RESAMPLE_MAX_IN) == \
        (rs.MAX_FACTOR, rs.MAX_TAPS_PER_PHASE, rs.MAX_TAPS, rs.MAX_IN)
    # the tile: at least one output and at most a workgroup's lanes
    for L_, M_, P_ in ((1, 1, 1), (3, 2, 8), (123, 125, 16), (512, 511, 16), (1, 8, 64), (8, 1, 4)):
        assert 1 <= S.resample_tile_outputs(**dict(OK, interp=L_, decim=M_, taps_per_phase=P_)) <= 256
    t = ctypes.c_int32()
    c = S.ResampleConfig(**OK)
    assert L.sdrg_resample_tile_outputs(None, ctypes.byref(t)) == -1
    assert L.sdrg_resample_tile_outputs(ctypes.byref(c), None) == -1
    c.interp = 125
    assert L.sdrg_resample_tile_outputs(ctypes.byref(c), ctypes.byref(t)) == -1


@pytest.mark.parametrize("L,M,P,cut", [(123, 125, 16, 0.9), (147, 160, 24, 0.8), (3, 2, 8, 1.0), (2, 3, 8, 0.5),
                                       (3, 2, 7, 0.9), (512, 511, 16, 0.9), (8, 1, 4, 0.9), (1, 8, 64, 0.9),
                                       (7, 5, 1, 0.9), (1, 1, 2, 1.0)])
def test_design_agrees_with_the_formula(S, L, M, P, cut):
    """Within one float ulp of the stated formula (the library sums the window one by one, NumPy in pairs), for L P
    odd and even; the tail of an even prototype is +0 and the DC gain of the whole prototype is L."""
    got = S.resample_design(**dict(OK, interp=L, decim=M, taps_per_phase=P, cutoff_rel=cut))
    want = rs.design_formula(L, M, P, cut)
    n = L * P
    assert got.dtype == np.float32 and got.shape == (n,)
    assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32)).astype(np.float64))
    if n % 2 == 0:
        assert got[n - 1] == 0 and not np.signbit(got[n - 1]) and want[n - 1] == 0
    assert abs(float(got.astype(np.float64).sum()) - L) <= n * 2.0 ** -24 * float(np.abs(want).sum())
    # symmetric about (T - 1) / 2 to the last bit but one: a linear-phase low-pass
    T = n if n % 2 else n - 1
    assert np.all(np.abs(got[:T] - got[:T][::-1]) <= np.spacing(np.abs(got[:T])))


def test_design_edges(S):
    assert S.resample_design(**dict(OK, interp=1, decim=1, taps_per_phase=1)).tolist() == [1.0]
    h = S.resample_design(**dict(OK, interp=1, decim=1, taps_per_phase=2))
    assert h.tolist() == [1.0, 0.0]
    L = S.load()
    c = S.ResampleConfig(**OK)
    taps = np.zeros(123 * 16, np.float32)
    assert L.sdrg_resample_design(None, taps.ctypes.data_as(ctypes.c_void_p)) == -1
    assert L.sdrg_resample_design(ctypes.byref(c), None) == -1
    assert L.sdrg_resample_design(ctypes.byref(c), taps.ctypes.data_as(ctypes.c_void_p)) == 0
    assert taps.tobytes() == S.resample_design(**OK).tobytes()


def test_design_refuses_each_bad_field_on_its_own(S):
    S.resample_design(**OK)
    assert rs.valid_config(OK)
    nan, inf = float("nan"), float("inf")
    bad = [dict(interp=0), dict(interp=-1), dict(interp=513, decim=512), dict(decim=0), dict(decim=-3),
           dict(interp=512, decim=513), dict(interp=6, decim=4), dict(interp=246, decim=250), dict(interp=2, decim=2),
           dict(interp=9, decim=1, taps_per_phase=4), dict(interp=1, decim=9), dict(interp=17, decim=2, taps_per_phase=4),
           dict(taps_per_phase=0), dict(taps_per_phase=65), dict(taps_per_phase=-1), dict(taps_per_phase=67),
           dict(interp=511, decim=512, taps_per_phase=17), dict(interp=129, decim=128, taps_per_phase=64),
           dict(cutoff_rel=0.0), dict(cutoff_rel=-0.5), dict(cutoff_rel=1.0001), dict(cutoff_rel=nan),
           dict(cutoff_rel=inf), dict(components=0), dict(components=3), dict(out_format=2), dict(out_format=-1),
           dict(gain=nan), dict(gain=inf), dict(max_in=0), dict(max_in=(1 << 20) + 1), dict(max_in=-1)]
    for b in bad:
        cfg = dict(OK, **b)
        assert not rs.valid_config(cfg), b
        with pytest.raises(S.SdrgError) as ei:
            S.resample_design(**cfg)
        assert "SDRG_E_INVALID" in str(ei.value), b
        with pytest.raises(S.SdrgError):
            S.resample_tile_outputs(**cfg)
    # one message per rule
    msgs = set()
    for b in (dict(interp=0), dict(decim=0), dict(interp=6, decim=4), dict(interp=9, decim=1, taps_per_phase=4),
              dict(taps_per_phase=0), dict(interp=511, decim=512, taps_per_phase=17), dict(cutoff_rel=0.0),
              dict(components=0), dict(out_format=2), dict(gain=nan), dict(max_in=0)):
        with pytest.raises(S.SdrgError) as ei:
            S.resample_design(**dict(OK, **b))
        msgs.add(str(ei.value))
    assert len(msgs) == 11
    # the limits themselves
    for good in (dict(interp=512, decim=511, taps_per_phase=16), dict(interp=8, decim=1, taps_per_phase=64),
                 dict(interp=1, decim=8, taps_per_phase=64), dict(interp=128, decim=127, taps_per_phase=64),
                 dict(interp=1, decim=1, taps_per_phase=1, cutoff_rel=1.0, max_in=1, gain=-3.0, components=2,
                      out_format=rs.OUT_S16), dict(max_in=1 << 20)):
        assert rs.valid_config(dict(OK, **good)), good
        S.resample_design(**dict(OK, **good))


def test_ratio(S):
    assert S.resample_ratio(2_000_000, 41, 48_000) == (123, 125)
    assert S.resample_ratio(48_000, 1, 44_100) == (147, 160)
    assert S.resample_ratio(48_000, 1, 48_000) == (1, 1)
    assert S.resample_ratio(1, 8, 1) == (8, 1) and S.resample_ratio(8, 1, 1) == (1, 8)
    assert S.resample_ratio(200_000, 1, 48_000) == (6, 25)
    assert S.resample_ratio(1 << 62, 1 << 61, 2) == (1, 1)  # out_hz in_den passes 2^64
    for bad in ((2_500_000, 52, 48_000),   # 624 / 625: above 512
                (2_000_000, 1, 48_000),    # 3 / 125: below 1 / 8
                (1, 9, 1), (9, 1, 1), (0, 1, 48_000), (48_000, 0, 48_000), (48_000, 1, 0)):
        with pytest.raises(S.SdrgError) as ei:
            S.resample_ratio(*bad)
        assert "SDRG_E_INVALID" in str(ei.value), bad
    L = S.load()
    a, b = ctypes.c_int32(-7), ctypes.c_int32(-7)
    assert L.sdrg_resample_ratio(2_500_000, 52, 48_000, ctypes.byref(a), ctypes.byref(b)) == -1
    assert L.sdrg_resample_ratio(48_000, 1, 44_100, None, ctypes.byref(b)) == -1
    assert L.sdrg_resample_ratio(48_000, 1, 44_100, ctypes.byref(a), None) == -1
    assert (a.value, b.value) == (-7, -7)
    for bad in (-1, 1 << 64):
        with pytest.raises(S.SdrgError):
            S.resample_ratio(bad, 1, 48_000)


def test_hand_worked_3_over_2(S):
    """L = 3, M = 2, P = 2: output m reads q = floor(2 m / 3) with the phase (2 m) mod 3, y = h[phi] x[q] +
    h[phi + 3] x[q - 1]."""
    h = S.resample_design(**dict(OK, interp=3, decim=2, taps_per_phase=2, cutoff_rel=1.0))
    assert h.size == 6 and h[5] == 0
    r = rs.Resampler(1, 3, 2, h, gain=2.0)
    x = np.array([[1, 2, 4]], f32)
    out, n_out = r.call(x)
    want = [h[0] * f32(1), h[2] * f32(1), h[1] * f32(2) + h[4] * f32(1), h[0] * f32(4) + h[3] * f32(2),
            h[2] * f32(4) + h[5] * f32(2)]
    assert n_out == 5 and out.shape == (1, 5) and out[0].tolist() == [w * f32(2) for w in want]
    out, n_out = r.call(np.array([[8]], f32))  # g = 3: m in [ceil(9 / 2), ceil(12 / 2)) = {5}: q = 3, phi = 1
    assert n_out == 1 and out.shape == (1, 2) and out[0].tolist() == [(h[1] * f32(8) + h[4] * f32(4)) * f32(2), 0.0]
    assert r.g == 4 and r.hist.reshape(-1).tolist() == [8.0]


def test_hand_worked_2_over_3(S):
    """L = 2, M = 3, P = 2: q = floor(3 m / 2), phi = (3 m) mod 2; the inputs 2, 5, ... are read by the history tap
    only."""
    h = S.resample_design(**dict(OK, interp=2, decim=3, taps_per_phase=2, cutoff_rel=1.0))
    assert h.size == 4 and h[3] == 0
    r = rs.Resampler(1, 2, 3, h)
    out, n_out = r.call(np.array([[1, 2, 4, 8, 16]], f32))
    want = [h[0] * f32(1), h[1] * f32(2) + h[3] * f32(1), h[0] * f32(8) + h[2] * f32(4), h[1] * f32(16) + h[3] * f32(8)]
    assert n_out == 4 and out[0].tolist() == want
    out, n_out = r.call(np.array([[32]], f32))  # g = 5: m in [ceil(10 / 3), ceil(12 / 3)) is empty
    assert n_out == 0 and out.shape == (1, 1) and not out.any() and r.g == 6 and r.hist.reshape(-1).tolist() == [32.0]
    out, n_out = r.call(np.array([[64]], f32))  # g = 6: m = 4, q = 6, phi = 0
    assert n_out == 1 and out[0].tolist() == [h[0] * f32(64) + h[2] * f32(32)]
    # complex rows are done componentwise
    z = np.array([[1 + 10j, 2 + 20j, 4 + 40j, 8 + 80j, 16 + 160j]], np.complex64)
    out, n_out = rs.Resampler(1, 2, 3, h, components=2).call(z)
    assert out.shape == (1, 4, 2) and out[0, :, 0].tolist() == want
    assert out[0, 3, 1] == h[1] * f32(160) + h[3] * f32(80)


@pytest.mark.parametrize("components,out_format", [(1, rs.OUT_F32), (2, rs.OUT_F32), (1, rs.OUT_S16), (2, rs.OUT_S16)])
@pytest.mark.parametrize("L,M,P", [(3, 2, 8), (2, 3, 8), (7, 5, 1), (8, 1, 4), (1, 8, 16)])
def test_continuity_over_any_cut(S, L, M, P, components, out_format):
    """A stream cut in two anywhere, with n = 0 and n = 1 pieces in between, and cut into single samples, equals one
    call byte for byte."""
    B, n = 2, 41
    h = S.resample_design(**dict(OK, interp=L, decim=M, taps_per_phase=P))
    x = rs.noise(B, n, seed=L * 100 + M, components=components)
    kw = dict(gain=1.3, out_format=out_format, components=components)
    whole, n_whole = rs.Resampler(B, L, M, h, **kw).call(x)
    whole = whole[:, :n_whole]
    assert n_whole == rs.ceil_div(n * L, M)

    def run(cuts):
        r, parts, at = rs.Resampler(B, L, M, h, **kw), [], 0
        for c in list(cuts) + [n]:
            out, n_out = r.call(x[:, at:c])
            assert not out[:, n_out:].any()
            parts.append(out[:, :n_out])
            at = c
        assert r.g == n
        return np.concatenate(parts, axis=1)

    for a in range(n + 1):
        assert run([a]).tobytes() == whole.tobytes(), a
        assert run([a, a, min(a + 1, n)]).tobytes() == whole.tobytes(), a
    assert run(range(1, n)).tobytes() == whole.tobytes()


@pytest.mark.parametrize("L,M,P,components", [(123, 125, 16, 1), (147, 160, 24, 1), (3, 2, 8, 2), (2, 3, 8, 2),
                                              (1, 8, 64, 1), (512, 511, 16, 1)])
def test_restatement_within_the_error_bound(S, L, M, P, components):
    B, n, gain = 3, 1500, 0.7
    h = S.resample_design(**dict(OK, interp=L, decim=M, taps_per_phase=P))
    x = rs.noise(B, n, seed=7, components=components)
    out, n_out = rs.Resampler(B, L, M, h, gain=gain, components=components).call(x)
    y, s = rs.model_f64(x, L, M, h, gain=f32(gain), components=components)
    assert y.shape[1] == n_out
    x_max = float(np.abs(rs.as_rows(x, B, components)).max())
    bound = rs.error_bound(P, s, x_max, f32(gain))
    err = np.abs(out[:, :n_out].reshape(y.shape).astype(np.float64) - y)
    assert np.all(err <= bound[None, :, None]), float((err / bound[None, :, None]).max())
    assert err.max() > 0 and np.abs(y).max() > 0.1


def test_tone_at_48000_hz(S):
    """A 1 kHz tone at 2 000 000 / 41 Hz through 123 / 125 (P = 16, cutoff_rel 0.9) against the ideal tone at 48 000
    Hz, delayed by the group delay (T - 1) / 2 upsampled samples, after the first P outputs.  The error stays within
    the prototype's passband deviation (|H(f) / L - 1| up to the tone) plus its worst stopband gain, both from the
    float64 frequency response of the library's taps.  The stopband starts where the Hann window's main lobe has left
    the cutoff, at f_c + 2 / (T + 1) cycles per upsampled sample (its first side lobe is the worst, about -44 dB),
    and every image of the tone, k / L +- f0, lies in it."""
    L, M, P, amp = 123, 125, 16, 0.8
    fs_in, f0, n = 2_000_000 / 41, 1000.0, 6000
    assert S.resample_ratio(2_000_000, 41, 48_000) == (L, M)
    h = S.resample_design(**dict(OK, interp=L, decim=M, taps_per_phase=P, cutoff_rel=0.9))
    T = L * P - 1
    i = np.arange(n, dtype=np.float64)
    x = np.stack([amp * np.sin(2 * np.pi * f0 * i / fs_in + ph) for ph in (0.0, 1.1)]).astype(np.float32)
    out, n_out = rs.Resampler(2, L, M, h).call(x)
    assert n_out == rs.ceil_div(n * L, M)
    m = np.arange(n_out, dtype=np.float64)
    t_in = (m * M - (T - 1) / 2.0) / L  # the output's time in input samples
    ideal = np.stack([amp * np.sin(2 * np.pi * f0 * t_in / fs_in + ph) for ph in (0.0, 1.1)])
    assert abs(48_000.0 * M / L - fs_in) < 1e-9
    fu = f0 / (fs_in * L)  # the tone, in cycles per upsampled sample
    f_pass = np.linspace(0.0, fu, 65)
    passband = float(np.abs(rs.response(h, f_pass) * np.exp(2j * np.pi * f_pass * (T - 1) / 2.0) / L - 1.0).max())
    edge = 0.9 / (2.0 * M) + 2.0 / (T + 1)
    assert edge < 1.0 / L - fu
    f_stop = np.linspace(edge, 0.5, 20001)
    stopband = float(np.abs(rs.response(h, f_stop)).max()) / L
    err =float(np.abs(out[:, P:n_out].astype(np.float64) - ideal[:, P:]).max())
    print(f"tone error {err:.3e}, passband deviation {passband:.3e}, stopband gain {stopband:.3e} "
          f"({20 * np.log10(stopband):.1f} dB)")
    assert stopband < 10 ** (-40 / 20) and passband < 1e-3
    assert err <= amp * (passband + stopband)


def test_s16_clamps_and_rounds_ties_to_even(S):
    """(int16) rintf(min(max(o, -1), 1) * 32767): through the identity resampler (1, 1, 1), h = [1.0]."""
    h = S.resample_design(**dict(OK, interp=1, decim=1, taps_per_phase=1))
    assert h.tolist() == [1.0]
    half = [f32((k + 0.5) / 32767.0) for k in (0, 1, 2, 3, 100, 101)]
    x = np.array([[0.0, 1.0, -1.0, 1.5, -1.5, 1e9, -1e9, 0.5, -0.5, 1e-9, -1e-9] + half + [-v for v in half]], f32)
    out, n_out = rs.Resampler(1, 1, 1, h, out_format=rs.OUT_S16).call(x)
    assert out.dtype == np.int16 and n_out == x.size
    want = np.rint(np.clip(x, -1, 1) * f32(32767)).astype(np.int16)
    assert out.tolist() == want.tolist()
    assert out[0, :7].tolist() == [0, 32767, -32767, 32767, -32767, 32767, -32767]
    assert out[0, 7:11].tolist() == [16384, -16384, 0, 0]  # 16383.5 rounds to the even 16384
    ties = x[0, 11:17] * f32(32767)
    for k, (v, o) in zip((0, 1, 2, 3, 100, 101), zip(ties, out[0, 11:17])):
        if v == f32(k + 0.5):  # an exact tie in float: to the even neighbour
            assert o == (k if k % 2 == 0 else k + 1), (k, v, o)
    # the gain comes before the clamp
    out, _ = rs.Resampler(1, 1, 1, h, gain=4.0, out_format=rs.OUT_S16).call(np.array([[0.25, 0.3, -0.125]], f32))
    assert out[0].tolist() == [32767, 32767, -16384]


class Library:
    """A stand-in for libsdrg.so: every function returns 0 and is listed in `calls`."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def test_wrapper_argument_checks(S, monkeypatch):
    fake = Library()
    monkeypatch.setattr(S, "load", lambda: fake)
    eng = S.Engine.__new__(S.Engine)
    eng._h, eng._cbs, eng.n_streams, eng.cfg = None, None, 3, S.SDRConfig(samplesPerReading=8)
    for fn in (S.resample_design, S.resample_tile_outputs, eng.set_resample):
        with pytest.raises(TypeError) as ei:
            fn(x=1)
        assert str(ei.value) == "unknown resample field 'x'"
    with pytest.raises(TypeError) as ei:
        eng.set_resample(off=True, interp=3)
    assert str(ei.value) == "off=True takes no other field"
    for bad in ((-1, 1, 1), (1, 1 << 64, 1), (1, 1, -5)):
        with pytest.raises(S.SdrgError):
            S.resample_ratio(*bad)
    assert fake.calls == []
    eng.set_resample(off=True)
    assert fake.calls == [("sdrg_engine_set_resample", (None, None))]
    fake.calls.clear()
    eng.set_resample(interp=3, decim=2, taps_per_phase=8, gain=0.5)
    (name, (_, ref)), = fake.calls
    c = ref._obj
    assert name == "sdrg_engine_set_resample" and type(c) is S.ResampleConfig
    assert (c.interp, c.decim, c.taps_per_phase, c.gain, c.cutoff_rel, c.components, c.max_in) == (3, 2, 8, 0.5, 0, 0, 0)
    fake.calls.clear()
    with pytest.raises(S.SdrgError):  # 7 values are no rows of 3 streams
        eng.resample_host(np.zeros(7, f32))
    with pytest.raises(S.SdrgError):  # iq of the wrong size
        eng.ddc_demod_resample_host(np.zeros((3, 15), np.int8))
    assert [c[0] for c in fake.calls if "host" in c[0]] == []
