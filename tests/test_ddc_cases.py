"""CPU tests of the DDC stage: its NumPy restatement (tests/ddc_cases.py) on hand-worked streams, its continuity over
calls of any length, its accuracy against a float64 model within a derived bound, the tuning, the tap design and the
boundary (the header declares the entry points, the library and sdrg.EXPORTS carry them, sdrg_nco_tables).  No device is
touched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import ddc_cases as dd

f32 = np.float32
FS = 2_000_000
NEW_SYMBOLS = ("sdrg_engine_set_ddc", "sdrg_engine_get_ddc", "sdrg_engine_ddc_reset", "sdrg_engine_ddc_max_out",
               "sdrg_engine_ddc_device", "sdrg_engine_ddc_host", "sdrg_ddc_design", "sdrg_nco_tables",
               "sdrg_ddc_tile_outputs")


@pytest.fixture(scope="module")
def S():
    import sdrg
    return sdrg


@pytest.fixture(scope="module")
def tab(S):
    return S.nco_tables()


def cf32(z):
    z = np.asarray(z, np.complex64)
    return z.view(np.float32).reshape(1, -1)


def test_hand_worked_stream(tab):
    """T = 3, D = 2, inc = 0, h = [1, 2, 3], x = 1+2j, 3-j, -2, 4+4j, 5-3j | 1+j, -2j, 2.
    y[0] = h0 x0 = 1+2j;  y[1] = h0 x2 + h1 x1 + h2 x0 = -2 + (6-2j) + (3+6j) = 7+4j;
    y[2] = h0 x4 + h1 x3 + h2 x2 = (5-3j) + (8+8j) - 6 = 7+5j;  second call (g0 = 5, N = 3: only m = 3 has 5 <= 2m < 8):
    y[3] = h0 x6 + h1 x5 + h2 x4 = -2j + (2+2j) + (15-9j) = 17-9j, and cap = 2 leaves one zero entry."""
    d = dd.Ddc(1, [1, 2, 3], tab, 0, 2)
    out, n = d.call(dd.CF32, cf32([1 + 2j, 3 - 1j, -2, 4 + 4j, 5 - 3j]))
    assert n == 3 and out.shape == (1, 3) and out[0].tolist() == [1 + 2j, 7 + 4j, 7 + 5j]
    out, n = d.call(dd.CF32, cf32([1 + 1j, -2j, 2]))
    assert n == 1 and out.shape == (1, 2) and out[0].tolist() == [17 - 9j, 0]
    assert d.g0 == 8 and d.hr[0].tolist() == [0, 2] and d.hi[0].tolist() == [-2, 0]


def test_one_tap_no_decimation_returns_the_input(tab):
    x = dd.noise(dd.CF32, 2, 37, seed=3)
    d = dd.Ddc(2, [1.0], tab, 0, 1)
    out, n = d.call(dd.CF32, x)
    assert n == 37 and out.view(np.float32).reshape(2, -1).tobytes() == x.tobytes()  # hi[0] lo[0] = 1 exactly
    raw = dd.noise(dd.CS16, 1, 9, seed=4)
    out, n = dd.Ddc(1, [1.0], tab, 0, 1).call(dd.CS16, raw)
    assert np.array_equal(out[0].real, raw[0, 0::2] / 32768.0) and np.array_equal(out[0].imag, raw[0, 1::2] / 32768.0)


def test_unpack_conventions():
    xr, xi = dd.unpack(dd.CU8, np.array([[0, 255, 127, 128]], np.uint8))
    assert xr.dtype == np.float32
    assert xr[0].tolist() == [float((f32(0) - f32(127.4)) * f32(1 / 128)), float((f32(127) - f32(127.4)) * f32(1 / 128))]
    assert xi[0].tolist() == [float((f32(255) - f32(127.4)) * f32(1 / 128)), float((f32(128) - f32(127.4)) * f32(1 / 128))]
    xr, xi = dd.unpack(dd.CS8, np.array([[-128, 127]], np.int8))
    assert (xr[0, 0], xi[0, 0]) == (-1.0, 127 / 128)
    xr, xi = dd.unpack(dd.CS16, np.array([[-32768, 1]], np.int16))
    assert (xr[0, 0], xi[0, 0]) == (-1.0, 1 / 32768)


@pytest.mark.parametrize("fmt", [dd.CS8, dd.CF32])
def test_continuity_over_any_cut(S, tab, fmt):
    """One call of 1000 samples equals calls of 1, 7, 250 and 742, byte for byte and in n_out."""
    B, T, D = 2, 63, 8
    h = S.ddc_design(FS, cutoff_hz=100e3, decimation=D, taps=T)
    inc = dd.nco_increment(-312_500.0, FS)
    raw = dd.noise(fmt, B, 1000, seed=5)
    whole, n_whole = dd.Ddc(B, h, tab, inc, D).call(fmt, raw)
    assert n_whole == 125
    d = dd.Ddc(B, h, tab, inc, D)
    parts, at = [], 0
    for n in (1, 7, 250, 742):
        out, n_out = d.call(fmt, raw[:, 2 * at:2 * (at + n)])
        assert n_out == dd.n_out_for(at, n, D) and out.shape == (B, -(-n // D))
        assert not out[:, n_out:].view(np.uint32).any()
        parts.append(out[:, :n_out])
        at += n
    assert np.concatenate(parts, axis=1).tobytes() == whole.tobytes()


def test_n_out_follows_the_formula(tab):
    d = dd.Ddc(1, [1.0], tab, 0, 41)
    got = [d.call(dd.CS8, np.zeros((1, 2 * 16384), np.int8))[1] for _ in range(41)]
    assert set(got) == {399, 400} and sum(got) == 16384 and got[:3] == [400, 400, 399]
    assert got == [-(-(16384 * (i + 1)) // 41) - -(-(16384 * i) // 41) for i in range(41)]
    d = dd.Ddc(1, [1.0], tab, 0, 512)
    got = [d.call(dd.CS8, np.zeros((1, 200), np.int8))[1] for _ in range(128)]
    assert got[0] == 1 and sum(got) == 25 and got.count(0) == 103 and max(got) == 1


@pytest.mark.parametrize("fmt,T,D,offset", [(dd.CS8, 63, 8, 250_000.0), (dd.CU8, 255, 41, -700_123.0),
                                            (dd.CS16, 511, 3, 999_999.0), (dd.CF32, 127, 16, 1234.5)])
def test_accuracy_against_the_float64_model(S, tab, fmt, T, D, offset):
    """|err| <= (1.3e-5 + (T + 3) 2^-24) max|x| sum|h| per component: 1.2e-5 for the two-level phasor plus
    the mix's four products and two sums, then one rounding per product and per sum of the T taps."""
    B, n = 2, 6000
    h = S.ddc_design(FS, offset_hz=offset, cutoff_hz=FS / (2.5 * D), decimation=D, taps=T)
    inc = dd.nco_increment(offset, FS)
    raw = dd.noise(fmt, B, n, seed=7)
    d = dd.Ddc(B, h, tab, inc, D)
    parts, at = [], 0
    for m in (2500, 3500):
        out, n_out = d.call(fmt, raw[:, 2 * at:2 * (at + m)])
        parts.append(out[:, :n_out])
        at += m
    got = np.concatenate(parts, axis=1)
    want = dd.model_f64(fmt, raw, h, inc, D)
    xr, xi = dd.unpack(fmt, raw)
    bound = dd.error_bound(T, np.hypot(xr.astype(np.float64), xi.astype(np.float64)).max(), h)
    assert got.shape == want.shape
    err = max(np.abs(got.real - want.real).max(), np.abs(got.imag - want.imag).max())
    print(f"fmt {fmt} T {T} D {D}: max error {err:.3g}, bound {bound:.3g}")
    assert err <= bound


def test_tuning_passband_and_stopband(S, tab):
    """A tone at offset + f1 comes out at f1 with the gain H(f1), one outside the passband at the level |H| the taps
    have there (computed in double from the library's taps): no fixed dB figure.  The input is CF32, whose rounding of
    the tone adds at most 2^-24 max|x| sum|h| to the bound."""
    T, D, n, amp = 255, 16, 16384, 0.5
    offset, cutoff = 300_000.0, 40_000.0
    h = S.ddc_design(FS, offset_hz=offset, cutoff_hz=cutoff, decimation=D, taps=T)
    inc = dd.nco_increment(offset, FS)
    bound = dd.error_bound(T, amp, h) + 2.0 ** -24 * amp * np.abs(h.astype(np.float64)).sum()
    m = np.arange(-(-n // D))
    settled = m * D >= T - 1
    for f1 in (12_500.0, -30_000.0, 90_000.0, 400_000.0):
        f_in = (offset + f1) / FS
        raw = dd.tone(dd.CF32, 1, n, f_in, amp)
        out, n_out = dd.Ddc(1, h, tab, inc, D).call(dd.CF32, raw)
        assert n_out == m.size
        f_res = f_in - inc / 2.0 ** 32  # what the NCO leaves, cycles per input sample (inc is a rounded offset)
        assert abs(f_res * FS - f1) <= FS * 2.0 ** -33
        # y[m] = sum_k h[k] A e^{j 2 pi f_res (m D - k)} = A H(f_res) e^{j 2 pi f_res m D}
        want = amp * dd.response(h, f_res) * np.exp(2j * np.pi * f_res * D * m)
        err = np.abs(np.stack([out[0].real - want.real, out[0].imag - want.imag]))[:, settled].max()
        gain = abs(dd.response(h, f_res))
        print(f"f1 {f1}: |H| {gain:.3g}, max error {err:.3g}, bound {bound:.3g}")
        assert err <= bound
        if abs(f1) < cutoff:  # inside the passband: the output's strongest bin is f1's
            spec = np.abs(np.fft.fft(out[0][settled][:512]))
            assert int(np.argmax(spec)) == int(round(f1 / (FS / D) * 512)) % 512
        else:
            assert abs(np.abs(out[0][settled]).max() - amp * gain) <= bound * np.sqrt(2)


def test_design(S):
    for fs, cutoff, T in ((FS, 40_000.0, 255), (FS, FS / 2, 63), (48_000, 1.0, 511), (2_400_000, 100e3, 1), (FS, 3e5, 3)):
        h = S.ddc_design(fs, offset_hz=1e3, cutoff_hz=cutoff, decimation=4, taps=T)
        assert h.dtype == np.float32 and h.shape == (T,)
        assert h.tobytes() == h[::-1].tobytes()
        assert abs(h.astype(np.float64).sum() - 1.0) <= T * 2.0 ** -24
        assert np.abs(h - dd.taps_formula(fs, cutoff, T)).max() <= 1e-7
    assert S.ddc_design(FS, cutoff_hz=1e5, decimation=1, taps=1).tolist() == [1.0]


def test_design_refuses_invalid_configurations(S):
    ok = dict(offset_hz=1e5, cutoff_hz=1e5, decimation=8, taps=63)
    S.ddc_design(FS, **ok)
    bad = [dict(offset_hz=float("nan")), dict(offset_hz=float("inf")), dict(offset_hz=-float("inf")),
           dict(decimation=0), dict(decimation=-1), dict(decimation=513), dict(taps=0), dict(taps=-3), dict(taps=62),
           dict(taps=512), dict(taps=513), dict(cutoff_hz=0.0), dict(cutoff_hz=-1.0), dict(cutoff_hz=FS / 2 + 1),
           dict(cutoff_hz=float("nan")), dict(cutoff_hz=float("inf"))]
    for b in bad:
        cfg = dict(ok, **b)
        assert not dd.valid_config(FS, cfg["offset_hz"], cfg["cutoff_hz"], cfg["decimation"], cfg["taps"])
        with pytest.raises(S.SdrgError) as ei:
            S.ddc_design(FS, **cfg)
        assert "SDRG_E_INVALID" in str(ei.value), b
    S.ddc_design(FS, **dict(ok, cutoff_hz=FS / 2, decimation=512, taps=511))
    L = S.load()
    c = S.DdcConfig(1e5, 1e5, 8, 63)
    buf = (ctypes.c_float * 63)()
    assert L.sdrg_ddc_design(FS, None, buf) == -1 and L.sdrg_ddc_design(FS, ctypes.byref(c), None) == -1
    assert L.sdrg_ddc_design(0, ctypes.byref(c), buf) == -1 and L.sdrg_ddc_design(FS, ctypes.byref(c), buf) == 0


def test_nco_increment_restated(S):
    for hz, fs in ((250_000.0, FS), (-250_000.0, FS), (0.0, FS), (1.0, 48_000), (-999_999.5, 2_400_000), (3e6, FS)):
        inc = dd.nco_increment(hz, fs)
        assert 0 <= inc < 2 ** 32
        assert abs(((inc / 2.0 ** 32 - hz / fs + 0.5) % 1.0) - 0.5) <= 2.0 ** -33
    assert dd.nco_increment(500_000.0, FS) == 1 << 30 and dd.nco_increment(-500_000.0, FS) == 3 << 30


def test_header_library_and_mirror_carry_the_stage(S, tab):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sdrg.h")).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", S.lib_path()], capture_output=True, text=True, check=True).stdout
    L = S.load()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert re.search(r"\bT %s$" % s, nm, flags=re.M), s
        assert s in S.EXPORTS and hasattr(L, s)
    for s in ("sdrg_ddc_config", "#define SDRG_DDC_MAX_TAPS 511", "#define SDRG_DDC_MAX_DECIMATION 512"):
        assert s in text
    assert L.sdrg_abi_version() == 1
    assert ctypes.sizeof(S.DdcConfig) == 24
    assert (S.DDC_MAX_TAPS, S.DDC_MAX_DECIMATION) == (dd.MAX_TAPS, dd.MAX_DECIMATION)
    # the phasor tables: the stated formula within 1 ulp of float
    want = dd.tables_formula()
    assert tab.shape == (2, 1024, 2) and tab.dtype == np.float32
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(tab.astype(np.float64) - want) <= ulp)
    assert tab[0, 0].tolist() == [1.0, 0.0] and tab[1, 0].tolist() == [1.0, 0.0]
    assert L.sdrg_nco_tables(None) == -1
    # the launcher's tile: at least one output, at most a workgroup's lanes, and its window fits the LDS samples
    for D in (1, 2, 3, 41, 64, 512):
        for T in (1, 3, 255, 511):
            tile = S.ddc_tile_outputs(D, T)
            assert 1 <= tile <= 256 and (tile - 1) * D + T <= 3072
    assert L.sdrg_ddc_tile_outputs(0, 3, ctypes.byref(ctypes.c_int32())) == -1
