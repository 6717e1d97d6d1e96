"""CPU tests of the channelizer stage: the boundary (the header declares the entry points and constants, the library and
sdrg.EXPORTS carry them), the prototype design and its refusals, and the NumPy restatement (tests/channelizer_cases.py):
its accuracy against the float64 model within the derived bound, its equivalence with the DDC restatement, tones, the
(-1)^{c m} rule, n_out and the invariance under any cut of the stream, and the span of rows.  No device is touched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import channelizer_cases as cc
import ddc_cases as dd

FS = 2_000_000
NEW_SYMBOLS = ("sdrg_channelizer_design", "sdrg_channelizer_tile_outputs", "sdrg_engine_set_channelizer",
               "sdrg_engine_get_channelizer", "sdrg_engine_channelizer_reset", "sdrg_engine_channelizer_max_out",
               "sdrg_engine_channelizer_device", "sdrg_engine_channelizer_host")
SHAPES = [(4, 3, 2), (8, 1, 1), (16, 8, 1), (64, 8, 2), (256, 16, 1), (256, 16, 2), (32, 32, 2)]  # (M, P, O)
GOOD = dict(cutoff_rel=0.5, channels=16, taps_per_channel=8, oversample=1, first_channel=0, n_channels=16)


@pytest.fixture(scope="module")
def S():
    import sdrg
    return sdrg


def design(S, M, P, cutoff_rel=0.5):
    return S.channelizer_design(cutoff_rel=cutoff_rel, channels=M, taps_per_channel=P, oversample=1, first_channel=0,
                                n_channels=M)


def close_to_formula(h, want):
    """The double formula rounded to float: half an ulp of each tap, plus what two libms may differ by in double."""
    return bool(np.all(np.abs(h.astype(np.float64) - want) <= 2.0 ** -24 * np.abs(want) + 1e-13))


def invalid(S, fn, *a, **k):
    with pytest.raises(S.SdrgError) as ei:
        fn(*a, **k)
    assert "SDRG_E_INVALID" in str(ei.value)


def test_header_library_and_exports_carry_the_stage(S):
    text = open(os.path.join(ROOT, "include", "sdrg.h")).read()
    for name, value in (("SDRG_CHANNELIZER_MAX_CHANNELS", 256), ("SDRG_CHANNELIZER_MAX_TAPS_PER_CHANNEL", 32),
                        ("SDRG_CHANNELIZER_MAX_TAPS", 4096)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", text), name
    assert (S.CHANNELIZER_MAX_CHANNELS, S.CHANNELIZER_MAX_TAPS_PER_CHANNEL, S.CHANNELIZER_MAX_TAPS) == (256, 32, 4096)
    assert "typedef struct sdrg_channelizer_config" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", S.lib_path()], capture_output=True, text=True, check=True).stdout
    L = S.load()
    for s in NEW_SYMBOLS:
        assert re.search(rf"\b{s}\s*\(", code), s
        assert s in S.EXPORTS and re.search(rf"\bT {s}$", nm, flags=re.M) and hasattr(L, s), s
    assert ctypes.sizeof(S.ChannelizerConfig) == 32
    assert [k for k, _ in S.ChannelizerConfig._fields_] == ["cutoff_rel", "channels", "taps_per_channel", "oversample",
                                                           "first_channel", "n_channels"]


@pytest.mark.parametrize("M,P", [(16, 8), (64, 8)])
def test_design_is_the_ddc_design_plus_a_zero(S, M, P):
    L = M * P
    h = design(S, M, P)
    ddc = S.ddc_design(FS, cutoff_hz=0.5 * FS / M, decimation=1, taps=L - 1)
    assert h.dtype == np.float32 and h.shape == (L,)
    assert h[:L - 1].tobytes() == ddc.tobytes()
    assert h[L - 1:].tobytes() == np.zeros(1, np.float32).tobytes()  # +0, not -0
    assert abs(float(h.astype(np.float64).sum()) - 1.0) <= 1e-6
    assert close_to_formula(h, cc.taps_formula(0.5, M, P))


def test_design_of_the_longest_prototype(S):
    """L = 4096: the design's products no longer fit the DDC's 511 entries."""
    h = design(S, 256, 16, cutoff_rel=0.6)
    assert close_to_formula(h, cc.taps_formula(0.6, 256, 16)) and h[-1] == 0
    assert abs(float(h.astype(np.float64).sum()) - 1.0) <= 1e-6


@pytest.mark.parametrize("bad", [dict(channels=0), dict(channels=3), dict(channels=512), dict(taps_per_channel=0),
                                 dict(taps_per_channel=33), dict(channels=256, taps_per_channel=17, n_channels=1),
                                 dict(oversample=0), dict(oversample=3), dict(cutoff_rel=0.0), dict(cutoff_rel=-0.5),
                                 dict(cutoff_rel=8.001), dict(cutoff_rel=float("nan")), dict(first_channel=-1),
                                 dict(n_channels=0), dict(first_channel=1), dict(n_channels=17),
                                 dict(first_channel=16, n_channels=1)])
def test_each_bad_field_is_refused_on_its_own(S, bad):
    cfg = dict(GOOD, **bad)
    assert not cc.valid_config(cfg["cutoff_rel"], cfg["channels"], cfg["taps_per_channel"], cfg["oversample"],
                               cfg["first_channel"], cfg["n_channels"])
    invalid(S, S.channelizer_design, **cfg)
    invalid(S, S.channelizer_tile_outputs, **cfg)


def test_good_configurations_and_null_pointers(S):
    for cfg in (GOOD, dict(GOOD, cutoff_rel=8.0), dict(GOOD, first_channel=15, n_channels=1),
                dict(GOOD, channels=256, taps_per_channel=16, n_channels=256), dict(GOOD, channels=2, n_channels=2,
                                                                                   taps_per_channel=32, oversample=2)):
        assert cc.valid_config(cfg["cutoff_rel"], cfg["channels"], cfg["taps_per_channel"], cfg["oversample"],
                               cfg["first_channel"], cfg["n_channels"])
        assert S.channelizer_design(**cfg).size == cfg["channels"] * cfg["taps_per_channel"]
        assert S.channelizer_tile_outputs(**cfg) >= 1
    L, c = S.load(), S.ChannelizerConfig(0.5, 16, 8, 1, 0, 16)
    h, t = np.zeros(128, np.float32), ctypes.c_int32()
    assert L.sdrg_channelizer_design(None, h.ctypes.data_as(ctypes.c_void_p)) == -1
    assert L.sdrg_channelizer_design(ctypes.byref(c), None) == -1
    assert L.sdrg_channelizer_tile_outputs(None, ctypes.byref(t)) == -1
    assert L.sdrg_channelizer_tile_outputs(ctypes.byref(c), None) == -1
    assert L.sdrg_engine_set_channelizer(None, ctypes.byref(c)) == -1
    assert L.sdrg_engine_get_channelizer(None, ctypes.byref(c), None) == -1
    assert L.sdrg_engine_channelizer_reset(None) == -1
    assert L.sdrg_engine_channelizer_max_out(None, ctypes.byref(t)) == -1
    assert L.sdrg_engine_channelizer_device(None, None, 1, None, ctypes.byref(t)) == -1
    assert L.sdrg_engine_channelizer_host(None, None, 1, None, ctypes.byref(t)) == -1


@pytest.mark.parametrize("M,P,O", SHAPES)
def test_restatement_is_within_the_bound_of_the_model(S, M, P, O):
    h = design(S, M, P)
    n = (3 * P + 5) * M + 3
    for fmt in (dd.CS8, dd.CU8, dd.CS16, dd.CF32):
        raw = dd.noise(fmt, 2, n, seed=200 + fmt)
        y32, y64, bound, m0, n_out = cc.Bank(2, h, M, P, O).call(fmt, raw)
        assert n_out == -(-n // (M // O)) and y32.dtype == np.complex64 and y64.shape == (2, M, n_out)
        worst = cc.assert_within(y32, y64, bound, m0, P, O, (M, P, O, fmt))
        assert worst <= 0.25, worst  # the restatement uses a fraction of the bound: room for another FFT and for FMAs
        past = np.arange(n_out) >= P * O
        ratio = bound[:, past].mean() / np.abs(y64[:, :, past]).mean()
        assert 1e-6 <= ratio <= 3e-4, ratio


@pytest.mark.parametrize("M,P", [(16, 8), (64, 8)])
@pytest.mark.parametrize("O", [1, 2])
def test_rows_equal_the_ddc_at_the_channel_centres(S, M, P, O):
    """Row k against the DDC restatement at offset_hz = (k - M / 2) fs / M with the same taps and D = M / O."""
    B, L, D, fmt = 2, M * P, M // O, dd.CS16
    h, tab = design(S, M, P), S.nco_tables()
    n = 40 * M + 5
    raw = dd.noise(fmt, B, n, seed=210)
    y32, y64, bound, m0, n_out = cc.Bank(B, h, M, P, O).call(fmt, raw)
    for k in (0, M // 2, M // 2 + 1, M - 1):
        inc = dd.nco_increment((k - M // 2) * FS / M, FS)
        ddc, ddc_n = dd.Ddc(B, h[:L - 1], tab, inc, D).call(fmt, raw)
        assert ddc_n == n_out
        both = bound + dd.error_bound(L - 1, 1.0, h[:L - 1])
        err = np.abs(y32[:, k].astype(np.complex128) - ddc[:, :n_out])
        assert np.all(err <= both), (k, float((err / both).max()))
        assert np.abs(ddc[:, P * O:n_out]).mean() > 100 * both.mean()


def test_tones_land_in_their_rows(S):
    """A CS16 tone at a channel's centre comes out in its row as a constant of modulus amp |H(0)|; half a channel off it
    comes out at |H(0.5 / M)| in both neighbours; every other row stays below the prototype's stopband peak."""
    M, P, O, amp, fmt = 16, 8, 1, 0.5, dd.CS16
    h = design(S, M, P)
    n = 64 * M
    stop = max(abs(dd.response(h, f)) for f in np.arange(1.0 / M, 0.5, 0.05 / M))  # from the next channel's centre on
    assert stop < 0.02
    for k in (3, 8, 12):
        c = cc.channel_of_row(k, M)
        y = cc.model_f32(fmt, dd.tone(fmt, 1, n, c / M, amp=amp), h, M, P, O)[0, :, P + 1:]
        assert np.allclose(np.abs(y[k]), amp * abs(dd.response(h, 0.0)), rtol=0, atol=2e-4)
        assert np.abs(y[k] - y[k, :1]).max() <= 2e-4  # a constant: the channel's own centre is DC in its row
        others = np.delete(np.abs(y), k, axis=0)
        assert others.max() <= amp * stop + 2e-4
    k = 5
    c = cc.channel_of_row(k, M)
    y = np.abs(cc.model_f32(fmt, dd.tone(fmt, 1, n, (c + 0.5) / M, amp=amp), h, M, P, O)[0, :, P + 1:])
    edge = amp * abs(dd.response(h, 0.5 / M))
    assert np.allclose(y[k], edge, rtol=0, atol=2e-4) and np.allclose(y[k + 1], edge, rtol=0, atol=2e-4)
    assert np.delete(y, (k, k + 1), axis=0).max() <= amp * stop + 2e-4


def test_oversampled_rows_alternate_in_sign_for_odd_channels(S):
    """O = 2: y_c[m] = (-1)^{c m} Y_c[m], so that a tone at the channel's centre stays a constant in its row."""
    M, P, fmt = 8, 4, dd.CF32
    h = design(S, M, P)
    raw = dd.noise(fmt, 1, 40 * M, seed=220)
    x = cc.exact_samples(fmt, raw)[0].astype(np.complex128)
    y, _ = cc.model_f64(fmt, raw, h, M, P, 2)
    D, L = M // 2, M * P
    e = np.concatenate([np.zeros(L - 1, np.complex128), x])
    for k in range(M):
        c = cc.channel_of_row(k, M)
        for m in (0, 1, 6, 7, 33):
            w = e[L - 1 + m * D - np.arange(L)]
            Y = np.sum(h.astype(np.float64) * w * np.exp(2j * np.pi * c * np.arange(L) / M))
            assert abs(y[0, k, m] - (-1) ** (c * m) * Y) <= 1e-12, (k, m)
    for k in (1, 5):  # odd channels: c = 5 and c = 1
        c = cc.channel_of_row(k, M)
        assert c % 2 == 1
        row = cc.model_f32(dd.CS16, dd.tone(dd.CS16, 1, 64 * M, c / M), h, M, P, 2)[0, k, 2 * P + 2:]
        assert np.abs(row - row[0]).max() <= 2e-4 and abs(row[0]) > 0.4


@pytest.mark.parametrize("M,P,O", [(4, 3, 2), (16, 8, 1), (64, 2, 2)])
def test_any_cut_of_a_stream_gives_the_same_bytes(S, M, P, O):
    """n_out follows ceil((g0 + N) / D) - ceil(g0 / D), and calls of any lengths (N = 1 and N < D included) and
    formats' worth of samples give the bytes of one call."""
    B, D, fmt = 2, M // O, dd.CS8
    h = design(S, M, P)
    n = 11 * M + 7
    raw = dd.noise(fmt, B, n, seed=230)
    whole = cc.model_f32(fmt, raw, h, M, P, O)
    assert whole.shape == (B, M, -(-n // D))
    for cuts in ([1, 1, D - 1, 3 * M + 1, 2], [n // 2], [D, D, D + 1, 1, 1, 1, 5 * M]):
        bank, parts, at = cc.Bank(B, h, M, P, O), [], 0
        for ln in cuts + [n - sum(cuts)]:
            y32, _, _, m0, n_out = bank.call(fmt, raw[:, 2 * at:2 * (at + ln)])
            assert n_out == -(-(at + ln) // D) - -(-at // D) and m0 == -(-at // D)
            parts.append(y32)
            at += ln
        assert bank.g0 == n and np.concatenate(parts, axis=2).tobytes() == whole.tobytes(), cuts


def test_span_is_a_slice_of_the_rows():
    """Rows [first, first + n) of the fftshifted order: row k is centred at sdrg_bin_offset_hz(M, fs, k)."""
    import sdrg
    M = 16
    for k in range(M):
        c = cc.channel_of_row(k, M)
        off = sdrg.bin_offset_hz(M, FS, k)
        assert off == (c if c < M // 2 else c - M) * FS / M
    assert [cc.channel_of_row(k, 4) for k in range(4)] == [2, 3, 0, 1]
