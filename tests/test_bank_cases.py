"""CPU tests of the DDC bank stage: its NumPy restatement (tests/bank_cases.py), which keeps the unmixed history, against
the DDC's (tests/ddc_cases.py), which keeps the mixed one, row by row in bytes; the retune law; continuity over any cut;
the accuracy bound; what a bank of tuned channels does to two tones; the refusals that need no device; and the boundary
(the header declares the entry points, the library and sdrg.EXPORTS carry them).  No device is touched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import bank_cases as bk
import ddc_cases as dd

FS = 2_000_000
NEW_SYMBOLS = ("sdrg_bank_geometry", "sdrg_engine_set_bank", "sdrg_engine_bank_retune", "sdrg_engine_get_bank",
               "sdrg_engine_bank_offsets", "sdrg_engine_bank_reset", "sdrg_engine_bank_max_out",
               "sdrg_engine_bank_device", "sdrg_engine_bank_host")


@pytest.fixture(scope="module")
def S():
    import sdrg
    return sdrg


@pytest.fixture(scope="module")
def tab(S):
    return S.nco_tables()


OFFSETS = np.array([[0.0, 250_000.0, -312_500.0, 999_999.0, 0.25],
                    [-700_123.0, 250_000.0, 2_750_000.0, 1234.5, -0.25]])


@pytest.mark.parametrize("fmt", [dd.CS8, dd.CU8, dd.CS16, dd.CF32])
@pytest.mark.parametrize("D,T", [(1, 1), (2, 3), (8, 63), (41, 255)])
def test_every_row_is_the_ddcs(S, tab, fmt, D, T):
    """Two streams of five channels (offsets that differ per stream and per channel, one shared by both streams), calls
    of uneven lengths, two of them shorter than T - 1: row s C + c equals, in bytes, a DDC of stream s at that offset."""
    B, C = OFFSETS.shape
    h = S.ddc_design(FS, cutoff_hz=min(FS / 2, 0.4 * FS / D), decimation=D, taps=T)
    incs = bk.increments(OFFSETS, FS)
    bank = bk.Bank(B, h, tab, incs, D)
    ddcs = [[dd.Ddc(1, h, tab, int(incs[b, c]), D) for c in range(C)] for b in range(B)]
    lengths = (700, 1, 37, 2048, 5, 300)
    raw = dd.noise(fmt, B, sum(lengths), seed=11 * fmt + D)
    at = 0
    for n in lengths:
        part = raw[:, 2 * at:2 * (at + n)]
        out, n_out = bank.call(fmt, part)
        assert out.shape == (B, C, -(-n // D)) and out.dtype == np.complex64
        for b in range(B):
            for c in range(C):
                want, want_n = ddcs[b][c].call(fmt, part[b:b + 1])
                assert n_out == want_n and out[b, c].tobytes() == want[0].tobytes(), (n, b, c)
        at += n
    assert bank.g0 == sum(lengths)
    assert np.array_equal(bank.xr, dd.unpack(fmt, raw)[0][:, raw.shape[1] // 2 - (T - 1):])


def test_equal_offsets_give_equal_rows(S, tab):
    h = S.ddc_design(FS, cutoff_hz=50e3, decimation=4, taps=31)
    incs = bk.increments([[1e5, -3e5, 1e5]], FS)
    out, _ = bk.Bank(1, h, tab, incs, 4).call(dd.CS16, dd.noise(dd.CS16, 1, 500, seed=2))
    assert out[0, 0].tobytes() == out[0, 2].tobytes() and out[0, 0].tobytes() != out[0, 1].tobytes()


def test_a_retune_equals_a_fresh_bank_fed_the_whole_stream(S, tab):
    """Calls 0 and 1 at offsets A, a retune to B before call 2, back to A before call 4: from each retune on, every row
    is what a bank that had the new offsets since the stream's start writes for the same raw samples."""
    B, D, T, fmt = 2, 6, 127, dd.CS8
    h = S.ddc_design(FS, cutoff_hz=60e3, decimation=D, taps=T)
    a = bk.increments([[100_000.0, -200_000.0], [5_000.0, 0.0]], FS)
    b_ = bk.increments([[-100_000.0, 640_000.0], [5_000.0, 123_456.0]], FS)
    lengths = (500, 90, 333, 40, 700)
    raws = [dd.noise(fmt, B, n, seed=20 + i) for i, n in enumerate(lengths)]
    bank, only_a, only_b = bk.Bank(B, h, tab, a, D), bk.Bank(B, h, tab, a, D), bk.Bank(B, h, tab, b_, D)
    for i, raw in enumerate(raws):
        if i == 2:
            bank.retune(b_)
        if i == 4:
            bank.retune(a)
        got, n_out = bank.call(fmt, raw)
        wa, na = only_a.call(fmt, raw)
        wb, nb = only_b.call(fmt, raw)
        want = wb if i in (2, 3) else wa
        assert n_out == na == nb and got.tobytes() == want.tobytes(), i
        if i in (2, 3):  # the stream's second channel moved, its first (stream 1: 5 kHz in both) did not
            assert got[0].tobytes() != wa[0].tobytes() and got[1, 0].tobytes() == wa[1, 0].tobytes()


@pytest.mark.parametrize("fmt", [dd.CS8, dd.CF32])
def test_continuity_over_any_cut(S, tab, fmt):
    """One call of 1000 samples equals calls of 1, 7, 250 and 742, byte for byte and in n_out."""
    B, T, D = 2, 63, 8
    h = S.ddc_design(FS, cutoff_hz=100e3, decimation=D, taps=T)
    incs = bk.increments(OFFSETS[:, :3], FS)
    raw = dd.noise(fmt, B, 1000, seed=5)
    whole, n_whole = bk.Bank(B, h, tab, incs, D).call(fmt, raw)
    assert n_whole == 125
    d = bk.Bank(B, h, tab, incs, D)
    parts, at = [], 0
    for n in (1, 7, 250, 742):
        out, n_out = d.call(fmt, raw[:, 2 * at:2 * (at + n)])
        assert n_out == dd.n_out_for(at, n, D) and out.shape == (B, 3, -(-n // D))
        assert not out[:, :, n_out:].view(np.uint32).any()
        parts.append(out[:, :, :n_out])
        at += n
    assert np.concatenate(parts, axis=2).tobytes() == whole.tobytes()


@pytest.mark.parametrize("fmt,T,D", [(dd.CS8, 63, 8), (dd.CU8, 255, 41), (dd.CS16, 511, 3), (dd.CF32, 127, 16)])
def test_accuracy_against_the_float64_model(S, tab, fmt, T, D):
    """Every row within ddc_cases.error_bound of the float64 model at its own increment."""
    B, n = 2, 6000
    h = S.ddc_design(FS, cutoff_hz=FS / (2.5 * D), decimation=D, taps=T)
    incs = bk.increments(OFFSETS[:, :4], FS)
    raw = dd.noise(fmt, B, n, seed=7)
    d = bk.Bank(B, h, tab, incs, D)
    parts, at = [], 0
    for m in (2500, 3500):
        out, n_out = d.call(fmt, raw[:, 2 * at:2 * (at + m)])
        parts.append(out[:, :, :n_out])
        at += m
    got = np.concatenate(parts, axis=2)
    xr, xi = dd.unpack(fmt, raw)
    bound = dd.error_bound(T, np.hypot(xr.astype(np.float64), xi.astype(np.float64)).max(), h)
    for c in range(4):
        for b in range(B):
            want = dd.model_f64(fmt, raw[b:b + 1], h, int(incs[b, c]), D)[0]
            err = max(np.abs(got[b, c].real - want.real).max(), np.abs(got[b, c].imag - want.imag).max())
            print(f"fmt {fmt} T {T} D {D} row ({b}, {c}): max error {err:.3g}, bound {bound:.3g}")
            assert err <= bound


def test_two_tones_three_channels(S, tab):
    """One CS16 stream with tones at +300 kHz and -450 kHz of 2 MHz; channels tuned to each and to an empty +700 kHz.
    A row is the sum of the two tones' responses, each A H(f_res) e^{j (2 pi f_res m D + phase)} with f_res what the
    channel's NCO leaves of the tone: the tuned tone sits at DC with the gain H(0) = 1, the other at the level the taps
    have at its distance.  The bound is the restatement's error_bound for max|x| = the two amplitudes' sum, plus what
    CS16's rounding of the input adds: at most 2^-16 sqrt(2) per sample through sum|h|."""
    T, D, n = 255, 16, 8192
    amps, tones = (0.4, 0.25), (300_000.0, -450_000.0)
    offsets = np.array([[300_000.0, -450_000.0, 700_000.0]])
    h = S.ddc_design(FS, cutoff_hz=40_000.0, decimation=D, taps=T)
    incs = bk.increments(offsets, FS)
    t = np.arange(n, dtype=np.float64)
    z = sum(a * np.exp(2j * np.pi * f / FS * t) for a, f in zip(amps, tones))
    raw = np.empty((1, 2 * n), np.int16)
    raw[0, 0::2], raw[0, 1::2] = np.round(z.real * 32768.0), np.round(z.imag * 32768.0)
    out, n_out = bk.Bank(1, h, tab, incs, D).call(dd.CS16, raw)
    m = np.arange(n_out)
    settled = m * D >= T - 1
    sum_h = np.abs(h.astype(np.float64)).sum()
    bound = dd.error_bound(T, sum(amps), h) + 2.0 ** -16 * np.sqrt(2.0) * sum_h
    for c in range(3):
        want = np.zeros(n_out, np.complex128)
        levels = []
        for a, f in zip(amps, tones):
            f_res = f / FS - int(incs[0, c]) / 2.0 ** 32
            H = dd.response(h, f_res)
            levels.append(a * abs(H))
            want += a * H * np.exp(2j * np.pi * f_res * D * m)
        err = np.abs(np.stack([out[0, c].real - want.real, out[0, c].imag - want.imag]))[:, settled].max()
        print(f"channel {c}: tone levels {levels[0]:.3g}, {levels[1]:.3g}, max error {err:.3g}, bound {bound:.3g}")
        assert err <= bound
        mean = out[0, c][settled].mean()  # what sits at DC
        if c < 2:  # the tuned tone at DC with gain 1; the other tone at its predicted level around it
            assert abs(abs(mean) - amps[c]) <= bound * np.sqrt(2) + levels[1 - c]
            assert np.abs(np.abs(out[0, c][settled] - amps[c] * dd.response(h, 0.0)) - levels[1 - c]).max() \
                <= bound * np.sqrt(2) + 2.0 ** -33 * 2 * np.pi * n * amps[c]
            assert levels[c] > 0.99 * amps[c] and levels[1 - c] < 1e-3
        else:  # the empty channel holds both tones at their stopband levels and nothing else
            assert np.abs(out[0, c][settled]).max() <= levels[0] + levels[1] + bound * np.sqrt(2)


def test_refusals(S):
    ok = dict(fs=FS, cutoff_hz=1e5, D=8, T=63, C=3, B=2, offsets_hz=np.zeros((2, 3)))
    assert bk.valid_config(**ok)
    nan, inf = np.zeros((2, 3)), np.zeros((2, 3))
    nan[1, 2], inf[0, 0] = np.nan, -np.inf
    bad = [dict(D=0), dict(D=513), dict(T=0), dict(T=62), dict(T=513), dict(cutoff_hz=0.0), dict(cutoff_hz=FS / 2 + 1),
           dict(C=0, offsets_hz=np.zeros((2, 0))), dict(C=4097, offsets_hz=np.zeros((2, 4097))),
           dict(B=16, C=4096, offsets_hz=np.zeros((16, 4096))), dict(offsets_hz=nan), dict(offsets_hz=inf),
           dict(offsets_hz=np.zeros((2, 2)))]
    for b in bad:
        assert not bk.valid_config(**dict(ok, **b)), b
    assert bk.valid_config(**dict(ok, B=17, C=3855, offsets_hz=np.zeros((17, 3855))))
    assert bk.valid_config(**dict(ok, B=1, C=4096, offsets_hz=np.zeros((1, 4096))))
    # the geometry call makes the same checks of (D, T, C, n_streams)
    for D, T, C, B in ((0, 3, 1, 1), (513, 3, 1, 1), (8, 62, 1, 1), (8, 513, 1, 1), (8, 63, 0, 1), (8, 63, 4097, 1),
                       (8, 63, 1, 0), (8, 63, 4096, 16), (8, 63, 21845, 3), (8, 63, 4369, 15)):
        with pytest.raises(S.SdrgError) as ei:
            S.bank_geometry(D, T, C, B)
        assert "SDRG_E_INVALID" in str(ei.value), (D, T, C, B)
    S.bank_geometry(8, 3, 3855, 17)  # 65535 rows
    # without an engine every engine call is refused
    L = S.load()
    z = (ctypes.c_double * 4)()
    cfg = S.BankConfig(1e5, 8, 63, 2)
    assert L.sdrg_engine_set_bank(None, ctypes.byref(cfg), z) == -1 and L.sdrg_engine_bank_retune(None, z) == -1
    assert L.sdrg_engine_get_bank(None, None, None) == -1 and L.sdrg_engine_bank_offsets(None, z, None) == -1
    assert L.sdrg_engine_bank_reset(None) == -1
    assert L.sdrg_engine_bank_max_out(None, ctypes.byref(ctypes.c_int32())) == -1
    n_out = ctypes.c_int32()
    assert L.sdrg_engine_bank_device(None, z, dd.CS8, z, ctypes.byref(n_out)) == -1
    assert L.sdrg_engine_bank_host(None, z, dd.CS8, z, ctypes.byref(n_out)) == -1


def test_header_library_and_mirror_carry_the_stage(S):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sdrg.h")).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", S.lib_path()], capture_output=True, text=True, check=True).stdout
    L = S.load()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert re.search(r"\bT %s$" % s, nm, flags=re.M), s
        assert s in S.EXPORTS and hasattr(L, s)
    for s in ("sdrg_bank_config", "#define SDRG_BANK_MAX_CHANNELS 4096"):
        assert s in text
    assert ctypes.sizeof(S.BankConfig) == 24
    assert S.BANK_MAX_CHANNELS == bk.MAX_CHANNELS
    for m in ("set_bank", "bank_retune", "bank_config", "bank_offsets", "bank_reset", "bank_max_out", "bank_device",
              "bank"):
        assert callable(getattr(S.Engine, m)), m
    # the geometry: a tile of at least one output and at most a workgroup's lanes; a group of at least one channel and at
    # most the stream's; and a function of the four arguments alone
    for D in (1, 2, 3, 41, 64, 512):
        for T in (1, 3, 255, 511):
            for C, B in ((1, 1), (5, 3), (64, 64), (4096, 1), (3855, 17)):
                tile, group = S.bank_geometry(D, T, C, B)
                assert 1 <= tile <= 256 and 1 <= group <= C
                assert (tile, group) == S.bank_geometry(D, T, C, B)
    assert S.bank_geometry(41, 255, 16, 1)[1] == 1 and S.bank_geometry(41, 255, 4096, 1)[1] > 1
