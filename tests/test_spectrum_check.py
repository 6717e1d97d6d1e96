"""The spectrum checker of tests/spectrum_cases.py, tested on the CPU so it cannot rot: it accepts numpy's complex64
transform for every (format, N) the GPU suite runs, and rejects each planted defect with the assertion named here.

Which assertion catches what (check_spectrum's order: input condition, per-bin bound, rms bound, odd tail):
  a tone over weak noise as input (the older tests' input)      input condition
  one bin zeroed                                                per-bin bound
  two adjacent bins swapped                                     per-bin bound
  frame b's row written to frame b+1                            per-bin bound
  fftshift with ceil(N/2) at an odd N                           per-bin bound (and the odd tail, checked apart)
  CU8 unpacked with 127.5 in place of 127.4                     per-bin bound (the DC bin)
  the whole spectrum scaled by 1 + 1e-5                         rms bound (the per-bin bound passes)
  bins k = 5 (mod 32) scaled by 1 + 3e-5 (a wrong twiddle)      rms bound (the per-bin bound passes)
"""
import os
import re

import numpy as np
import pytest

import spectrum_cases as sc
from conftest import ROOT

CSRC = os.path.join(ROOT, "sdr-for-android-lib_amd", "csrc")
SEED = sc.SEED


def cpu_frames(n, frames):
    """The GPU suite's batch where that is cheap, fewer frames for the large N."""
    return frames if n * frames <= (1 << 18) else (3 if n <= 16384 else 2 if n <= 65536 else 1)


MATRIX = [(fmt, n, 3 if n <= 16384 else 2) for n in sc.POW2_SIZES for fmt in sc.FORMATS] + \
         [(fmt, n, cpu_frames(n, sc.any_case_frames(n, fr))) for n, fmts, _, fr in sc.ANY_CASES for fmt in fmts]


@pytest.mark.parametrize("fmt,n,B", MATRIX, ids=[f"{sc.FMT_NAMES[f]}-{n}-{b}" for f, n, b in MATRIX])
def test_accepts_numpy_complex64(fmt, n, B):
    """Same generator, batch and seed as the GPU test of this (format, N) where B is the same: its input condition is
    known to hold before a GPU is involved."""
    x = sc.unpack(fmt, sc.dense_frames(fmt, n, B, SEED))
    ref = sc.reference(x)
    fig = sc.check_spectrum(ref[1], x, ref=ref)
    if n > 1:
        assert fig["E"] == fig["E_ref32"] and fig["E_over_bound"] <= 1.0 / sc.RMS_MARGIN + 1e-12


def exact(fmt, n, B):
    x = sc.unpack(fmt, sc.dense_frames(fmt, n, B, SEED))
    ref = sc.reference(x)
    return x, ref, ref[0].astype(np.float32)


def per_bin_passes(got, p64):
    return (np.abs(got - p64) <= sc.RTOL * p64 + sc.ATOL_MAX * p64.max(axis=1, keepdims=True)).all()


@pytest.mark.parametrize("n", [64, 4096, 65536])
def test_accepts_the_rounded_float64_spectrum(n):
    x, ref, got = exact(sc.CS8, n, 3)
    assert sc.check_spectrum(got, x, ref=ref)["E"] < 5e-8  # half an ulp per bin


@pytest.mark.parametrize("n", [64, 4096, 65536])
def test_rejects_one_bin_zeroed(n):
    x, ref, got = exact(sc.CS8, n, 3)
    k = int(np.argsort(ref[0][1])[n // 2])  # a bin of median power
    got[1, k] = 0.0
    with pytest.raises(AssertionError, match="^per-bin bound"):
        sc.check_spectrum(got, x, ref=ref)


@pytest.mark.parametrize("n", [64, 4096, 65536])
def test_rejects_adjacent_bins_swapped(n):
    x, ref, got = exact(sc.CU8, n, 3)
    k = int(np.argmax(np.abs(np.diff(ref[0][2]))))
    got[2, [k, k + 1]] = got[2, [k + 1, k]]
    with pytest.raises(AssertionError, match="^per-bin bound"):
        sc.check_spectrum(got, x, ref=ref)


def test_rejects_a_row_in_the_next_frame():
    x, ref, got = exact(sc.CS16, 4096, 3)
    got[2] = got[1]
    with pytest.raises(AssertionError, match="^per-bin bound"):
        sc.check_spectrum(got, x, ref=ref)


def test_rejects_ceil_fftshift_at_odd_n():
    n = 4099
    x, ref, got = exact(sc.CS8, n, 3)
    X = np.fft.fft(x, axis=1)
    wrong = np.fft.fftshift(np.abs(X) ** 2, axes=1).astype(np.float32)  # numpy's shift: P[ceil(N/2):] first
    np.testing.assert_array_equal(wrong[:, n // 2:n - 1], got[:, n // 2:n - 1])  # the second half is in place
    with pytest.raises(AssertionError, match="^per-bin bound"):
        sc.check_spectrum(wrong, x, ref=ref)
    got[:, n - 1] = wrong[:, n - 1]  # every transform output right, but element N-1 written
    with pytest.raises(AssertionError, match="^odd tail"):
        sc.check_spectrum(got, x, ref=ref)
    sc.check_spectrum(got, x, ref=ref, fresh=False)


@pytest.mark.parametrize("n", [64, 4096, 65536])
def test_rejects_cu8_offset_127_5(n):
    raw = sc.dense_frames(sc.CU8, n, 3, SEED)
    x = sc.unpack(sc.CU8, raw)
    wrong = sc.reference(sc.unpack(sc.CU8, raw, cu8_offset=127.5))[0].astype(np.float32)
    with pytest.raises(AssertionError, match="^per-bin bound.*first \\(frame, bin\\) \\[\\[0, %d\\]" % (n // 2)):
        sc.check_spectrum(wrong, x)


@pytest.mark.parametrize("n", [64, 4096, 65536, 999983])
def test_rejects_scale_1e_5(n):
    x, ref, _ = exact(sc.CS8, n, 2)
    got = (ref[0] * (1.0 + 1e-5)).astype(np.float32)
    assert per_bin_passes(got, ref[0])
    with pytest.raises(AssertionError, match="^rms bound"):
        sc.check_spectrum(got, x, ref=ref)


@pytest.mark.parametrize("n", [4096, 65536])
def test_rejects_one_residue_class_scaled(n):
    x, ref, _ = exact(sc.CF32, n, 2)
    p = ref[0].copy()
    p[:, 5::32] *= 1.0 + 3e-5  # N/2 is a multiple of 32: the shift keeps k mod 32
    got = p.astype(np.float32)
    assert per_bin_passes(got, ref[0])
    with pytest.raises(AssertionError, match="^rms bound"):
        sc.check_spectrum(got, x, ref=ref)


def test_rejects_a_tone_over_weak_noise_as_input():
    import oracle as O
    n = 16384
    raw = O.synth_frames(3, n, O.CS8, tone_hz=1500.0, fs=2e6, seed=1)
    x = sc.unpack(sc.CS8, raw)
    ref = sc.reference(x)
    with pytest.raises(AssertionError, match="^input condition: 0.0 passes"):
        sc.check_spectrum(ref[0].astype(np.float32), x, ref=ref)


def test_rejects_nan():
    x, ref, got = exact(sc.CS8, 256, 3)
    got[0, 17] = np.nan
    with pytest.raises(AssertionError, match="^per-bin bound"):
        sc.check_spectrum(got, x, ref=ref)


def test_unpack_is_the_oracles():
    import oracle as O
    for fmt in sc.FORMATS:
        raw = sc.dense_frames(fmt, 513, 2, SEED)
        x = sc.unpack(fmt, raw)
        for b in range(2):
            iq = O.unpack(fmt, raw[b], 513)
            np.testing.assert_array_equal(x[b].real.astype(np.float32), iq[0::2])
            np.testing.assert_array_equal(x[b].imag.astype(np.float32), iq[1::2])


def test_dense_frames_differ_and_fill_the_range():
    for fmt in sc.FORMATS:
        raw = sc.dense_frames(fmt, 4096, 4, SEED)
        assert raw.dtype == sc.NUMPY_DTYPE[fmt] and raw.shape == (4, 8192)
        assert len({r.tobytes() for r in raw}) == 4
        v = raw.astype(np.float64) - (127.4 if fmt == sc.CU8 else 0.0)
        assert abs(v.std() / sc.SIGMA[fmt] - 1.0) < 0.05 and abs(v.mean()) < 0.05 * sc.SIGMA[fmt]


# --------------------------------------------------------------------------------------------------
# the restated batch arithmetic against the sources
# --------------------------------------------------------------------------------------------------
def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_restated_constants_match_the_sources():
    fa, si, st = source("fftany.hip"), source("sdrg_internal.h"), source("stats.hip")
    assert int(re.search(r"constexpr int TILE_MAX = (\d+);", fa).group(1)) == sc.TILE_MAX
    assert int(re.search(r"constexpr int TILE_TARGET = (\d+);", fa).group(1)) == sc.TILE_TARGET
    assert re.search(r"std::min\(n_frames, TILE_TARGET / P\.m\)", fa)
    assert int(re.search(r"\(\(size_t\)(\d+) << 20\) / per", fa).group(1)) << 20 == sc.WAVE_BYTES
    assert int(re.search(r"SPECTRUM_WAVE_BYTES = \(size_t\)(\d+) << 20;", si).group(1)) << 20 == sc.WAVE_BYTES
    assert re.search(r"SPECTRUM_WAVE_BYTES / \(\(size_t\)n \* 8\)", si)
    assert int(re.search(r"constexpr int STAGE_MAX = (\d+);", st).group(1)) == sc.STATS_STAGE_MAX
    assert re.search(r"return stage_bins\(geo\) > STAGE_MAX;", st)


def test_any_cases_reach_the_paths_they_name():
    for n, _, mode, fr in sc.ANY_CASES:
        assert not sc.pow2_kernels(n) and sc.any_plan(n)["mode"] == mode, n
        B = sc.any_case_frames(n, fr)
        if mode in ("ONE", "BLUE_ONE") and sc.any_plan(n)["m"] < sc.TILE_TARGET and (n, fr) != (7, 515):
            C = sc.fft1_tile_frames(n, B)
            assert B > C and B % C, (n, B, C)  # more than one workgroup, the last one ragged
        if fr == "wave":
            assert B == sc.any_wave_frames(n) + 1
    assert sc.any_case_frames(786432, "wave") == 22 and sc.any_case_frames(999983, "wave") == 5
    assert sc.spectrum_wave_frames(65536) == 256 and sc.spectrum_wave_frames(32768) == 512
    assert all(sc.pow2_kernels(n) for n in sc.POW2_SIZES) and len(sc.POW2_SIZES) == 11


def test_wide_statistics_focus():
    """200 kHz at 2 Msps takes the wide statistics kernel at 65536 and at 32768 (the non-persistent four-step pair
    then runs), 5 kHz does not."""
    import oracle as O
    for n in (32768, 65536):
        assert sc.stats_stage_bins(O, 2_000_000, n, 200) > sc.STATS_STAGE_MAX
        assert sc.stats_stage_bins(O, 2_000_000, n, 5) <= sc.STATS_STAGE_MAX
