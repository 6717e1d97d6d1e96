"""CPU tests of the peak table stage: its NumPy restatement (tests/peaks_cases.py) on hand-worked rows, the fast
candidate rule against brute force, the two forms of the result, and the boundary (the header declares the entry points,
the library and sdrg.EXPORTS carry them, sdrg_bin_offset_hz).  No device is touched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import display_cases as dc
import peaks_cases as pc

f32 = np.float32
NEW_SYMBOLS = ("sdrg_bin_offset_hz", "sdrg_engine_set_peaks", "sdrg_engine_get_peaks", "sdrg_engine_peaks_device",
               "sdrg_engine_peaks_host", "sdrg_engine_peaks_integrated_host")


def cand_bins(row, d, fn=pc.candidates):
    return np.flatnonzero(fn(np.array(row, np.float32), d)).tolist()


def test_the_worked_row():
    """[1, 3, 3, 2, 5, 1]: d = 1: bin 1 (the plateau's lowest bin; bin 2 is not above bin 1) and bin 4.  d = 2: bin 1
    still (bin 3 = 2 is inside its window, bin 4 is not) and bin 4.  d = 3: bin 4 is inside bin 1's window."""
    row = [1, 3, 3, 2, 5, 1]
    for fn in (pc.candidates_brute, pc.candidates):
        assert cand_bins(row, 1, fn) == [1, 4]
        assert cand_bins(row, 2, fn) == [1, 4]
        assert cand_bins(row, 3, fn) == [4]
        assert cand_bins(row, 100, fn) == [4]


def test_constant_rows_ramps_and_one_bin():
    for fn in (pc.candidates_brute, pc.candidates):
        for d in (1, 2, 7, 8, 9, 4096):
            assert cand_bins([2.5] * 8, d, fn) == [0]
            assert cand_bins([0.0] * 8, d, fn) == [0]
            assert cand_bins(np.arange(8), d, fn) == [7]       # rising: only the last bin has nothing above it
            assert cand_bins(np.arange(8)[::-1], d, fn) == [0]  # a falling skirt yields nothing after its top
            assert cand_bins([3.0], d, fn) == [0]
        # greedy suppression would mark the shoulder d + 1 bins from the top; the window rule does not
        assert cand_bins([9, 8, 7, 6, 5, 4, 3], 2, fn) == [0]
        # equal maxima exactly d and d + 1 apart: the second is inside the first's window, or not
        assert cand_bins([0, 5, 0, 0, 5, 0], 3, fn) == [1]
        assert cand_bins([0, 5, 0, 0, 0, 5, 0], 3, fn) == [1, 5]
        assert cand_bins([np.inf, 0, 0, np.inf], 2, fn) == [0, 3]


def test_floor_rank_for_even_and_odd_lengths():
    assert pc.floor_power([4, 1, 3, 2]) == 3          # sorted [1 2 3 4], rank 2
    assert pc.floor_power([5, 4, 1, 3, 2]) == 3       # sorted [1 2 3 4 5], rank 2
    assert pc.floor_power([7]) == 7
    assert pc.floor_power([1, 2]) == 2
    assert pc.floor_power([2, 2, 2, 9, 0, 2]) == 2    # duplicates of the median
    assert pc.floor_power([np.inf, np.inf, 1.0]) == np.inf


def test_a_table_by_hand():
    # floor: sorted [0 1 1 1 2 3 3 5] -> rank 4 = 2; dB(2) = 3.0103, dB(5) = 6.9897, dB(3) = 4.7712
    row = np.array([1, 3, 3, 2, 5, 0, 1, 1], np.float32)
    pk, sm = pc.table(row, lo=100, d=1, max_peaks=4, threshold_db=-np.inf)
    assert sm["floor_power"] == 2 and sm["floor_db"] == dc.db(f32(2))
    assert sm["n_above"] == 3 and sm["count"] == 3    # bins 1, 4 and the plateau 6..7 at its lowest bin
    assert pk["bin"].tolist() == [104, 101, 106, -1]
    assert pk["power"].tolist() == [5, 3, 1, 0]
    assert pk["db"][0] == dc.db(f32(5)) and pk["snr_db"][0] == f32(dc.db(f32(5)) - dc.db(f32(2)))
    assert pk[3].tobytes() == np.array([-1, 0, 0, 0], np.int32).tobytes()
    pk, sm = pc.table(row, lo=0, d=1, max_peaks=1, threshold_db=1.0)  # 3 is 1.76 dB over the floor, 1 is below it
    assert sm["n_above"] == 2 and sm["count"] == 1 and pk["bin"].tolist() == [4]
    pk, sm = pc.table(np.zeros(5, np.float32), lo=0, d=2, max_peaks=2, threshold_db=0.0)
    assert abs(float(sm["floor_db"]) + 200.0) < 1e-3 and sm["n_above"] == 1 and pk["bin"].tolist() == [0, -1]
    assert pk["snr_db"][0] == 0
    # more than half +inf: the floor is +inf, an infinite candidate's snr is NaN and is not above
    pk, sm = pc.table(np.array([np.inf, np.inf, 1.0, np.inf], np.float32), lo=0, d=4, max_peaks=2, threshold_db=-np.inf)
    assert np.isposinf(sm["floor_db"]) and sm["n_above"] == 0 and pk["bin"].tolist() == [-1, -1]


def test_equal_powers_order_by_bin_and_ulp_neighbours_by_power():
    a, b = pc.ulp_pair_sharing_db()
    assert b == np.nextafter(a, f32(np.inf)) and dc.db(a) == dc.db(b)
    row = np.array([0, a, 0, b, 0, a, 0], np.float32)
    pk, _ = pc.table(row, lo=0, d=1, max_peaks=3, threshold_db=-np.inf)
    assert pk["bin"].tolist() == [3, 1, 5]


def test_fast_candidates_equal_brute_force():
    rng = np.random.default_rng(1)
    for nb in (1, 2, 3, 5, 17, 64, 65, 300):
        rows = [rng.integers(0, 4, nb), rng.integers(0, 9, nb), rng.exponential(1.0, nb), np.zeros(nb),
                np.sort(rng.integers(0, 50, nb))]
        for row in rows:
            row = np.asarray(row, dtype=np.float32)
            for d in range(1, nb + 3):
                got, want = pc.candidates(row, d), pc.candidates_brute(row, d)
                assert np.array_equal(got, want), (nb, d)
                bins = np.flatnonzero(want)
                assert bins.size >= 1 and np.all(np.diff(bins) > d)  # two candidates are more than d apart


def test_the_two_forms_of_the_result_agree():
    rng = np.random.default_rng(2)
    for trial in range(60):
        nb = int(rng.integers(1, 200))
        row = (rng.integers(0, 16, nb) * rng.choice([0.25, 1.0, 3.0])).astype(np.float32)
        d, k = int(rng.integers(1, 12)), int(rng.integers(1, 9))
        thr = float(rng.choice([-np.inf, -3.0, 0.0, 1.5, 6.0]))
        a = pc.table(row, 7, d, k, thr)
        b = pc.table(row, 7, d, k, thr, drop_last=True)
        c = pc.table(row, 7, d, k, thr, cand_fn=pc.candidates_brute)
        assert a[0].tobytes() == b[0].tobytes() == c[0].tobytes() and a[1].tobytes() == b[1].tobytes() == c[1].tobytes()


def test_header_library_and_mirror_carry_the_stage():
    import sdrg
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sdrg.h")).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", sdrg.lib_path()], capture_output=True, text=True, check=True).stdout
    L = sdrg.load()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert re.search(r"\bT %s$" % s, nm, flags=re.M), s
        assert s in sdrg.EXPORTS and hasattr(L, s)
    for s in ("sdrg_peaks_config", "sdrg_peak", "sdrg_peaks_summary", "SDRG_PEAKS_MAX = 64", "SDRG_PEAKS_MAX_SEPARATION = 4096"):
        assert s in text
    assert L.sdrg_abi_version() == 1
    assert sdrg.PEAK_DTYPE == pc.PEAK_DTYPE and sdrg.PEAK_DTYPE.itemsize == 16
    assert sdrg.PEAKS_SUMMARY_DTYPE == pc.SUMMARY_DTYPE and sdrg.PEAKS_SUMMARY_DTYPE.itemsize == 16
    assert ctypes.sizeof(sdrg.PeaksConfig) == 24
    assert (sdrg.PEAKS_MAX, sdrg.PEAKS_MAX_SEPARATION) == (pc.MAX_PEAKS, pc.MAX_SEPARATION)


def test_bin_offset_hz():
    import sdrg
    for n, fs in ((16384, 2_000_000), (1001, 2_400_000), (4099, 2_500_000), (1, 48_000), (2 ** 20, 10_000_000)):
        for b in sorted({0, n // 2, n - 1, n // 3}):
            assert sdrg.bin_offset_hz(n, fs, b) == pc.bin_offset_hz(n, fs, b)
    assert sdrg.bin_offset_hz(16384, 2_000_000, 8192) == 0.0
    assert sdrg.bin_offset_hz(16384, 2_000_000, 0) == -1_000_000.0
    assert sdrg.bin_offset_hz(16384, 2_000_000, 8192 + 41) == 41 * 2_000_000 / 16384
    assert sdrg.bin_offset_hz(1001, 2_400_000, 500) == 0.0  # odd n: the centre bin is n // 2
    for args in ((0, 1000, 0), (8, 1000, 8), (8, 1000, -1)):
        with pytest.raises(sdrg.SdrgError) as ei:
            sdrg.bin_offset_hz(*args)
        assert "SDRG_E_INVALID" in str(ei.value)
    assert sdrg.load().sdrg_bin_offset_hz(8, 1000, 0, None) == -1
