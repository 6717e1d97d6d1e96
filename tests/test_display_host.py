"""CPU tests of the display stage's host helpers (include/sdrg.h: sdrg_display_column_range, sdrg_display_code) against
the NumPy restatement in tests/display_cases.py.  No device is touched."""
import ctypes

import numpy as np
import pytest

import display_cases as dc

import sdrg

PAIRS = [(16384, 1024), (16384, 1000), (4099, 64), (81, 128), (1, 4), (1000, 7), (2 ** 20, 2 ** 20 - 1), (2 ** 20, 1)]


def lib_ranges(nb, W):
    L = sdrg.load()
    first, count = ctypes.c_int32(), ctypes.c_int32()
    out = np.empty((W, 2), np.int64)
    for c in range(W):
        assert L.sdrg_display_column_range(nb, W, c, ctypes.byref(first), ctypes.byref(count)) == 0
        out[c] = first.value, count.value
    return out


@pytest.mark.parametrize("nb,W", PAIRS, ids=[f"{nb}to{W}" for nb, W in PAIRS])
def test_column_ranges_match_the_restatement(nb, W):
    got = lib_ranges(nb, W)
    b = dc.column_bounds(nb, W)  # Python integers: (c * nb) // W needs 40 bits for the large pair
    np.testing.assert_array_equal(got[:, 0], b[:-1])
    np.testing.assert_array_equal(got[:, 1], np.maximum(b[1:] - b[:-1], 1))
    assert got[:, 1].min() >= 1
    assert np.all(got[:, 0] + got[:, 1] <= nb)
    for c in (0, W // 2, W - 1):
        assert sdrg.display_column_range(nb, W, c) == dc.column_range(nb, W, c)
    if W <= nb:  # the ranges tile [0, nb) exactly
        assert got[0, 0] == 0 and got[-1, 0] + got[-1, 1] == nb
        np.testing.assert_array_equal(got[1:, 0], got[:-1, 0] + got[:-1, 1])
    else:  # nearest-bin repetition: every bin shown, in order
        assert np.all(got[:, 1] == 1) and np.all(np.diff(got[:, 0]) >= 0)
        np.testing.assert_array_equal(np.unique(got[:, 0]), np.arange(nb))


@pytest.mark.parametrize("args", [(0, 4, 0), (4, 0, 0), (4, 4, 4), (4, 4, -1), (2 ** 20 + 1, 4, 0), (4, 2 ** 20 + 1, 0)])
def test_column_range_rejects_out_of_range_arguments(args):
    with pytest.raises(sdrg.SdrgError) as ei:
        sdrg.display_column_range(*args)
    assert "SDRG_E_INVALID" in str(ei.value)
    first, count = ctypes.c_int32(), ctypes.c_int32()
    assert sdrg.load().sdrg_display_column_range(4, 4, 0, None, ctypes.byref(count)) == -1
    assert sdrg.load().sdrg_display_column_range(4, 4, 0, ctypes.byref(first), None) == -1


def lib_codes(d, db_min, db_max):
    L = sdrg.load()
    c = ctypes.c_uint8()
    out = np.empty(len(d), np.uint8)
    for i, x in enumerate(d):
        assert L.sdrg_display_code(ctypes.c_float(x), db_min, db_max, ctypes.byref(c)) == 0
        out[i] = c.value
    return out


def test_codes_on_the_boundary_sweep():
    """The 1215 powers around 15 code boundaries: their dB values straddle each boundary, and the codes follow the
    specified float32 operation order -- a quantiser that fuses the multiply with the add, or works in double, gives
    other codes on some of them, so this input tells the orders apart."""
    p = dc.boundary_sweep_powers()
    assert p.size == 1215
    d = dc.db(p)
    want = dc.code(d, dc.SWEEP_DB_MIN, dc.SWEEP_DB_MAX)
    for i, k in enumerate(dc.SWEEP_KS):
        assert set(want[81 * i:81 * (i + 1)]) == {k, k + 1}, k
    np.testing.assert_array_equal(lib_codes(d, dc.SWEEP_DB_MIN, dc.SWEEP_DB_MAX), want)
    # sensitivity: the same dB values quantised in double
    dd = d.astype(np.float64)
    in_double = np.floor((dd - dc.SWEEP_DB_MIN) * (255.0 / (dc.SWEEP_DB_MAX - dc.SWEEP_DB_MIN)) + 0.5).astype(np.int64)
    assert np.count_nonzero(in_double != want) > 0


def test_codes_of_special_values():
    d = np.array([-200.0, np.inf, -np.inf, np.nan, -120.0, 0.0, 1e30, -1e30], np.float32)
    want = dc.code(d, -120.0, 0.0)
    np.testing.assert_array_equal(want, [0, 255, 0, 0, 0, 255, 255, 0])
    np.testing.assert_array_equal(lib_codes(d, -120.0, 0.0), want)
    assert sdrg.display_code(float(dc.db(np.float32(0.0))), -120.0, 0.0) == 0      # a zero power: -200 dB
    assert sdrg.display_code(float(dc.db(np.float32(np.inf))), -120.0, 0.0) == 255
    assert sdrg.display_code(float("nan"), -120.0, 0.0) == 0
    for lo, hi in ((0.0, 0.0), (0.0, -1.0), (float("nan"), 0.0), (-120.0, float("inf")), (float("-inf"), 0.0)):
        with pytest.raises(sdrg.SdrgError) as ei:
            sdrg.display_code(-50.0, lo, hi)
        assert "SDRG_E_INVALID" in str(ei.value)
    assert sdrg.load().sdrg_display_code(0.0, -120.0, 0.0, None) == -1


def test_restatement_columns_on_a_small_row():
    """The restatement itself, by hand: 10 bins to 4 columns and to 15."""
    row = np.array([1, 5, 2, 0, 7, 3, 3, 9, 4, 6], np.float32)
    # (c * 10) // 4 = 0, 2, 5, 7, 10
    np.testing.assert_array_equal(dc.column_values(row, 4, dc.MAX), [5, 7, 3, 9])
    np.testing.assert_array_equal(dc.column_values(row, 4, dc.MEAN), np.array([3, 3, 3, 19 / 3], np.float32))
    # (c * 10) // 15 = 0 0 1 2 2 3 4 4 5 6 6 7 8 8 9
    np.testing.assert_array_equal(dc.column_values(row, 15, dc.MEAN), row[[0, 0, 1, 2, 2, 3, 4, 4, 5, 6, 6, 7, 8, 8, 9]])
    np.testing.assert_array_equal(dc.rows(row[None], 2, 6, 6, dc.MAX, dc.DB_F32)[0], dc.db(row[2:8]))
