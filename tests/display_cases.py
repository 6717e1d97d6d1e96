"""The display stage (include/sdrg.h, sdrg_engine_display_*) restated in NumPy, and the inputs its tests share.

Per row of N powers: a span [lo, lo + nb) reduced to W columns, column c covering the span's bins
j0 = (c nb) // W .. j1 - 1, j1 = ((c + 1) nb) // W in Python integers (the one bin j0 when that range is empty);
the column value is the largest power (MAX) or (float)(S / (double)count) with S the exact sum rounded once
(math.fsum; the engine may add the doubles in any order); d = 10.0f * log10f(v + 1e-20f) with libm's log10f
(oracle/stats_np.log10f, the function csrc/glibc_logf.h restates bit for bit); the U8 code from d in float32, one
operation at a time.  tests/test_display_host.py checks the library's host helpers against it, tests/test_gpu_display.py
the kernels."""
import functools
import math

import numpy as np

import stats_np

f32 = np.float32
MAX, MEAN = 0, 1
DB_F32, U8 = 0, 1


@functools.lru_cache(maxsize=32)
def column_bounds(nb: int, W: int) -> np.ndarray:
    """first[c] for c in [0, W], in Python integers: column c covers [first[c], first[c + 1]) when that is not empty."""
    return np.array([(c * nb) // W for c in range(W + 1)], dtype=np.int64)


def column_range(nb: int, W: int, c: int):
    j0, j1 = (c * nb) // W, ((c + 1) * nb) // W
    return j0, (j1 - j0 if j1 > j0 else 1)


def column_values(span: np.ndarray, W: int, reduce: int) -> np.ndarray:
    """The W column values (float32) of one span of powers."""
    span = np.asarray(span, dtype=np.float32)
    nb = span.size
    b = column_bounds(nb, W)
    first, count = b[:-1], np.maximum(b[1:] - b[:-1], 1)
    if W >= nb:  # every column is one bin, and a mean of one value is the value
        assert np.all(count == 1)
        return span[first].copy()
    if reduce == MAX:
        return np.maximum.reduceat(span, first)  # W < nb: the ranges are non-empty and tile the span
    as_double = span.astype(np.float64)
    return np.array([f32(math.fsum(as_double[j:j + k]) / float(k)) for j, k in zip(first, count)], dtype=np.float32)


def db(v) -> np.ndarray:
    """10.0f * log10f(v + 1e-20f), float32 throughout (libm's log10f, evaluated once per distinct value)."""
    x = (np.asarray(v, dtype=np.float32) + f32(1e-20)).astype(np.float32)
    u, inv = np.unique(x.view(np.uint32), return_inverse=True)
    lg = stats_np.log10f(u.view(np.float32))
    return (f32(10.0) * lg).astype(np.float32)[inv].reshape(x.shape)


def code(d, db_min, db_max) -> np.ndarray:
    """The U8 code of dB values: scale = 255.0f / (db_max - db_min); t = (d - db_min) * scale as two float32
    operations; 255 if t >= 255, 0 if t <= 0 or NaN, else (int)(t + 0.5f)."""
    d = np.asarray(d, dtype=np.float32)
    scale = f32(255.0) / (f32(db_max) - f32(db_min))
    with np.errstate(invalid="ignore", over="ignore"):
        t = ((d - f32(db_min)).astype(np.float32) * scale).astype(np.float32)
        mid = (t + f32(0.5)).astype(np.float32)
        inner = np.where((t > 0) & (t < 255), mid, f32(0)).astype(np.int32)  # truncation
    return np.where(t >= 255, 255, np.where(t > 0, inner, 0)).astype(np.uint8)


def rows(spectra: np.ndarray, lo: int, nb: int, W: int, reduce: int, fmt: int, db_min=-120.0, db_max=0.0) -> np.ndarray:
    """[B][W] float32 dB or uint8 codes of [B][N] spectra."""
    spectra = np.asarray(spectra, dtype=np.float32)
    assert 0 <= lo and nb >= 1 and lo + nb <= spectra.shape[1]
    d = np.stack([db(column_values(r[lo:lo + nb], W, reduce)) for r in spectra])
    return code(d, db_min, db_max) if fmt == U8 else d


# ---- inputs -------------------------------------------------------------------------------------------------------

SWEEP_DB_MIN, SWEEP_DB_MAX = -100.0, 0.0
SWEEP_KS = tuple(range(0, 239, 17))  # 15 code boundaries k + 0.5


def boundary_sweep_powers() -> np.ndarray:
    """For each k of SWEEP_KS the 81 consecutive floats around 10^((db_min + (k + 0.5) / scale) / 10): powers whose dB
    values straddle the boundary between the codes k and k + 1 (1215 values)."""
    scale = 255.0 / (SWEEP_DB_MAX - SWEEP_DB_MIN)
    out = []
    for k in SWEEP_KS:
        centre = f32(10.0 ** ((SWEEP_DB_MIN + (k + 0.5) / scale) / 10.0))
        bits = np.array([centre], dtype=np.float32).view(np.uint32)[0]
        out.append((bits + np.arange(-40, 41, dtype=np.int64)).astype(np.uint32).view(np.float32))
    return np.concatenate(out)


def special_powers() -> np.ndarray:
    """Zeros, denormals, the smallest normal, FLT_MAX and +inf."""
    tiny = np.array([1, 2, 0x7FFFFF, 0x800000], dtype=np.uint32).view(np.float32)
    return np.concatenate([np.zeros(2, np.float32), tiny, np.array([np.finfo(np.float32).max, np.inf], np.float32)])


def noise_spectra(B: int, n: int, seed: int) -> np.ndarray:
    """Exponential (chi-square, 2 degrees) powers around 1e-3 with a few strong bins per row."""
    rng = np.random.default_rng(seed)
    s = (rng.exponential(1e-3, size=(B, n))).astype(np.float32)
    for b in range(B):
        s[b, rng.integers(0, n, size=3)] *= f32(1e4)
    return s


def summable_spectra(B: int, n: int, seed: int) -> np.ndarray:
    """Powers k * 2^-10, k a random integer in [0, 4095]: every double sum of up to 2^41 of them is exact, in any
    order, so the MEAN columns have one right answer."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 4096, size=(B, n)).astype(np.float32) * f32(2.0 ** -10)).astype(np.float32)
