"""The peak table stage (include/sdrg.h, sdrg_engine_peaks_*) restated in NumPy, and the inputs its tests share.

Per row of N powers and a span p = x[lo : lo + nb]: the floor F = sorted(p)[nb // 2]; dB(v) = 10.0f * log10f(v + 1e-20f)
(display_cases.db: libm's log10f through oracle/stats_np.log10f); bin j is a candidate iff p_j > p_i for every i in
[max(0, j - d), j) and p_j >= p_i for every i in (j, min(nb - 1, j + d)]; a candidate is above iff
dB(p_j) - dB(F) >= threshold_db in float32; the table holds the first min(n_above, max_peaks) above candidates by power
descending, then bin ascending, and {-1, 0, 0, 0} after them.  The candidate rule is stated twice: brute force,
O(nb d), and with log2-many shifted maxima; tests/test_peaks_cases.py checks one against the other and
tests/test_gpu_peaks.py the kernels against the fast one, as bytes."""
import numpy as np

import display_cases as dc

f32 = np.float32
PEAK_DTYPE = np.dtype([("bin", "<i4"), ("power", "<f4"), ("db", "<f4"), ("snr_db", "<f4")])
SUMMARY_DTYPE = np.dtype([("count", "<i4"), ("n_above", "<i4"), ("floor_power", "<f4"), ("floor_db", "<f4")])
MAX_PEAKS, MAX_SEPARATION = 64, 4096


def _bits(span) -> np.ndarray:
    """The powers' bit patterns as int64: finite powers >= +0 and +inf order as these integers."""
    return np.ascontiguousarray(span, dtype=np.float32).view(np.uint32).astype(np.int64)


def floor_power(span) -> np.float32:
    span = np.asarray(span, dtype=np.float32)
    return np.sort(span)[span.size // 2]


def candidates_brute(span, d: int) -> np.ndarray:
    """The definition, bin by bin."""
    p = _bits(span)
    nb = p.size
    out = np.zeros(nb, bool)
    for j in range(nb):
        left = p[max(0, j - d):j]
        right = p[j + 1:min(nb - 1, j + d) + 1]
        out[j] = bool(np.all(p[j] > left)) and bool(np.all(p[j] >= right))
    return out


def _shift(a: np.ndarray, s: int) -> np.ndarray:
    """out[j] = a[j - s], -1 (below every power) where j - s < 0."""
    out = np.full_like(a, -1)
    if s < a.size:
        out[s:] = a[:a.size - s]
    return out


def _trailing_max(a: np.ndarray, d: int) -> np.ndarray:
    """out[j] = max(a[max(0, j - d) : j]), -1 for j = 0: doubling up to the largest power of two <= d, then two
    overlapping windows of that size."""
    cur, size = a.copy(), 1
    while 2 * size <= d:
        cur = np.maximum(cur, _shift(cur, size))
        size *= 2
    return _shift(np.maximum(cur, _shift(cur, d - size)), 1)


def candidates(span, d: int) -> np.ndarray:
    p = _bits(span)
    return (p > _trailing_max(p, d)) & (p >= _trailing_max(p[::-1].copy(), d)[::-1])


def _above(span, cand_bins, threshold_db):
    """(db, snr, above) of the candidate bins: one float32 subtraction, a comparison NaN fails."""
    span = np.asarray(span, dtype=np.float32)
    floor_db = dc.db(floor_power(span))
    db = dc.db(span[cand_bins])
    with np.errstate(invalid="ignore"):
        snr = (db - floor_db).astype(np.float32)
        above = snr >= f32(threshold_db)
    return db, snr, above


def _strongest_first(span, bins) -> np.ndarray:
    """bins ordered by power descending, then bin ascending."""
    p = _bits(span)
    bins = np.asarray(bins, dtype=np.int64)
    return bins[np.lexsort((bins, -p[bins]))]


def table(span, lo: int, d: int, max_peaks: int, threshold_db, cand_fn=candidates, drop_last=False):
    """(peaks [max_peaks] PEAK_DTYPE, summary SUMMARY_DTYPE scalar) of one span.  drop_last: the other form of the
    result -- the top max_peaks candidates first, then those below the threshold dropped."""
    span = np.ascontiguousarray(span, dtype=np.float32)
    bins = np.flatnonzero(cand_fn(span, d))
    db, snr, above = _above(span, bins, threshold_db)
    n_above = int(above.sum())
    if drop_last:
        top = _strongest_first(span, bins)[:max_peaks]
        keep = top[above[np.searchsorted(bins, top)]]
    else:
        keep = _strongest_first(span, bins[above])[:max_peaks]
    at = np.searchsorted(bins, keep)
    pk = np.zeros(max_peaks, PEAK_DTYPE)
    pk["bin"] = -1
    k = keep.size
    pk["bin"][:k] = lo + keep
    pk["power"][:k] = span[keep]
    pk["db"][:k] = db[at]
    pk["snr_db"][:k] = snr[at]
    sm = np.zeros((), SUMMARY_DTYPE)
    sm["count"], sm["n_above"] = k, n_above
    sm["floor_power"] = floor_power(span)
    sm["floor_db"] = dc.db(floor_power(span))
    assert k == min(n_above, max_peaks) or drop_last
    return pk, sm


def tables(spectra, lo: int, nb: int, d: int, max_peaks: int, threshold_db):
    """(peaks [B][max_peaks], summary [B]) of [B][N] spectra."""
    spectra = np.asarray(spectra, dtype=np.float32)
    assert 0 <= lo and nb >= 1 and lo + nb <= spectra.shape[1]
    both = [table(r[lo:lo + nb], lo, d, max_peaks, threshold_db) for r in spectra]
    return np.stack([b[0] for b in both]), np.stack([b[1] for b in both])


def bin_offset_hz(n: int, sample_rate: int, b: int) -> float:
    return (float(b - n // 2) * float(sample_rate)) / float(n)


# ---- inputs -------------------------------------------------------------------------------------------------------

def quantised_rows(B: int, n: int, seed: int, levels: int = 8) -> np.ndarray:
    """Powers k / 8, k a random integer in [0, levels): ties everywhere."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, levels, size=(B, n)).astype(np.float32) * f32(0.125)).astype(np.float32)


def noise_rows(B: int, n: int, seed: int, tones: int = 0, tone_power: float = 1.0) -> np.ndarray:
    """Exponential powers around 1e-3, and `tones` bins per row of about tone_power with a skirt on both sides."""
    rng = np.random.default_rng(seed)
    s = rng.exponential(1e-3, size=(B, n)).astype(np.float32)
    for b in range(B):
        for j in rng.integers(0, n, size=tones):
            for k in range(-3, 4):
                if 0 <= j + k < n:
                    s[b, j + k] += f32(tone_power * rng.uniform(0.5, 1.0) / (1 + 4 * k * k))
    return s


def shared_high_bits_rows(B: int, n: int, seed: int) -> np.ndarray:
    """Powers whose bit patterns differ in the low 10 bits only (the select's first digit starts there)."""
    rng = np.random.default_rng(seed)
    base = np.array([0.001], np.float32).view(np.uint32)[0] & ~np.uint32(0x3FF)
    return (base + rng.integers(0, 1024, size=(B, n)).astype(np.uint32)).view(np.float32)


def ulp_pair_sharing_db(start: float = 1e6):
    """(a, b): two consecutive floats a < b near `start` with the same dB value (at 60 dB a float ulp of the dB value
    spans about ten ulps of the power)."""
    a = f32(start)
    for _ in range(64):
        b = np.nextafter(a, f32(np.inf))
        if dc.db(a) == dc.db(b):
            return a, b
        a = b
    raise AssertionError("no such pair")
