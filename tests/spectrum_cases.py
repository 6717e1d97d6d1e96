"""Dense inputs, a numpy-only float64 reference and the checker for the spectrum tests (DESIGN.md section 4,
"Dense-input bar").

The spectrum's per-bin bar |dP| <= 1e-4 P + 1e-6 max(P) says little about a tone over weak noise: 1e-6 max(P) is
then larger than most bins, so zeros or a neighbour's value pass.  White noise has max(P) / mean(P) ~ ln N, so the
same bar constrains every bin; check_spectrum first asserts that the input has this property, then the per-bin
bar, then an RMS bar relative to numpy's own complex64 transform.

  dense_frames(fmt, n, B, seed) -> raw [B][2n]      white Gaussian IQ, no tone, quantised as oracle.synth_frames does
  unpack(fmt, raw)              -> complex128 [B][n] the samples the engine's convert_scaled produces (spectrum.hip)
  reference(x)                  -> (P64, P32)        fftshifted |FFT|^2 in float64, and numpy's complex64 transform
  check_spectrum(got, x)        -> dict of figures   asserts, in order: input condition, per-bin, RMS, odd tail

and restatements of the launchers' batch arithmetic (fftany.hip any_plan / any_wave_frames / fft1 tile,
sdrg_internal.h spectrum_wave_frames, stats.hip stage_bins), which the GPU tests size their batches with;
tests/test_spectrum_check.py compares their constants with the sources.
"""
from __future__ import annotations

import numpy as np

CF32, CS8, CU8, CS16 = 0, 1, 2, 3  # sdrg / oracle format codes
FMT_NAMES = {CF32: "CF32", CS8: "CS8", CU8: "CU8", CS16: "CS16"}
NUMPY_DTYPE = {CF32: np.float32, CS8: np.int8, CU8: np.uint8, CS16: np.int16}
SIGMA = {CS8: 30.0, CU8: 30.0, CS16: 8000.0, CF32: 0.25}

RTOL, ATOL_MAX = 1e-4, 1e-6          # the project's per-bin bar
ZERO_SHARE, NEIGHBOUR_SHARE = 1e-3, 5e-3
RMS_MARGIN, RMS_FLOOR = 16.0, 5e-8
CHUNK_POINTS = 1 << 22               # frames per numpy transform: bounds the float64 temporaries
SEED = 7                             # of every batch both test files build (dense_frames also mixes in fmt, n, B)


# --------------------------------------------------------------------------------------------------
# input
# --------------------------------------------------------------------------------------------------
def dense_frames(fmt: int, n: int, B: int, seed: int) -> np.ndarray:
    """[B][2n] raw interleaved IQ: independent Gaussian I and Q for every sample of every frame."""
    rng = np.random.default_rng([seed, fmt, n, B])
    iq = rng.normal(0.0, SIGMA[fmt], (B, 2 * n))
    if fmt == CS8:
        return np.clip(np.round(iq), -128, 127).astype(np.int8)
    if fmt == CU8:
        return np.clip(np.round(iq + 127.4), 0, 255).astype(np.uint8)
    if fmt == CS16:
        return np.clip(np.round(iq), -32768, 32767).astype(np.int16)
    return iq.astype(np.float32)


def unpack(fmt: int, raw: np.ndarray, cu8_offset: float = 127.4) -> np.ndarray:
    """convert_scaled's values, in its float32 arithmetic (every result is a float32, so the complex64 cast of
    reference() is exact and both transforms see the numbers the kernels see)."""
    raw = np.asarray(raw)
    v = raw.astype(np.float32)
    if fmt == CS8:
        v = v * np.float32(1.0 / 128.0)
    elif fmt == CU8:
        v = (v - np.float32(cu8_offset)) * np.float32(1.0 / 128.0)
    elif fmt == CS16:
        v = v * np.float32(1.0 / 32768.0)
    assert v.dtype == np.float32
    v = v.reshape(raw.shape[0], -1, 2).astype(np.float64)
    return v[..., 0] + 1j * v[..., 1]


# --------------------------------------------------------------------------------------------------
# reference
# --------------------------------------------------------------------------------------------------
def shift_reference(power: np.ndarray) -> np.ndarray:
    """The reference's fftshift loop over the last axis (out[i] = P[i + N/2], out[i + N/2] = P[i], i < N/2): for
    odd N element N-1 of a fresh vector stays 0 and P[N-1] is dropped."""
    half = power.shape[-1] // 2
    out = np.zeros_like(power)
    out[..., :half] = power[..., half:2 * half]
    out[..., half:2 * half] = power[..., :half]
    return out


def reference(x: np.ndarray):
    """x complex [B][n] -> (P64 float64 [B][n], P32 float32 [B][n]), both fftshifted as the reference does."""
    x = np.asarray(x, dtype=np.complex128)
    B, n = x.shape
    p64 = np.empty((B, n), np.float64)
    p32 = np.empty((B, n), np.float32)
    step = max(1, CHUNK_POINTS // n)
    for b0 in range(0, B, step):
        xc = x[b0:b0 + step]
        X = np.fft.fft(xc, axis=1)
        assert X.dtype == np.complex128
        p64[b0:b0 + step] = shift_reference(X.real * X.real + X.imag * X.imag)
        X32 = np.fft.fft(xc.astype(np.complex64), axis=1)
        assert X32.dtype == np.complex64, "numpy computed the complex64 transform in another precision"
        p = X32.real * X32.real + X32.imag * X32.imag
        assert p.dtype == np.float32
        p32[b0:b0 + step] = shift_reference(p)
    return p64, p32


def rms_error(got: np.ndarray, p64: np.ndarray, pooled: bool) -> np.ndarray:
    """E = sqrt(mean((got - P64)^2)) / mean(P64): per frame [B], or one value over the whole batch [1]."""
    d = got.astype(np.float64) - p64
    if pooled:
        return np.array([np.sqrt(np.mean(d * d)) / np.mean(p64)])
    return np.sqrt(np.mean(d * d, axis=1)) / np.mean(p64, axis=1)


# --------------------------------------------------------------------------------------------------
# checker
# --------------------------------------------------------------------------------------------------
def check_spectrum(got: np.ndarray, x: np.ndarray, fresh: bool = True, ref=None) -> dict:
    """Assert that got [B][n] (float32) is the spectrum of x [B][n] (complex, unpack()'s values).

    In order (the message of the AssertionError starts with the name):
      input condition  share of bins where 0.0 would pass the per-bin bar <= 1e-3 and, for N >= 64, share where the
                       next bin's value would pass <= 5e-3: a property of x alone, it keeps the test from going blind
      per-bin bound    |dP| <= 1e-4 P + 1e-6 max(P), every bin of every frame, max(P) per frame
      rms bound        E <= 16 max(E_ref32, 5e-8), E_ref32 numpy's complex64 transform with the power in float32.
                       Per frame for N >= 64; for N < 64 one value over the batch (a frame has too few bins for a
                       mean, and E_ref32 was only measured per frame from 64 up)
      odd tail         odd N, fresh engine: got[N-1] == 0.0 exactly
    For odd N element N-1 takes no part in the first three (it is no output of the transform); N = 1 has nothing else.
    ref: a (P64, P32) pair computed before with reference(x), to share among checks of the same input.
    Returns the figures (shares, worst per-bin ratio, E, E_ref32, E / bound)."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.ndim == 2, (got.dtype, got.shape)
    B, n = got.shape
    assert x.shape == (B, n), (x.shape, got.shape)
    p64, p32 = reference(x) if ref is None else ref
    last = n - 1 if n % 2 else n
    fig = {"n": n, "frames": B}
    if last > 0:
        P, G = p64[:, :last], got[:, :last].astype(np.float64)
        tol = RTOL * P + ATOL_MAX * P.max(axis=1, keepdims=True)
        fig["zero_share"] = float(np.mean(P <= tol))
        assert fig["zero_share"] <= ZERO_SHARE, f"input condition: 0.0 passes at {fig['zero_share']:.2e} of the bins"
        if n >= 64:
            nb = np.abs(P[:, 1:] - P[:, :-1])
            fig["neighbour_share"] = float(np.mean(nb <= tol[:, :-1]))
            assert fig["neighbour_share"] <= NEIGHBOUR_SHARE, \
                f"input condition: a neighbour's value passes at {fig['neighbour_share']:.2e} of the bins"
        err = np.abs(G - P)
        bad = ~(err <= tol)  # NaN fails
        with np.errstate(divide="ignore", invalid="ignore"):
            fig["per_bin_worst"] = float(np.nanmax(err / tol))
        assert not bad.any(), (f"per-bin bound: {int(bad.sum())} bins of {bad.size}, first (frame, bin) "
                               f"{np.argwhere(bad)[:4].tolist()}, got {G[bad][:4]}, want {P[bad][:4]}")
        pooled = n < 64
        e = rms_error(G, P, pooled)
        e32 = rms_error(p32[:, :last], P, pooled)
        bound = RMS_MARGIN * np.maximum(e32, RMS_FLOOR)
        w = int(np.argmax(e / bound))
        fig.update(E=float(e.max()), E_ref32=float(e32.max()), E_over_bound=float(e[w] / bound[w]))
        assert (e <= bound).all(), (f"rms bound: E = {e[w]:.3e} > 16 max(E_ref32 = {e32[w]:.3e}, 5e-8) at frame "
                                    f"{'(all)' if pooled else w}; {int((e > bound).sum())} of {e.size} over")
    if n % 2 and fresh:
        tail = got[:, n - 1]
        assert (tail == 0.0).all(), f"odd tail: element N-1 is {tail[tail != 0.0][:4]} at frames {np.flatnonzero(tail)[:4]}"
    return fig


# --------------------------------------------------------------------------------------------------
# the launchers' batch arithmetic, restated
# --------------------------------------------------------------------------------------------------
TILE_MAX, TILE_TARGET = 16384, 8192  # fftany.hip
WAVE_BYTES = 128 << 20               # sdrg_internal.h SPECTRUM_WAVE_BYTES, fftany.hip any_wave_frames
STATS_STAGE_MAX = 8192               # stats.hip STAGE_MAX


def smooth13(n: int) -> bool:
    for p in (2, 3, 5, 7, 11, 13):
        while n % p == 0:
            n //= p
    return n == 1


def pow2_kernels(n: int) -> bool:
    """launch_spectrum's dedicated instantiations (spectrum.hip); every other N goes through any_plan."""
    return 64 <= n <= 65536 and n & (n - 1) == 0


def any_plan(n: int) -> dict:
    """fftany.hip any_plan: mode ONE / FOUR / BLUE_ONE / BLUE_FOUR and the transform length m."""
    if smooth13(n) and n <= TILE_MAX:
        return {"mode": "ONE", "n": n, "m": n}
    if smooth13(n):
        best, d = 0, 1
        while d * d <= n:
            if n % d == 0 and n // d <= TILE_MAX:
                best = d
            d += 1
        if best:
            return {"mode": "FOUR", "n": n, "m": n, "n1": best, "n2": n // best}
    m = 1
    while m < 2 * n - 1:
        m <<= 1
    return {"mode": "BLUE_ONE" if m <= TILE_MAX else "BLUE_FOUR", "n": n, "m": m}


def fft1_tile_frames(n: int, B: int) -> int:
    """Frames one fft1_kernel workgroup packs (launch_any_fmt: C = max(1, min(B, TILE_TARGET / m)))."""
    return max(1, min(B, TILE_TARGET // any_plan(n)["m"]))


def any_wave_frames(n: int) -> int:
    """Frames per four-step wave of fftany.hip before the min with the batch (any_wave_frames)."""
    p = any_plan(n)
    per = p["m"] * 8 * (2 if p["mode"] == "BLUE_FOUR" else 1)
    return max(1, WAVE_BYTES // per)


def spectrum_wave_frames(n: int) -> int:
    """sdrg_internal.h spectrum_wave_frames (N = 32768 / 65536)."""
    return WAVE_BYTES // (n * 8)


def stats_stage_bins(oracle, fs: int, n: int, focus_khz: int) -> int:
    """stats.hip stage_bins: stats_uses_wide(geo) is stage_bins > STAGE_MAX.  The geometry is the oracle's
    (tests/test_oracle.py pins it; design.cpp computes the same windows)."""
    lo, hi, _, wins = oracle.window_geometry(fs, n, focus_khz)
    return max(0, hi - lo + 1) + sum(max(0, h - l + 1) for l, h in wins[:10])


# --------------------------------------------------------------------------------------------------
# the case matrix (tests/test_gpu_spectrum_dense.py runs it on the GPU, tests/test_spectrum_check.py feeds the
# checker numpy's complex64 result for every entry)
# --------------------------------------------------------------------------------------------------
FORMATS = (CS8, CU8, CS16, CF32)
POW2_SIZES = tuple(1 << k for k in range(6, 17))  # one launch_spectrum instantiation each, x 4 formats

# fftany.hip: (n, formats, mode any_plan must give, frames).  frames: an int, or "tile" = three more than one fft1
# workgroup can pack (a second, ragged tile), or "wave" = one more than a four-step wave holds.  Odd N runs with both
# 1-byte formats (frames from 1 on start 2-byte aligned only); the others with a format tests/test_gpu_any_n.py
# (fmts[n % 3] of CS8, CS16, CF32) does not give them.
ANY_CASES = (
    (1536, (CU8,), "ONE", 7),          # C = 5: tiles of 5 and 2
    (1000, (CF32,), "ONE", 19),        # C = 8: 8, 8, 3
    (7, (CS8, CU8), "ONE", 515),       # 13-smooth, so no Bluestein: one full tile of 515 frames
    (7, (CS8, CU8), "ONE", "tile"),    # C = 1170: 1170 and 3
    (3, (CS8, CU8), "ONE", 3000),      # C = 2730
    (2, (CS16,), "ONE", 4100),         # C = 4096
    (1, (CS8, CU8), "ONE", 8200),      # C = 8192
    (97, (CS8, CU8), "BLUE_ONE", 37),  # M = 256, C = 32: 32 and 5
    (17, (CS8, CU8), "BLUE_ONE", "tile"),  # the smallest N that is not 13-smooth: M = 64, C = 128
    (4099, (CS8, CU8), "BLUE_ONE", 3),     # M = 8192, C = 1
    (20000, (CS16,), "FOUR", 3),
    (786432, (CU8,), "FOUR", "wave"),      # 21 frames per wave
    (12289, (CS8, CU8), "BLUE_FOUR", 3),
    (65537, (CS8, CU8), "BLUE_FOUR", 3),
    (999983, (CS8, CU8), "BLUE_FOUR", "wave"),  # M = 2^21, 4 frames per wave
)


def any_case_frames(n: int, frames) -> int:
    if frames == "tile":
        return TILE_TARGET // any_plan(n)["m"] + 3
    if frames == "wave":
        return any_wave_frames(n) + 1
    return frames
