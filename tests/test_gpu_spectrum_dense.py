"""The spectrum kernels on dense (white-noise) input, where the per-bin bar constrains every bin, plus the RMS bar of
tests/spectrum_cases.py ("Dense-input bar"): every dedicated power-of-two instantiation in every
format, the persistent loops and the waves of the large batches, and the tiles and waves of csrc/fftany.hip.

Every case is one sdrg.Engine.process call of STAGE_SPECTRUM unless it says otherwise.  The two pipelined cases go
through process_device: process() joins the SSB stream in the call, so launch_spectrum's beside_ssb is never set on it.
Batch sizes come from the launchers' own arithmetic, restated in spectrum_cases.py and checked against the sources in
tests/test_spectrum_check.py.  Each test prints its figures (a line starting DENSE) before it asserts."""
import json

import numpy as np
import pytest

import spectrum_cases as sc

pytestmark = pytest.mark.gpu

FS, CF, WIDE_FOCUS_KHZ = 2_000_000, 100_000_000, 200
SPECTRUM, STATS, SSB = 1, 2, 4


@pytest.fixture(scope="module")
def S():
    import sdrg
    assert (sdrg.STAGE_SPECTRUM, sdrg.STAGE_STATS, sdrg.STAGE_SSB) == (SPECTRUM, STATS, SSB)
    assert (sdrg.CF32, sdrg.CS8, sdrg.CU8, sdrg.CS16) == (sc.CF32, sc.CS8, sc.CU8, sc.CS16)
    return sdrg


@pytest.fixture(scope="module")
def O():
    import oracle
    return oracle


@pytest.fixture(scope="module")
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


_inputs = {}  # (fmt, n, B) -> (raw, x, reference): the small batches two tests share


def batch(fmt, n, B):
    key = (fmt, n, B)
    if key in _inputs:
        return _inputs[key]
    raw = sc.dense_frames(fmt, n, B, sc.SEED)
    x = sc.unpack(fmt, raw)
    out = (raw, x, sc.reference(x))
    if n * B <= 1 << 18:
        _inputs[key] = out
    return out


def report(what, fmt, fig):
    print("DENSE", json.dumps({"case": what, "fmt": sc.FMT_NAMES[fmt], **fig}))


def run(S, fmt, n, B, stages=SPECTRUM, focus=5):
    raw, x, ref = batch(fmt, n, B)
    cfg = S.SDRConfig(centerFrequency=CF, samplesPerReading=n, sampleRate=FS, freqFocusRangeKhz=focus, soundMode=1)
    eng = S.Engine(cfg, B)
    try:
        spec = eng.process(raw, fmt=fmt, stages=stages, now_ms=1000)[0]
    finally:
        eng.close()
    return spec, x, ref


def check(what, fmt, spec, x, ref, fresh=True):
    """Figures first (computed without asserting), then the checker."""
    n = spec.shape[1]
    last = n - 1 if n % 2 else n
    if last > 0:
        pooled = n < 64
        e = sc.rms_error(spec[:, :last].astype(np.float64), ref[0][:, :last], pooled)
        e32 = sc.rms_error(ref[1][:, :last], ref[0][:, :last], pooled)
        report(what, fmt, {"n": n, "frames": spec.shape[0], "E_max": float(e.max()), "E_mean": float(e.mean()),
                           "E_ref32_max": float(e32.max()),
                           "E_over_bound": float(np.max(e / (sc.RMS_MARGIN * np.maximum(e32, sc.RMS_FLOOR))))})
    return sc.check_spectrum(spec, x, fresh=fresh, ref=ref)


# --------------------------------------------------------------------------------------------------
# A. every dedicated instantiation: 11 sizes x 4 formats
# --------------------------------------------------------------------------------------------------
def small_b(n):
    return 3 if n <= 16384 else 2


@pytest.mark.parametrize("fmt", sc.FORMATS, ids=sc.FMT_NAMES.get)
@pytest.mark.parametrize("n", sc.POW2_SIZES)
def test_every_instantiation(S, n, fmt):
    assert sc.pow2_kernels(n)
    check(f"A n{n}", fmt, *run(S, fmt, n, small_b(n)))


@pytest.mark.parametrize("fmt", sc.FORMATS, ids=sc.FMT_NAMES.get)
@pytest.mark.parametrize("n", [32768, 65536])
def test_non_persistent_four_step_beside_wide_stats(S, O, n, fmt):
    """STAGE_STATS with a focus that takes the wide statistics kernel: launch_spectrum then runs four_step_a /
    four_step_b, one tile per workgroup, in place of the persistent pair."""
    assert sc.stats_stage_bins(O, FS, n, WIDE_FOCUS_KHZ) > sc.STATS_STAGE_MAX
    check(f"A wide n{n}", fmt, *run(S, fmt, n, small_b(n), stages=SPECTRUM | STATS, focus=WIDE_FOCUS_KHZ))


def run_pipelined(S, fmt, n, B):
    """One pipelined device-path call with the SSB stage: beside_ssb (one workgroup per CU at 16384, no issue priority
    at 32768 / 65536).  The spectrum alone is checked; its buffer is not a fresh engine's."""
    import torch
    dev = torch.device("cuda:0")
    raw, x, ref = batch(fmt, n, B)
    cfg = S.SDRConfig(centerFrequency=CF, samplesPerReading=n, sampleRate=FS, freqFocusRangeKhz=5, soundMode=1)
    eng = S.Engine(cfg, B)
    try:
        eng.set_pipelining(S.PIPELINE_ON)
        d_iq = torch.from_numpy(raw).to(dev)
        d_spec = torch.full((B, n), float("nan"), dtype=torch.float32, device=dev)
        d_pcm = torch.empty((B, eng.pcm_len), dtype=torch.int16, device=dev)
        torch.cuda.synchronize()
        eng.process_device(d_iq.data_ptr(), fmt, SPECTRUM | SSB, d_spec.data_ptr(), None, d_pcm.data_ptr(), 1000)
        eng.synchronize()
        spec = d_spec.cpu().numpy()
    finally:
        eng.close()
    return spec, x, ref


def test_pipelined_beside_ssb_16384(S, cus):
    """One workgroup per CU: 2 CUs + 3 frames make every workgroup loop at least twice."""
    check("A beside_ssb n16384", sc.CS8, *run_pipelined(S, sc.CS8, 16384, 2 * cus + 3), fresh=False)


def test_pipelined_beside_ssb_65536(S):
    check("A beside_ssb n65536", sc.CS16, *run_pipelined(S, sc.CS16, 65536, 3), fresh=False)


# --------------------------------------------------------------------------------------------------
# B. persistent loops and waves
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", sc.FORMATS, ids=sc.FMT_NAMES.get)
def test_persistent_16384_loops(S, cus, fmt):
    """spectrum16k_kernel: two workgroups per CU, so 2 CUs + 3 frames run the frame += gridDim.x loop and its
    next-frame prefetch, three workgroups once more than the others."""
    check("B n16384", fmt, *run(S, fmt, 16384, 2 * cus + 3))


def test_four_step_two_waves_cs8(S):
    """65536: a full wave (the tile loops of four_step_a_p / four_step_b_p iterate, with prefetch) and a second wave
    of one frame (f0 > 0)."""
    B = sc.spectrum_wave_frames(65536) + 1
    assert B == 257
    check("B n65536 waves", sc.CS8, *run(S, sc.CS8, 65536, B))


def test_four_step_tile_loop_cf32(S):
    """65536 CF32, above 64 frames: four_step_a_p's loop on its path without the raw-word prefetch."""
    check("B n65536 cf32", sc.CF32, *run(S, sc.CF32, 65536, 70))


def test_non_persistent_two_waves_cu8(S, O):
    assert sc.stats_stage_bins(O, FS, 65536, WIDE_FOCUS_KHZ) > sc.STATS_STAGE_MAX
    B = sc.spectrum_wave_frames(65536) + 1
    check("B wide n65536 waves", sc.CU8, *run(S, sc.CU8, 65536, B, stages=SPECTRUM | STATS, focus=WIDE_FOCUS_KHZ))


def test_four_step_two_waves_32768_cs16(S):
    B = sc.spectrum_wave_frames(32768) + 1
    assert B == 513
    check("B n32768 waves", sc.CS16, *run(S, sc.CS16, 32768, B))


# --------------------------------------------------------------------------------------------------
# C. fftany.hip: ragged tiles of the one-workgroup kernels, waves of the four-step ones
# --------------------------------------------------------------------------------------------------
ANY = [(n, fmt, mode, fr) for n, fmts, mode, fr in sc.ANY_CASES for fmt in fmts]


@pytest.mark.parametrize("n,fmt,mode,frames", ANY, ids=[f"{m}-{n}-{sc.FMT_NAMES[f]}-{fr}" for n, f, m, fr in ANY])
def test_any_n_tiles_and_waves(S, n, fmt, mode, frames):
    assert sc.any_plan(n)["mode"] == mode
    check(f"C {mode} n{n}", fmt, *run(S, fmt, n, sc.any_case_frames(n, frames)))
