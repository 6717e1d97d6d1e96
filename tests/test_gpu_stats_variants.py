"""Every statistics kernel variant launch_stats (csrc/stats.hip) picks, and every branch the geometry selects inside
them, against the oracle, every record field bit for bit: the rows of tests/stats_cases.py CASES (the three narrow
instantiations with every reference-window count, stats_wide_multi_kernel<true> and <false>, stats_wide_kernel with
one bottom window and its gaps in registers or in HBM scratch, and with several), each on a selection threshold or
one step past it where the geometry allows.  tests/test_stats_cases.py checks on the CPU that the labels are what the
launcher's arithmetic gives, that no variant a sweep of geometries reaches lacks a row, and that the spectra fed here
put the decisions where the kernels differ (stats_cases.py, "input kinds").

Then one engine walked across the variants with setFrequencyFocusRange (the stream state and the pool scratch pass
from kernel to kernel), and two wide geometries end to end through process(), joined and with the statistics on a
stream of their own."""
import numpy as np
import pytest

import stats_cases as sc
from test_gpu_parity import assert_records_equal

pytestmark = pytest.mark.gpu

CF = 100_000_000
RUNS = [(i, row, sc.case_streams(row[3])) for i, row in enumerate(sc.CASES)] + \
       [(sc.CASES.index(row), row, 1) for row in sc.SINGLE_STREAM_ROWS]


@pytest.fixture(scope="module")
def S():
    import sdrg
    return sdrg


@pytest.fixture(scope="module")
def O():
    import oracle
    return oracle


def config(S, n, fs, focus):
    return S.SDRConfig(centerFrequency=CF, samplesPerReading=n, sampleRate=fs, freqFocusRangeKhz=focus, soundMode=1)


def oracle_records(fst, spec, now, dtype):
    want = np.zeros(len(fst), dtype=dtype)
    for b, st in enumerate(fst):
        want[b] = st.signal_strength(spec[b], now)
    return want


@pytest.mark.parametrize("index,row,B", RUNS, ids=[f"{r[3]}-{sc.case_id(r)}-B{B}" for _, r, B in RUNS])
def test_variant_bit_exact(S, O, index, row, B):
    n, fs, focus, label = row
    assert sc.plan(sc.geometry(fs, n, focus)) == label
    eng = S.Engine(config(S, n, fs, focus), B)
    fst = [O.FftState(CF, fs, n, focus) for _ in range(B)]
    for call in range(sc.CALLS):
        spec = sc.case_spectra(row, index, B, call)
        now = 1000 + 333 * call
        rec = eng.signal_strength(spec, now)
        assert_records_equal(rec, oracle_records(fst, spec, now, rec.dtype),
                             msg=f"{label} {sc.case_id(row)} B{B} call{call} kinds "
                                 f"{[sc.kind_of(b, call) for b in range(B)]}")
    eng.close()


def test_one_engine_across_the_variants(S, O):
    """setFrequencyFocusRange 5 -> 200 -> 225 -> 400 -> 60 -> 5 kHz at 65536 bins: narrow, multi<true>, the single-frame
    kernel with one bottom window, multi<false>, the single-frame kernel with three, narrow again.  Each stream's
    state (the stale outputs through the invalid stretch at 400 kHz, the tracking latch, the detection ring) goes
    from kernel to kernel, and the engine's pool scratch is grown and reused."""
    n, fs, B = sc.WALK_N, sc.WALK_FS, sc.WALK_STREAMS
    eng = S.Engine(config(S, n, fs, sc.WALK[0][0]), B)
    fst = [O.FftState(CF, fs, n, sc.WALK[0][0]) for _ in range(B)]
    for step, (focus, label) in enumerate(sc.WALK):
        assert sc.plan(sc.geometry(fs, n, focus)) == label
        eng.setFrequencyFocusRange(focus)
        for st in fst:
            st.configure(CF, fs, n, focus)
        for k in range(sc.WALK_CALLS):
            spec = sc.walk_spectra(step, k)
            now = 1000 + 150 * (sc.WALK_CALLS * step + k)
            rec = eng.signal_strength(spec, now)
            assert_records_equal(rec, oracle_records(fst, spec, now, rec.dtype), msg=f"step{step} {label} call{k}")
    eng.close()


@pytest.mark.parametrize("focus,label", sc.E2E, ids=[label for _, label in sc.E2E])
def test_end_to_end_joined_and_async(S, O, focus, label):
    """process() with the spectrum and the statistics at 65536 CS16 samples: the records equal the oracle's on the
    GPU's own spectrum, and three calls on ONE spectra buffer with the statistics on a stream of their own
    (PIPELINE_INPUTS_READY | PIPELINE_STATS_ASYNC: the kernel then runs on that stream with the engine's pool) give
    the joined schedule's records byte for byte."""
    import torch
    n, fs, B, F = sc.E2E_N, sc.E2E_FS, sc.E2E_STREAMS, sc.E2E_CALLS
    assert sc.plan(sc.geometry(fs, n, focus)) == label
    dev = torch.device("cuda:0")
    tones = [0.3 * focus * 1e3, -0.45 * focus * 1e3, 0.4 * fs, 700.0, 0.0, -0.2 * focus * 1e3]
    amps = [4000.0, 1500.0, 3000.0, 80.0, 0.0, 400.0]  # in and out of the focus, weak, noise only
    raws = [torch.from_numpy(np.stack([O.synth_frames(1, n, O.CS16, tone_hz=tones[b], fs=fs, amp=amps[b],
                                                      seed=1000 * focus + 10 * f + b)[0] for b in range(B)])).to(dev)
            for f in range(F)]
    stages = S.STAGE_SPECTRUM | S.STAGE_STATS
    got = {}
    for mode in (S.PIPELINE_OFF, S.PIPELINE_INPUTS_READY | S.PIPELINE_STATS_ASYNC):
        eng = S.Engine(config(S, n, fs, focus), B)
        eng.set_pipelining(mode)
        spec = torch.empty((B, n), dtype=torch.float32, device=dev)
        rec = [torch.zeros((B, S.RECORD_DTYPE.itemsize), dtype=torch.uint8, device=dev) for _ in range(F)]
        fst = [O.FftState(CF, fs, n, focus) for _ in range(B)]
        torch.cuda.synchronize()
        for f in range(F):
            now = 1000 + 120 * f
            eng.process_device(raws[f].data_ptr(), O.CS16, stages, spec.data_ptr(), rec[f].data_ptr(), None, now)
            if mode == S.PIPELINE_OFF:  # joined: this call's spectrum is still in the buffer
                eng.synchronize()
                have = np.frombuffer(rec[f].cpu().numpy().tobytes(), dtype=S.RECORD_DTYPE)
                assert_records_equal(have, oracle_records(fst, spec.cpu().numpy(), now, have.dtype),
                                     msg=f"{label} joined call{f}")
        eng.synchronize()
        torch.cuda.synchronize()
        got[mode] = torch.stack(rec).cpu()
        eng.close()
    assert torch.equal(got[S.PIPELINE_OFF], got[S.PIPELINE_INPUTS_READY | S.PIPELINE_STATS_ASYNC])
