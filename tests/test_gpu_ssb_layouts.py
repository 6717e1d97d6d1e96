"""Every FIR slot layout and both kernel families of the SSB chain (csrc/ssb.hip) on the GPU: the shapes of
tests/ssb_cases.py (proved on the CPU by tests/test_ssb_cases.py to reach the 4-, 8-, 16- and 32-slot layouts with 255
and with 127 taps, the lane-per-stream kernels with the plain reference chain, 8 outputs per chunk, D > chunk and
D > chunk + taps, both loaders per format and the output-count boundaries), 45 streams, three calls.

Bar: every PCM sample of every stream and call equals the oracle's processSSB_opt restatement (pinned to the
reference build by tests/golden); no tolerance."""
import numpy as np
import pytest

from conftest import load_golden

import ssb_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import sdrg
    return sdrg


@pytest.fixture(scope="module")
def O():
    import oracle
    return oracle


@pytest.fixture(scope="module")
def ref(O):
    """(raw[stream][call], want[call][stream]) per shape, computed once and shared"""
    cache = {}

    def get(c, calls=C.CALLS, modes=None, seed=0x55B):
        key = (C.case_id(c), calls, seed)
        if key not in cache:
            raw = C.batch(c["fmt"], C.B, calls, c["n"], c["fs"], seed)
            want = C.oracle_pcm(O, raw, c["fmt"], c["n"], c["fs"], modes or [1] * calls, True, c.get("taps", 0),
                                c.get("nco", 0.0))
            cache[key] = (raw, want)
        return cache[key]
    return get


def engine(S, c, B=C.B):
    eng = S.Engine(S.SDRConfig(centerFrequency=100_000_000, samplesPerReading=c["n"], sampleRate=c["fs"],
                               freqFocusRangeKhz=5, soundMode=1), B)
    if c.get("taps") or c.get("nco"):
        eng.set_ssb_variant(c.get("nco", 0.0), c.get("taps", 0))
    return eng


def check(pcm, want, fmt, what):
    for b in range(pcm.shape[0]):
        np.testing.assert_array_equal(pcm[b], want[b], err_msg=f"{what} stream {b} (family {C.family_of(fmt, b) + 1})")


@pytest.mark.parametrize("c", C.SHAPES + C.BOUNDARIES, ids=C.case_id)
def test_layout_pcm_bit_exact(S, O, ref, c):
    L = S.ssb_layout(c["fs"], c["n"], c["taps"])
    raw, want = ref(c)
    eng = engine(S, c)
    assert eng.pcm_len == L["pcm_len"] == O.ssb_pcm_len(c["n"], c["fs"], c["taps"])
    for f in range(C.CALLS):
        _, _, pcm = eng.process(np.ascontiguousarray(raw[:, f]), fmt=getattr(O, c["fmt"]), stages=S.STAGE_SSB)
        assert pcm.shape == (C.B, L["pcm_len"])
        check(pcm, want[f], c["fmt"], f"{C.case_id(c)} slots {L['slots']} call {f}")
    eng.close()


@pytest.mark.parametrize("c", C.SWITCH_BACK, ids=C.case_id)
def test_short_fir_switched_off_again(S, O, c):
    """127 taps for two calls, then the reference's 255: the taps and the chunk table are re-derived for the 16- and
    the 32-slot layout (as test_variant_switch_back_to_reference_chain does at 8 slots), filter state carried over"""
    fmt, n, fs, F = getattr(O, c["fmt"]), c["n"], c["fs"], 4
    raw = C.batch(c["fmt"], C.B, F, n, fs, seed=0x5B1)
    eng = engine(S, c)
    sst = [O.SsbState() for _ in range(C.B)]
    for f in range(F):
        taps = 127 if f < 2 else 0
        if f in (0, 2):
            eng.set_ssb_variant(0.0, taps)
            for st in sst:
                st.set_variant(0.0, fs, taps)
        _, _, pcm = eng.process(np.ascontiguousarray(raw[:, f]), fmt=fmt, stages=S.STAGE_SSB)
        assert pcm.shape[1] == eng.pcm_len == S.ssb_layout(fs, n, taps)["pcm_len"]
        for b in range(C.B):
            np.testing.assert_array_equal(pcm[b], sst[b].process(O.unpack(fmt, raw[b, f], n), fs, 1),
                                          err_msg=f"{C.case_id(c)} stream {b} call {f}")
    eng.close()


@pytest.mark.parametrize("c", C.PIPELINED, ids=C.case_id)
def test_pipelined_schedule_equals_joined(S, O, ref, c):
    """three calls enqueued back to back, one synchronisation: byte-equal to the joined run (and so to the oracle),
    at 16 and at 32 slots (tests/test_gpu_ssb_chunk_tail.py does this at 8)"""
    import torch
    fmt = getattr(O, c["fmt"])
    raw, want = ref(c)
    eng = engine(S, c)
    joined = []
    for f in range(C.CALLS):
        _, _, pcm = eng.process(np.ascontiguousarray(raw[:, f]), fmt=fmt, stages=S.STAGE_SSB)
        check(pcm, want[f], c["fmt"], f"{C.case_id(c)} joined call {f}")
        joined.append(np.array(pcm, copy=True))
    eng.close()
    dev = torch.device("cuda:0")
    eng = engine(S, c)
    eng.set_pipelining(S.PIPELINE_ON)
    src = [torch.from_numpy(np.ascontiguousarray(raw[:, f])).to(dev) for f in range(C.CALLS)]
    out = [torch.empty((C.B, eng.pcm_len), dtype=torch.int16, device=dev) for _ in range(C.CALLS)]
    torch.cuda.synchronize()
    for f in range(C.CALLS):
        eng.process_device(src[f].data_ptr(), fmt, S.STAGE_SSB, None, None, out[f].data_ptr(), 1000 + 8 * f)
    eng.synchronize()
    for f in range(C.CALLS):
        assert out[f].cpu().numpy().tobytes() == joined[f].tobytes(), f"pipelined call {f}"
    eng.close()


@pytest.mark.parametrize("case", C.GOLDEN_SSB_CASES)
def test_ssb_pcm_bit_exact_vs_reference_fixtures_at_the_new_rates(S, case):
    """the reference build's own PCM (tests/golden/make_golden.py) at D = 5, 10, 21 and 208"""
    g = load_golden(case)
    St, F = g["raw"].shape[:2]
    n, fs, fmt = int(g["n"]), int(g["fs"]), int(g["fmt"])
    for s in range(St):  # one engine per stream: its sound-mode sequence and its sideband are its own
        eng = S.Engine(S.SDRConfig(centerFrequency=100_000_000, samplesPerReading=n, sampleRate=fs,
                                   freqFocusRangeKhz=5, soundMode=int(g["modes"][s, 0])), 1)
        eng.setUpperSideband(bool(g["upper"][s]))
        for f in range(F):
            eng.setSoundMode(int(g["modes"][s, f]))
            _, _, pcm = eng.process(g["raw"][s, f][None], fmt=fmt, stages=S.STAGE_SSB)
            np.testing.assert_array_equal(pcm[0], g["pcm"][s, f], err_msg=f"{case} stream {s} frame {f}")
        eng.close()
