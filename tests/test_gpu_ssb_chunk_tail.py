"""The low-pass wave's rotated chunk loop (csrc/ssb_lpf_asm.h, SDRG_LPF_LOOP_IL_ASM): each chunk's first quad runs
before the previous chunk's barrier and is stored after it.  Frames of 1, 2, 3, 4 and 7 whole chunks cover the first
chunk's entry in mid-body, each chunk-mod-3 body as first and as last, the wrap and the dropped run-ahead quad after
the last chunk; 200 samples (not whole chunks) take the per-chunk path.  One full, one nearly empty and several
workgroups; three calls in a row, so the state carried over the rotated boundary is checked; PCM bit-exact against
the oracle's processSSB_opt restatement (as tests/test_gpu_ssb_schedule.py), joined and pipelined schedules equal."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FS, F, BMAX = 2_000_000, 3, 45
SIZES = [64, 128, 192, 256, 448, 200]
CASES = [("CS8", n) for n in SIZES] + [(f, 192) for f in ("CU8", "CS16", "CF32")]


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
    """(raw[stream, call], want[call][stream]) per (format, size), for BMAX streams, computed once: stream b's input
    and expected PCM do not depend on the batch it runs in"""
    cache = {}

    def get(fmt_name, n):
        if (fmt_name, n) not in cache:
            fmt = getattr(O, fmt_name)
            raw = np.stack([O.synth_frames(F, n, fmt, tone_hz=300.0 * (b + 1) - 3000.0, fs=FS, seed=501 + b)
                            for b in range(BMAX)])
            want = [[None] * BMAX for _ in range(F)]
            for b in range(BMAX):
                st = O.SsbState()
                for f in range(F):
                    want[f][b] = st.process(O.unpack(fmt, raw[b, f], n), FS, 1)
            cache[fmt_name, n] = (raw, want)
        return cache[fmt_name, n]
    return get


def engine(S, n, B):
    return S.Engine(S.SDRConfig(centerFrequency=100_000_000, samplesPerReading=n, sampleRate=FS, freqFocusRangeKhz=5,
                                soundMode=1), B)


@pytest.mark.parametrize("B", [1, 16, 17, 45])
@pytest.mark.parametrize("fmt_name,n", CASES)
def test_chunk_tail_vs_oracle_joined_and_pipelined(S, O, ref, fmt_name, n, B):
    import torch
    fmt = getattr(O, fmt_name)
    raw, want = ref(fmt_name, n)
    raw = np.ascontiguousarray(raw[:B])
    # joined: one synchronised call per frame
    eng = engine(S, n, B)
    joined = []
    for f in range(F):
        _, _, pcm = eng.process(raw[:, f], fmt=fmt, stages=S.STAGE_SSB)
        for b in range(B):
            np.testing.assert_array_equal(pcm[b], want[f][b], err_msg=f"{fmt_name} n={n} B={B} stream {b} call {f}")
        joined.append(np.array(pcm, copy=True))
    eng.close()
    # pipelined: the three calls enqueued back to back, one synchronisation at the end
    dev = torch.device("cuda:0")
    eng = engine(S, n, B)
    eng.set_pipelining(S.PIPELINE_ON)
    src = [torch.from_numpy(np.ascontiguousarray(raw[:, f])).to(dev) for f in range(F)]
    out = [torch.empty((B, eng.pcm_len), dtype=torch.int16, device=dev) for _ in range(F)]
    torch.cuda.synchronize()
    for f in range(F):
        eng.process_device(src[f].data_ptr(), fmt, S.STAGE_SSB, None, None, out[f].data_ptr(), 1000 + 8 * f)
    eng.synchronize()
    for f in range(F):
        assert out[f].cpu().numpy().tobytes() == joined[f].tobytes(), f"pipelined call {f}"
    eng.close()
