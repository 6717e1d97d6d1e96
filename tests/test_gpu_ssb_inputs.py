"""The SSB chain on the GPU over the input families of tests/ssb_cases.py: whole-range random codes, full-scale square
waves, tone / silence / tone, single impulses at the chunk seams, full-scale steps and (CF32) magnitudes from 2^-149 to
2^100, at one shape per FIR slot count and on the lane-per-stream kernels, under sound modes 0, 1, 2 and a switching
schedule, upper and lower sideband.  tests/test_ssb_cases.py proves with the oracle's stage taps that these inputs
drive the AGC clamp and the PCM clamp to both rails, reach an all-zero PCM call after a loud one and stay finite.

Bar: PCM bit-exact against the oracle, every stream, every call; the lower sideband's PCM is all zero as well
(demodSSB gives y - y).  Also here: a stream of NaN and infinities leaves its workgroup's neighbours untouched, and the
audio pulse front end fused into the chain takes several energy frames per call."""
import numpy as np
import pytest

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


def engine(S, n, fs, B, mode=1):
    return S.Engine(S.SDRConfig(centerFrequency=100_000_000, samplesPerReading=n, sampleRate=fs, freqFocusRangeKhz=5,
                                soundMode=mode), B)


@pytest.mark.parametrize("c", C.INPUT_CASES, ids=C.case_id)
def test_input_families_pcm_bit_exact(S, O, c):
    fmt, n, fs, F = getattr(O, c["fmt"]), c["n"], c["fs"], c["calls"]
    modes = C.modes_of(c["sched"], F)
    raw = C.batch(c["fmt"], C.B, F, n, fs)
    want = C.oracle_pcm(O, raw, c["fmt"], n, fs, modes, c["upper"])
    eng = engine(S, n, fs, C.B, modes[0])
    eng.setUpperSideband(c["upper"])
    for f in range(F):
        eng.setSoundMode(modes[f])
        _, _, pcm = eng.process(np.ascontiguousarray(raw[:, f]), fmt=fmt, stages=S.STAGE_SSB)
        for b in range(C.B):
            np.testing.assert_array_equal(pcm[b], want[f][b], err_msg=f"{C.case_id(c)} stream {b} (family "
                                          f"{C.family_of(c['fmt'], b) + 1}) call {f} mode {modes[f]}")
        if not c["upper"]:
            assert not pcm.any(), f"lower sideband call {f}"
    eng.close()


@pytest.mark.parametrize("fmt_name,fs,n", [("CS16", 1_024_000, 2048), ("CF32", 250_000, 2048)])
def test_sideband_switched_between_calls(S, O, fmt_name, fs, n):
    """upper, lower, upper, lower, upper: a lower-sideband call feeds the FIR zeros, so its PCM is the equaliser's
    ringing alone, and the low-pass runs on under it: the PCM after it is the oracle's only if the low-pass state was
    carried through the y * 0 calls"""
    fmt, F = getattr(O, fmt_name), 5
    ups = [f % 2 == 0 for f in range(F)]
    modes = C.modes_of("switch", F)
    raw = C.batch(fmt_name, C.B, F, n, fs, seed=0x5B2)
    want = C.oracle_pcm(O, raw, fmt_name, n, fs, modes, ups)
    eng = engine(S, n, fs, C.B)
    for f in range(F):
        eng.setSoundMode(modes[f])
        eng.setUpperSideband(ups[f])
        _, _, pcm = eng.process(np.ascontiguousarray(raw[:, f]), fmt=fmt, stages=S.STAGE_SSB)
        for b in range(C.B):
            np.testing.assert_array_equal(pcm[b], want[f][b], err_msg=f"stream {b} call {f} upper {ups[f]}")
    eng.close()


@pytest.mark.parametrize("fs,n", [(1_024_000, 2048), (480_000, 2005), (250_000, 2048)])
def test_nan_and_infinities_stay_in_their_stream(S, O, fs, n):
    """CF32, every stream family 1; stream 7 of each 16-stream group also carries NaN, +Inf and -Inf.  Every other
    stream is bit-exact for three calls (16 slots, 32 slots, lane per stream).  The poisoned streams' own PCM is not
    compared: the reference converts NaN to int16_t, which C leaves undefined."""
    F = 3
    raw = np.stack([np.stack([C.fam_uniform("CF32", b, f, n, fs, 0x5B3) for f in range(F)]) for b in range(C.B)])
    bad = [b for b in range(C.B) if b % 16 == 7]
    rng = np.random.default_rng(0x5B3)
    for b in bad:
        for f in range(F):
            pos = rng.permutation(2 * n)[:48]
            raw[b, f, pos[0::3]] = np.nan
            raw[b, f, pos[1::3]] = np.inf
            raw[b, f, pos[2::3]] = -np.inf
    good = [b for b in range(C.B) if b not in bad]
    want = C.oracle_pcm(O, raw, "CF32", n, fs, [1, 2, 0], True, streams=good)
    eng = engine(S, n, fs, C.B)
    for f, mode in enumerate([1, 2, 0]):
        eng.setSoundMode(mode)
        _, _, pcm = eng.process(np.ascontiguousarray(raw[:, f]), fmt=O.CF32, stages=S.STAGE_SSB)
        for b in good:
            np.testing.assert_array_equal(pcm[b], want[f][b], err_msg=f"fs {fs} stream {b} call {f}")
    eng.close()


def _keyed_tone(B, n, fs, call):
    """CS8: a 1.5 kHz carrier keyed on for 10 ms in every 30 ms (a different phase per stream) over weak noise"""
    rng = np.random.default_rng(0x5B4 + call)
    t = (call * n + np.arange(n))[None, :] / fs
    on = (np.mod(t + 0.003 * np.arange(B)[:, None], 0.03) < 0.01).astype(np.float64)
    amp = 3.0 + 50.0 * on
    ph = 2 * np.pi * 1500.0 * t
    iq = np.empty((B, 2 * n), np.int8)
    iq[:, 0::2] = np.clip(np.round(amp * np.cos(ph) + rng.normal(0, 2.0, (B, n))), -128, 127)
    iq[:, 1::2] = np.clip(np.round(amp * np.sin(ph) + rng.normal(0, 2.0, (B, n))), -128, 127)
    return iq


@pytest.mark.parametrize("fs", [480_000, 250_000])
def test_pulse_front_end_with_several_energy_frames_per_call(S, O, fs):
    """STAGE_ALL at 16384 samples: 1613 PCM samples per call from the pipeline kernel at 480 kHz (32 slots), 3226 from
    the lane-per-stream kernels at 250 kHz, so the audio detector's front end (fused into the chain's last stage) hands
    over 3 to 7 energy frames of 480 samples per call.  Its outputs equal the oracle detector fed the GPU's own PCM,
    field for field, and the PCM equals the oracle's."""
    n, B, F = 16384, 20, 6
    L = S.ssb_layout(fs, n)
    assert L["pcm_len"] == {480_000: 1613, 250_000: 3226}[fs] and L["pipeline"] == (fs == 480_000)
    eng = engine(S, n, fs, B)
    det = [O.PulseDetector(O.PULSE_AUDIO) for _ in range(B)]
    sst = [O.SsbState() for _ in range(B)]
    held = np.zeros(B, np.int64)
    for f in range(F):
        raw = _keyed_tone(B, n, fs, f)
        _, _, pcm = eng.process(raw, fmt=S.CS8, stages=S.STAGE_ALL, now_ms=1000 + 34 * f)
        _, pa = eng.pulse_outputs()
        for b in range(B):
            np.testing.assert_array_equal(pcm[b], sst[b].process(O.unpack(O.CS8, raw[b], n), fs, 1),
                                          err_msg=f"pcm stream {b} call {f}")
            wa = det[b].audio(pcm[b])
            for k in ("strength", "live_etat", "level", "locked", "period_s", "n_energy", "n_rois"):
                assert np.asarray(pa[b][k]).tobytes() == np.asarray(wa[k]).tobytes(), (k, b, f, pa[b][k], wa[k])
        assert (pa["overflow"] == 0).all()
        # the detector keeps these energy frames for seconds: each call added its whole frames
        assert ((pa["n_energy"] - held) >= L["pcm_len"] // 480).all(), (f, pa["n_energy"], held)
        held = pa["n_energy"].astype(np.int64)
    eng.close()
