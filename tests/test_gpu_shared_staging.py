"""GPU test of the staging buffer the four host calls that read spectra share (sdrg_engine_signal_strength_host,
_display_host, _integrate_host, _peaks_host): a caller sees four independent calls.  Each stages its caller's spectra
and none of them leaks into another stage's result, into the spectra process_host left on the device (the NULL
source, and the carried bin N-1 of an odd N), or into the integrated rows.  Every comparison is of bytes, against the
restatements the stages' own tests use (display_cases.rows, integrate_cases.Integrator, peaks_cases.tables)."""
import ctypes

import numpy as np
import pytest

import display_cases as dc
import integrate_cases as ic
import peaks_cases as pc

pytestmark = pytest.mark.gpu

FS = 2_000_000
N, B, W, K, SEP, THRESHOLD = 1023, 2, 100, 4, 8, 10.0  # N odd: process_host carries bin N-1 on the device


def engine(S, n):
    eng = S.Engine(S.SDRConfig(centerFrequency=100_000_000, samplesPerReading=n, sampleRate=FS, freqFocusRangeKhz=5,
                               soundMode=1), B)
    eng.set_display(span=S.DISPLAY_SPAN_FULL, width=W, reduce=S.DISPLAY_MAX, format=S.DISPLAY_DB_F32)
    eng.set_integration(mode=S.INTEGRATE_MEAN, period=2)
    eng.set_peaks(span=S.DISPLAY_SPAN_FULL, max_peaks=K, min_separation=SEP, threshold_db=THRESHOLD)
    return eng


def invalid(S, fn, *a, **k):
    with pytest.raises(S.SdrgError) as ei:
        fn(*a, **k)
    assert "SDRG_E_INVALID" in str(ei.value)


def rows(spec):
    return dc.rows(spec, 0, spec.shape[1], W, dc.MAX, dc.DB_F32).tobytes()


def tables(spec):
    pk, sm = pc.tables(spec, 0, spec.shape[1], SEP, K, THRESHOLD)
    return pk.tobytes(), sm.tobytes()


def as_bytes(got):
    return tuple(a.tobytes() for a in got)


def test_four_host_calls_share_one_staging_buffer():
    import oracle as O
    import sdrg as S
    stages = S.STAGE_SPECTRUM | S.STAGE_STATS
    raw = np.stack([np.stack([O.synth_frames(1, N, O.CS8, tone_hz=900.0 * b - 800.0, fs=FS, seed=31 + b + 5 * f)[0]
                              for b in range(B)]) for f in range(2)])
    a, b_, d = dc.noise_spectra(B, N, seed=11), dc.noise_spectra(B, N, seed=12), pc.noise_rows(B, N, seed=14, tones=3)
    c = ic.spread_frames(1, B, N, seed=13)[0]
    for x in (a, b_, c, d):  # a leak into the carried bin N-1 would show
        assert np.all(x[:, N - 1] != 0)
    assert len({x.tobytes() for x in (a, b_, c, d)}) == 4

    # the reference engine: the spectra of the process call, and the records of signal_strength(a) after it
    ref = engine(S, N)
    spec = ref.process(raw[0], fmt=S.CS8, stages=stages, now_ms=1000)[0].copy()
    want_rec = ref.signal_strength(a, now_ms=1010).tobytes()
    ref.close()
    assert np.all(spec[:, N - 1] == 0)

    eng = engine(S, N)
    rec = np.zeros(B, S.RECORD_DTYPE)
    rc = S.load().sdrg_engine_process_host(eng._h, raw[0].ctypes.data_as(ctypes.c_void_p), S.CS8, stages, None,
                                           rec.ctypes.data_as(ctypes.c_void_p), None, 1000)
    assert rc == 0
    it = ic.Integrator(ic.MEAN, period=2)

    # four caller arrays through the four stages, one after the other
    assert eng.signal_strength(a, now_ms=1010).tobytes() == want_rec
    assert eng.display(b_).tobytes() == rows(b_)
    assert eng.integrate(c).tobytes() == it.push(c).tobytes()
    assert as_bytes(eng.peaks(d)) == tables(d)

    # the NULL source is still the process call's spectra
    assert eng.display().tobytes() == rows(spec)
    assert as_bytes(eng.peaks()) == tables(spec)
    integrated = it.push(spec)
    assert eng.integrate().tobytes() == integrated.tobytes()
    assert eng.display_integrated().tobytes() == rows(integrated)
    assert as_bytes(eng.peaks_integrated()) == tables(integrated)

    # and bin N-1 of every stream is still the value process_host carries
    spec2 = eng.process(raw[1], fmt=S.CS8, stages=stages, now_ms=1020)[0]
    assert np.all(spec2[:, N - 1] == 0), spec2[:, N - 1]

    # a longer frame: the shared buffer grows between stages
    n2 = 2048
    eng.setSamplesPerReading(n2)
    small = [dc.noise_spectra(B, n2, seed=15), pc.noise_rows(B, n2, seed=16, tones=3), ic.spread_frames(1, B, n2, seed=17)[0]]
    assert eng.display(small[0]).tobytes() == rows(small[0])
    assert as_bytes(eng.peaks(small[1])) == tables(small[1])
    for call in (eng.display, eng.peaks, eng.integrate, eng.display_integrated, eng.peaks_integrated):
        invalid(S, call)  # the spectra and the integrated rows on the device are 1023 bins wide
    assert eng.integration_depth() == 2  # the refused calls advanced nothing
    it.reset()  # another frame size: the history is forgotten
    integrated = it.push(small[2])
    assert eng.integrate(small[2]).tobytes() == integrated.tobytes()
    assert eng.display_integrated().tobytes() == rows(integrated)
    assert as_bytes(eng.peaks_integrated()) == tables(integrated)
    for call in (eng.display, eng.peaks, eng.integrate):
        invalid(S, call)
    eng.close()
