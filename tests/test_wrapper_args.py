"""CPU test of the Python wrapper's argument handling (sdrg/__init__.py): filling a configuration structure from
keyword fields and reading it back, set_<stage>(off=True), and the spectra and iq checks.  No GPU, no engine and no
libsdrg.so: the calls go through the public entry points on an Engine object that was never created in the library,
with sdrg.load() replaced by a stand-in that keeps what set_<stage> is given and hands it back to get_<stage>.  Every
exception is raised by the wrapper before it would call the library."""
import copy
import ctypes

import numpy as np
import pytest

import sdrg

B, N = 3, 8
STAGES = ("display", "integration", "peaks", "ddc", "demod", "channelizer", "resample")


class Library:
    """Every function returns 0.  sdrg_engine_set_<stage>(h, cfg) keeps a copy of *cfg (None for a null pointer),
    sdrg_engine_get_<stage>(h, cfg, ...) writes it to *cfg; `calls` lists (name, arguments) and `read` holds the bytes
    behind the pointers named in `capture` (name -> (argument index, byte count)) at the time of the call."""

    def __init__(self):
        self.kept, self.calls, self.capture, self.read = {}, [], {}, {}

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            stage = name[len("sdrg_engine_set_"):]
            if name.startswith("sdrg_engine_set_") and stage in STAGES:
                self.kept[stage] = None if args[1] is None else copy.copy(args[1]._obj)
            elif name.startswith("sdrg_engine_get_") and stage in STAGES and args[1] is not None:
                if self.kept.get(stage) is not None:
                    ctypes.memmove(ctypes.addressof(args[1]._obj), ctypes.addressof(self.kept[stage]),
                                   ctypes.sizeof(self.kept[stage]))
            if name in self.capture:
                index, nbytes = self.capture[name]
                self.read[name] = ctypes.string_at(args[index].value, nbytes)
            return 0
        return call


@pytest.fixture
def lib(monkeypatch):
    fake = Library()
    monkeypatch.setattr(sdrg, "load", lambda: fake)
    return fake


@pytest.fixture
def eng(lib):
    e = sdrg.Engine.__new__(sdrg.Engine)
    e._h, e._cbs, e.n_streams, e.cfg = None, None, B, sdrg.SDRConfig(samplesPerReading=N)
    return e


CONFIGS = [  # (structure, its setter, its getter, the fields given)
    (sdrg.DisplayConfig, "set_display", "display_config", dict(width=100, format=1, db_min=-3.5)),
    (sdrg.IntegrateConfig, "set_integration", "integration", dict(mode=2, alpha=0.25)),
    (sdrg.PeaksConfig, "set_peaks", "peaks_config", dict(max_peaks=4, threshold_db=-1.5, first_bin=7)),
    (sdrg.DdcConfig, "set_ddc", "ddc_config", dict(offset_hz=-1250.5, taps=41)),
    (sdrg.DemodConfig, "set_demod", "demod_config", dict(deviation_hz=5000.0, audio_taps=3, gain=0.5, max_in=64)),
    (sdrg.ChannelizerConfig, "set_channelizer", "channelizer_config", dict(cutoff_rel=0.75, channels=16, n_channels=2)),
    (sdrg.ResampleConfig, "set_resample", "resample_config", dict(interp=3, taps_per_phase=8, gain=0.5, max_in=64)),
]


@pytest.mark.parametrize("cls,setter,getter,given", CONFIGS, ids=[c[1] for c in CONFIGS])
def test_fields_fill_a_structure_and_read_back(eng, lib, cls, setter, getter, given):
    getattr(eng, setter)(**given)
    stage = setter[len("set_"):]
    kept = lib.kept[stage]
    assert type(kept) is cls
    names = [k for k, _ in cls._fields_]
    assert {k: getattr(kept, k) for k in names} == {**dict.fromkeys(names, 0), **given}
    got = getattr(eng, getter)()
    assert {k: got[k] for k in names} == {**dict.fromkeys(names, 0), **given}
    assert all(type(got[k]) is type(getattr(kept, k)) for k in names)


@pytest.mark.parametrize("what", ("display", "peaks", "ddc", "demod", "channelizer", "resample"))
def test_unknown_field(eng, lib, what):
    with pytest.raises(TypeError) as ei:
        getattr(eng, "set_" + what)(x=1)
    assert str(ei.value) == f"unknown {what} field 'x'"
    assert lib.calls == []


@pytest.mark.parametrize("fn,what", ((sdrg.demod_design, "demod"), (sdrg.channelizer_design, "channelizer"),
                                     (sdrg.channelizer_tile_outputs, "channelizer"), (sdrg.resample_design, "resample"),
                                     (sdrg.resample_tile_outputs, "resample")))
def test_unknown_field_of_a_design_function(lib, fn, what):
    with pytest.raises(TypeError) as ei:
        fn(x=1)
    assert str(ei.value) == f"unknown {what} field 'x'"
    assert lib.calls == []


@pytest.mark.parametrize("what", ("ddc", "demod", "channelizer", "resample"))
def test_off(eng, lib, what):
    setter = getattr(eng, "set_" + what)
    with pytest.raises(TypeError) as ei:
        setter(off=True, x=1)
    assert str(ei.value) == "off=True takes no other field"
    assert lib.calls == []
    setter(off=True)
    assert lib.calls == [("sdrg_engine_set_" + what, (None, None))]  # a null configuration switches the stage off
    lib.calls.clear()
    with pytest.raises(TypeError) as ei:
        setter(off=False, x=1)  # off=False is no field
    assert str(ei.value) == f"unknown {what} field 'x'"


def strided(shape, dtype=np.float64):
    """A non-contiguous array of `shape`: every other column of one twice as wide, small whole numbers."""
    rows, cols = shape
    a = (np.arange(rows * cols * 2) % 100 - 50).astype(dtype).reshape(rows, cols * 2)[:, ::2]
    assert a.shape == shape and not a.flags.c_contiguous
    return a


SPECTRA_CALLS = (("signal_strength", "sdrg_engine_signal_strength_host"), ("display", "sdrg_engine_display_host"),
                 ("integrate", "sdrg_engine_integrate_host"), ("peaks", "sdrg_engine_peaks_host"))


@pytest.mark.parametrize("method,entry", SPECTRA_CALLS, ids=[c[0] for c in SPECTRA_CALLS])
def test_spectra(eng, lib, method, entry):
    eng.set_display(width=4)
    eng.set_peaks(max_peaks=2)
    call = getattr(eng, method)
    for bad in (np.zeros((B, N + 1), np.float32), np.zeros((B + 1, N), np.float32), np.zeros(B * N, np.float32)):
        with pytest.raises(sdrg.SdrgError) as ei:
            call(bad)
        assert str(ei.value) == f"spectra {bad.shape}: expected ({B}, {N})"
    assert not [c for c in lib.calls if c[0] == entry]
    a = strided((B, N))
    lib.capture[entry] = (1, B * N * 4)
    call(a)
    assert lib.read[entry] == np.ascontiguousarray(a, dtype=np.float32).tobytes()


@pytest.mark.parametrize("method", ("display", "integrate", "peaks"))
def test_no_spectra_is_a_null_pointer(eng, lib, method):
    eng.set_display(width=4)
    eng.set_peaks(max_peaks=2)
    getattr(eng, method)()
    name, args = lib.calls[-1]
    assert name == f"sdrg_engine_{method}_host" and args[1] is None


IQ_CALLS = (("ddc", "sdrg_engine_ddc_host"), ("ddc_demod", "sdrg_engine_ddc_demod_host"),
            ("channelizer", "sdrg_engine_channelizer_host"),
            ("ddc_demod_resample_host", "sdrg_engine_ddc_demod_resample_host"))


@pytest.mark.parametrize("fmt", (sdrg.CF32, sdrg.CS8, sdrg.CU8, sdrg.CS16))
@pytest.mark.parametrize("method,entry", IQ_CALLS, ids=[c[0] for c in IQ_CALLS])
def test_iq(eng, lib, method, entry, fmt):
    call = getattr(eng, method)
    if method == "ddc_demod_resample_host":  # sizes its output from the resampler's configuration
        eng.set_resample(interp=3, decim=2, taps_per_phase=8, components=1, max_in=64)
        lib.calls.clear()
    for bad in (np.zeros((B, 2 * N + 1), np.int8), np.zeros(B * N, np.int8)):
        with pytest.raises(sdrg.SdrgError) as ei:
            call(bad, fmt=fmt)
        assert str(ei.value) == f"iq has {bad.size} values, expected {B}x{N}x2"
    assert lib.calls == []
    a = np.abs(strided((B, 2 * N)))
    dtype = sdrg.NUMPY_DTYPE[fmt]
    lib.capture[entry] = (1, B * 2 * N * np.dtype(dtype).itemsize)
    call(a, fmt=fmt)
    assert lib.read[entry] == np.ascontiguousarray(a, dtype=dtype).tobytes()


@pytest.mark.parametrize("fmt,dtype", ((sdrg.DISPLAY_DB_F32, np.float32), (sdrg.DISPLAY_U8, np.uint8)))
def test_display_rows(eng, lib, fmt, dtype):
    eng.set_display(width=5, format=fmt, db_min=-1.0, db_max=1.0)
    for rows in (eng.display(), eng.display_integrated()):
        assert rows.shape == (B, 5) and rows.dtype == dtype and rows.flags.c_contiguous
