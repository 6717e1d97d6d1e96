"""GPU tests of the resampler stage (csrc/resample.hip, sdrg_engine_resample_*, sdrg_engine_ddc_demod_resample_host):
the rows of each stream against the NumPy restatement in tests/resample_cases.py fed the library's own prototype.  Every
comparison is of the bytes of the whole output (the stage is specified product by product and sum by sum: no
tolerances).  `out` is pre-filled with 0xAA between 64 guard bytes on either side, every stream has its own data, and
the input rows hold NaN past the call's n values.

The kernel works in tiles of `tile` consecutive outputs (sdrg.resample_tile_outputs), the last workgroup of a stream
moves the history: the shapes below put outputs on each side of every tile seam and calls on each side of the history's
length."""
import ctypes

import numpy as np
import pytest

import ddc_cases as dd
import demod_cases as dm
import resample_cases as rs
from stage_harness import GUARD, engine, invalid, out_buffer, read_out, same

pytestmark = pytest.mark.gpu

BASE = dict(interp=3, decim=2, taps_per_phase=8, cutoff_rel=0.9, components=1, out_format=rs.OUT_F32, gain=0.7,
            max_in=1024)
RATIOS = [(3, 2, 8), (2, 3, 8), (123, 125, 16), (147, 160, 24), (8, 1, 4), (1, 8, 64), (512, 511, 16), (7, 5, 1)]


@pytest.fixture(scope="module")
def S():
    import sdrg
    return sdrg


@pytest.fixture(scope="module")
def T():
    import torch
    return torch


def rows_on_device(T, x, stride, components):
    """x [B][n] (float32, or complex64 at components 2) -> a device tensor [B][stride][components] float32, NaN past
    n."""
    v = rs.as_rows(x, x.shape[0], components)
    B, n = v.shape[:2]
    rows = np.full((B, max(stride, 1), components), np.nan, np.float32)
    rows[:, :n] = v
    return T.from_numpy(rows).to("cuda:0")


class Rows:
    """An engine with the resampler set, and the restatement that follows it call by call."""

    def __init__(self, S, T, B, n=1024, **cfg):
        self.S, self.T, self.B = S, T, B
        self.eng = engine(S, B, n)
        self.configure(**cfg)

    def configure(self, **cfg):
        self.cfg = cfg
        self.eng.set_resample(**cfg)
        self.remodel()

    def remodel(self):
        """A fresh restatement from the library's prototype of the configuration in force."""
        d = self.eng.resample_config()
        assert all(d[k] == (np.float32(v) if k == "gain" else v) for k, v in self.cfg.items()), d
        assert d["samples_consumed"] == 0
        assert self.S.resample_design(**self.cfg).tobytes() == d["taps"].tobytes()
        self.dtype, self.comps = rs.OUT_DTYPE[d["out_format"]], d["components"]
        self.model = rs.Resampler(self.B, d["interp"], d["decim"], d["taps"], d["gain"], d["out_format"], self.comps,
                                  d["max_in"])
        self.cap = self.eng.resample_max_out()
        assert self.cap == rs.ceil_div(d["max_in"] * d["interp"], d["decim"])
        self.shape = (self.B, self.cap) + ((2,) if self.comps == 2 else ())

    def noise(self, n, seed):
        return rs.noise(self.B, n, seed, self.comps)

    def device_call(self, x, stride=None):
        """resample_device into a 0xAA-filled buffer between guard bytes: (out, n_out)."""
        T, eng = self.T, self.eng
        n = x.shape[1]
        stride = self.cfg["max_in"] if stride is None else stride
        in_t = rows_on_device(T, x, stride, self.comps)
        out_t = out_buffer(T, int(np.prod(self.shape)) * np.dtype(self.dtype).itemsize)
        T.cuda.synchronize()
        n_out = eng.resample_device(in_t.data_ptr(), stride, n, out_t.data_ptr() + GUARD)
        eng.synchronize()
        return read_out(out_t, self.shape, self.dtype), n_out

    def check(self, x, what=None, stride=None):
        got, n_out = self.device_call(x, stride)
        want, want_n = self.model.call(x)
        same(got, n_out, want, want_n, what)
        assert self.eng.resample_config()["samples_consumed"] == self.model.g
        return got, n_out

    def close(self):
        self.eng.close()


def test_identity(S, T):
    """(1, 1, 1) with the gain 1: h = [1.0], and out is in, byte for byte (0 + 1 x = x, x 1 = x)."""
    B, n = 3, 700
    for comps in (1, 2):
        r = Rows(S, T, B, **dict(BASE, interp=1, decim=1, taps_per_phase=1, gain=1.0, components=comps, max_in=n))
        assert r.model.h.tolist() == [1.0]
        x = r.noise(n, seed=1)
        got, n_out = r.check(x)
        assert n_out == n and got.tobytes() == rs.as_rows(x, B, comps).tobytes()
        r.close()


@pytest.mark.parametrize("L,M,P", RATIOS)
def test_ratios_formats_and_tile_seams(S, T, L, M, P):
    """Two tiles and a part of a third, then a second call, for both row types and both output formats: every window
    near a multiple of the tile size reads values the neighbouring tile also stages, the first tile's the history; the
    second call starts at another phase."""
    B = 2
    tile = S.resample_tile_outputs(**dict(BASE, interp=L, decim=M, taps_per_phase=P))
    n = rs.ceil_div((2 * tile + 3) * M, L) + 1
    r = Rows(S, T, B, **dict(BASE, interp=L, decim=M, taps_per_phase=P, max_in=n))
    for comps in (1, 2):
        for fmt in (rs.OUT_F32, rs.OUT_S16):
            r.configure(**dict(BASE, interp=L, decim=M, taps_per_phase=P, max_in=n, components=comps, out_format=fmt,
                               gain=0.7 if fmt == rs.OUT_F32 else 1.4))
            for f, nn in enumerate((n, n - 1)):
                got, n_out = r.check(r.noise(nn, seed=10 + f), (L, M, P, comps, fmt, f))
                assert n_out > 2 * tile and np.abs(got[:, :n_out].astype(np.float64)).max() > 1e-3
                assert not got[:, n_out:].any()
            if fmt == rs.OUT_S16:  # the gain clamps a part of the samples, unless the low-pass has taken most of the noise
                assert np.any((np.abs(got) > 100) & (np.abs(got) < 32767))
                assert M > L or np.any(np.abs(got) == 32767)
    r.close()


@pytest.mark.parametrize("L,M,P", [(3, 2, 8), (123, 125, 16), (2, 3, 8)])
def test_an_output_on_each_side_of_every_seam(S, T, L, M, P):
    """Calls whose n_out is tile - 1, tile, tile + 1, 2 tile - 1, 2 tile and 2 tile + 1, from a running stream: the
    last tile is full, short by one output, or a single output.  (At L > M one more sample adds one or two outputs:
    there the call is the shortest with at least that many.)"""
    B = 2
    tile = S.resample_tile_outputs(**dict(BASE, interp=L, decim=M, taps_per_phase=P))
    max_in = rs.ceil_div((2 * tile + 2) * M, L) + 2
    r = Rows(S, T, B, **dict(BASE, interp=L, decim=M, taps_per_phase=P, max_in=max_in))
    for f, want_out in enumerate((tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 1)):
        g = r.model.g
        n = next(n for n in range(1, max_in + 1) if rs.outputs_of(g, n, L, M)[1] >= want_out)
        got, n_out = r.check(r.noise(n, seed=20 + f), (want_out, n))
        assert n_out == want_out if L <= M else want_out <= n_out <= want_out + 1
    r.close()


@pytest.mark.parametrize("B", [1, 9, 65, 130])
def test_stream_counts(S, T, B):
    n = 200
    r = Rows(S, T, B, **dict(BASE, components=2, max_in=256))
    for f in range(2):
        r.check(r.noise(n, seed=30 + f), (B, f))
    r.close()


@pytest.mark.parametrize("comps", [1, 2])
def test_short_calls(S, T, comps):
    """n = 0, 1, 2, 63, 64, 65 in one stream: a call without samples changes nothing but out."""
    B = 3
    r = Rows(S, T, B, **dict(BASE, interp=7, decim=5, taps_per_phase=12, components=comps, max_in=65))
    for f, n in enumerate((65, 0, 1, 2, 63, 0, 64, 65, 0)):
        got, n_out = r.check(r.noise(n, seed=40 + f), (f, n))
        if n == 0:
            assert n_out == 0 and not got.any()
    assert r.model.g == 2 * 65 + 1 + 2 + 63 + 64
    r.close()


def test_first_call_without_samples(S, T):
    B = 2
    r = Rows(S, T, B, **BASE)
    got, n_out = r.check(r.noise(0, seed=45))
    assert n_out == 0 and not got.any() and got.shape == (B, 1536)
    r.check(r.noise(300, seed=46))
    r.close()


@pytest.mark.parametrize("comps", [1, 2])
def test_calls_shorter_than_the_history(S, T, comps):
    """n = 10 < P - 1 = 63: most of each call's new history is the old one moved down."""
    B, n = 3, 10
    r = Rows(S, T, B, **dict(BASE, interp=8, decim=7, taps_per_phase=64, components=comps, max_in=16))
    for f in range(9):
        r.check(r.noise(n, seed=50 + f), f)
    r.close()


def test_calls_without_outputs_advance_the_history(S, T):
    """(1, 8, 64) at n = 3: most calls hold no output, and still every byte of out is written and the history moves."""
    B, n = 2, 3
    r = Rows(S, T, B, **dict(BASE, interp=1, decim=8, taps_per_phase=64, max_in=3))
    counts = []
    for f in range(12):
        got, n_out = r.check(r.noise(n, seed=60 + f), f)
        assert got.shape == (B, 1)
        if n_out == 0:
            assert not got.view(np.uint32).any()
        counts.append(n_out)
    assert counts == [1, 0, 1, 0, 0, 1, 0, 0, 1, 0, 1, 0]  # inputs 0, 8, 16, 24, 32 of the stream
    r.close()


def test_five_calls_are_one_stream(S, T):
    B, lens = 4, (700, 33, 1, 2050, 127)
    r = Rows(S, T, B, **dict(BASE, interp=123, decim=125, taps_per_phase=16, components=2, max_in=2050))
    x = r.noise(sum(lens), seed=70)
    parts, at = [], 0
    for n in lens:
        got, n_out = r.check(x[:, at:at + n], n)
        parts.append(got[:, :n_out])
        at += n
    m = r.model
    whole, n_whole = rs.Resampler(B, m.L, m.M, m.h, m.gain, m.out_format, 2).call(x)
    assert n_whole == rs.ceil_div(sum(lens) * 123, 125)
    assert np.concatenate(parts, axis=1).tobytes() == whole[:, :n_whole].tobytes()
    r.close()


@pytest.mark.parametrize("comps", [1, 2])
def test_in_stride_longer_than_n(S, T, comps):
    """Rows n + 7 apart, and rows further apart than max_in."""
    B, n = 5, 333
    r = Rows(S, T, B, **dict(BASE, components=comps, max_in=400))
    r.check(r.noise(n, seed=80), "n + 7", stride=n + 7)
    r.check(r.noise(n, seed=81), "n", stride=n)
    r.check(r.noise(n, seed=82), "max_in + 5", stride=405)
    in_t = rows_on_device(T, r.noise(n, seed=83), n, comps)
    out_t = out_buffer(T, 16)
    T.cuda.synchronize()
    invalid(S, r.eng.resample_device, in_t.data_ptr(), n - 1, n, out_t.data_ptr() + GUARD)  # in_stride < n
    r.close()


def test_reset_and_set_again_between_calls(S, T):
    """resample_reset and an accepted set_resample restart the streams; a rejected one changes nothing."""
    B, n = 2, 500
    r = Rows(S, T, B, **BASE)
    r.check(r.noise(n, seed=90))
    nan = float("nan")
    for bad in (dict(interp=0), dict(decim=513), dict(interp=6, decim=4), dict(interp=9, decim=1), dict(interp=1, decim=9),
                dict(taps_per_phase=65), dict(interp=511, decim=512, taps_per_phase=17), dict(cutoff_rel=0.0),
                dict(cutoff_rel=1.5), dict(components=3), dict(out_format=2), dict(gain=nan), dict(max_in=0),
                dict(max_in=(1 << 20) + 1)):
        invalid(S, r.eng.set_resample, **dict(BASE, **bad))
    got = r.eng.resample_config()
    assert got["samples_consumed"] == n and all(got[k] == np.float32(v) if k == "gain" else got[k] == v
                                                for k, v in BASE.items())
    r.check(r.noise(n, seed=91), "after rejected set_resample")
    r.eng.resample_reset()
    r.model.reset()
    assert r.eng.resample_config()["samples_consumed"] == 0
    r.check(r.noise(n, seed=92), "after reset")
    r.check(r.noise(n, seed=93), "second after reset")
    r.configure(**BASE)
    r.check(r.noise(n, seed=94), "after the same set_resample")
    r.configure(**dict(BASE, interp=147, decim=160, taps_per_phase=24, components=2, out_format=rs.OUT_S16, gain=1.5))
    r.check(r.noise(n, seed=95), "after another set_resample")
    r.check(r.noise(n, seed=96), "second after another set_resample")
    r.close()


def test_the_far_end_of_the_index_arithmetic(S, T):
    """1 x 2^20 at (8, 1, 2): 2^23 outputs in 32768 tiles, j M and n L up to 2^23."""
    n = 1 << 20
    r = Rows(S, T, 1, **dict(BASE, interp=8, decim=1, taps_per_phase=2, max_in=n))
    got, n_out = r.check(r.noise(n, seed=100))
    assert n_out == 1 << 23 and got[0, -1] != 0
    r.close()


def test_refusals_write_nothing_and_commit_nothing(S, T):
    B, n = 2, 300
    eng = engine(S, B)
    x = rs.noise(B, n, seed=110)
    in_t = rows_on_device(T, x, 1024, 1)
    out_t = out_buffer(T, B * 1536 * 4)
    T.cuda.synchronize()
    invalid(S, eng.resample_device, in_t.data_ptr(), 1024, n, out_t.data_ptr() + GUARD)  # before any set_resample
    invalid(S, eng.resample_max_out)
    invalid(S, eng.resample_config)
    invalid(S, eng.resample_host, x)
    eng.close()

    r = Rows(S, T, B, **BASE)
    r.check(x)
    for bad_n in (1025, -1, 1 << 30):
        invalid(S, r.eng.resample_device, in_t.data_ptr(), 1 << 30, bad_n, out_t.data_ptr() + GUARD)
    L = S.load()
    n_out = ctypes.c_int32(-7)
    o = out_t.data_ptr() + GUARD
    assert L.sdrg_engine_resample_device(r.eng._h, None, 1024, n, o, ctypes.byref(n_out)) == -1
    assert L.sdrg_engine_resample_device(r.eng._h, in_t.data_ptr(), 1024, n, None, ctypes.byref(n_out)) == -1
    assert L.sdrg_engine_resample_device(r.eng._h, in_t.data_ptr(), 1024, n, o, None) == -1
    assert L.sdrg_engine_resample_device(None, in_t.data_ptr(), 1024, n, o, ctypes.byref(n_out)) == -1
    assert L.sdrg_engine_resample_host(r.eng._h, None, 1024, n, o, ctypes.byref(n_out)) == -1
    assert n_out.value == -7 and r.eng.resample_config()["samples_consumed"] == n
    r.check(rs.noise(B, n, seed=111), "after refused calls")
    r.eng.set_resample(off=True)
    invalid(S, r.eng.resample_device, in_t.data_ptr(), 1024, n, o)
    r.eng.synchronize()
    assert np.all(out_t.cpu().numpy() == 0xAA), "a refused call wrote to out"
    r.configure(**BASE)
    r.check(rs.noise(B, n, seed=112), "after off and on")
    r.close()


@pytest.mark.parametrize("comps,fmt", [(1, rs.OUT_F32), (2, rs.OUT_S16)])
def test_host_path_equals_device_path(S, T, comps, fmt):
    B, n = 5, 777
    cfg = dict(BASE, interp=123, decim=125, taps_per_phase=16, components=comps, out_format=fmt)
    dev = Rows(S, T, B, **cfg)
    host = engine(S, B)
    host.set_resample(**cfg)
    for f in range(3):
        x = dev.noise(n - 100 * f, seed=120 + f)
        got, n_out = dev.check(x, f)
        h = host.resample_host(x)
        assert h.dtype == dev.dtype and h.shape == got[:, :n_out].shape and h.tobytes() == got[:, :n_out].tobytes()
    assert host.resample_host(dev.noise(0, seed=1)).shape[:2] == (B, 0)
    assert host.resample_config()["samples_consumed"] == dev.model.g
    invalid(S, host.resample_host, dev.noise(1025, seed=2))
    dev.close()
    host.close()


def test_process_device_and_demod_device_between_resample_calls(S, T):
    """resample, process_device, demod_device, resample, ...: the rows are the restatement's, the audio its
    restatement's, and the spectra, records and PCM are those of an engine that configured neither stage."""
    n, B, fmt = 16384, 4, dd.CS8
    stages = S.STAGE_SPECTRUM | S.STAGE_STATS | S.STAGE_SSB
    raws = [dd.tone(fmt, B, n, 0.01 + 0.001 * f, amp=0.4) for f in range(2)]
    demod_cfg = dict(mode=dm.FM, channel_rate_hz=200_000.0, deviation_hz=75_000.0, dc_cutoff_hz=300.0,
                     deemphasis_us=75.0, audio_decimation=4, audio_taps=31, audio_cutoff_hz=15_000.0, gain=0.7,
                     out_format=dm.OUT_F32, max_in=1024)

    def process(eng, f):
        iq_t = T.from_numpy(raws[f]).to("cuda:0")
        spec = T.zeros((B, n), dtype=T.float32, device="cuda:0")
        rec = T.zeros((B * S.RECORD_DTYPE.itemsize,), dtype=T.uint8, device="cuda:0")
        pcm = T.zeros((B, max(eng.pcm_len, 1)), dtype=T.int16, device="cuda:0")
        T.cuda.synchronize()
        eng.process_device(iq_t.data_ptr(), fmt, stages, spec.data_ptr(), rec.data_ptr(), pcm.data_ptr(), 1000 + f)
        return iq_t, spec, rec, pcm

    r = Rows(S, T, B, n, **dict(BASE, interp=123, decim=125, taps_per_phase=16))
    r.eng.set_demod(**demod_cfg)
    d = r.eng.demod_config()
    demod_model = dm.Demod(B, d["mode"], d["kf"], d["alpha"], d["a"], d["taps"], 4, d["gain"], dm.OUT_F32, 1024)
    plain = engine(S, B, n)
    demod_cap = r.eng.demod_max_out()
    xs = [r.noise(900 + f, seed=130 + f) for f in range(3)]
    chans = [dm.noise(B, 800 + f, seed=140 + f) for f in range(2)]
    held, outs, demod_outs = [], [], []
    for f in range(3):
        in_t = rows_on_device(T, xs[f], 1024, 1)
        out_t = out_buffer(T, B * r.cap * 4)
        T.cuda.synchronize()
        n_out = r.eng.resample_device(in_t.data_ptr(), 1024, xs[f].shape[1], out_t.data_ptr() + GUARD)
        outs.append((out_t, n_out, in_t))
        if f < 2:
            held.append((process(r.eng, f), process(plain, f)))
            rows = np.full((B, 1024, 2), np.nan, np.float32)
            rows[:, :chans[f].shape[1]] = np.ascontiguousarray(chans[f]).view(np.float32).reshape(B, -1, 2)
            chan_t = T.from_numpy(rows).to("cuda:0")
            a_t = T.full((B * demod_cap * 4,), 0xAA, dtype=T.uint8, device="cuda:0")
            T.cuda.synchronize()
            demod_outs.append((a_t, r.eng.demod_device(chan_t.data_ptr(), chans[f].shape[1], a_t.data_ptr()), chan_t))
    r.eng.synchronize()
    plain.synchronize()
    for f, (out_t, n_out, _) in enumerate(outs):
        want, want_n = r.model.call(xs[f])
        same(read_out(out_t, r.shape, np.float32), n_out, want, want_n, f)
    for f, (a_t, n_out, _) in enumerate(demod_outs):
        want, want_n = demod_model.call(chans[f])
        assert n_out == want_n and a_t.cpu().numpy().tobytes() == want.tobytes(), f
    for f, (a, b) in enumerate(held):
        for x, y, name in zip(a[1:], b[1:], ("spectra", "records", "pcm")):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), (f, name)
    assert held[0][0][1].cpu().numpy().max() > 0
    r.close()
    plain.close()


def test_tune_and_listen_at_48000_hz(S, T):
    """fs = 2 MHz, N = 16384, CS8: an FM carrier 250 kHz above the centre, deviated 3 kHz by a 1 kHz tone, through
    ddc_demod_resample_host (D = 41, T = 255 -> 48 780.49 Hz; FM, 5 kHz, R = 1 -> float audio; 123 / 125, P = 16 ->
    int16 at 48 000 Hz).  Over eight frames the PCM has exactly ceil(g 123 / 125) samples for the g audio samples before
    it, its strongest bin is the tone's, and its bytes are the three restatements chained."""
    fs, n, B, frames = 2_000_000, 16384, 3, 8
    fc = fs / 41
    t = np.arange(frames * n, dtype=np.float64)
    raw = np.empty((B, 2 * frames * n), np.int8)
    for b in range(B):
        phi = 2 * np.pi * 250_000.0 * t / fs + 3.0 * np.sin(2 * np.pi * 1000.0 * t / fs + 0.7 * b) + 0.3 * b
        z = 0.5 * np.exp(1j * phi)
        raw[b, 0::2], raw[b, 1::2] = np.round(z.real * 128).astype(np.int8), np.round(z.imag * 128).astype(np.int8)
    ddc_cfg = dict(offset_hz=250_000.0, cutoff_hz=12_000.0, decimation=41, taps=255)
    demod_cfg = dict(mode=dm.FM, channel_rate_hz=fc, deviation_hz=5000.0, dc_cutoff_hz=20.0, deemphasis_us=0.0,
                     audio_decimation=1, audio_taps=31, audio_cutoff_hz=8000.0, gain=1.0, out_format=dm.OUT_F32,
                     max_in=400)
    L, M = S.resample_ratio(fs, 41, 48_000)
    assert (L, M) == (123, 125)
    rs_cfg = dict(interp=L, decim=M, taps_per_phase=16, cutoff_rel=0.9, components=1, out_format=rs.OUT_S16, gain=1.0,
                  max_in=400)
    first = raw[:, :2 * n]
    eng = engine(S, B, n, fs)
    invalid(S, eng.ddc_demod_resample_host, first, dd.CS8)  # every stage off
    eng.set_ddc(**ddc_cfg)
    eng.set_demod(**demod_cfg)
    invalid(S, eng.ddc_demod_resample_host, first, dd.CS8)  # the resampler off
    assert eng.ddc_max_out() == 400 and eng.demod_max_out() == 400
    for bad in (dict(components=2), dict(max_in=399)):
        eng.set_resample(**dict(rs_cfg, **bad))
        invalid(S, eng.ddc_demod_resample_host, first, dd.CS8)
    eng.set_resample(**rs_cfg)
    eng.set_demod(**dict(demod_cfg, out_format=dm.OUT_S16))
    invalid(S, eng.ddc_demod_resample_host, first, dd.CS8)  # the resampler reads float audio
    eng.set_demod(**dict(demod_cfg, max_in=399))
    invalid(S, eng.ddc_demod_resample_host, first, dd.CS8)  # the demodulator's max_in below the DDC's cap
    eng.set_demod(off=True)
    invalid(S, eng.ddc_demod_resample_host, first, dd.CS8)
    eng.set_demod(**demod_cfg)
    assert eng.ddc_config()["samples_consumed"] == 0 and eng.demod_config()["samples_consumed"] == 0 and \
        eng.resample_config()["samples_consumed"] == 0
    assert eng.resample_max_out() == 394
    d, c = eng.demod_config(), eng.resample_config()
    ddc_model = dd.Ddc(B, S.ddc_design(fs, **ddc_cfg), S.nco_tables(), eng.ddc_config()["nco_increment"], 41)
    demod_model = dm.Demod(B, d["mode"], d["kf"], d["alpha"], d["a"], d["taps"], 1, d["gain"], dm.OUT_F32, 400)
    model = rs.Resampler(B, L, M, c["taps"], c["gain"], rs.OUT_S16, 1, 400)
    pcm = []
    for f in range(frames):
        part = raw[:, 2 * n * f:2 * n * (f + 1)]
        got = eng.ddc_demod_resample_host(part, dd.CS8)
        chan, n_chan = ddc_model.call(dd.CS8, part)
        audio, n_audio = demod_model.call(chan[:, :n_chan])
        want, want_n = model.call(audio[:, :n_audio])
        assert got.dtype == np.int16 and got.shape == (B, want_n) and got.tobytes() == want[:, :want_n].tobytes(), f
        pcm.append(got)
        g = demod_model.g
        assert g == rs.ceil_div((f + 1) * n, 41) and eng.resample_config()["samples_consumed"] == g
        assert sum(p.shape[1] for p in pcm) == rs.ceil_div(g * 123, 125)
    assert eng.ddc_config()["samples_consumed"] == frames * n and eng.demod_config()["samples_consumed"] == g
    pcm = np.concatenate(pcm, axis=1).astype(np.float64)
    assert np.abs(pcm).max() > 10000
    y = pcm[:, 400:]  # past the filters' transients
    spec = np.abs(np.fft.rfft((y - y.mean(axis=1, keepdims=True)) * np.hanning(y.shape[1]), axis=1))
    assert np.argmax(spec, axis=1).tolist() == [int(round(1000.0 / 48_000.0 * y.shape[1]))] * B
    eng.set_resample(off=True)
    invalid(S, eng.ddc_demod_resample_host, first, dd.CS8)
    eng.close()
