"""GPU tests of the sideband stage (csrc/sideband.hip, sdrg_engine_sideband_*, sdrg_engine_listen_sideband_host): the
audio of each stream against the NumPy restatement in tests/sideband_cases.py fed the library's own cr and ci.  Every
comparison is of the bytes of the whole output (the stage is specified operation by operation: no tolerances).  `out` is
pre-filled with 0xAA between 64 guard bytes on either side, every stream has its own data, and the input rows hold NaN
past the call's n samples.

The kernel works in tiles of `tile` outputs (sdrg.sideband_geometry), stages its window by 16-byte loads where the row
is aligned and sample by sample at the window's ends, and reads the first T - 1 samples of a call's first window from
the history: the shapes below put data across each of these seams."""
import ctypes

import numpy as np
import pytest

import agc_cases as ag
import ddc_cases as dd
import demod_cases as dm
import resample_cases as rs
import sideband_cases as sb
import squelch_cases as sq
from stage_harness import GUARD, engine, invalid, out_buffer, read_out, same

pytestmark = pytest.mark.gpu

FC = 2_000_000 / 41
BASE = dict(channel_rate_hz=FC, low_hz=300.0, high_hz=2700.0, mode=sb.UPPER, audio_decimation=4, taps=63,
            out_format=sb.OUT_F32, max_in=1024, gain=0.7)


@pytest.fixture(scope="module")
def S():
    import sdrg
    return sdrg


@pytest.fixture(scope="module")
def T():
    import torch
    return torch


def rows_on_device(T, chan, max_in):
    """chan complex64 [B][n] -> a device tensor [B][max_in][2] float32, NaN past n."""
    B, n = chan.shape
    rows = np.full((B, max_in, 2), np.nan, np.float32)
    rows[:, :n] = np.ascontiguousarray(chan).view(np.float32).reshape(B, n, 2)
    return T.from_numpy(rows).to("cuda:0")


class Band:
    """An engine with the sideband stage set, and the restatement that follows it call by call."""

    def __init__(self, S, T, B, n=1024, **cfg):
        self.S, self.T, self.B = S, T, B
        self.eng = engine(S, B, n)
        self.configure(**cfg)

    def configure(self, **cfg):
        self.cfg = cfg
        self.eng.set_sideband(**cfg)
        self.remodel()

    def remodel(self):
        """A fresh restatement from the library's design of the configuration in force."""
        d = self.eng.sideband_config()
        assert all(d[k] == (np.float32(v) if k == "gain" else v) for k, v in self.cfg.items()), d
        assert d["samples_consumed"] == 0
        des = self.S.sideband_design(**self.cfg)
        assert des["cr"].tobytes() == d["cr"].tobytes() and des["ci"].tobytes() == d["ci"].tobytes()
        self.dtype = sb.OUT_DTYPE[d["out_format"]]
        self.model = sb.Sideband(self.B, d["cr"], d["ci"], d["audio_decimation"], d["mode"], d["gain"], d["out_format"],
                                 d["max_in"])

    def shape(self):
        cap = self.eng.sideband_max_out()
        return (self.B, cap, 2) if self.cfg["mode"] == sb.BOTH else (self.B, cap)

    def device_call(self, chan):
        """sideband_device into a 0xAA-filled buffer between guard bytes: (out [B][cap] or [B][cap][2], n_out)."""
        T, eng = self.T, self.eng
        shape = self.shape()
        chan_t = rows_on_device(T, chan, self.cfg["max_in"])
        out_t = out_buffer(T, int(np.prod(shape)) * np.dtype(self.dtype).itemsize)
        T.cuda.synchronize()
        n_out = eng.sideband_device(chan_t.data_ptr(), chan.shape[1], out_t.data_ptr() + GUARD)
        eng.synchronize()
        return read_out(out_t, shape, self.dtype), n_out

    def check(self, chan, what=None):
        got, n_out = self.device_call(chan)
        want, want_n = self.model.call(chan)
        same(got, n_out, want, want_n, what)
        assert self.eng.sideband_config()["samples_consumed"] == self.model.g
        return got, n_out

    def close(self):
        self.eng.close()


@pytest.mark.parametrize("fmt", [sb.OUT_F32, sb.OUT_S16])
@pytest.mark.parametrize("mode", [sb.UPPER, sb.LOWER, sb.BOTH])
def test_modes_and_formats(S, T, mode, fmt):
    """int16 with a gain that clamps a part of the samples, and an odd cap (the rows are 2-byte aligned only)."""
    B, n = 5, 999
    bd = Band(S, T, B, **dict(BASE, mode=mode, out_format=fmt, audio_decimation=3, max_in=999,
                              gain=8.0 if fmt == sb.OUT_S16 else 0.7))
    for f in range(3):
        got, n_out = bd.check(sb.noise(B, n, seed=10 + f), (mode, fmt, f))
        assert n_out == 333 and not got[:, n_out:].any()
    if fmt == sb.OUT_S16:
        assert got.dtype == np.int16 and np.any(np.abs(got) == 32767) and np.any((np.abs(got) > 100) & (np.abs(got) < 32767))
    else:
        assert np.abs(got[:, :n_out]).max() > 1e-3
    bd.close()


@pytest.mark.parametrize("B", [1, 9, 65])
def test_stream_counts(S, T, B):
    n = 200
    bd = Band(S, T, B, **dict(BASE, mode=sb.BOTH, audio_decimation=3, taps=15, max_in=256))
    for f in range(2):
        bd.check(sb.noise(B, n, seed=20 + f), (B, f))
    bd.close()


def test_short_calls_in_one_stream(S, T):
    """n = 0, 1, 2 and 63, 64, 65 in one stream: a call without samples changes nothing but out, and a window's end
    falls on either side of a 16-byte chunk."""
    B = 3
    bd = Band(S, T, B, **dict(BASE, max_in=65))
    for f, n in enumerate((65, 0, 1, 2, 63, 0, 64, 65, 0)):
        got, n_out = bd.check(sb.noise(B, n, seed=30 + f), (f, n))
        if n == 0:
            assert n_out == 0 and not got.any()
    assert bd.model.g == 65 + 1 + 2 + 63 + 64 + 65
    bd.close()


def test_first_call_without_samples(S, T):
    B = 2
    bd = Band(S, T, B, **BASE)
    got, n_out = bd.check(np.zeros((B, 0), np.complex64))
    assert n_out == 0 and not got.any() and got.shape == (B, 256)
    bd.check(sb.noise(B, 300, seed=35))
    bd.close()


@pytest.mark.parametrize("R,T2", [(1, 1), (1, 3), (3, 255), (4, 127), (16, 511), (64, 511)])
def test_tile_seams(S, T, R, T2):
    """Two tiles and a part of a third, two calls: with T > 1 every window near a multiple of the tile size reads
    samples the neighbouring tile also stages, the first tile's the history.  R = 1, T = 1 is the tap (1, 0)."""
    tile = S.sideband_geometry(R, T2)
    B, n = 2, (2 * tile + 3) * R + 5
    bd = Band(S, T, B, **dict(BASE, mode=sb.BOTH, audio_decimation=R, taps=T2, max_in=n))
    if T2 == 1:
        assert bd.model.cr.tolist() == [1.0] and bd.model.ci.tolist() == [0.0]
    for f in range(2):
        got, n_out = bd.check(sb.noise(B, n, seed=40 + f), (tile, f))
        assert n_out > 2 * tile
    bd.close()


def test_calls_shorter_than_the_history(S, T):
    """n = 100 < T - 1 = 510: most of each call's new history is the old one moved down."""
    B, n = 3, 100
    bd = Band(S, T, B, **dict(BASE, audio_decimation=7, taps=511, max_in=128))
    for f in range(7):
        bd.check(sb.noise(B, n, seed=50 + f), f)
    bd.close()


def test_five_calls_are_one_stream(S, T):
    B, lens = 4, (700, 33, 1, 2050, 127)
    bd = Band(S, T, B, **dict(BASE, mode=sb.BOTH, audio_decimation=6, taps=127, max_in=2050))
    chan = sb.noise(B, sum(lens), seed=60)
    parts, at = [], 0
    for n in lens:
        got, n_out = bd.check(chan[:, at:at + n], n)
        parts.append(got[:, :n_out])
        at += n
    m = bd.model
    whole, n_whole = sb.Sideband(B, m.cr, m.ci, m.R, m.mode, m.gain, m.out_format).call(chan)
    assert np.concatenate(parts, axis=1).tobytes() == whole[:, :n_whole].tobytes()
    bd.close()


def test_calls_without_outputs_write_zeros(S, T):
    """R = 64 at n = 10: most calls hold no multiple of 64, and still every byte of out is written."""
    B, n = 2, 10
    bd = Band(S, T, B, **dict(BASE, audio_decimation=64, taps=63, max_in=10))
    counts = []
    for f in range(14):
        got, n_out = bd.check(sb.noise(B, n, seed=70 + f), f)
        assert got.shape == (B, 1)
        if n_out == 0:
            assert not got.view(np.uint32).any()
        counts.append(n_out)
    assert counts == [1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0]  # samples 0, 64 and 128 of the stream
    bd.close()


def test_amplitudes_down_to_denormal_products(S, T):
    """Stream b at the amplitude 10^(-3 b), b = 0 .. 7, and a gain of 1e-18: from b = 6 on the outputs are denormal
    floats, kept as the restatement keeps them."""
    B, n = 8, 400
    chan = sb.noise(B, n, seed=90)
    chan = (chan * (10.0 ** (-3.0 * np.arange(B)))[:, None]).astype(np.complex64)
    bd = Band(S, T, B, **dict(BASE, mode=sb.BOTH, gain=1e-18, audio_decimation=2, taps=127, max_in=512))
    for f in range(2):
        got, n_out = bd.check(chan[:, 200 * f:200 * (f + 1)], f)
    tiny = np.abs(got[7, :n_out])
    assert 0 < tiny.max() < 1.2e-38 and np.abs(got[0]).max() > 0
    bd.close()


def test_one_longer_row(S, T):
    """B = 64, n = 16384, R = 1, T = 511: 64 tiles and the history block per stream."""
    B, n = 64, 16384
    bd = Band(S, T, B, **dict(BASE, audio_decimation=1, taps=511, max_in=n))
    got, n_out = bd.check(sb.noise(B, n, seed=100))
    assert n_out == n
    bd.close()


def test_reset_and_set_again_between_calls(S, T):
    """sideband_reset and an accepted set_sideband restart the streams; a rejected one changes nothing."""
    B, n = 2, 500
    bd = Band(S, T, B, **BASE)
    bd.check(sb.noise(B, n, seed=80))
    nan = float("nan")
    for bad in (dict(mode=3), dict(mode=-1), dict(channel_rate_hz=0.0), dict(low_hz=-1.0), dict(low_hz=2700.0),
                dict(high_hz=FC / 2 + 1), dict(high_hz=nan), dict(audio_decimation=0), dict(audio_decimation=65),
                dict(taps=64), dict(taps=513), dict(gain=float("inf")), dict(out_format=2), dict(max_in=0),
                dict(max_in=(1 << 20) + 1)):
        invalid(S, bd.eng.set_sideband, **dict(BASE, **bad))
    got = bd.eng.sideband_config()
    assert got["samples_consumed"] == n and all(got[k] == np.float32(v) if k == "gain" else got[k] == v
                                                for k, v in BASE.items())
    bd.check(sb.noise(B, n, seed=81), "after rejected set_sideband")
    bd.eng.sideband_reset()
    bd.model.reset()
    assert bd.eng.sideband_config()["samples_consumed"] == 0
    bd.check(sb.noise(B, n, seed=82), "after reset")
    bd.check(sb.noise(B, n, seed=83), "second after reset")
    bd.configure(**BASE)
    bd.check(sb.noise(B, n, seed=84), "after the same set_sideband")
    bd.configure(**dict(BASE, mode=sb.BOTH, taps=127, audio_decimation=5, out_format=sb.OUT_S16, gain=1.5))
    bd.check(sb.noise(B, n, seed=85), "after another set_sideband")
    bd.check(sb.noise(B, n, seed=86), "second after another set_sideband")
    bd.close()


def test_refusals_write_nothing_and_commit_nothing(S, T):
    B, n = 2, 300
    eng = engine(S, B)
    chan = sb.noise(B, n, seed=120)
    chan_t = rows_on_device(T, chan, 1024)
    out_t = out_buffer(T, B * 256 * 4)
    T.cuda.synchronize()
    invalid(S, eng.sideband_device, chan_t.data_ptr(), n, out_t.data_ptr() + GUARD)  # before any set_sideband
    invalid(S, eng.sideband_max_out)
    invalid(S, eng.sideband_config)
    eng.close()

    bd = Band(S, T, B, **BASE)
    bd.check(chan)
    for bad_n in (1025, -1, 1 << 30):
        invalid(S, bd.eng.sideband_device, chan_t.data_ptr(), bad_n, out_t.data_ptr() + GUARD)
    L = S.load()
    n_out = ctypes.c_int32(-7)
    assert L.sdrg_engine_sideband_device(bd.eng._h, None, n, out_t.data_ptr() + GUARD, ctypes.byref(n_out)) == -1
    assert L.sdrg_engine_sideband_device(bd.eng._h, chan_t.data_ptr(), n, None, ctypes.byref(n_out)) == -1
    assert L.sdrg_engine_sideband_device(bd.eng._h, chan_t.data_ptr(), n, out_t.data_ptr() + GUARD, None) == -1
    assert L.sdrg_engine_sideband_device(None, chan_t.data_ptr(), n, out_t.data_ptr() + GUARD, ctypes.byref(n_out)) == -1
    assert n_out.value == -7 and bd.eng.sideband_config()["samples_consumed"] == n
    bd.check(sb.noise(B, n, seed=121), "after refused calls")
    bd.eng.set_sideband(off=True)
    invalid(S, bd.eng.sideband_device, chan_t.data_ptr(), n, out_t.data_ptr() + GUARD)
    bd.eng.synchronize()
    assert np.all(out_t.cpu().numpy() == 0xAA), "a refused call wrote to out"
    bd.configure(**BASE)
    bd.check(sb.noise(B, n, seed=122), "after off and on")
    bd.close()


@pytest.mark.parametrize("mode", [sb.UPPER, sb.BOTH])
def test_host_path_equals_device_path(S, T, mode):
    B, n = 5, 777
    cfg = dict(BASE, mode=mode)
    dev = Band(S, T, B, **cfg)
    host = engine(S, B)
    host.set_sideband(**cfg)
    for f in range(3):
        chan = sb.noise(B, n - 100 * f, seed=130 + f)
        got, n_out = dev.check(chan, f)
        h = host.sideband(chan)
        assert h.dtype == np.float32 and h.shape == got[:, :n_out].shape and h.tobytes() == got[:, :n_out].tobytes()
    assert host.sideband(np.zeros((B, 0), np.complex64)).shape[:2] == (B, 0)
    with pytest.raises(S.SdrgError):
        host.sideband(np.zeros((B, 1025), np.complex64))
    dev.close()
    host.close()


def test_process_device_and_demod_device_between_sideband_calls(S, T):
    """sideband, process_device, demod_device, sideband, ...: the sideband audio is the restatement's, the
    demodulator's its restatement's, and the spectra, records and PCM are those of an engine that configured neither."""
    n, B, fmt = 16384, 4, dd.CS8
    stages = S.STAGE_SPECTRUM | S.STAGE_STATS | S.STAGE_SSB
    raws = [dd.tone(fmt, B, n, 0.01 + 0.001 * f, amp=0.4) for f in range(2)]
    demod_cfg = dict(mode=dm.AM, channel_rate_hz=200_000.0, deviation_hz=0.0, dc_cutoff_hz=300.0, deemphasis_us=0.0,
                     audio_decimation=4, audio_taps=31, audio_cutoff_hz=15_000.0, gain=0.7, out_format=dm.OUT_F32,
                     max_in=1024)

    def process(eng, f):
        iq_t = T.from_numpy(raws[f]).to("cuda:0")
        spec = T.zeros((B, n), dtype=T.float32, device="cuda:0")
        rec = T.zeros((B * S.RECORD_DTYPE.itemsize,), dtype=T.uint8, device="cuda:0")
        pcm = T.zeros((B, max(eng.pcm_len, 1)), dtype=T.int16, device="cuda:0")
        T.cuda.synchronize()
        eng.process_device(iq_t.data_ptr(), fmt, stages, spec.data_ptr(), rec.data_ptr(), pcm.data_ptr(), 1000 + f)
        return iq_t, spec, rec, pcm

    bd = Band(S, T, B, n, **BASE)
    bd.eng.set_demod(**demod_cfg)
    d = bd.eng.demod_config()
    demod = dm.Demod(B, d["mode"], d["kf"], d["alpha"], d["a"], d["taps"], 4, d["gain"], dm.OUT_F32, 1024)
    plain = engine(S, B, n)
    cap, demod_cap = bd.eng.sideband_max_out(), bd.eng.demod_max_out()
    chans = [sb.noise(B, 900 + f, seed=150 + f) for f in range(3)]
    held, outs, demod_outs = [], [], []
    for f in range(3):
        chan_t, out_t = rows_on_device(T, chans[f], 1024), out_buffer(T, B * cap * 4)
        T.cuda.synchronize()
        n_out = bd.eng.sideband_device(chan_t.data_ptr(), chans[f].shape[1], out_t.data_ptr() + GUARD)
        outs.append((out_t, n_out, chan_t))
        if f < 2:
            held.append((process(bd.eng, f), process(plain, f)))
            d_t = out_buffer(T, B * demod_cap * 4)
            T.cuda.synchronize()
            demod_outs.append((d_t, bd.eng.demod_device(chan_t.data_ptr(), chans[f].shape[1], d_t.data_ptr() + GUARD)))
    bd.eng.synchronize()
    plain.synchronize()
    for f, (out_t, n_out, _) in enumerate(outs):
        want, want_n = bd.model.call(chans[f])
        same(read_out(out_t, (B, cap), np.float32), n_out, want, want_n, f)
    for f, (d_t, n_out) in enumerate(demod_outs):
        want, want_n = demod.call(chans[f])
        same(read_out(d_t, (B, demod_cap), np.float32), n_out, want, want_n, ("demod", f))
    for f, (a, b) in enumerate(held):
        for x, y, name in zip(a[1:], b[1:], ("spectra", "records", "pcm")):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), (f, name)
    assert held[0][0][1].cpu().numpy().max() > 0
    bd.close()
    plain.close()


# ---- sdrg_engine_listen_sideband_host: fs = 2 MHz, N = 4096, CS8 noise of 3 LSB rms; from the middle of the second frame
# a carrier at +252 kHz and a weaker one at +247 kHz.  DDC at +250 kHz, D = 10, T = 63 (cap 410); squelch and AGC S = 16;
# sideband 300 - 20000 Hz, R = 4, T = 63, float; resampler 24 / 25.

LISTEN_FS, LISTEN_N, LISTEN_B, LISTEN_FRAMES, LISTEN_CAP = 2_000_000, 4096, 2, 4, 410
DDC_CFG = dict(offset_hz=250_000.0, cutoff_hz=60_000.0, decimation=10, taps=63)
SB_CFG = dict(channel_rate_hz=200_000.0, low_hz=300.0, high_hz=20_000.0, mode=sb.UPPER, audio_decimation=4, taps=63,
              out_format=sb.OUT_F32, max_in=LISTEN_CAP, gain=1.0)
DEMOD_CFG = dict(mode=dm.AM, channel_rate_hz=200_000.0, deviation_hz=0.0, dc_cutoff_hz=100.0, deemphasis_us=0.0,
                 audio_decimation=4, audio_taps=31, audio_cutoff_hz=15_000.0, gain=1.0, out_format=dm.OUT_F32,
                 max_in=LISTEN_CAP)
SQ_CFG = dict(open_db=-12.0, close_db=-18.0, tau_blocks=1.0, block=16, hang_blocks=2, max_in=LISTEN_CAP)
AGC_CFG = dict(target=0.5, max_gain_db=30.0, initial_gain_db=0.0, floor_db=-40.0, attack_blocks=0.0, decay_blocks=3.0,
               detector=ag.MEAN, block=16, hang_blocks=1, max_in=LISTEN_CAP)
RS_CFG = dict(interp=24, decim=25, taps_per_phase=8, cutoff_rel=0.9, components=1, out_format=rs.OUT_F32, gain=1.0,
              max_in=103)
MODE_OF = (sb.UPPER, sb.LOWER, sb.BOTH)  # the mode a mask is tested with: steps % 3 (BOTH with the resampler at 5)


@pytest.fixture(scope="module")
def keyed_carriers():
    """raw CS8 [B][2 N frames]: computed once."""
    fs, n, B, frames = LISTEN_FS, LISTEN_N, LISTEN_B, LISTEN_FRAMES
    t = np.arange(frames * n, dtype=np.float64)
    rng = np.random.default_rng(3)
    raw = np.empty((B, 2 * frames * n), np.int8)
    key = n + n // 2
    for b in range(B):
        z = 0.3 * (1 + b) * np.exp(2j * np.pi * 252_000.0 * t / fs + 0.3j * b)
        z = (t >= key) * (z + 0.1 * np.exp(2j * np.pi * 247_000.0 * t / fs))
        z = z + (3 / 128) * (rng.standard_normal(t.size) + 1j * rng.standard_normal(t.size))
        raw[b, 0::2] = np.round(z.real * 128).clip(-128, 127).astype(np.int8)
        raw[b, 1::2] = np.round(z.imag * 128).clip(-128, 127).astype(np.int8)
    return raw


def listen_engine(S, steps, mode, every_stage=False, demod=False):
    eng = engine(S, LISTEN_B, LISTEN_N, LISTEN_FS)
    eng.set_ddc(**DDC_CFG)
    eng.set_sideband(**dict(SB_CFG, mode=mode))
    if demod:
        eng.set_demod(**DEMOD_CFG)
    if every_stage or steps & S.LISTEN_SQUELCH:
        eng.set_squelch(**SQ_CFG)
    if every_stage or steps & S.LISTEN_AGC:
        eng.set_agc(**AGC_CFG)
    if every_stage or steps & S.LISTEN_RESAMPLE:
        eng.set_resample(**dict(RS_CFG, components=2 if mode == sb.BOTH else 1))
    return eng


@pytest.fixture(scope="module")
def ddc_restated(S, T, keyed_carriers):
    """The DDC's restatement of every frame, which every mask shares: [(chan [B][cap], n_chan)]."""
    eng = listen_engine(S, 0, sb.UPPER)
    taps, tab, inc = S.ddc_design(LISTEN_FS, **DDC_CFG), S.nco_tables(), eng.ddc_config()["nco_increment"]
    assert eng.ddc_max_out() == LISTEN_CAP
    eng.close()
    model = dd.Ddc(LISTEN_B, taps, tab, inc, 10)
    n = LISTEN_N
    return [model.call(dd.CS8, keyed_carriers[:, 2 * n * f:2 * n * (f + 1)]) for f in range(LISTEN_FRAMES)]


@pytest.mark.parametrize("steps", range(8))
def test_listen_sideband_equals_the_restatements_chained(S, T, keyed_carriers, ddc_restated, steps):
    B, n, mode = LISTEN_B, LISTEN_N, MODE_OF[steps % 3]
    comps = 2 if mode == sb.BOTH else 1
    eng = listen_engine(S, steps, mode, every_stage=True, demod=True)  # every stage set: the mask alone decides which run
    d, q, c = eng.sideband_config(), eng.squelch_config(), eng.resample_config()
    gate = sq.Squelch(B, q["open_thr"], q["close_thr"], q["beta"], 16, 2)
    agc = ag.Agc(B, AGC_CFG["target"], S.agc_design(**AGC_CFG), 16, 1)
    band = sb.Sideband(B, d["cr"], d["ci"], 4, mode, d["gain"], sb.OUT_F32, LISTEN_CAP)
    rsm = rs.Resampler(B, 24, 25, c["taps"], c["gain"], rs.OUT_F32, comps, 103)
    opened, gains = [], []
    for f in range(LISTEN_FRAMES):
        got, sq_rec, agc_rec = eng.listen_sideband(keyed_carriers[:, 2 * n * f:2 * n * (f + 1)], dd.CS8, steps)
        chan, n_chan = ddc_restated[f]
        chan = chan[:, :n_chan]
        if steps & S.LISTEN_SQUELCH:
            chan, want_rec, _ = gate.call(chan)
            assert sq_rec.tobytes() == want_rec.tobytes(), f
            opened.append(sq_rec["open"].tolist())
        else:
            assert sq_rec is None
        if steps & S.LISTEN_AGC:
            chan, want_rec, _ = agc.call(chan)
            assert agc_rec.tobytes() == want_rec.tobytes(), f
            gains.append(agc_rec["gain"].copy())
        else:
            assert agc_rec is None
        want, want_n = band.call(chan)
        want = want[:, :want_n]
        if steps & S.LISTEN_RESAMPLE:
            rows = np.ascontiguousarray(want).view(np.complex64)[..., 0] if comps == 2 else want
            want, want_n = rsm.call(rows)
            want = want[:, :want_n]
        assert got.dtype == np.float32 and got.shape == want.shape and got.tobytes() == want.tobytes(), f
    assert np.abs(got).max() > 0.05
    g = [eng.ddc_config()["samples_consumed"], eng.squelch_config()["samples_consumed"],
         eng.agc_config()["samples_consumed"], eng.sideband_config()["samples_consumed"],
         eng.demod_config()["samples_consumed"]]
    assert g == [LISTEN_FRAMES * n, gate.g, agc.g, sum(n_chan for _, n_chan in ddc_restated), 0]
    if steps & S.LISTEN_SQUELCH:
        assert opened[0] == [0] * B and opened[-1] == [1] * B
    if steps & S.LISTEN_AGC:
        assert gains[-1][1] < gains[-1][0]  # the stronger carrier ends on the smaller gain
    eng.close()


def test_listen_sideband_refusals(S, T, keyed_carriers):
    """Each stage off while in the mask, each max_in below the row it reads, the components rule, int16 ahead of the
    resampler, unknown bits, null pointers: SDRG_E_INVALID, and no stage has moved."""
    first = keyed_carriers[:, :2 * LISTEN_N]
    ALL = S.LISTEN_SQUELCH | S.LISTEN_AGC | S.LISTEN_RESAMPLE
    eng = listen_engine(S, ALL, sb.UPPER)
    sets = dict(ddc=(eng.set_ddc, DDC_CFG), sideband=(eng.set_sideband, SB_CFG), squelch=(eng.set_squelch, SQ_CFG),
                agc=(eng.set_agc, AGC_CFG), resample=(eng.set_resample, RS_CFG))
    L, n_out = S.load(), ctypes.c_int32(-7)
    out = np.full((LISTEN_B, 256), 7.0, np.float32)
    iq_p, out_p = first.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)

    def refused(steps=ALL):
        assert L.sdrg_engine_listen_sideband_host(eng._h, steps, iq_p, dd.CS8, out_p, ctypes.byref(n_out), None, None) == -1

    for name, (setter, cfg) in sets.items():
        setter(off=True)
        refused()
        invalid(S, eng.listen_sideband, first, dd.CS8, ALL)
        setter(**cfg)
    for name in ("sideband", "squelch", "agc"):
        setter, cfg = sets[name]
        setter(**dict(cfg, max_in=LISTEN_CAP - 1))
        refused()
        setter(**cfg)
    eng.set_resample(**dict(RS_CFG, max_in=102))
    refused()
    eng.set_resample(**dict(RS_CFG, components=2))  # UPPER writes one value per output
    refused()
    eng.set_sideband(**dict(SB_CFG, mode=sb.BOTH))  # and now the pair: accepted
    assert L.sdrg_engine_listen_sideband_host(eng._h, ALL, iq_p, dd.CS8, out_p, ctypes.byref(n_out), None, None) == 0
    eng.set_resample(**RS_CFG)  # BOTH into one component
    n_out.value = -7
    out[:] = 7.0
    refused()
    eng.set_sideband(**dict(SB_CFG, out_format=sb.OUT_S16))
    refused()
    got, _, _ = eng.listen_sideband(first, dd.CS8, S.LISTEN_SQUELCH | S.LISTEN_AGC)  # int16 is fine without the resampler
    assert got.dtype == np.int16
    eng.set_sideband(**SB_CFG)
    # a stage that is off and not in the mask does not matter, the demodulator among them
    eng.set_agc(off=True)
    invalid(S, eng.demod_config)
    got, sq_rec, agc_rec = eng.listen_sideband(first, dd.CS8, S.LISTEN_SQUELCH)
    assert agc_rec is None and sq_rec is not None
    eng.set_agc(**AGC_CFG)
    consumed = lambda: [eng.ddc_config()["samples_consumed"], eng.squelch_config()["samples_consumed"],  # noqa: E731
                        eng.agc_config()["samples_consumed"], eng.sideband_config()["samples_consumed"],
                        eng.resample_config()["samples_consumed"]]
    before = consumed()
    for bad in (8, 16, -1, ALL | 64):
        refused(bad)
    lsh = L.sdrg_engine_listen_sideband_host
    assert lsh(eng._h, ALL, None, dd.CS8, out_p, ctypes.byref(n_out), None, None) == -1
    assert lsh(eng._h, ALL, iq_p, dd.CS8, None, ctypes.byref(n_out), None, None) == -1
    assert lsh(eng._h, ALL, iq_p, dd.CS8, out_p, None, None, None) == -1
    assert lsh(None, ALL, iq_p, dd.CS8, out_p, ctypes.byref(n_out), None, None) == -1
    assert lsh(eng._h, ALL, iq_p, 99, out_p, ctypes.byref(n_out), None, None) == -1
    assert n_out.value == -7 and np.all(out == 7.0) and consumed() == before
    # records are optional, each on its own
    agc_only = np.zeros(LISTEN_B, S.AGC_RECORD_DTYPE)
    assert lsh(eng._h, ALL, iq_p, dd.CS8, out_p, ctypes.byref(n_out), None, agc_only.ctypes.data_as(ctypes.c_void_p)) == 0
    assert n_out.value > 0 and np.all(agc_only["gain"] > 0)
    eng.close()


@pytest.mark.parametrize("steps", [0, 7])
def test_listen_host_is_what_it_was_with_the_sideband_stage_set(S, T, keyed_carriers, steps):
    n = LISTEN_N
    a, b = listen_engine(S, steps, sb.BOTH, every_stage=True, demod=True), engine(S, LISTEN_B, LISTEN_N, LISTEN_FS)
    for setter, cfg in ((b.set_ddc, DDC_CFG), (b.set_demod, DEMOD_CFG), (b.set_squelch, SQ_CFG), (b.set_agc, AGC_CFG),
                        (b.set_resample, RS_CFG)):
        setter(**cfg)
    a.set_resample(**RS_CFG)
    for f in range(LISTEN_FRAMES):
        part = keyed_carriers[:, 2 * n * f:2 * n * (f + 1)]
        got, want = a.listen(part, dd.CS8, steps), b.listen(part, dd.CS8, steps)
        for x, y in zip(got, want):
            assert (x is None and y is None) or (x.shape == y.shape and x.tobytes() == y.tobytes()), f
    assert a.sideband_config()["samples_consumed"] == 0  # set, and not in the chain: it has not moved
    invalid(S, a.listen, keyed_carriers[:, :2 * n], dd.CS8, 8)
    a.close()
    b.close()


def test_two_tones_come_out_of_a_sideband_each(S, T):
    """The behavioural case of tests/sideband_cases.py through listen_sideband: the device's bytes are the restatements
    chained, the upper column peaks at the 1 kHz bin with the 1.5 kHz bin at least 60 dB below it, and the lower
    column the reverse (tests/test_sideband_cases.py holds the same on the restatements alone: 80.3 and 75.0 dB)."""
    fs, n, frames = sb.TWO_TONE_FS, sb.TWO_TONE_N, sb.TWO_TONE_FRAMES
    raw = sb.two_tone_raw()
    eng = engine(S, 1, n, fs)
    eng.set_ddc(**sb.TWO_TONE_DDC)
    eng.set_sideband(**sb.TWO_TONE_SIDEBAND)
    assert eng.ddc_max_out() == 400
    d = eng.sideband_config()
    ddc = dd.Ddc(1, S.ddc_design(fs, **sb.TWO_TONE_DDC), S.nco_tables(), eng.ddc_config()["nco_increment"], 41)
    band = sb.Sideband(1, d["cr"], d["ci"], 1, sb.BOTH, 1.0, sb.OUT_F32, 400)
    cols = []
    for f in range(frames):
        part = raw[:, 2 * n * f:2 * n * (f + 1)]
        got, _, _ = eng.listen_sideband(part, dd.CS8, 0)
        chan, n_chan = ddc.call(dd.CS8, part)
        want, want_n = band.call(chan[:, :n_chan])
        assert got.shape == (1, want_n, 2) and got.tobytes() == want[:, :want_n].tobytes(), f
        cols.append(got[0])
    cols = np.concatenate(cols)
    peak, k1, k15, up_db = sb.two_tone_separation_db(cols[:, 0])
    assert peak == k1 and up_db >= 60.0, (peak, k1, up_db)
    peak, k1, k15, lo_db = sb.two_tone_separation_db(cols[:, 1])
    assert peak == k15 and -lo_db >= 60.0, (peak, k15, lo_db)
    eng.close()
