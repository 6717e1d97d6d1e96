"""GPU tests of the demodulator stage (csrc/demod.hip, sdrg_engine_demod_*, sdrg_engine_ddc_demod_host): the audio of
each stream against the NumPy restatement in tests/demod_cases.py fed the library's own design values.  Every comparison
is of the bytes of the whole output (the stage is specified operation by operation: no tolerances); float output is the
main format, since int16 would hide a last-bit error.  `out` is pre-filled with 0xAA between 64 guard bytes on either
side, every stream has its own data, and the input rows hold NaN past the call's n samples.

The detector works in tiles of 256 samples, the recurrence kernel in groups of 16 streams and steps of `chunk` samples,
the FIR in tiles of `tile` outputs (sdrg.demod_geometry): the shapes below put data across each of these seams."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import ddc_cases as dd
import demod_cases as dm
from stage_harness import GUARD, engine, invalid, out_buffer, read_out, same

pytestmark = pytest.mark.gpu

BASE = dict(mode=dm.FM, channel_rate_hz=200_000.0, deviation_hz=75_000.0, dc_cutoff_hz=300.0, deemphasis_us=75.0,
            audio_decimation=4, audio_taps=31, audio_cutoff_hz=15_000.0, gain=0.7, out_format=dm.OUT_F32, max_in=1024)


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


class Audio:
    """An engine with the demodulator set, and the restatement that follows it call by call."""

    def __init__(self, S, T, B, n=1024, **cfg):
        self.S, self.T, self.B = S, T, B
        self.eng = engine(S, B, n)
        self.configure(**cfg)

    def configure(self, **cfg):
        self.cfg = cfg
        self.eng.set_demod(**cfg)
        self.remodel()

    def remodel(self):
        """A fresh restatement from the library's design of the configuration in force."""
        d = self.eng.demod_config()
        assert all(d[k] == (np.float32(v) if k == "gain" else v) for k, v in self.cfg.items()), d
        assert d["samples_consumed"] == 0
        des = self.S.demod_design(**self.cfg)
        assert des["taps"].tobytes() == d["taps"].tobytes() and (des["kf"], des["alpha"], des["a"]) == \
            (d["kf"], d["alpha"], d["a"])
        self.dtype = dm.OUT_DTYPE[d["out_format"]]
        self.model = dm.Demod(self.B, d["mode"], d["kf"], d["alpha"], d["a"], d["taps"], d["audio_decimation"],
                              d["gain"], d["out_format"], d["max_in"])

    def device_call(self, chan):
        """demod_device into a 0xAA-filled buffer between guard bytes: (out [B][cap], n_out)."""
        T, eng = self.T, self.eng
        cap = eng.demod_max_out()
        chan_t = rows_on_device(T, chan, self.cfg["max_in"])
        out_t = out_buffer(T, self.B * cap * np.dtype(self.dtype).itemsize)
        T.cuda.synchronize()
        n_out = eng.demod_device(chan_t.data_ptr(), chan.shape[1], out_t.data_ptr() + GUARD)
        eng.synchronize()
        return read_out(out_t, (self.B, cap), self.dtype), n_out

    def check(self, chan, what=None):
        got, n_out = self.device_call(chan)
        want, want_n = self.model.call(chan)
        same(got, n_out, want, want_n, what)
        assert self.eng.demod_config()["samples_consumed"] == self.model.g
        return got, n_out

    def close(self):
        self.eng.close()


@pytest.mark.parametrize("de", [0.0, 75.0])
@pytest.mark.parametrize("dc", [0.0, 300.0])
@pytest.mark.parametrize("mode", [dm.AM, dm.FM])
def test_modes_and_recurrences(S, T, mode, dc, de):
    B, n = 5, 700
    au = Audio(S, T, B, **dict(BASE, mode=mode, dc_cutoff_hz=dc, deemphasis_us=de))
    assert (au.model.alpha != 0) == (dc != 0) and (au.model.a != 0) == (de != 0)
    for f in range(3):
        got, n_out = au.check(dm.noise(B, n, seed=10 + f), (mode, dc, de, f))
        assert n_out == 175 and np.abs(got[:, :n_out]).max() > 1e-3 and not got[:, n_out:].any()
    au.close()


@pytest.mark.parametrize("B", [1, 9, 65, 130])
def test_stream_counts(S, T, B):
    """The recurrence kernel takes 16 streams per wave (64 in its first version): a group in part, whole groups and a
    stream, whole groups and two streams."""
    n = 200
    au = Audio(S, T, B, **dict(BASE, audio_decimation=3, audio_taps=15, max_in=256))
    for f in range(2):
        au.check(dm.noise(B, n, seed=20 + f), (B, f))
    au.close()


def test_calls_around_the_chunk(S, T):
    """n = 0, 1, 2 and chunk - 1, chunk, chunk + 1, in one stream: the recurrence kernel's last step is whole, short by
    one or a single sample, and a call without samples changes nothing but out."""
    B = 3
    _, chunk = S.demod_geometry(4, 31)
    au = Audio(S, T, B, **dict(BASE, max_in=chunk + 1))
    for f, n in enumerate((chunk + 1, 0, 1, 2, chunk - 1, 0, chunk, chunk + 1, 0)):
        got, n_out = au.check(dm.noise(B, n, seed=30 + f), (f, n))
        if n == 0:
            assert n_out == 0 and not got.any()
    assert au.model.g == 4 * chunk + 4
    au.close()


def test_first_call_without_samples(S, T):
    B = 2
    au = Audio(S, T, B, **BASE)
    got, n_out = au.check(np.zeros((B, 0), np.complex64))
    assert n_out == 0 and not got.any() and got.shape == (B, 256)
    au.check(dm.noise(B, 300, seed=35))
    au.close()


@pytest.mark.parametrize("T2", [1, 3, 255])
@pytest.mark.parametrize("R", [1, 3, 16, 64])
def test_tile_seams(S, T, R, T2):
    """Two FIR tiles and a part of a third, two calls: with T2 > 1 every window near a multiple of the tile size reads
    values the neighbouring tile also stages, the first tile's the history.  R = 1, T2 = 1 is the tap 1.0."""
    tile, _ = S.demod_geometry(R, T2)
    B, n = 2, (2 * tile + 3) * R + 5
    fc = 200_000.0
    au = Audio(S, T, B, **dict(BASE, mode=dm.AM, dc_cutoff_hz=0.0, audio_decimation=R, audio_taps=T2,
                               audio_cutoff_hz=min(fc / 2, 0.4 * fc / R), max_in=n))
    if R == 1 and T2 == 1:
        assert au.model.h.tolist() == [1.0]
    for f in range(2):
        got, n_out = au.check(dm.noise(B, n, seed=40 + f), (tile, f))
        assert n_out > 2 * tile
    au.close()


def test_calls_shorter_than_the_history(S, T):
    """n = 100 < T2 - 1 = 254: most of each call's new history is the old one moved down."""
    B, n = 3, 100
    au = Audio(S, T, B, **dict(BASE, audio_decimation=7, audio_taps=255, audio_cutoff_hz=10_000.0, max_in=128))
    for f in range(6):
        au.check(dm.noise(B, n, seed=50 + f), f)
    au.close()


def test_five_calls_are_one_stream(S, T):
    B, lens = 4, (700, 33, 1, 2050, 127)
    au = Audio(S, T, B, **dict(BASE, audio_decimation=6, audio_taps=127, max_in=2050))
    chan = dm.noise(B, sum(lens), seed=60)
    parts, at = [], 0
    for n in lens:
        got, n_out = au.check(chan[:, at:at + n], n)
        parts.append(got[:, :n_out])
        at += n
    m = au.model
    whole, n_whole = dm.Demod(B, m.mode, m.kf, m.alpha, m.a, m.h, m.R, m.gain, m.out_format).call(chan)
    assert np.concatenate(parts, axis=1).tobytes() == whole[:, :n_whole].tobytes()
    au.close()


def test_calls_without_outputs_write_zeros(S, T):
    """R = 64 at n = 10: most calls hold no multiple of 64, and still every byte of out is written."""
    B, n = 2, 10
    au = Audio(S, T, B, **dict(BASE, audio_decimation=64, audio_taps=63, audio_cutoff_hz=1000.0, max_in=10))
    counts = []
    for f in range(14):
        got, n_out = au.check(dm.noise(B, n, seed=70 + f), f)
        assert got.shape == (B, 1)
        if n_out == 0:
            assert not got.view(np.uint32).any()
        counts.append(n_out)
    assert counts == [1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0]  # samples 0, 64 and 128 of the stream
    au.close()


def test_reset_and_set_again_between_calls(S, T):
    """demod_reset and an accepted set_demod restart the streams; a rejected one changes nothing."""
    B, n = 2, 500
    au = Audio(S, T, B, **BASE)
    au.check(dm.noise(B, n, seed=80))
    nan = float("nan")
    for bad in (dict(mode=2), dict(channel_rate_hz=0.0), dict(deviation_hz=0.0), dict(dc_cutoff_hz=-1.0),
                dict(deemphasis_us=nan), dict(audio_decimation=65), dict(audio_taps=32), dict(audio_taps=257),
                dict(audio_cutoff_hz=100_001.0), dict(gain=nan), dict(out_format=2), dict(max_in=0),
                dict(max_in=(1 << 20) + 1)):
        invalid(S, au.eng.set_demod, **dict(BASE, **bad))
    got = au.eng.demod_config()
    assert got["samples_consumed"] == n and all(got[k] == np.float32(v) if k == "gain" else got[k] == v
                                                for k, v in BASE.items())
    au.check(dm.noise(B, n, seed=81), "after rejected set_demod")
    au.eng.demod_reset()
    au.model.reset()
    assert au.eng.demod_config()["samples_consumed"] == 0
    au.check(dm.noise(B, n, seed=82), "after reset")
    au.check(dm.noise(B, n, seed=83), "second after reset")
    au.configure(**BASE)
    au.check(dm.noise(B, n, seed=84), "after the same set_demod")
    au.configure(**dict(BASE, mode=dm.AM, audio_taps=63, audio_decimation=5, out_format=dm.OUT_S16, gain=1.5))
    au.check(dm.noise(B, n, seed=85), "after another set_demod")
    au.check(dm.noise(B, n, seed=86), "second after another set_demod")
    au.close()


@pytest.mark.parametrize("mode", [dm.AM, dm.FM])
def test_amplitudes_down_to_denormal_products(S, T, mode):
    """Stream b at the amplitude 10^(-3 b), b = 0 .. 7: from 1e-21 down the products zr zr, zr wr are denormal floats
    (1e-42), and the quotient and the root work on denormal operands."""
    B, n = 8, 400
    chan = dm.noise(B, n, seed=90)
    chan = (chan * (10.0 ** (-3.0 * np.arange(B)))[:, None]).astype(np.complex64)
    assert 0 < np.abs(chan[7].real).max() ** 2 < 1.2e-38
    au = Audio(S, T, B, **dict(BASE, mode=mode, gain=1.0, audio_decimation=2, max_in=512))
    for f in range(2):
        got, n_out = au.check(chan[:, 200 * f:200 * (f + 1)], (mode, f))
    assert np.abs(got[7]).max() > 0
    au.close()


def test_fm_steps_in_every_quadrant_and_at_pi(S, T):
    """kf = 1, no filters: the output is the phase step itself.  Axis and diagonal steps, +pi and -pi (the sign of a
    zero imaginary product), zero samples (p = (+-0, +-0)) and random steps over the whole circle."""
    B, nz = 4, np.float32(-0.0)
    head = np.array([1, 1j, -1, -1j, 1 + 1j, -1 - 1j, 1, -1, 0, 0, 1, 0.5 - 0.5j, -2 + 2j], np.complex64)
    tail = np.zeros(4, np.complex64)
    tail.real[:], tail.imag[:] = [1, -1, 1, -1], [nz, nz, 0.0, nz]  # (1, -0) -> (-1, -0): pi = -0, pr = -1: -pi
    rng = np.random.default_rng(95)
    chan = np.empty((B, head.size + tail.size + 600), np.complex64)
    for b in range(B):
        ph = np.cumsum(rng.uniform(-np.pi, np.pi, 600))
        chan[b] = np.concatenate([head * (b + 1), tail, (0.3 * (b + 1) * np.exp(1j * ph)).astype(np.complex64)])
    cfg = dict(BASE, deviation_hz=200_000.0 / (2 * np.pi), dc_cutoff_hz=0.0, deemphasis_us=0.0, audio_decimation=1,
               audio_taps=1, audio_cutoff_hz=100_000.0, gain=1.0)
    au = Audio(S, T, B, **cfg)
    assert abs(float(au.model.kf) - 1.0) < 1e-6
    got, n_out = au.check(chan)
    e = got[0, :n_out] / au.model.kf
    assert n_out == chan.shape[1]
    for lo, hi in ((0, np.pi / 2), (np.pi / 2, np.pi), (-np.pi / 2, 0), (-np.pi, -np.pi / 2)):
        assert np.any((e > lo) & (e < hi))
    assert np.any(got[0] == dm.PI * au.model.kf) and np.any(got[0] == -dm.PI * au.model.kf)
    au.close()


def test_one_longer_row(S, T):
    """B = 64, n = 16384, R = 1: 256 steps of the recurrence kernel in four whole groups of streams, 64 FIR tiles."""
    B, n = 64, 16384
    au = Audio(S, T, B, **dict(BASE, audio_decimation=1, max_in=n))
    got, n_out = au.check(dm.noise(B, n, seed=100))
    assert n_out == n
    au.close()


@pytest.mark.parametrize("mode", [dm.AM, dm.FM])
def test_s16_output(S, T, mode):
    """int16 PCM: a gain that clamps a part of the samples, odd cap (the rows are 2-byte aligned only)."""
    B, n = 5, 999
    au = Audio(S, T, B, **dict(BASE, mode=mode, out_format=dm.OUT_S16, gain=12.0 if mode == dm.AM else 8.0,
                               audio_decimation=3, max_in=999))
    for f in range(2):
        got, n_out = au.check(dm.noise(B, n, seed=110 + f), (mode, f))
    assert got.dtype == np.int16 and n_out == 333
    assert np.any(np.abs(got) == 32767) and np.any((np.abs(got) > 100) & (np.abs(got) < 32767))
    au.close()


def test_refusals_write_nothing_and_commit_nothing(S, T):
    B, n = 2, 300
    eng = engine(S, B)
    chan = dm.noise(B, n, seed=120)
    chan_t = rows_on_device(T, chan, 1024)
    out_t = out_buffer(T, B * 256 * 4)
    T.cuda.synchronize()
    invalid(S, eng.demod_device, chan_t.data_ptr(), n, out_t.data_ptr() + GUARD)  # before any set_demod
    invalid(S, eng.demod_max_out)
    invalid(S, eng.demod_config)
    eng.close()

    au = Audio(S, T, B, **BASE)
    au.check(chan)
    for bad_n in (1025, -1, 1 << 30):
        invalid(S, au.eng.demod_device, chan_t.data_ptr(), bad_n, out_t.data_ptr() + GUARD)
    L = S.load()
    n_out = ctypes.c_int32(-7)
    assert L.sdrg_engine_demod_device(au.eng._h, None, n, out_t.data_ptr() + GUARD, ctypes.byref(n_out)) == -1
    assert L.sdrg_engine_demod_device(au.eng._h, chan_t.data_ptr(), n, None, ctypes.byref(n_out)) == -1
    assert L.sdrg_engine_demod_device(au.eng._h, chan_t.data_ptr(), n, out_t.data_ptr() + GUARD, None) == -1
    assert L.sdrg_engine_demod_device(None, chan_t.data_ptr(), n, out_t.data_ptr() + GUARD, ctypes.byref(n_out)) == -1
    assert n_out.value == -7 and au.eng.demod_config()["samples_consumed"] == n
    au.check(dm.noise(B, n, seed=121), "after refused calls")
    au.eng.set_demod(off=True)
    invalid(S, au.eng.demod_device, chan_t.data_ptr(), n, out_t.data_ptr() + GUARD)
    au.eng.synchronize()
    assert np.all(out_t.cpu().numpy() == 0xAA), "a refused call wrote to out"
    au.configure(**BASE)
    au.check(dm.noise(B, n, seed=122), "after off and on")
    au.close()


def test_host_path_equals_device_path(S, T):
    B, n = 5, 777
    dev = Audio(S, T, B, **BASE)
    host = engine(S, B)
    host.set_demod(**BASE)
    for f in range(3):
        chan = dm.noise(B, n - 100 * f, seed=130 + f)
        got, n_out = dev.check(chan, f)
        h = host.demod(chan)
        assert h.dtype == np.float32 and h.shape == (B, n_out) and h.tobytes() == got[:, :n_out].tobytes()
    assert host.demod(np.zeros((B, 0), np.complex64)).shape == (B, 0)
    with pytest.raises(S.SdrgError):
        host.demod(np.zeros((B, 1025), np.complex64))
    dev.close()
    host.close()


def test_wait_outputs_orders_a_consumer_stream(S, T):
    B, n = 16, 4096
    au = Audio(S, T, B, **dict(BASE, max_in=n))
    cap = au.eng.demod_max_out()
    consumer = T.cuda.Stream("cuda:0")
    out_t = out_buffer(T, B * cap * 4)
    copy = T.zeros_like(out_t)
    T.cuda.synchronize()
    for f in range(3):
        chan = dm.noise(B, n, seed=140 + f)
        chan_t = rows_on_device(T, chan, n)
        T.cuda.synchronize()
        n_out = au.eng.demod_device(chan_t.data_ptr(), n, out_t.data_ptr() + GUARD)
        au.eng.wait_outputs(consumer.cuda_stream)
        with T.cuda.stream(consumer):
            copy.copy_(out_t)
        consumer.synchronize()
        want, want_n = au.model.call(chan)
        same(read_out(copy, (B, cap), np.float32), n_out, want, want_n, f)
    au.close()


def test_process_device_and_ddc_device_between_demod_calls(S, T):
    """demod, process_device, ddc_device, demod, ...: the audio is the restatement's, the DDC's channel its
    restatement's, and the spectra, records and PCM are those of an engine that configured neither stage."""
    n, B, fmt = 16384, 4, dd.CS8
    stages = S.STAGE_SPECTRUM | S.STAGE_STATS | S.STAGE_SSB
    raws = [dd.tone(fmt, B, n, 0.01 + 0.001 * f, amp=0.4) for f in range(2)]
    tab = S.nco_tables()
    ddc_cfg = dict(offset_hz=20_000.0, cutoff_hz=20_000.0, decimation=41, taps=255)

    def process(eng, f):
        iq_t = T.from_numpy(raws[f]).to("cuda:0")
        spec = T.zeros((B, n), dtype=T.float32, device="cuda:0")
        rec = T.zeros((B * S.RECORD_DTYPE.itemsize,), dtype=T.uint8, device="cuda:0")
        pcm = T.zeros((B, max(eng.pcm_len, 1)), dtype=T.int16, device="cuda:0")
        T.cuda.synchronize()
        eng.process_device(iq_t.data_ptr(), fmt, stages, spec.data_ptr(), rec.data_ptr(), pcm.data_ptr(), 1000 + f)
        return iq_t, spec, rec, pcm

    au = Audio(S, T, B, n, **BASE)
    au.eng.set_ddc(**ddc_cfg)
    ddc_model = dd.Ddc(B, S.ddc_design(2_000_000, **ddc_cfg), tab, au.eng.ddc_config()["nco_increment"], 41)
    plain = engine(S, B, n)
    cap, ddc_cap = au.eng.demod_max_out(), au.eng.ddc_max_out()
    chans = [dm.noise(B, 900 + f, seed=150 + f) for f in range(3)]
    held, outs, ddc_outs = [], [], []
    for f in range(3):
        chan_t, out_t = rows_on_device(T, chans[f], 1024), out_buffer(T, B * cap * 4)
        T.cuda.synchronize()
        n_out = au.eng.demod_device(chan_t.data_ptr(), chans[f].shape[1], out_t.data_ptr() + GUARD)
        outs.append((out_t, n_out, chan_t))
        if f < 2:
            held.append((process(au.eng, f), process(plain, f)))
            iq_t = T.from_numpy(raws[f]).to("cuda:0")
            d_t = T.full((B * ddc_cap * 8,), 0xAA, dtype=T.uint8, device="cuda:0")
            T.cuda.synchronize()
            ddc_outs.append((d_t, au.eng.ddc_device(iq_t.data_ptr(), fmt, d_t.data_ptr()), iq_t))
    au.eng.synchronize()
    plain.synchronize()
    for f, (out_t, n_out, _) in enumerate(outs):
        want, want_n = au.model.call(chans[f])
        same(read_out(out_t, (B, cap), np.float32), n_out, want, want_n, f)
    for f, (d_t, n_out, _) in enumerate(ddc_outs):
        want, want_n = ddc_model.call(fmt, raws[f])
        assert n_out == want_n and d_t.cpu().numpy().tobytes() == want.tobytes(), f
    for f, (a, b) in enumerate(held):
        for x, y, name in zip(a[1:], b[1:], ("spectra", "records", "pcm")):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), (f, name)
    assert held[0][0][1].cpu().numpy().max() > 0
    au.close()
    plain.close()


def test_tune_and_listen_end_to_end(S, T):
    """fs = 2 MHz, N = 16384, CS8: an FM carrier 250 kHz above the centre, deviated 50 kHz by a 1 kHz tone, through
    ddc_demod_host (D = 10, T = 127 -> 200 kHz; FM, 75 kHz, DC block, 75 us, R = 4, T2 = 127 -> int16 at 50 kHz).  Over
    three frames the PCM's strongest bin is the tone's, and its bytes are the restated DDC's through the restated
    demodulator."""
    fs, n, B, frames = 2_000_000, 16384, 3, 3
    t = np.arange(frames * n, dtype=np.float64)
    raw = np.empty((B, 2 * frames * n), np.int8)
    for b in range(B):
        phi = 2 * np.pi * 250_000.0 * t / fs + 50.0 * np.sin(2 * np.pi * 1000.0 * t / fs + 0.7 * b) + 0.3 * b
        z = 0.5 * np.exp(1j * phi)
        raw[b, 0::2], raw[b, 1::2] = np.round(z.real * 128).astype(np.int8), np.round(z.imag * 128).astype(np.int8)
    ddc_cfg = dict(offset_hz=250_000.0, cutoff_hz=100_000.0, decimation=10, taps=127)
    cfg = dict(BASE, dc_cutoff_hz=20.0, audio_taps=127, out_format=dm.OUT_S16, gain=1.0, max_in=1639)
    eng = engine(S, B, n, fs)
    invalid(S, eng.ddc_demod, raw[:, :2 * n], dd.CS8)  # both stages off
    eng.set_demod(**cfg)
    invalid(S, eng.ddc_demod, raw[:, :2 * n], dd.CS8)  # the DDC off
    eng.set_ddc(**ddc_cfg)
    assert eng.ddc_max_out() == 1639 and eng.demod_max_out() == 410
    eng.set_demod(**dict(cfg, max_in=1638))
    invalid(S, eng.ddc_demod, raw[:, :2 * n], dd.CS8)  # max_in below the DDC's cap
    assert eng.ddc_config()["samples_consumed"] == 0 and eng.demod_config()["samples_consumed"] == 0
    eng.set_demod(**cfg)
    d = eng.demod_config()
    ddc_model = dd.Ddc(B, S.ddc_design(fs, **ddc_cfg), S.nco_tables(), eng.ddc_config()["nco_increment"], 10)
    model = dm.Demod(B, d["mode"], d["kf"], d["alpha"], d["a"], d["taps"], 4, d["gain"], dm.OUT_S16, 1639)
    pcm = []
    for f in range(frames):
        part = raw[:, 2 * n * f:2 * n * (f + 1)]
        got = eng.ddc_demod(part, dd.CS8)
        chan, n_chan = ddc_model.call(dd.CS8, part)
        want, want_n = model.call(chan[:, :n_chan])
        assert got.dtype == np.int16 and got.shape == (B, want_n) and got.tobytes() == want[:, :want_n].tobytes(), f
        pcm.append(got)
    assert eng.ddc_config()["samples_consumed"] == frames * n and eng.demod_config()["samples_consumed"] == model.g
    pcm = np.concatenate(pcm, axis=1).astype(np.float64)
    assert pcm.shape[1] == -(-(-(-frames * n // 10)) // 4) and np.abs(pcm).max() > 10000
    y = pcm[:, 200:]  # past the filters' transients
    spec = np.abs(np.fft.rfft((y - y.mean(axis=1, keepdims=True)) * np.hanning(y.shape[1]), axis=1))
    assert np.argmax(spec, axis=1).tolist() == [int(round(1000.0 / 50_000.0 * y.shape[1]))] * B
    eng.set_ddc(off=True)
    invalid(S, eng.ddc_demod, raw[:, :2 * n], dd.CS8)
    eng.close()


def test_divide_and_root_are_correctly_rounded(tmp_path):
    """csrc/demod.hip's `/` and sqrtf against NumPy's float32 on 2^20 finite operand pairs: random bit patterns (every
    exponent, denormals, both signs) and, for a quarter, the detector's own shape (mn <= mx, both denormal or tiny)."""
    n = 1 << 20
    rng = np.random.default_rng(7)
    bits = rng.integers(0, 1 << 32, 2 * n, dtype=np.uint64).astype(np.uint32)
    bits = np.where((bits & 0x7F800000) == 0x7F800000, bits & 0xBFFFFFFF, bits)  # no infinity, no NaN
    xy = bits.view(np.float32).reshape(2, n).copy()
    q = n // 4
    a, b = np.abs(xy[0, :q]) * np.float32(1e-30), np.abs(xy[1, :q]) * np.float32(1e-30)
    xy[0, :q], xy[1, :q] = np.minimum(a, b), np.maximum(a, b)
    xy[1, :64], xy[0, 64:128] = 0.0, 0.0
    assert np.isfinite(xy).all() and np.any((xy != 0) & (np.abs(xy) < 1.17e-38))
    exe, fin, fout = tmp_path / "demod_math", tmp_path / "in.bin", tmp_path / "out.bin"
    xy.tofile(fin)
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "cpp", "demod_math.hip"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and f"pairs {n}" in r.stdout, r.stdout + r.stderr
    got = np.fromfile(fout, np.float32).reshape(2, n)
    with np.errstate(all="ignore"):
        want_q, want_r = xy[0] / xy[1], np.sqrt(np.abs(xy[0]))
    nan = np.isnan(want_q)  # 0 / 0 only (the products with 1e-30 underflow to 0 often): any NaN will do
    assert np.array_equal(np.isnan(got[0]), nan)
    bad = np.flatnonzero((got[0].view(np.uint32) != want_q.view(np.uint32)) & ~nan)
    assert bad.size == 0, [(xy[0, i], xy[1, i], got[0, i], want_q[i]) for i in bad[:4]]
    bad = np.flatnonzero(got[1].view(np.uint32) != want_r.view(np.uint32))
    assert bad.size == 0, [(xy[0, i], got[1, i], want_r[i]) for i in bad[:4]]
