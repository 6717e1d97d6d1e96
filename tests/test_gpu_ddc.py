"""GPU tests of the DDC stage (csrc/ddc.hip, sdrg_engine_ddc_*): the tuned, filtered, decimated CF32 channel of each
stream against the NumPy restatement in tests/ddc_cases.py fed the library's own taps and phasor tables.  Every
comparison is of the bytes of the whole output (the stage is specified operation by operation: no tolerances), `out` is
pre-filled with 0xAA between 64 guard bytes on either side (tests/stage_harness.py).

The kernel works in tiles of sdrg.ddc_tile_outputs(D, T) outputs, each staging its window of mixed samples in LDS from
aligned 16-byte loads (the ends of a window, and rows that are not 16-byte aligned, sample by sample), with the samples
before the frame taken from the history of the previous call: the shapes below put windows across every tile seam, rows
off every alignment, and the history through shifts (N < T - 1), format switches and frames of other lengths."""
import ctypes

import numpy as np
import pytest

import ddc_cases as dd
from stage_harness import FS, GUARD, engine, invalid, out_buffer, read_out, same, to_device

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def S():
    import sdrg
    return sdrg


@pytest.fixture(scope="module")
def T():
    import torch
    return torch


@pytest.fixture(scope="module")
def tab(S):
    return S.nco_tables()


class Channel:
    """An engine with the DDC set, and the restatement that follows it call by call."""

    def __init__(self, S, T, tab, n, B, fs=FS, **cfg):
        self.S, self.T, self.tab, self.B, self.fs = S, T, tab, B, fs
        self.eng = engine(S, B, n, fs)
        self.configure(**cfg)

    def configure(self, **cfg):
        self.cfg = cfg
        self.eng.set_ddc(**cfg)
        self.remodel()

    def remodel(self):
        """A fresh restatement for the configuration and sample rate in force (the engine restarted its streams)."""
        got = self.eng.ddc_config()
        assert got["nco_increment"] == dd.nco_increment(self.cfg["offset_hz"], self.fs)
        h = self.S.ddc_design(self.fs, **self.cfg)
        self.model = dd.Ddc(self.B, h, self.tab, got["nco_increment"], self.cfg["decimation"])

    def device_call(self, fmt, raw):
        """ddc_device into a 0xAA-filled buffer between guard bytes: (out [B][cap] complex64, n_out)."""
        T, eng = self.T, self.eng
        cap = eng.ddc_max_out()
        iq_t, out_t = to_device(T, raw), out_buffer(T, self.B * cap * 8)
        T.cuda.synchronize()
        n_out = eng.ddc_device(iq_t.data_ptr(), fmt, out_t.data_ptr() + GUARD)
        eng.synchronize()
        return read_out(out_t, (self.B, cap), np.complex64), n_out

    def check(self, fmt, raw, what=None):
        got, n_out = self.device_call(fmt, raw)
        want, want_n = self.model.call(fmt, raw)
        same(got, n_out, want, want_n, what)
        assert self.eng.ddc_config()["samples_consumed"] == self.model.g0
        return got, n_out

    def close(self):
        self.eng.close()


@pytest.mark.parametrize("fmt", [dd.CS8, dd.CU8, dd.CS16, dd.CF32])
def test_formats(S, T, tab, fmt):
    n, B = 4096, 6
    ch = Channel(S, T, tab, n, B, offset_hz=250_000.0, cutoff_hz=100_000.0, decimation=8, taps=63)
    for f in range(2):
        got, n_out = ch.check(fmt, dd.noise(fmt, B, n, seed=10 * fmt + f), f)
        assert n_out == 512 and np.abs(got).max() > 0.01
    ch.close()


@pytest.mark.parametrize("B", [1, 9, 17])
def test_stream_counts(S, T, tab, B):
    n = 1500
    ch = Channel(S, T, tab, n, B, offset_hz=-123_456.0, cutoff_hz=60_000.0, decimation=5, taps=31)
    for f in range(2):
        ch.check(dd.CS8, dd.noise(dd.CS8, B, n, seed=20 + f), f)
    ch.close()


@pytest.mark.parametrize("fmt", [dd.CS8, dd.CS16])
def test_odd_rows_are_misaligned(S, T, tab, fmt):
    """N = 4099: rows start 2 (CS8) or 4 (CS16) bytes further off a 16-byte boundary each."""
    n, B = 4099, 3
    ch = Channel(S, T, tab, n, B, offset_hz=250_000.0, cutoff_hz=100_000.0, decimation=8, taps=63)
    for f in range(3):
        ch.check(fmt, dd.noise(fmt, B, n, seed=30 + f), f)
    ch.close()


def test_iq_base_off_every_alignment(S, T, tab):
    """The caller's iq at 2, 6 and 14 bytes past a 16-byte boundary, and at an odd byte (no sample is then aligned)."""
    n, B, fmt = 1031, 2, dd.CS8
    ch = Channel(S, T, tab, n, B, offset_hz=1000.0, cutoff_hz=200_000.0, decimation=3, taps=15)
    cap = ch.eng.ddc_max_out()
    for shift in (2, 6, 14, 1, 3):
        raw = dd.noise(fmt, B, n, seed=40 + shift)
        buf = T.zeros((B * n * 2 + 32,), dtype=T.uint8, device="cuda:0")
        buf[shift:shift + B * n * 2] = to_device(T, raw.view(np.uint8).reshape(-1))
        out_t = out_buffer(T, B * cap * 8)
        T.cuda.synchronize()
        n_out = ch.eng.ddc_device(buf.data_ptr() + shift, fmt, out_t.data_ptr() + GUARD)
        ch.eng.synchronize()
        want, want_n = ch.model.call(fmt, raw)
        same(read_out(out_t, (B, cap), np.complex64), n_out, want, want_n, shift)
    ch.close()


@pytest.mark.parametrize("taps", [1, 3, 255, 511])
@pytest.mark.parametrize("D", [1, 2, 3, 41, 64, 512])
def test_tile_seams(S, T, tab, D, taps):
    """Two tiles and a part of a third, two calls: with T > 1 every window near a multiple of the tile size reads samples
    the neighbouring tile also stages, the first tile's the history."""
    tile = S.ddc_tile_outputs(D, taps)
    B, n = 2, (2 * tile + 3) * D + 5
    ch = Channel(S, T, tab, n, B, offset_hz=333_333.0, cutoff_hz=min(FS / 2, 0.4 * FS / D), decimation=D, taps=taps)
    for f in range(2):
        got, n_out = ch.check(dd.CS8, dd.noise(dd.CS8, B, n, seed=50 + f), (tile, f))
        assert n_out > 2 * tile
    ch.close()


def test_five_calls_are_one_stream(S, T, tab):
    n, B, fmt = 3000, 4, dd.CS16
    cfg = dict(offset_hz=-400_000.0, cutoff_hz=20_000.0, decimation=41, taps=255)
    ch = Channel(S, T, tab, n, B, **cfg)
    raw = dd.noise(fmt, B, 5 * n, seed=60)
    parts = []
    for f in range(5):
        got, n_out = ch.check(fmt, raw[:, 2 * n * f:2 * n * (f + 1)], f)
        parts.append(got[:, :n_out])
    whole, n_whole = dd.Ddc(B, ch.model.h, tab, ch.model.inc, 41).call(fmt, raw)
    assert np.concatenate(parts, axis=1).tobytes() == whole[:, :n_whole].tobytes()
    ch.close()


def test_short_frames_shift_the_history(S, T, tab):
    """N = 100 < T - 1 = 510: most of each call's new history is the old one moved down."""
    n, B = 100, 3
    ch = Channel(S, T, tab, n, B, offset_hz=50_000.0, cutoff_hz=30_000.0, decimation=7, taps=511)
    for f in range(8):
        ch.check(dd.CU8, dd.noise(dd.CU8, B, n, seed=70 + f), f)
    ch.close()


def test_calls_without_outputs_write_zeros(S, T, tab):
    """D = 512 at N = 100: four calls in five hold no multiple of 512, and still every byte of out is written."""
    n, B = 100, 2
    ch = Channel(S, T, tab, n, B, offset_hz=0.0, cutoff_hz=1000.0, decimation=512, taps=63)
    counts = []
    for f in range(12):
        got, n_out = ch.check(dd.CS8, dd.noise(dd.CS8, B, n, seed=80 + f), f)
        assert got.shape == (B, 1)
        if n_out == 0:
            assert not got.view(np.uint32).any()
        counts.append(n_out)
    assert counts == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]  # samples 0, 512 and 1024 of the stream
    ch.close()


def test_format_and_frame_length_change_between_calls(S, T, tab):
    B = 3
    ch = Channel(S, T, tab, 700, B, offset_hz=250_000.0, cutoff_hz=50_000.0, decimation=6, taps=127)
    seq = [(dd.CS8, 700), (dd.CF32, 700), (dd.CS16, 33), (dd.CU8, 1), (dd.CS8, 2050), (dd.CF32, 127), (dd.CS16, 700)]
    for i, (fmt, n) in enumerate(seq):
        if n != ch.eng.cfg.samplesPerReading:
            ch.eng.setSamplesPerReading(n)
        assert ch.eng.ddc_max_out() == -(-n // 6)
        ch.check(fmt, dd.noise(fmt, B, n, seed=90 + i), (i, fmt, n))
    assert ch.model.g0 == sum(n for _, n in seq)
    ch.close()


@pytest.mark.parametrize("offset", [0.0, -250_000.0, 999_999.0, 2_750_000.0, 0.25])
def test_phase(S, T, tab, offset):
    """inc * g passes 2^32 within a call for every offset but the smallest; a negative offset and one beyond fs wrap
    into [0, 2^32); offset 0 still multiplies by hi[0] lo[0]."""
    n, B = 5000, 2
    ch = Channel(S, T, tab, n, B, offset_hz=offset, cutoff_hz=100_000.0, decimation=4, taps=31)
    inc = ch.model.inc
    assert (inc == 0) == (offset == 0.0)
    if abs(offset) > 1:
        assert inc * (2 * n) > 2 ** 32
    for f in range(2):
        ch.check(dd.CS16, dd.noise(dd.CS16, B, n, seed=100 + f), f)
    ch.close()


def test_one_long_row(S, T, tab):
    n, B = 1 << 20, 1
    ch = Channel(S, T, tab, n, B, offset_hz=123_000.0, cutoff_hz=50_000.0, decimation=16, taps=127)
    got, n_out = ch.check(dd.CS8, dd.noise(dd.CS8, B, n, seed=110))
    assert n_out == 65536
    ch.close()


def test_many_streams_at_the_benchmark_frame(S, T, tab):
    n, B = 16384, 64
    ch = Channel(S, T, tab, n, B, offset_hz=-300_000.0, cutoff_hz=20_000.0, decimation=41, taps=255)
    got, n_out = ch.check(dd.CS8, dd.noise(dd.CS8, B, n, seed=120))
    assert n_out == 400
    ch.close()


def test_restarts(S, T, tab):
    """set_ddc, ddc_reset and a sample-rate change restart the streams; a rejected set_ddc changes nothing."""
    n, B, fmt = 900, 2, dd.CS8
    cfg = dict(offset_hz=100_000.0, cutoff_hz=80_000.0, decimation=7, taps=63)
    ch = Channel(S, T, tab, n, B, **cfg)
    ch.check(fmt, dd.noise(fmt, B, n, seed=130))
    # rejected: the old configuration, g0 and history stay
    for bad in (dict(cfg, taps=64), dict(cfg, decimation=0), dict(cfg, decimation=513), dict(cfg, taps=513),
                dict(cfg, cutoff_hz=0.0), dict(cfg, cutoff_hz=FS / 2 + 1), dict(cfg, offset_hz=float("nan")),
                dict(cfg, offset_hz=float("inf"))):
        invalid(S, ch.eng.set_ddc, **bad)
    got = ch.eng.ddc_config()
    assert {k: got[k] for k in cfg} == cfg and got["samples_consumed"] == n
    ch.check(fmt, dd.noise(fmt, B, n, seed=131), "after rejected set_ddc")
    # ddc_reset
    ch.eng.ddc_reset()
    ch.model.reset()
    assert ch.eng.ddc_config()["samples_consumed"] == 0
    ch.check(fmt, dd.noise(fmt, B, n, seed=132), "after reset")
    ch.check(fmt, dd.noise(fmt, B, n, seed=133), "second after reset")
    # the same configuration set again
    ch.configure(**cfg)
    ch.check(fmt, dd.noise(fmt, B, n, seed=134), "after set_ddc")
    ch.check(fmt, dd.noise(fmt, B, n, seed=135), "second after set_ddc")
    # a sample-rate change: restart at the next call, with the increment and taps of the new rate
    ch.eng.setSampleRate(2_400_000)
    ch.fs = 2_400_000
    ch.remodel()
    ch.check(fmt, dd.noise(fmt, B, n, seed=136), "after setSampleRate")
    ch.check(fmt, dd.noise(fmt, B, n, seed=137), "second after setSampleRate")
    ch.close()


def test_refusals_write_nothing_and_commit_nothing(S, T, tab):
    n, B, fmt = 800, 2, dd.CS16
    eng = engine(S, B, n)
    iq_t = to_device(T, dd.noise(fmt, B, n, seed=140))
    out_t = out_buffer(T, B * n * 8)
    T.cuda.synchronize()
    invalid(S, eng.ddc_device, iq_t.data_ptr(), fmt, out_t.data_ptr() + GUARD)  # before any set_ddc
    invalid(S, eng.ddc_max_out)
    invalid(S, eng.ddc_config)
    eng.close()

    cfg = dict(offset_hz=-50_000.0, cutoff_hz=900_000.0, decimation=3, taps=33)
    ch = Channel(S, T, tab, n, B, **cfg)
    ch.check(fmt, dd.noise(fmt, B, n, seed=141))
    # the rate drops so that cutoff_hz > fs / 2: the call fails, g0 and the history stay
    ch.eng.setSampleRate(1_000_000)
    invalid(S, ch.eng.ddc_device, iq_t.data_ptr(), fmt, out_t.data_ptr() + GUARD)
    invalid(S, ch.eng.ddc_device, iq_t.data_ptr(), 99, out_t.data_ptr() + GUARD)
    assert ch.eng.ddc_config()["samples_consumed"] == n
    ch.eng.setSampleRate(FS)
    ch.check(fmt, dd.noise(fmt, B, n, seed=142), "after a refused call")
    # off: refused again, and set once more it starts afresh
    ch.eng.set_ddc(off=True)
    invalid(S, ch.eng.ddc_device, iq_t.data_ptr(), fmt, out_t.data_ptr() + GUARD)
    ch.eng.synchronize()
    assert np.all(out_t.cpu().numpy() == 0xAA), "a refused call wrote to out"
    ch.configure(**cfg)
    ch.check(fmt, dd.noise(fmt, B, n, seed=143), "after off and on")
    L = S.load()
    n_out = ctypes.c_int32()
    assert L.sdrg_engine_ddc_device(ch.eng._h, None, fmt, out_t.data_ptr() + GUARD, ctypes.byref(n_out)) == -1
    assert L.sdrg_engine_ddc_device(ch.eng._h, iq_t.data_ptr(), fmt, out_t.data_ptr() + GUARD, None) == -1
    ch.check(fmt, dd.noise(fmt, B, n, seed=144), "after null arguments")
    ch.close()


def test_host_path_equals_device_path(S, T, tab):
    n, B, fmt = 2500, 5, dd.CU8
    cfg = dict(offset_hz=77_000.0, cutoff_hz=40_000.0, decimation=9, taps=95)
    dev = Channel(S, T, tab, n, B, **cfg)
    host = engine(S, B, n)
    host.set_ddc(**cfg)
    for f in range(3):
        raw = dd.noise(fmt, B, n, seed=150 + f)
        got, n_out = dev.check(fmt, raw, f)
        h = host.ddc(raw, fmt)
        assert h.dtype == np.complex64 and h.shape == (B, n_out) and h.tobytes() == got[:, :n_out].tobytes()
    dev.close()
    host.close()


def test_wait_outputs_orders_a_consumer_stream(S, T, tab):
    n, B, fmt = 16384, 16, dd.CS8
    ch = Channel(S, T, tab, n, B, offset_hz=10_000.0, cutoff_hz=20_000.0, decimation=41, taps=255)
    cap = ch.eng.ddc_max_out()
    consumer = T.cuda.Stream("cuda:0")
    out_t = out_buffer(T, B * cap * 8)
    copy = T.zeros_like(out_t)
    T.cuda.synchronize()
    for f in range(3):
        raw = dd.noise(fmt, B, n, seed=160 + f)
        iq_t = to_device(T, raw)
        T.cuda.synchronize()
        n_out = ch.eng.ddc_device(iq_t.data_ptr(), fmt, out_t.data_ptr() + GUARD)
        ch.eng.wait_outputs(consumer.cuda_stream)
        with T.cuda.stream(consumer):
            copy.copy_(out_t)
        consumer.synchronize()
        want, want_n = ch.model.call(fmt, raw)
        same(read_out(copy, (B, cap), np.complex64), n_out, want, want_n, f)
    ch.close()


@pytest.mark.parametrize("mode", ["OFF", "ON", "INPUTS_READY", "ON|STATS_ASYNC", "INPUTS_READY|STATS_ASYNC"])
def test_process_device_between_ddc_calls(S, T, tab, mode):
    """ddc, process_device, ddc in every pipelining mode: the ddc bytes are the restatement's, and the spectra, records
    and PCM are those of an engine that never configured the DDC."""
    n, B, fmt = 16384, 4, dd.CS8
    bits = 0
    for name in mode.split("|"):
        bits |= getattr(S, "PIPELINE_" + name)
    stages = S.STAGE_SPECTRUM | S.STAGE_STATS | S.STAGE_SSB
    raws = [dd.tone(fmt, B, n, 0.01 + 0.001 * f, amp=0.4) for f in range(3)]

    def process(eng, f):
        iq_t = to_device(T, raws[f])
        spec = T.zeros((B, n), dtype=T.float32, device="cuda:0")
        rec = T.zeros((B * S.RECORD_DTYPE.itemsize,), dtype=T.uint8, device="cuda:0")
        pcm = T.zeros((B, max(eng.pcm_len, 1)), dtype=T.int16, device="cuda:0")
        T.cuda.synchronize()
        eng.process_device(iq_t.data_ptr(), fmt, stages, spec.data_ptr(), rec.data_ptr(), pcm.data_ptr(), 1000 + f)
        return iq_t, spec, rec, pcm

    ch = Channel(S, T, tab, n, B, offset_hz=20_000.0, cutoff_hz=20_000.0, decimation=41, taps=255)
    ch.eng.set_pipelining(bits)
    plain = engine(S, B, n)
    plain.set_pipelining(bits)
    cap = ch.eng.ddc_max_out()
    outs, iqs, held = [], [], []
    for f in range(3):
        iq_t, out_t = to_device(T, raws[f]), out_buffer(T, B * cap * 8)
        T.cuda.synchronize()
        n_out = ch.eng.ddc_device(iq_t.data_ptr(), fmt, out_t.data_ptr() + GUARD)
        outs.append((out_t, n_out))
        iqs.append(iq_t)
        if f < 2:
            held.append((process(ch.eng, f), process(plain, f)))
    ch.eng.synchronize()
    plain.synchronize()
    for f, (out_t, n_out) in enumerate(outs):
        want, want_n = ch.model.call(fmt, raws[f])
        same(read_out(out_t, (B, cap), np.complex64), n_out, want, want_n, (mode, f))
    for f, (a, b) in enumerate(held):
        for x, y, name in zip(a[1:], b[1:], ("spectra", "records", "pcm")):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), (mode, f, name)
    assert held[0][0][1].cpu().numpy().max() > 0
    ch.close()
    plain.close()


def test_zoom_fft(S, T, tab):
    """fs = 2 MHz, N = 16384, D = 16, T = 255, CS16: the channel's 1024 outputs go on the device, as CF32, into a second
    engine of N = 1024 at fs = 125000.  A tone 25 bins of that spectrum above the channel's centre peaks at bin
    512 + 25 = 537, and the spectrum's bytes are those of the same engine fed the restatement's output."""
    n, B, D, fmt = 16384, 2, 16, dd.CS16
    offset = 300_000.0
    f_tone = offset + 25 * (125000 / 1024)
    ch = Channel(S, T, tab, n, B, offset_hz=offset, cutoff_hz=50_000.0, decimation=D, taps=255)
    zoom = engine(S, B, 1024, fs=125000)
    cap = ch.eng.ddc_max_out()
    assert cap == 1024
    spec = T.zeros((B, 1024), dtype=T.float32, device="cuda:0")
    out_t = out_buffer(T, B * cap * 8)
    for f in range(2):  # the second frame is past the filter's transient
        raw = dd.tone(fmt, B, 2 * n, f_tone / FS, amp=0.5)[:, 2 * n * f:2 * n * (f + 1)]
        iq_t = to_device(T, raw)
        T.cuda.synchronize()
        n_out = ch.eng.ddc_device(iq_t.data_ptr(), fmt, out_t.data_ptr() + GUARD)
        assert n_out == 1024
        ch.eng.synchronize()
        zoom.process_device(out_t.data_ptr() + GUARD, S.CF32, S.STAGE_SPECTRUM, spec.data_ptr(), None, None, 1000 + f)
        zoom.synchronize()
        want, _ = ch.model.call(fmt, raw)
    got_spec = spec.cpu().numpy()
    assert read_out(out_t, (B, cap), np.complex64).tobytes() == want.tobytes()
    assert np.argmax(got_spec, axis=1).tolist() == [537] * B
    ref = engine(S, B, 1024, fs=125000)
    ref_spec, _, _ = ref.process(want.view(np.float32).reshape(B, -1), fmt=S.CF32, stages=S.STAGE_SPECTRUM, now_ms=1001)
    assert got_spec.tobytes() == ref_spec.tobytes()
    for e in (ch, zoom, ref):
        e.close()
