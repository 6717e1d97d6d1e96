"""GPU tests of the DDC bank stage (csrc/bank.hip, sdrg_engine_bank_*): C channels at their own offsets from each stream,
against the NumPy restatement in tests/bank_cases.py fed the library's own taps and phasor tables.  Every comparison is of
the bytes of the whole output (the stage is specified operation by operation: no tolerances), `out` is pre-filled with
0xAA between 64 guard bytes on either side (tests/stage_harness.py).

The kernel works in tiles of outputs and groups of channels (sdrg.bank_geometry): a workgroup stages its window of
unmixed samples once, then mixes and filters it for each channel of its group.  The shapes below put windows across every
tile seam, channel counts across group seams (a last group in part, of one channel), rows off every alignment, and the
unmixed history through shifts (N < T - 1), format switches, retunes and frames of other lengths."""
import ctypes

import numpy as np
import pytest

import bank_cases as bk
import ddc_cases as dd
import demod_cases as dm
import squelch_cases as sq
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


def spread(B, C, seed=0):
    """B x C distinct offsets over (-fs / 2, fs / 2), none on a round figure."""
    rng = np.random.default_rng(1000 + seed)
    return np.round((rng.random((B, C)) - 0.5) * FS, 1) + 0.3


class Rig:
    """An engine with the bank set, and the restatement that follows it call by call."""

    def __init__(self, S, T, tab, n, B, offsets, fs=FS, **cfg):
        self.S, self.T, self.tab, self.B, self.fs = S, T, tab, B, fs
        self.eng = engine(S, B, n, fs)
        self.configure(offsets, **cfg)

    def configure(self, offsets, **cfg):
        self.cfg, self.offsets = cfg, np.asarray(offsets, np.float64)
        self.C = self.offsets.shape[1]
        self.eng.set_bank(offsets_hz=self.offsets, **cfg)
        self.remodel()

    def remodel(self):
        """A fresh restatement for the configuration, offsets and sample rate in force (the engine restarted)."""
        got = self.eng.bank_config()
        assert {k: got[k] for k in self.cfg} == self.cfg and got["channels"] == self.C
        h = self.S.ddc_design(self.fs, cutoff_hz=self.cfg["cutoff_hz"], decimation=self.cfg["decimation"],
                              taps=self.cfg["taps"])
        self.model = bk.Bank(self.B, h, self.tab, self.increments(), self.cfg["decimation"])

    def increments(self):
        o, inc = self.eng.bank_offsets()
        want = bk.increments(self.offsets, self.fs)
        assert o.tobytes() == self.offsets.tobytes() and inc.tobytes() == want.tobytes()
        return want

    def retune(self, offsets):
        self.offsets = np.asarray(offsets, np.float64)
        self.eng.bank_retune(self.offsets)
        self.model.retune(self.increments())

    def launch(self, fmt, raw):
        """bank_device into a 0xAA-filled buffer between guard bytes, not waited for: (iq, out, n_out)."""
        cap = self.eng.bank_max_out()
        iq_t, out_t = to_device(self.T, raw), out_buffer(self.T, self.B * self.C * cap * 8)
        self.T.cuda.synchronize()
        return iq_t, out_t, self.eng.bank_device(iq_t.data_ptr(), fmt, out_t.data_ptr() + GUARD)

    def device_call(self, fmt, raw):
        """(out [B][C][cap] complex64, n_out)"""
        _, out_t, n_out = self.launch(fmt, raw)
        self.eng.synchronize()
        return read_out(out_t, (self.B, self.C, self.eng.bank_max_out()), np.complex64), n_out

    def check(self, fmt, raw, what=None):
        got, n_out = self.device_call(fmt, raw)
        want, want_n = self.model.call(fmt, raw)
        same(got, n_out, want, want_n, what)
        assert self.eng.bank_config()["samples_consumed"] == self.model.g0
        return got, n_out

    def close(self):
        self.eng.close()


@pytest.mark.parametrize("fmt", [dd.CS8, dd.CU8, dd.CS16, dd.CF32])
def test_formats(S, T, tab, fmt):
    n, B, C = 4096, 3, 5
    r = Rig(S, T, tab, n, B, spread(B, C, fmt), cutoff_hz=100_000.0, decimation=8, taps=63)
    for f in range(2):
        got, n_out = r.check(fmt, dd.noise(fmt, B, n, seed=10 * fmt + f), f)
        assert n_out == 512 and np.abs(got).max() > 0.01
    r.close()


# Channel counts per stream count: 1, 2, 5 and 64 in groups of one channel; then, since the group size follows
# n_streams * C, counts at which sdrg.bank_geometry gives groups of 2 and of 8 with a whole last group, a last group of one
# channel (group + 1 and 2 group + 1 modulo the group) and a last group in part.
COUNTS = {1: [(1, 1, 0), (2, 1, 0), (5, 1, 0), (64, 1, 0), (512, 2, 0), (513, 2, 1), (2048, 8, 0), (2049, 8, 1),
              (2053, 8, 5)],
          3: [(1, 1, 0), (2, 1, 0), (5, 1, 0), (64, 1, 0), (172, 2, 0), (173, 2, 1), (688, 8, 0), (689, 8, 1),
              (683, 8, 3)]}


@pytest.mark.parametrize("B,C,group,rest", [(B, *c) for B in COUNTS for c in COUNTS[B]])
def test_channel_counts_across_group_seams(S, T, tab, B, C, group, rest):
    n, D, taps = 201, 2, 3
    assert S.bank_geometry(D, taps, C, B)[1] == group and C % group == rest
    r = Rig(S, T, tab, n, B, spread(B, C, C), cutoff_hz=300_000.0, decimation=D, taps=taps)
    for f in range(2):
        r.check(dd.CS8, dd.noise(dd.CS8, B, n, seed=20 + f), f)
    r.close()


@pytest.mark.parametrize("D,taps", [(1, 1), (2, 3), (3, 255), (41, 255), (64, 511), (512, 255)])
def test_tile_seams(S, T, tab, D, taps):
    """Two tiles and a part of a third, two calls: with T > 1 every window near a multiple of the tile size reads samples
    the neighbouring tile also stages, the first tile's the history.  N passes 4096 at D = 512 only."""
    B, C = 2, 3
    tile, _ = S.bank_geometry(D, taps, C, B)
    n = (2 * tile + 3) * D + 5
    r = Rig(S, T, tab, n, B, spread(B, C, D), cutoff_hz=min(FS / 2, 0.4 * FS / D), decimation=D, taps=taps)
    for f in range(2):
        got, n_out = r.check(dd.CS8, dd.noise(dd.CS8, B, n, seed=50 + f), (tile, f))
        assert n_out > 2 * tile
    r.close()


def test_iq_base_off_every_alignment(S, T, tab):
    """The caller's iq at 2, 6 and 14 bytes past a 16-byte boundary, and at odd bytes (no sample is then aligned)."""
    n, B, C, fmt = 1031, 2, 3, dd.CS8
    r = Rig(S, T, tab, n, B, spread(B, C, 1), cutoff_hz=200_000.0, decimation=3, taps=15)
    cap = r.eng.bank_max_out()
    for shift in (2, 6, 14, 1, 3):
        raw = dd.noise(fmt, B, n, seed=40 + shift)
        buf = T.zeros((B * n * 2 + 32,), dtype=T.uint8, device="cuda:0")
        buf[shift:shift + B * n * 2] = to_device(T, raw.view(np.uint8).reshape(-1))
        out_t = out_buffer(T, B * C * cap * 8)
        T.cuda.synchronize()
        n_out = r.eng.bank_device(buf.data_ptr() + shift, fmt, out_t.data_ptr() + GUARD)
        r.eng.synchronize()
        want, want_n = r.model.call(fmt, raw)
        same(read_out(out_t, (B, C, cap), np.complex64), n_out, want, want_n, shift)
    r.close()


@pytest.mark.parametrize("fmt", [dd.CS8, dd.CS16])
def test_odd_rows_are_misaligned(S, T, tab, fmt):
    """N = 1027: rows start 2 (CS8) or 4 (CS16) bytes further off a 16-byte boundary each."""
    n, B, C = 1027, 3, 2
    r = Rig(S, T, tab, n, B, spread(B, C, 2), cutoff_hz=100_000.0, decimation=8, taps=63)
    for f in range(3):
        r.check(fmt, dd.noise(fmt, B, n, seed=30 + f), f)
    r.close()


def test_five_calls_are_one_stream(S, T, tab):
    n, B, C, fmt = 3000, 2, 3, dd.CS16
    r = Rig(S, T, tab, n, B, spread(B, C, 3), cutoff_hz=20_000.0, decimation=41, taps=255)
    raw = dd.noise(fmt, B, 5 * n, seed=60)
    parts = []
    for f in range(5):
        got, n_out = r.check(fmt, raw[:, 2 * n * f:2 * n * (f + 1)], f)
        parts.append(got[:, :, :n_out])
    whole, n_whole = bk.Bank(B, r.model.h, tab, r.model.incs, 41).call(fmt, raw)
    assert np.concatenate(parts, axis=2).tobytes() == whole[:, :, :n_whole].tobytes()
    r.close()


def test_short_frames_shift_the_history(S, T, tab):
    """N = 100 < T - 1 = 510: most of each call's new history is the old one moved down."""
    n, B, C = 100, 3, 2
    r = Rig(S, T, tab, n, B, spread(B, C, 4), cutoff_hz=30_000.0, decimation=7, taps=511)
    for f in range(8):
        r.check(dd.CU8, dd.noise(dd.CU8, B, n, seed=70 + f), f)
    r.close()


def test_calls_without_outputs_write_zeros(S, T, tab):
    """D = 512 at N = 100: four calls in five hold no multiple of 512, and still every byte of out is written."""
    n, B, C = 100, 2, 3
    r = Rig(S, T, tab, n, B, spread(B, C, 5), cutoff_hz=1000.0, decimation=512, taps=63)
    counts = []
    for f in range(12):
        got, n_out = r.check(dd.CS8, dd.noise(dd.CS8, B, n, seed=80 + f), f)
        assert got.shape == (B, C, 1)
        if n_out == 0:
            assert not got.view(np.uint32).any()
        counts.append(n_out)
    assert counts == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]  # samples 0, 512 and 1024 of the stream
    r.close()


def test_format_and_frame_length_change_between_calls(S, T, tab):
    B, C = 3, 2
    r = Rig(S, T, tab, 700, B, spread(B, C, 6), cutoff_hz=50_000.0, decimation=6, taps=127)
    seq = [(dd.CS8, 700), (dd.CF32, 700), (dd.CS16, 33), (dd.CU8, 1), (dd.CS8, 2050), (dd.CF32, 127), (dd.CS16, 700)]
    for i, (fmt, n) in enumerate(seq):
        if n != r.eng.cfg.samplesPerReading:
            r.eng.setSamplesPerReading(n)
        assert r.eng.bank_max_out() == -(-n // 6)
        r.check(fmt, dd.noise(fmt, B, n, seed=90 + i), (i, fmt, n))
    assert r.model.g0 == sum(n for _, n in seq)
    r.close()


def test_offsets(S, T, tab):
    """Offset 0 (still multiplied by hi[0] lo[0]), a negative one and one beyond fs (both wrap into [0, 2^32)), one beyond
    fs / 2, and 0.25 Hz; inc * g passes 2^32 within a call for all but the first and last.  Channels 1 and 5 share an
    offset and so their rows; the two streams carry the same input at different offsets but for channel 0."""
    n, B = 5000, 2
    offsets = np.array([[0.0, -250_000.0, 999_999.0, 2_750_000.0, 0.25, -250_000.0],
                        [0.0, 250_000.0, 1_200_000.0, -2_750_000.0, -0.25, 17.0]])
    r = Rig(S, T, tab, n, B, offsets, cutoff_hz=100_000.0, decimation=4, taps=31)
    incs = r.model.incs
    assert incs[0, 0] == 0 and incs[0, 1] == incs[0, 5] and all(int(i) * 2 * n > 2 ** 32 for i in incs[0, 1:4])
    for f in range(2):
        one = dd.noise(dd.CS16, 1, n, seed=100 + f)
        got, n_out = r.check(dd.CS16, np.concatenate([one, one]), f)
        assert got[0, 1].tobytes() == got[0, 5].tobytes() and got[0, 0].tobytes() == got[1, 0].tobytes()
        assert all(got[0, c].tobytes() != got[1, c].tobytes() for c in range(1, 6))
    r.close()


def test_largest_channel_count(S, T, tab):
    n, B, C = 256, 1, 4096
    assert C == S.BANK_MAX_CHANNELS
    r = Rig(S, T, tab, n, B, spread(B, C, 7), cutoff_hz=100_000.0, decimation=8, taps=31)
    for f in range(2):
        got, n_out = r.check(dd.CS8, dd.noise(dd.CS8, B, n, seed=110 + f), f)
        assert n_out == 32
    eng = engine(S, B, n)
    invalid(S, eng.set_bank, offsets_hz=np.zeros((B, C + 1)), cutoff_hz=100_000.0, decimation=8, taps=31)
    eng.close()
    r.close()


def test_row_limit(S, T, tab):
    """n_streams * C = 65535 = 17 * 3855 rows are accepted (65535 = 3 * 5 * 17 * 257 has no other split with C <= 4096 and
    fewer streams); 65536 = 16 * 4096 are refused.  257 distinct offsets, so the rows of a group and of a stream differ."""
    n, B, C = 64, 17, 3855
    offsets = np.resize(spread(1, 257, 8), (B, C))
    r = Rig(S, T, tab, n, B, offsets, cutoff_hz=100_000.0, decimation=8, taps=3)
    for f in range(2):
        got, n_out = r.check(dd.CS8, dd.noise(dd.CS8, B, n, seed=120 + f), f)
        assert n_out == 8
    r.close()
    eng = engine(S, 16, n)
    invalid(S, eng.set_bank, offsets_hz=np.zeros((16, 4096)), cutoff_hz=100_000.0, decimation=8, taps=3)
    invalid(S, eng.bank_config)
    eng.close()


def test_retune_between_calls_and_back(S, T, tab):
    n, B, C, fmt = 900, 2, 3, dd.CS8
    a, b = spread(B, C, 9), spread(B, C, 10)
    b[1, 0] = a[1, 0]  # a channel that stays
    r = Rig(S, T, tab, n, B, a, cutoff_hz=60_000.0, decimation=6, taps=127)
    fresh_b = Rig(S, T, tab, n, B, b, cutoff_hz=60_000.0, decimation=6, taps=127)
    for f in range(6):
        if f == 2:
            r.retune(b)
        if f == 4:
            r.retune(a)
        raw = dd.noise(fmt, B, n, seed=130 + f)
        got, _ = r.check(fmt, raw, f)
        other, _ = fresh_b.check(fmt, raw, ("fresh", f))
        assert (got.tobytes() == other.tobytes()) == (f in (2, 3)), f  # the new offsets as if since the stream's start
        assert got[1, 0].tobytes() == other[1, 0].tobytes()
        assert r.eng.bank_config()["samples_consumed"] == (f + 1) * n  # a retune restarts nothing
    # refused retunes change nothing
    bad = a.copy()
    bad[0, 1] = np.nan
    invalid(S, r.eng.bank_retune, bad)
    assert S.load().sdrg_engine_bank_retune(r.eng._h, None) == -1
    r.increments()
    r.check(fmt, dd.noise(fmt, B, n, seed=137), "after refused retunes")
    fresh_b.close()
    r.close()


def test_retune_right_after_a_call_does_not_disturb_it(S, T, tab):
    """Three calls with a retune issued after each and nothing waited for in between: each call's rows are those of the
    offsets in force when it was issued."""
    n, B, C, fmt = 16384, 4, 64, dd.CS8
    sets = [spread(B, C, 11 + i) for i in range(4)]
    r = Rig(S, T, tab, n, B, sets[0], cutoff_hz=20_000.0, decimation=41, taps=255)
    held, wants = [], []
    raws = [dd.noise(fmt, B, n, seed=140 + f) for f in range(3)]
    for f in range(3):
        held.append(r.launch(fmt, raws[f]))
        wants.append(r.model.call(fmt, raws[f]))
        r.retune(sets[f + 1])
    r.eng.synchronize()
    cap = r.eng.bank_max_out()
    for f in range(3):
        same(read_out(held[f][1], (B, C, cap), np.complex64), held[f][2], *wants[f], f)
    r.close()


def test_restarts(S, T, tab):
    """set_bank, bank_reset and a sample-rate change restart the streams; a rejected set_bank changes nothing."""
    n, B, C, fmt = 900, 2, 3, dd.CS8
    offsets = spread(B, C, 15)
    cfg = dict(cutoff_hz=80_000.0, decimation=7, taps=63)
    r = Rig(S, T, tab, n, B, offsets, **cfg)
    r.check(fmt, dd.noise(fmt, B, n, seed=150))
    nan = offsets.copy()
    nan[1, 2] = np.inf
    for bad in (dict(cfg, taps=64), dict(cfg, decimation=0), dict(cfg, decimation=513), dict(cfg, taps=513),
                dict(cfg, cutoff_hz=0.0), dict(cfg, cutoff_hz=FS / 2 + 1)):
        invalid(S, r.eng.set_bank, offsets_hz=offsets, **bad)
    invalid(S, r.eng.set_bank, offsets_hz=nan, **cfg)
    invalid(S, r.eng.set_bank, offsets_hz=np.zeros((B, 0)), **cfg)
    c = S.BankConfig(80_000.0, 7, 63, C)
    assert S.load().sdrg_engine_set_bank(r.eng._h, ctypes.byref(c), None) == -1
    got = r.eng.bank_config()
    assert {k: got[k] for k in cfg} == cfg and got["samples_consumed"] == n
    r.increments()
    r.check(fmt, dd.noise(fmt, B, n, seed=151), "after rejected set_bank")
    r.eng.bank_reset()
    r.model.reset()
    assert r.eng.bank_config()["samples_consumed"] == 0
    r.check(fmt, dd.noise(fmt, B, n, seed=152), "after reset")
    r.check(fmt, dd.noise(fmt, B, n, seed=153), "second after reset")
    r.configure(spread(B, 4, 16), **cfg)  # another channel count too
    r.check(fmt, dd.noise(fmt, B, n, seed=154), "after set_bank")
    r.check(fmt, dd.noise(fmt, B, n, seed=155), "second after set_bank")
    r.eng.setSampleRate(2_400_000)  # restart at the next call, with the increments and taps of the new rate
    r.fs = 2_400_000
    r.remodel()
    r.check(fmt, dd.noise(fmt, B, n, seed=156), "after setSampleRate")
    r.check(fmt, dd.noise(fmt, B, n, seed=157), "second after setSampleRate")
    r.close()


def test_refusals_write_nothing_and_commit_nothing(S, T, tab):
    n, B, C, fmt = 800, 2, 3, dd.CS16
    eng = engine(S, B, n)
    iq_t = to_device(T, dd.noise(fmt, B, n, seed=160))
    out_t = out_buffer(T, B * C * n * 8)
    T.cuda.synchronize()
    invalid(S, eng.bank_device, iq_t.data_ptr(), fmt, out_t.data_ptr() + GUARD)  # before any set_bank
    invalid(S, eng.bank_max_out)
    invalid(S, eng.bank_config)
    invalid(S, eng.bank_offsets)
    invalid(S, eng.bank_retune, np.zeros((B, C)))
    eng.close()

    offsets = spread(B, C, 17)
    cfg = dict(cutoff_hz=900_000.0, decimation=3, taps=33)
    r = Rig(S, T, tab, n, B, offsets, **cfg)
    r.check(fmt, dd.noise(fmt, B, n, seed=161))
    # the rate drops so that cutoff_hz > fs / 2: the call fails, g0 and the history stay
    r.eng.setSampleRate(1_000_000)
    invalid(S, r.eng.bank_device, iq_t.data_ptr(), fmt, out_t.data_ptr() + GUARD)
    invalid(S, r.eng.bank_device, iq_t.data_ptr(), 99, out_t.data_ptr() + GUARD)
    assert r.eng.bank_config()["samples_consumed"] == n
    r.eng.setSampleRate(FS)
    r.check(fmt, dd.noise(fmt, B, n, seed=162), "after a refused call")
    r.eng.set_bank(off=True)
    invalid(S, r.eng.bank_device, iq_t.data_ptr(), fmt, out_t.data_ptr() + GUARD)
    invalid(S, r.eng.bank_retune, offsets)
    r.eng.synchronize()
    assert np.all(out_t.cpu().numpy() == 0xAA), "a refused call wrote to out"
    r.configure(offsets, **cfg)
    r.check(fmt, dd.noise(fmt, B, n, seed=163), "after off and on")
    L = S.load()
    n_out = ctypes.c_int32()
    assert L.sdrg_engine_bank_device(r.eng._h, None, fmt, out_t.data_ptr() + GUARD, ctypes.byref(n_out)) == -1
    assert L.sdrg_engine_bank_device(r.eng._h, iq_t.data_ptr(), fmt, None, ctypes.byref(n_out)) == -1
    assert L.sdrg_engine_bank_device(r.eng._h, iq_t.data_ptr(), fmt, out_t.data_ptr() + GUARD, None) == -1
    r.check(fmt, dd.noise(fmt, B, n, seed=164), "after null arguments")
    assert np.all(out_t.cpu().numpy() == 0xAA)
    r.close()


def test_host_path_equals_device_path(S, T, tab):
    n, B, C, fmt = 2500, 3, 5, dd.CU8
    offsets = spread(B, C, 18)
    cfg = dict(cutoff_hz=40_000.0, decimation=9, taps=95)
    dev = Rig(S, T, tab, n, B, offsets, **cfg)
    host = engine(S, B, n)
    host.set_bank(offsets_hz=offsets, **cfg)
    for f in range(3):
        if f == 2:
            dev.retune(spread(B, C, 19))
            host.bank_retune(dev.offsets)
        raw = dd.noise(fmt, B, n, seed=170 + f)
        got, n_out = dev.check(fmt, raw, f)
        h = host.bank(raw, fmt)
        assert h.dtype == np.complex64 and h.shape == (B, C, n_out) and h.tobytes() == got[:, :, :n_out].tobytes()
    dev.close()
    host.close()


def test_wait_outputs_orders_a_consumer_stream(S, T, tab):
    n, B, C, fmt = 16384, 4, 16, dd.CS8
    r = Rig(S, T, tab, n, B, spread(B, C, 20), cutoff_hz=20_000.0, decimation=41, taps=255)
    cap = r.eng.bank_max_out()
    consumer = T.cuda.Stream("cuda:0")
    out_t = out_buffer(T, B * C * cap * 8)
    copy = T.zeros_like(out_t)
    T.cuda.synchronize()
    for f in range(3):
        raw = dd.noise(fmt, B, n, seed=180 + f)
        iq_t = to_device(T, raw)
        T.cuda.synchronize()
        n_out = r.eng.bank_device(iq_t.data_ptr(), fmt, out_t.data_ptr() + GUARD)
        r.eng.wait_outputs(consumer.cuda_stream)
        with T.cuda.stream(consumer):
            copy.copy_(out_t)
        consumer.synchronize()
        want, want_n = r.model.call(fmt, raw)
        same(read_out(copy, (B, C, cap), np.complex64), n_out, want, want_n, f)
    r.close()


def test_process_and_ddc_between_bank_calls(S, T, tab):
    """bank, process_device, ddc_device, bank ...: the bank's bytes are the restatement's, and the spectra, records, PCM
    and DDC rows are those of an engine that never configured the bank."""
    n, B, C, fmt = 16384, 2, 3, dd.CS8
    stages = S.STAGE_SPECTRUM | S.STAGE_STATS | S.STAGE_SSB
    ddc_cfg = dict(offset_hz=20_000.0, cutoff_hz=20_000.0, decimation=41, taps=255)
    raws = [dd.tone(fmt, B, n, 0.01 + 0.001 * f, amp=0.4) for f in range(3)]
    r = Rig(S, T, tab, n, B, spread(B, C, 21), cutoff_hz=20_000.0, decimation=41, taps=255)
    plain = engine(S, B, n)
    for e in (r.eng, plain):
        e.set_ddc(**ddc_cfg)
    cap = r.eng.ddc_max_out()

    def others(eng, f):
        iq_t = to_device(T, raws[f])
        spec = T.zeros((B, n), dtype=T.float32, device="cuda:0")
        rec = T.zeros((B * S.RECORD_DTYPE.itemsize,), dtype=T.uint8, device="cuda:0")
        pcm = T.zeros((B, max(eng.pcm_len, 1)), dtype=T.int16, device="cuda:0")
        chan = out_buffer(T, B * cap * 8)
        T.cuda.synchronize()
        eng.process_device(iq_t.data_ptr(), fmt, stages, spec.data_ptr(), rec.data_ptr(), pcm.data_ptr(), 1000 + f)
        eng.ddc_device(iq_t.data_ptr(), fmt, chan.data_ptr() + GUARD)
        return iq_t, spec, rec, pcm, chan

    outs, held = [], []
    for f in range(3):
        outs.append(r.launch(fmt, raws[f]))
        if f < 2:
            held.append((others(r.eng, f), others(plain, f)))
    r.eng.synchronize()
    plain.synchronize()
    for f, (_, out_t, n_out) in enumerate(outs):
        want, want_n = r.model.call(fmt, raws[f])
        same(read_out(out_t, (B, C, r.eng.bank_max_out()), np.complex64), n_out, want, want_n, f)
    for f, (a, b) in enumerate(held):
        for x, y, name in zip(a[1:], b[1:], ("spectra", "records", "pcm", "ddc")):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), (f, name)
    assert held[0][0][1].cpu().numpy().max() > 0 and np.abs(read_out(held[1][0][4], (B, cap), np.complex64)).max() > 0
    r.close()
    plain.close()


@pytest.mark.parametrize("offset", [0.0, -312_500.0])
def test_one_channel_is_the_ddc(S, T, tab, offset):
    """C = 1: bank_device and another engine's ddc_device give the same bytes, call after call."""
    n, B, fmt = 3000, 3, dd.CS16
    cfg = dict(cutoff_hz=30_000.0, decimation=12, taps=191)
    r = Rig(S, T, tab, n, B, np.full((B, 1), offset), **cfg)
    ddc = engine(S, B, n)
    ddc.set_ddc(offset_hz=offset, **cfg)
    cap = ddc.ddc_max_out()
    assert cap == r.eng.bank_max_out()
    for f in range(3):
        raw = dd.noise(fmt, B, n, seed=190 + f)
        got, n_out = r.check(fmt, raw, f)
        iq_t, out_t = to_device(T, raw), out_buffer(T, B * cap * 8)
        T.cuda.synchronize()
        assert ddc.ddc_device(iq_t.data_ptr(), fmt, out_t.data_ptr() + GUARD) == n_out
        ddc.synchronize()
        assert read_out(out_t, (B, cap), np.complex64).tobytes() == got.tobytes(), f
    ddc.close()
    r.close()


def test_hand_off_to_a_second_engine(S, T, tab):
    """2 streams x 3 channels, CS16: stream 0 carries FM signals at the offsets of its channels 0 and 1, stream 1 one at
    the offset of its channel 2; the other three channels are empty.  `out` goes on the device, as it lies, to an engine
    of 6 streams: demod_device gives the bytes of demod_cases applied to the restatement's rows, and squelch_device, in
    place on the same rows, those of squelch_cases, with the three occupied rows open in the records."""
    n, B, C, D, fmt = 4096, 2, 3, 16, dd.CS16
    offsets = np.array([[300_000.0, -450_000.0, 700_000.0], [-650_000.0, 120_000.0, 700_000.0]])
    occupied = [(0, 0), (0, 1), (1, 2)]
    t = np.arange(2 * n, dtype=np.float64)
    z = np.zeros((B, 2 * n), np.complex128)
    for i, (b, c) in enumerate(occupied):
        phi = 2.0 * np.pi * offsets[b, c] * t / FS + 2.0 * np.sin(2.0 * np.pi * (1000.0 + 500.0 * i) * t / FS)
        z[b] += 0.3 * np.exp(1j * phi)
    raws = np.empty((B, 4 * n), np.int16)
    raws[:, 0::2], raws[:, 1::2] = np.round(z.real * 32768.0), np.round(z.imag * 32768.0)
    r = Rig(S, T, tab, n, B, offsets, cutoff_hz=50_000.0, decimation=D, taps=255)
    cap = r.eng.bank_max_out()
    assert cap == 256
    second = engine(S, B * C, cap, fs=FS // D)
    dcfg = dict(mode=dm.FM, channel_rate_hz=FS / D, deviation_hz=5_000.0, dc_cutoff_hz=0.0, deemphasis_us=0.0,
                audio_decimation=4, audio_taps=31, audio_cutoff_hz=8_000.0, gain=1.0, out_format=dm.OUT_F32, max_in=cap)
    second.set_demod(**dcfg)
    d = second.demod_config()
    demod = dm.Demod(B * C, d["mode"], d["kf"], d["alpha"], d["a"], d["taps"], 4, d["gain"], d["out_format"], cap)
    scfg = dict(open_db=-30.0, close_db=-40.0, tau_blocks=0.0, block=64, hang_blocks=1, max_in=cap)
    second.set_squelch(**scfg)
    s = second.squelch_config()
    gate = sq.Squelch(B * C, s["open_thr"], s["close_thr"], s["beta"], 64, 1)
    acap = second.demod_max_out()
    for f in range(2):
        raw = raws[:, 2 * n * f:2 * n * (f + 1)]
        _, out_t, n_out = r.launch(fmt, raw)
        audio_t, rec_t = out_buffer(T, B * C * acap * 4), out_buffer(T, B * C * 16)
        r.eng.synchronize()
        rows = out_t.data_ptr() + GUARD
        assert second.demod_device(rows, n_out, audio_t.data_ptr() + GUARD) == acap
        assert second.squelch_device(rows, cap, n_out, rows, rec_t.data_ptr() + GUARD) == cap // 64
        second.synchronize()
        want, want_n = r.model.call(fmt, raw)
        assert want_n == n_out == cap
        chan = want.reshape(B * C, cap)
        want_audio, _ = demod.call(chan)
        assert read_out(audio_t, (B * C, acap), np.float32).tobytes() == want_audio.tobytes(), f
        want_rows, want_rec, _ = gate.call(chan, in_stride=cap)
        assert read_out(out_t, (B * C, cap), np.complex64).tobytes() == want_rows.tobytes(), f
        rec = read_out(rec_t, (B * C,), S.SquelchRecord)
        assert rec.tobytes() == want_rec.tobytes(), f
        assert np.flatnonzero(rec["open"]).tolist() == [b * C + c for b, c in occupied], f
    second.close()
    r.close()
