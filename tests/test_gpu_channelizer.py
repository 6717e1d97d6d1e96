"""GPU tests of the channelizer stage (csrc/channelizer.hip, sdrg_engine_channelizer_*): every written row of every
stream against the float64 model of tests/channelizer_cases.py within its derived bound, on dense noise (the helper also
asserts that the bound tells the right value from +0, from the neighbouring row and from the previous output).  The zero
tails are compared as bytes, `out` is pre-filled with 0xAA between 64 guard bytes on either side
(tests/stage_harness.py).  Where the stage promises bytes (a stream cut into calls, the same call twice, the host path)
bytes are compared.

The kernel works in tiles of sdrg.channelizer_tile_outputs() output times, each staging its window of unpacked samples
in LDS from aligned 16-byte loads (the ends of a window, and rows that are not 16-byte aligned, sample by sample), with
the samples before the frame taken from the history of the previous call: the shapes below put windows across every tile
seam, rows off every alignment, every M (each has its own DFT) and the history through moves (N < L - 1), format
switches and frames of other lengths."""
import ctypes

import numpy as np
import pytest

import channelizer_cases as cc
import ddc_cases as dd
from stage_harness import FS, GUARD, engine, invalid, out_buffer, read_out, to_device

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def S():
    import sdrg
    return sdrg


@pytest.fixture(scope="module")
def T():
    import torch
    return torch


def config(M, P, O, first=0, rows=None, cutoff_rel=0.5):
    return dict(cutoff_rel=cutoff_rel, channels=M, taps_per_channel=P, oversample=O, first_channel=first,
                n_channels=M - first if rows is None else rows)


class Bank:
    """An engine with the channelizer set, and the model that follows it call by call."""

    def __init__(self, S, T, n, B, **cfg):
        self.S, self.T, self.B = S, T, B
        self.eng = engine(S, B, n)
        self.configure(**cfg)

    def configure(self, **cfg):
        self.cfg = cfg
        self.eng.set_channelizer(**cfg)
        got = self.eng.channelizer_config()
        assert {k: got[k] for k in cfg} == cfg and got["samples_consumed"] == 0
        self.M, self.P, self.O = cfg["channels"], cfg["taps_per_channel"], cfg["oversample"]
        self.rows = slice(cfg["first_channel"], cfg["first_channel"] + cfg["n_channels"])
        self.model = cc.Bank(self.B, self.S.channelizer_design(**cfg), self.M, self.P, self.O)

    def device_call(self, fmt, raw):
        """channelizer_device into a 0xAA-filled buffer between guard bytes: (out [B][rows][cap] complex64, n_out)."""
        T, eng, rows = self.T, self.eng, self.cfg["n_channels"]
        cap = eng.channelizer_max_out()
        assert cap == -(-eng.cfg.samplesPerReading // (self.M // self.O))
        iq_t, out_t = to_device(T, raw), out_buffer(T, self.B * rows * cap * 8)
        T.cuda.synchronize()
        n_out = eng.channelizer_device(iq_t.data_ptr(), fmt, out_t.data_ptr() + GUARD)
        eng.synchronize()
        return read_out(out_t, (self.B, rows, cap), np.complex64), n_out

    def expect(self, got, n_out, fmt, raw, what=None, in_step=True):
        """in_step: the engine has made no call beyond this one."""
        _, y64, bound, m0, want_n = self.model.call(fmt, raw, restate=False)
        assert n_out == want_n, (what, n_out, want_n)
        assert not got[:, :, n_out:].view(np.uint32).any(), (what, "the tail is not +0")
        worst = cc.assert_within(got[:, :, :n_out], y64[:, self.rows], bound, m0, self.P, self.O, what)
        print(f"channelizer {self.M, self.P, self.O} fmt {fmt} {what}: worst error / bound {worst:.3f}")
        assert not in_step or self.eng.channelizer_config()["samples_consumed"] == self.model.g0
        return worst

    def check(self, fmt, raw, what=None):
        got, n_out = self.device_call(fmt, raw)
        self.expect(got, n_out, fmt, raw, what)
        return got, n_out

    def close(self):
        self.eng.close()


@pytest.mark.parametrize("fmt", [dd.CS8, dd.CU8, dd.CS16, dd.CF32])
def test_formats(S, T, fmt):
    n, B = 1000, 3
    bk = Bank(S, T, n, B, **config(16, 4, 1))
    for f in range(2):
        got, n_out = bk.check(fmt, dd.noise(fmt, B, n, seed=10 * fmt + f), f)
        assert n_out == (63, 62)[f] and np.abs(got).max() > 0.01
    bk.close()


@pytest.mark.parametrize("B", [1, 9, 65])
def test_stream_counts(S, T, B):
    n = 700
    bk = Bank(S, T, n, B, **config(8, 3, 2))
    for f in range(2):
        bk.check(dd.CS8, dd.noise(dd.CS8, B, n, seed=20 + f), f)
    bk.close()


@pytest.mark.parametrize("O", [1, 2])
@pytest.mark.parametrize("M", [2, 4, 8, 16, 32, 64, 128, 256])
def test_every_channel_count(S, T, M, O):
    """Every M has a DFT of its own (in registers up to 32, two passes above), and N = 5 M + 3 is odd."""
    n, B = 5 * M + 3, 2
    bk = Bank(S, T, n, B, **config(M, 2, O))
    for f in range(3):
        bk.check(dd.CS16, dd.noise(dd.CS16, B, n, seed=30 + f), (M, O, f))
    bk.close()


@pytest.mark.parametrize("M,P,O", [(32, 1, 1), (32, 32, 2), (256, 16, 1), (256, 16, 2), (128, 32, 1), (64, 8, 2)])
def test_tap_counts(S, T, M, P, O):
    """P = 1 (no filter memory beyond one block), P = 32 (the remainder-free unrolled sums at their longest) and the
    longest prototypes, L = 4096."""
    n, B = (P + 9) * M + 1, 2
    bk = Bank(S, T, n, B, **config(M, P, O))
    for f in range(2):
        bk.check(dd.CS8, dd.noise(dd.CS8, B, n, seed=40 + f), (M, P, O, f))
    bk.close()


@pytest.mark.parametrize("P", [3, 5, 6, 7])
def test_tap_counts_off_the_unroll(S, T, P):
    """The sums take four taps per step and the rest one by one."""
    n, B = 333, 2
    bk = Bank(S, T, n, B, **config(16, P, 2))
    for f in range(2):
        bk.check(dd.CU8, dd.noise(dd.CU8, B, n, seed=50 + f), (P, f))
    bk.close()


@pytest.mark.parametrize("fmt", [dd.CS8, dd.CS16])
def test_odd_rows_are_misaligned(S, T, fmt):
    """N = 4099: rows start 2 (CS8) or 4 (CS16) bytes further off a 16-byte boundary each."""
    n, B = 4099, 3
    bk = Bank(S, T, n, B, **config(16, 8, 2))
    for f in range(2):
        bk.check(fmt, dd.noise(fmt, B, n, seed=60 + f), f)
    bk.close()


def test_iq_base_off_every_alignment(S, T):
    """The caller's iq at 2, 6 and 14 bytes past a 16-byte boundary, and at odd bytes (no sample is then aligned)."""
    n, B, fmt = 1031, 2, dd.CS8
    bk = Bank(S, T, n, B, **config(8, 4, 1))
    cap = bk.eng.channelizer_max_out()
    for shift in (1, 2, 3, 6, 14):
        raw = dd.noise(fmt, B, n, seed=70 + shift)
        buf = T.zeros((B * n * 2 + 32,), dtype=T.uint8, device="cuda:0")
        buf[shift:shift + B * n * 2] = to_device(T, raw.view(np.uint8).reshape(-1))
        out_t = out_buffer(T, B * 8 * cap * 8)
        T.cuda.synchronize()
        n_out = bk.eng.channelizer_device(buf.data_ptr() + shift, fmt, out_t.data_ptr() + GUARD)
        bk.eng.synchronize()
        bk.expect(read_out(out_t, (B, 8, cap), np.complex64), n_out, fmt, raw, shift)
    bk.close()


@pytest.mark.parametrize("M,P,O", [(4, 3, 2), (16, 8, 1), (64, 8, 2), (256, 4, 2)])
def test_tile_seams(S, T, M, P, O):
    """Two tiles and one output of a third, two calls: with P > 1 every window near a multiple of the tile size reads
    samples the neighbouring tile also stages, the first tile's the history; the last tile holds one output."""
    cfg = config(M, P, O)
    tile, D = S.channelizer_tile_outputs(**cfg), M // O
    assert tile == 2048 // M
    B, n = 2, 2 * tile * D + 1
    bk = Bank(S, T, n, B, **cfg)
    for f in range(2):
        got, n_out = bk.check(dd.CS8, dd.noise(dd.CS8, B, n, seed=80 + f), (tile, f))
        assert n_out == (2 * tile + 1, 2 * tile)[f]
    bk.close()


def test_five_calls_are_one_call(S, T):
    """Five calls of unequal N and changing format equal, byte for byte, one call of the concatenation on a second
    engine (CF32 throughout for the second: the first's samples, exactly unpacked)."""
    B, cfg = 3, config(32, 6, 2)
    seq = [(dd.CS8, 700), (dd.CF32, 33), (dd.CS16, 1), (dd.CU8, 2050), (dd.CS16, 517)]
    total = sum(n for _, n in seq)
    a = Bank(S, T, seq[0][1], B, **cfg)
    parts, exact = [], []
    for i, (fmt, n) in enumerate(seq):
        if n != a.eng.cfg.samplesPerReading:
            a.eng.setSamplesPerReading(n)
        raw = dd.noise(fmt, B, n, seed=90 + i)
        got, n_out = a.check(fmt, raw, (i, fmt, n))
        parts.append(got[:, :, :n_out])
        exact.append(cc.exact_samples(fmt, raw))
    whole = np.concatenate(exact, axis=1).view(np.float32).reshape(B, -1)
    b = Bank(S, T, total, B, **cfg)
    got, n_out = b.check(dd.CF32, whole, "one call")
    assert n_out == -(-total // 16)
    assert np.concatenate(parts, axis=2).tobytes() == got[:, :, :n_out].tobytes()
    a.close()
    b.close()


def test_the_same_call_twice_from_reset_gives_the_same_bytes(S, T):
    n, B = 3000, 4
    bk = Bank(S, T, n, B, **config(64, 8, 2))
    raw = dd.noise(dd.CS8, B, n, seed=100)
    first, n1 = bk.check(dd.CS8, raw)
    bk.eng.channelizer_reset()
    bk.model.reset()
    assert bk.eng.channelizer_config()["samples_consumed"] == 0
    second, n2 = bk.check(dd.CS8, raw)
    assert n1 == n2 and first.tobytes() == second.tobytes()
    bk.close()


def test_short_frames_move_the_history_down(S, T):
    """N = 100 < L - 1 = 511: most of each call's new history is the old one moved down."""
    n, B = 100, 3
    bk = Bank(S, T, n, B, **config(16, 32, 1))
    for f in range(8):
        bk.check(dd.CU8, dd.noise(dd.CU8, B, n, seed=110 + f), f)
    bk.close()


def test_calls_without_outputs_write_zeros(S, T):
    """D = 256 at N = 100: three calls in five hold no multiple of 256, and still every byte of out is written."""
    n, B = 100, 2
    bk = Bank(S, T, n, B, **config(256, 2, 1, first=100, rows=3))
    counts = []
    for f in range(8):
        got, n_out = bk.check(dd.CS8, dd.noise(dd.CS8, B, n, seed=120 + f), f)
        assert got.shape == (B, 3, 1)
        counts.append(n_out)
    assert counts == [1, 0, 1, 0, 0, 1, 0, 1]  # samples 0, 256, 512 and 768 of the stream
    bk.close()


@pytest.mark.parametrize("O", [1, 2])
@pytest.mark.parametrize("span", ["first", "last", "middle"])
def test_spans(S, T, span, O):
    """Only n_channels rows are written (the guard bytes follow them), and they are those rows of the full bank."""
    M, n, B = 64, 2000, 2
    first, rows = {"first": (0, 1), "last": (M - 1, 1), "middle": (M // 2 - 1, 3)}[span]
    bk = Bank(S, T, n, B, **config(M, 4, O, first=first, rows=rows))
    full = Bank(S, T, n, B, **config(M, 4, O))
    for f in range(2):
        raw = dd.noise(dd.CS16, B, n, seed=130 + f)
        got, n_out = bk.check(dd.CS16, raw, (span, f))
        all_rows, _ = full.check(dd.CS16, raw, ("full", f))
        assert got.shape[1] == rows and got.tobytes() == all_rows[:, first:first + rows].tobytes()
    bk.close()
    full.close()


def test_one_long_row(S, T):
    n, B = 1 << 20, 1
    bk = Bank(S, T, n, B, **config(256, 16, 2, first=126, rows=4))
    got, n_out = bk.check(dd.CS8, dd.noise(dd.CS8, B, n, seed=140))
    assert n_out == 8192
    bk.close()


def test_many_streams_at_the_benchmark_frame(S, T):
    n, B = 16384, 64
    bk = Bank(S, T, n, B, **config(64, 8, 2, first=28, rows=8))
    got, n_out = bk.check(dd.CS8, dd.noise(dd.CS8, B, n, seed=150))
    assert n_out == 512
    bk.close()


def test_restarts(S, T):
    """set_channelizer and channelizer_reset restart the streams; a rejected set_channelizer, a sample-rate change and a
    change of samples_per_reading change nothing."""
    n, B, fmt = 900, 2, dd.CS8
    cfg = config(16, 8, 2)
    bk = Bank(S, T, n, B, **cfg)
    bk.check(fmt, dd.noise(fmt, B, n, seed=160))
    for bad in (dict(cfg, channels=3), dict(cfg, channels=512), dict(cfg, taps_per_channel=0),
                dict(cfg, taps_per_channel=33), dict(cfg, oversample=3), dict(cfg, cutoff_rel=0.0),
                dict(cfg, cutoff_rel=8.5), dict(cfg, cutoff_rel=float("nan")), dict(cfg, first_channel=1),
                dict(cfg, n_channels=0)):
        invalid(S, bk.eng.set_channelizer, **bad)
    got = bk.eng.channelizer_config()
    assert {k: got[k] for k in cfg} == cfg and got["samples_consumed"] == n
    bk.check(fmt, dd.noise(fmt, B, n, seed=161), "after rejected set_channelizer")
    bk.eng.setSampleRate(2_400_000)
    bk.check(fmt, dd.noise(fmt, B, n, seed=162), "after setSampleRate")
    bk.eng.channelizer_reset()
    bk.model.reset()
    bk.check(fmt, dd.noise(fmt, B, n, seed=163), "after reset")
    bk.check(fmt, dd.noise(fmt, B, n, seed=164), "second after reset")
    bk.configure(**cfg)
    bk.check(fmt, dd.noise(fmt, B, n, seed=165), "after set_channelizer")
    bk.configure(**config(64, 3, 1, first=5, rows=9, cutoff_rel=0.7))  # a longer history than before
    bk.check(fmt, dd.noise(fmt, B, n, seed=166), "after another configuration")
    bk.check(fmt, dd.noise(fmt, B, n, seed=167), "second after another configuration")
    bk.close()


def test_refusals_write_nothing_and_commit_nothing(S, T):
    n, B, fmt = 800, 2, dd.CS16
    eng = engine(S, B, n)
    iq_t = to_device(T, dd.noise(fmt, B, n, seed=170))
    out_t = out_buffer(T, B * 16 * n * 8)
    T.cuda.synchronize()
    invalid(S, eng.channelizer_device, iq_t.data_ptr(), fmt, out_t.data_ptr() + GUARD)  # before any set_channelizer
    invalid(S, eng.channelizer_max_out)
    invalid(S, eng.channelizer_config)
    eng.close()

    cfg = config(16, 4, 1)
    bk = Bank(S, T, n, B, **cfg)
    bk.check(fmt, dd.noise(fmt, B, n, seed=171))
    invalid(S, bk.eng.channelizer_device, iq_t.data_ptr(), 99, out_t.data_ptr() + GUARD)
    L, n_out = S.load(), ctypes.c_int32(-7)
    assert L.sdrg_engine_channelizer_device(bk.eng._h, None, fmt, out_t.data_ptr() + GUARD, ctypes.byref(n_out)) == -1
    assert L.sdrg_engine_channelizer_device(bk.eng._h, iq_t.data_ptr(), fmt, None, ctypes.byref(n_out)) == -1
    assert L.sdrg_engine_channelizer_device(bk.eng._h, iq_t.data_ptr(), fmt, out_t.data_ptr() + GUARD, None) == -1
    assert L.sdrg_engine_channelizer_host(bk.eng._h, None, fmt, None, ctypes.byref(n_out)) == -1
    assert n_out.value == -7 and bk.eng.channelizer_config()["samples_consumed"] == n
    bk.check(fmt, dd.noise(fmt, B, n, seed=172), "after refused calls")
    bk.eng.set_channelizer(off=True)
    invalid(S, bk.eng.channelizer_device, iq_t.data_ptr(), fmt, out_t.data_ptr() + GUARD)
    bk.eng.synchronize()
    assert np.all(out_t.cpu().numpy() == 0xAA), "a refused call wrote to out"
    bk.configure(**cfg)
    bk.check(fmt, dd.noise(fmt, B, n, seed=173), "after off and on")
    bk.close()


def test_host_path_equals_device_path(S, T):
    n, B, fmt = 2500, 5, dd.CU8
    cfg = config(32, 5, 2, first=3, rows=20)
    dev = Bank(S, T, n, B, **cfg)
    host = engine(S, B, n)
    host.set_channelizer(**cfg)
    for f in range(3):
        raw = dd.noise(fmt, B, n, seed=180 + f)
        got, n_out = dev.check(fmt, raw, f)
        h = host.channelizer(raw, fmt)
        assert h.dtype == np.complex64 and h.shape == (B, 20, n_out) and h.tobytes() == got[:, :, :n_out].tobytes()
    dev.close()
    host.close()


def test_wait_outputs_orders_a_consumer_stream(S, T):
    n, B, fmt = 16384, 16, dd.CS8
    bk = Bank(S, T, n, B, **config(64, 8, 2, first=0, rows=16))
    cap = bk.eng.channelizer_max_out()
    consumer = T.cuda.Stream("cuda:0")
    out_t = out_buffer(T, B * 16 * cap * 8)
    copy = T.zeros_like(out_t)
    T.cuda.synchronize()
    for f in range(3):
        raw = dd.noise(fmt, B, n, seed=190 + f)
        iq_t = to_device(T, raw)
        T.cuda.synchronize()
        n_out = bk.eng.channelizer_device(iq_t.data_ptr(), fmt, out_t.data_ptr() + GUARD)
        bk.eng.wait_outputs(consumer.cuda_stream)
        with T.cuda.stream(consumer):
            copy.copy_(out_t)
        consumer.synchronize()
        bk.expect(read_out(copy, (B, 16, cap), np.complex64), n_out, fmt, raw, f)
    bk.close()


@pytest.mark.parametrize("mode", ["OFF", "ON", "INPUTS_READY", "ON|STATS_ASYNC", "INPUTS_READY|STATS_ASYNC"])
def test_process_device_and_ddc_between_channelizer_calls(S, T, mode):
    """channelizer, process_device, ddc, channelizer in every pipelining mode: the channelizer's rows stay within the
    bound, and the spectra, records, PCM and the DDC's rows are the bytes of an engine that never configured it."""
    n, B, fmt = 16384, 4, dd.CS8
    bits = 0
    for name in mode.split("|"):
        bits |= getattr(S, "PIPELINE_" + name)
    stages = S.STAGE_SPECTRUM | S.STAGE_STATS | S.STAGE_SSB
    raws = [dd.noise(fmt, B, n, seed=200 + f) for f in range(3)]
    ddc_cfg = dict(offset_hz=20_000.0, cutoff_hz=20_000.0, decimation=41, taps=255)

    def process(eng, f):
        iq_t = to_device(T, raws[f])
        spec = T.zeros((B, n), dtype=T.float32, device="cuda:0")
        rec = T.zeros((B * S.RECORD_DTYPE.itemsize,), dtype=T.uint8, device="cuda:0")
        pcm = T.zeros((B, max(eng.pcm_len, 1)), dtype=T.int16, device="cuda:0")
        ddc = T.zeros((B, eng.ddc_max_out(), 2), dtype=T.float32, device="cuda:0")
        T.cuda.synchronize()
        eng.process_device(iq_t.data_ptr(), fmt, stages, spec.data_ptr(), rec.data_ptr(), pcm.data_ptr(), 1000 + f)
        eng.ddc_device(iq_t.data_ptr(), fmt, ddc.data_ptr())
        return iq_t, spec, rec, pcm, ddc

    bk = Bank(S, T, n, B, **config(16, 8, 2))
    plain = engine(S, B, n)
    for eng in (bk.eng, plain):
        eng.set_pipelining(bits)
        eng.set_ddc(**ddc_cfg)
    cap = bk.eng.channelizer_max_out()
    outs, iqs, held = [], [], []
    for f in range(3):
        iq_t, out_t = to_device(T, raws[f]), out_buffer(T, B * 16 * cap * 8)
        T.cuda.synchronize()
        n_out = bk.eng.channelizer_device(iq_t.data_ptr(), fmt, out_t.data_ptr() + GUARD)
        outs.append((out_t, n_out))
        iqs.append(iq_t)
        if f < 2:
            held.append((process(bk.eng, f), process(plain, f)))
    bk.eng.synchronize()
    plain.synchronize()
    for f, (out_t, n_out) in enumerate(outs):
        bk.expect(read_out(out_t, (B, 16, cap), np.complex64), n_out, fmt, raws[f], (mode, f), in_step=False)
    assert bk.eng.channelizer_config()["samples_consumed"] == 3 * n
    for f, (a, b) in enumerate(held):
        for x, y, name in zip(a[1:], b[1:], ("spectra", "records", "pcm", "ddc")):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), (mode, f, name)
    assert held[0][0][1].cpu().numpy().max() > 0
    bk.close()
    plain.close()


def test_rows_against_the_engines_own_ddc(S, T):
    """(16, 8, 2): rows 3 and 12 against ddc_device on a second engine at those rows' offsets, cutoff_hz = 0.5 fs / 16,
    T = 127, D = 8, within the sum of the two stages' bounds; the two designs' taps are the same bytes."""
    M, P, O, n, B, fmt = 16, 8, 2, 4096, 2, dd.CS16
    L, D = M * P, M // O
    bk = Bank(S, T, n, B, **config(M, P, O))
    h = S.channelizer_design(**config(M, P, O))
    raws = [dd.noise(fmt, B, n, seed=210 + f) for f in range(2)]
    rows = [bk.check(fmt, raw, f) for f, raw in enumerate(raws)]
    bounds = [cc.Bank(B, h, M, P, O), []]
    for raw in raws:
        bounds[1].append(bounds[0].call(fmt, raw, restate=False)[2])
    for k in (3, 12):
        offset = S.bin_offset_hz(M, FS, k)
        assert offset == (k - M // 2) * FS / M
        cfg = dict(offset_hz=offset, cutoff_hz=0.5 * FS / M, decimation=D, taps=L - 1)
        assert S.ddc_design(FS, **cfg).tobytes() == h[:L - 1].tobytes()
        ddc = engine(S, B, n)
        ddc.set_ddc(**cfg)
        for f, raw in enumerate(raws):
            want = ddc.ddc(raw, fmt)
            got, n_out = rows[f]
            assert want.shape == (B, n_out)
            both = bounds[1][f] + dd.error_bound(L - 1, 1.0, h[:L - 1])
            err = np.abs(got[:, k, :n_out].astype(np.complex128) - want)
            assert np.all(err <= both), (k, f, float((err / both).max()))
            assert np.abs(want[:, P * O:]).mean() > 100 * both.mean()
        ddc.close()
    bk.close()


def test_two_fm_carriers_end_to_end(S, T):
    """A CS8 stream holds two FM carriers at the centres of rows 5 and 11 of a (16, 8, 2) bank, carrying 1 kHz and
    2.5 kHz tones at 25 kHz deviation, over a noise floor of 0.05 rms per component (a row without a carrier demodulates
    to noise; without a floor it demodulates what leaks from the carriers, at full scale).  The bank's out goes on the
    device, as 16 streams, to a second engine's demod_device.  Rows 5 and 11 of the audio peak at their own tone's bin;
    every other row's peak is at least 20 dB below theirs.  (A noise row's spectral peak falls against a tone's as the
    root of the duration: 0.79 s put it 24 to 28 dB down in the NumPy model of this test.)"""
    M, P, O, n, frames, B = 16, 8, 2, 1 << 18, 6, 1
    fc, R, dev = FS * O / M, 25, 25_000.0
    tones = {5: 1000.0, 11: 2500.0}
    t = np.arange(n * frames) / FS
    z = np.zeros(n * frames, np.complex128)
    for k, ft in tones.items():
        z += 0.4 * np.exp(1j * (2 * np.pi * S.bin_offset_hz(M, FS, k) * t + dev / ft * np.sin(2 * np.pi * ft * t)))
    rng = np.random.default_rng(7)
    z += 0.05 * (rng.standard_normal(z.size) + 1j * rng.standard_normal(z.size))
    iq = np.empty((B, 2 * z.size))
    iq[0, 0::2], iq[0, 1::2] = z.real, z.imag
    raw = np.round(iq * 128.0).clip(-128, 127).astype(np.int8)

    bank = engine(S, B, n)
    bank.set_channelizer(**config(M, P, O, cutoff_rel=0.4))
    cap = bank.channelizer_max_out()
    audio = engine(S, M * B, 1024)
    audio.set_demod(mode=S.DEMOD_FM, channel_rate_hz=fc, deviation_hz=dev, dc_cutoff_hz=0.0, deemphasis_us=0.0,
                    audio_decimation=R, audio_taps=255, audio_cutoff_hz=3000.0, gain=1.0, out_format=S.DEMOD_OUT_F32,
                    max_in=cap)
    acap = audio.demod_max_out()
    chan_t = T.zeros((M * B, cap, 2), dtype=T.float32, device="cuda:0")
    pcm_t = T.zeros((M * B, acap), dtype=T.float32, device="cuda:0")
    pcm = []
    for f in range(frames):
        iq_t = to_device(T, raw[:, 2 * n * f:2 * n * (f + 1)])
        T.cuda.synchronize()
        n_out = bank.channelizer_device(iq_t.data_ptr(), dd.CS8, chan_t.data_ptr())
        bank.synchronize()
        n_audio = audio.demod_device(chan_t.data_ptr(), n_out, pcm_t.data_ptr())
        audio.synchronize()
        pcm.append(pcm_t.cpu().numpy()[:, :n_audio].copy())
    a = np.concatenate(pcm, axis=1)[:, 64:].astype(np.float64)
    assert a.shape[1] > 7000
    a -= a.mean(axis=1, keepdims=True)
    sp = np.abs(np.fft.rfft(a * np.hanning(a.shape[1]), axis=1))
    peak, at = sp.max(axis=1), sp.argmax(axis=1)
    for k, ft in tones.items():
        assert abs(at[k] - ft * a.shape[1] / (fc / R)) <= 1, (k, at[k])
    others = np.delete(peak, list(tones))
    down = 20 * np.log10(others.max() / min(peak[k] for k in tones))
    print(f"end to end: the other rows' highest peak is {down:.1f} dB below the tones'")
    assert down <= -20.0, down
    bank.close()
    audio.close()
