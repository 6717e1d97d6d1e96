"""GPU tests of the squelch stage (csrc/squelch.hip, sdrg_engine_squelch_*, sdrg_engine_ddc_squelch_demod_host): the
gated channel and the records of each stream against the NumPy restatement in tests/squelch_cases.py fed the library's
own design values.  Every comparison is of the bytes of the whole `out` and of the records (the stage is specified
operation by operation: no tolerances).  `out` and `records` are pre-filled with 0xAA between 64 guard bytes on either
side, every stream has its own data, and the input rows hold NaN past the call's n samples.

The power kernel works in tiles of `tile` positions counted from the start of the block in progress, the gate kernel in
tiles of `tile` samples of the call (sdrg.squelch_geometry), blocks above 128 samples meet in LDS, and rows or offsets
that are not 16-byte aligned take 8-byte loads: the shapes below put data on each of these paths and seams."""
import ctypes

import numpy as np
import pytest

import channelizer_cases as cc
import ddc_cases as dd
import demod_cases as dm
import resample_cases as rs
import squelch_cases as sq
from stage_harness import FS, GUARD, BlockRig, engine, invalid, out_buffer, read_out, rows_bytes, same, to_device

pytestmark = pytest.mark.gpu

BASE = dict(open_db=-3.0, close_db=-9.0, tau_blocks=0.0, block=64, hang_blocks=1, max_in=1024)
PATTERN = (1, 1, 0, 0, 0, 1, 0, 1, 1, 1, 0, 0)  # loud and quiet blocks: every code, the hang used up and reloaded


@pytest.fixture(scope="module")
def S():
    import sdrg
    return sdrg


@pytest.fixture(scope="module")
def T():
    import torch
    return torch


class Gate(BlockRig):
    """An engine with the squelch set, and the restatement that follows it call by call."""
    stage = "squelch"
    record = "SquelchRecord"

    def make_model(self, d):
        des = self.S.squelch_design(**self.cfg)
        assert all(des[k].tobytes() == d[k].tobytes() for k in ("open_thr", "close_thr", "beta"))
        return sq.Squelch(self.B, d["open_thr"], d["close_thr"], d["beta"], d["block"], d["hang_blocks"])


@pytest.mark.parametrize("B", [1, 9, 65, 130])
def test_stream_counts(S, T, B):
    """The step kernel takes 64 streams per wave: a wave in part, a wave and a stream, two waves and two streams."""
    n = 5 * 64 + 9
    g = Gate(S, T, B, **BASE)
    z = sq.keyed(B, 3 * n, 20, 64, PATTERN)
    opened = 0
    for f in range(3):
        _, rec, nb = g.check(z[:, f * n:(f + 1) * n], (B, f))
        opened += int(rec["open_blocks"].sum())
    assert opened > B
    g.close()


@pytest.mark.parametrize("block", [16, 32, 64, 128, 256, 512, 1024])
def test_calls_around_the_block(S, T, block):
    """n = 0, 1, S - 1, S, S + 1, 2 S - 1 in one stream, for every width of the butterfly: in a wave (S <= 128), across the
    waves through LDS (256, 512), and across the workgroup's two passes (1024)."""
    B = 3
    g = Gate(S, T, B, **dict(BASE, block=block, max_in=2 * block))
    ns = (block + 1, 0, 1, block - 1, 0, block, block + 1, 2 * block - 1, 1, 2 * block, 0)
    z = sq.keyed(B, sum(ns), 30 + block, block, (1, 0, 1, 1, 0, 0))
    at, blocks = 0, 0
    for f, n in enumerate(ns):
        got, rec, nb = g.check(z[:, at:at + n], (block, f, n))
        at, blocks = at + n, blocks + nb
        if n == 0:
            assert nb == 0 and not got.view(np.uint32).any() and not rec["open_blocks"].any()
    assert blocks == sum(ns) // block and g.model.g == sum(ns)
    g.close()


def test_first_call_without_samples(S, T):
    B = 2
    g = Gate(S, T, B, **BASE)
    got, rec, nb = g.check(np.zeros((B, 0), np.complex64))
    assert nb == 0 and got.shape == (B, 1024) and not got.view(np.uint32).any()
    assert not rec["level"].view(np.uint32).any() and not rec["open"].any()
    g.check(sq.keyed(B, 300, 35, 64, PATTERN))
    g.close()


def test_a_stream_cut_at_every_offset_of_a_block(S, T):
    """S = 16: after a first call of `off` samples the next starts at every in-block offset, odd (8-byte loads in the
    power kernel) and even, and three calls share a block."""
    B, block = 3, 16
    g = Gate(S, T, B, **dict(BASE, block=block, max_in=64))
    z = sq.keyed(B, 16 + 3 + 45, 40, block, (1, 0, 1, 0, 0, 1))
    for off in range(block):
        g.eng.squelch_reset()
        g.model.reset()
        at = 0
        for n in (off, 3, 45):
            g.check(z[:, at:at + n], (off, n))
            at += n
    g.close()


def test_five_calls_are_one_stream(S, T):
    B = 4
    g = Gate(S, T, B, **dict(BASE, tau_blocks=2.0, hang_blocks=2))
    ns = (700, 64, 1, 1024, 333)
    z = sq.keyed(B, sum(ns), 50, 64, PATTERN)
    outs, at = [], 0
    for f, n in enumerate(ns):
        got, rec, _ = g.check(z[:, at:at + n], f)
        outs.append(got[:, :n])
        at += n
    d = g.eng.squelch_config()
    want, want_rec, _ = sq.one_call(z, d["open_thr"], d["close_thr"], d["beta"], 64, 2)
    assert np.concatenate(outs, axis=1).tobytes() == want.tobytes()
    assert rec["level"].tobytes() == want_rec["level"].tobytes() and rec["open"].tolist() == want_rec["open"].tolist()
    g.close()


@pytest.mark.parametrize("block", [16, 256, 1024])
def test_every_workgroup_seam(S, T, block):
    """A call over three seams and a bit, started 5 samples (8-byte loads) and 6 samples (16-byte loads) into a block:
    the power kernel's tiles start at the multiples of `tile` counted from the block's start, the gate kernel's at the
    multiples of `tile` in the call."""
    B, tile = 2, S.squelch_geometry(block)
    n = 3 * tile + 7
    g = Gate(S, T, B, **dict(BASE, block=block, max_in=n + 1))
    for off in (5, 6):
        g.eng.squelch_reset()
        g.model.reset()
        z = sq.keyed(B, off + 2 * n, 60 + off, block, (1, 1, 0, 1, 0, 0, 0))
        g.check(z[:, :off], (block, off, "head"))
        got, _, _ = g.check(z[:, off:off + n], (block, off, "first"), in_stride=n + 1)
        assert np.abs(got[:, :n]).max() > 0.1
        g.check(z[:, off + n:], (block, off, "second"), in_stride=n)
    g.close()


def test_row_strides_and_alignments(S, T):
    """in_stride above n, even and odd (odd rows are not 16-byte aligned), and chan and out 8 bytes off alignment."""
    B, n = 3, 333
    g = Gate(S, T, B, **BASE)
    z = sq.keyed(B, 6 * n, 70, 64, PATTERN)
    for f, (stride, shift) in enumerate(((1024, 0), (n, 0), (n + 1, 0), (n + 4, 8), (1000, 8), (n, 8))):
        got, _, _ = g.check(z[:, f * n:(f + 1) * n], (stride, shift), in_stride=stride, shift=shift)
        assert not got[:, n:].view(np.uint32).any()
    g.close()


def test_in_place_equals_out_of_place(S, T):
    B, n = 5, 900
    a, b = Gate(S, T, B, **dict(BASE, tau_blocks=1.0)), Gate(S, T, B, **dict(BASE, tau_blocks=1.0))
    z = sq.keyed(B, 3 * n, 80, 64, PATTERN)
    for f, stride in enumerate((1024, n + 1, n)):
        part = z[:, f * n:(f + 1) * n]
        out_a, rec_a, _ = a.check(part, (f, "out of place"), in_stride=stride)
        out_b, rec_b, _ = b.check(part, (f, "in place"), in_stride=stride, in_place=True)
        assert out_a.tobytes() == out_b.tobytes() and rec_a.tobytes() == rec_b.tobytes()
    a.close()
    b.close()


@pytest.mark.parametrize("tau", [0.0, 3.0])
def test_every_code_within_a_call_and_across_calls(S, T, tau):
    """One stream of blocks at 0 dB and -40 dB: closed, ramp up, open, the hang, ramp down, within a call; then cut at
    block ends, so that the decision of a call's last block shows in the next call's first sample, and in its record
    first."""
    B, block, H = 2, 16, 2
    g = Gate(S, T, B, **dict(BASE, block=block, hang_blocks=H, tau_blocks=tau, max_in=512))
    amps = [1, 1, 1] + [0] * 12 + [1, 1, 0, 1] + [0] * 12  # stretches long enough for the smoothed level to fall
    z = sq.noise(B, block * len(amps), 90) * np.repeat(np.where(np.array(amps) > 0, 1.0, 0.01), block)[None, :]
    z = z.astype(np.complex64)
    got, rec, nb = g.check(z, "one call")
    whole = got[:, :z.shape[1]].copy()
    codes = set()
    for j in range(len(amps)):
        blk_in, blk_out = z[0, j * block:(j + 1) * block], whole[0, j * block:(j + 1) * block]
        if not blk_out.view(np.uint32).any():
            codes.add(sq.CLOSED)
        elif blk_out.tobytes() == blk_in.tobytes():
            codes.add(sq.OPEN)
        elif blk_out[-1] == blk_in[-1]:
            codes.add(sq.RAMP_UP)
        elif abs(blk_out[-1]) == 0:
            codes.add(sq.RAMP_DOWN)
    assert codes == {sq.CLOSED, sq.RAMP_UP, sq.OPEN, sq.RAMP_DOWN} and nb == len(amps)
    # the same stream in calls of one block: each call's record says how the next call's block begins
    g.eng.squelch_reset()
    g.model.reset()
    before, last, seen = np.zeros(B, np.int32), np.zeros(B, np.int32), set()  # the gate after the two calls before
    for j in range(len(amps)):
        part = z[:, j * block:(j + 1) * block]
        got, rec, nb = g.check(part, ("block", j))
        assert nb == 1 and got[:, :block].tobytes() == whole[:, j * block:(j + 1) * block].tobytes()
        # code 2 was + open of the records before this call: its first weight is 0 only when closed (code 0), its last
        # only when closed or ramping down (open = 0)
        head, end = got[:, 0] != 0, got[:, block - 1] != 0
        assert head.tolist() == ((before == 1) | (last == 1)).tolist(), j
        assert end.tolist() == (last == 1).tolist(), j
        seen.add((int(last[0]), int(rec["open"][0])))
        before, last = last, rec["open"].copy()
    assert seen == {(0, 0), (0, 1), (1, 1), (1, 0)}
    g.close()


def test_a_decision_crosses_the_call_boundary(S, T):
    """The last block of a call opens the gate: the record says so at once, the samples only in the next call, which
    ramps up from its first sample; and likewise for the close after the hang."""
    B, block = 1, 16
    g = Gate(S, T, B, **dict(BASE, block=block, hang_blocks=0, max_in=64))
    loud = np.full((B, 2 * block), 1 + 0j, np.complex64)
    got, rec, nb = g.check(loud, "opens in its last block")
    r = np.float32(1.0) / np.float32(block)
    # block 0 closed; block 1 is the ramp up that block 0 decided; block 1 keeps the gate open for the next call
    assert nb == 2 and rec["open"][0] == 1 and rec["open_blocks"][0] == 2 and not got[0, :block].view(np.uint32).any()
    assert got[0, block] == np.complex64(r) and got[0, 2 * block - 1] == np.complex64(1)
    quiet = np.full((B, block), 0.01 + 0j, np.complex64)
    got, rec, nb = g.check(quiet, "open: decided before the call")
    assert got[0, :block].tobytes() == quiet[0].tobytes() and rec["open"][0] == 0 and rec["open_blocks"][0] == 0
    got, rec, nb = g.check(quiet[:, :5], "ramp down: decided by the last call's only block")
    assert [got[0, i] for i in range(5)] == [np.complex64(np.float32(0.01) * (np.float32(15 - i) * r)) for i in range(5)]
    got, rec, nb = g.check(quiet[:, :11], "the rest of the ramp")
    assert nb == 1 and got[0, 10] == 0 and got[0, 0] == np.complex64(np.float32(0.01) * (np.float32(10) * r))
    g.close()


def test_powers_down_to_denormal(S, T):
    """Amplitudes of 1e-21: every power is a denormal float, and so are the thresholds; a flushed power would read 0."""
    B, block = 3, 64
    cfg = dict(BASE, open_db=-425.0, close_db=-431.0, tau_blocks=1.5, max_in=1024)
    g = Gate(S, T, B, **cfg)
    assert 0 < g.model.close_thr < g.model.open_thr < np.float32(1.2e-38)
    z = (sq.keyed(B, 2048, 100, block, PATTERN, loud=1.0, quiet=0.03).astype(np.complex128) * 1e-21).astype(np.complex64)
    opened = 0
    for f in range(2):
        got, rec, _ = g.check(z[:, f * 1024:(f + 1) * 1024], f)
        assert np.all(rec["level"] > 0) and np.all(rec["level"] < np.float32(1.2e-38))
        opened += int(rec["open_blocks"].sum())
    assert 0 < opened < B * 32
    g.close()


def test_many_streams_long_rows(S, T):
    B, n = 64, 16384
    g = Gate(S, T, B, **dict(BASE, tau_blocks=0.7, hang_blocks=1, max_in=n))
    z = sq.keyed(B, n + 100, 110, 64, PATTERN)
    g.check(z[:, :100], "head")
    _, rec, nb = g.check(z[:, 100:], "64 x 16384")
    assert nb == 256 and 0 < rec["open_blocks"].min() and rec["open_blocks"].max() < 256
    g.close()


def test_the_most_blocks_a_call_completes(S, T):
    """S = 16 and a call that starts on a block's last sample: max_in / 16 + 1 blocks, the whole block scratch."""
    B, n = 2, 4096
    g = Gate(S, T, B, **dict(BASE, block=16, max_in=n))
    z = sq.keyed(B, 15 + n, 115, 16, PATTERN)
    g.check(z[:, :15])
    _, _, nb = g.check(z[:, 15:], "starts on a block's last sample")
    assert nb == 256 == (15 + n) // 16
    g.close()


def test_without_records(S, T):
    B, n = 3, 500
    g = Gate(S, T, B, **BASE)
    z = sq.keyed(B, 3 * n, 120, 64, PATTERN)
    g.check(z[:, :n], "no records", records=False)
    g.check(np.zeros((B, 0), np.complex64), "no records, no samples", records=False)
    g.check(z[:, n:2 * n], "records again")
    g.check(z[:, 2 * n:], "no records, in place", records=False, in_place=True)
    g.close()


def test_reset_and_set_again_between_calls(S, T):
    B, n = 3, 700
    g = Gate(S, T, B, **BASE)
    z = sq.keyed(B, n, 130, 64, (1, 1, 1, 0))
    _, first, _ = g.check(z)
    g.check(z, "a second call goes on from the first")
    g.eng.squelch_reset()
    g.model.reset()
    assert g.eng.squelch_config()["samples_consumed"] == 0
    _, again, _ = g.check(z, "after the reset")
    assert again.tobytes() == first.tobytes()
    g.configure(**dict(BASE, block=128, hang_blocks=0, tau_blocks=4.0))
    g.check(z[:, :300], "another configuration")
    invalid(S, g.eng.set_squelch, **dict(BASE, block=100))  # rejected: the configuration and the state stay
    assert g.eng.squelch_config()["samples_consumed"] == 300 and g.eng.squelch_config()["block"] == 128
    g.check(z[:, 300:], "after a rejected set_squelch")
    g.configure(**BASE)  # the same configuration again restarts as well
    _, third, _ = g.check(z, "set again")
    assert third.tobytes() == first.tobytes()
    g.close()


def test_refusals_write_nothing_and_commit_nothing(S, T):
    B, n = 2, 300
    eng = engine(S, B)
    z = sq.keyed(B, n, 140, 64, PATTERN)
    chan_t = to_device(T, rows_bytes(z, 1024))
    out_t, rec_t = out_buffer(T, B * 1024 * 8), out_buffer(T, B * 16)
    T.cuda.synchronize()
    args = (chan_t.data_ptr(), 1024, n, out_t.data_ptr() + GUARD, rec_t.data_ptr() + GUARD)
    invalid(S, eng.squelch_device, *args)  # before any set_squelch
    invalid(S, eng.squelch_config)
    eng.close()

    g = Gate(S, T, B, **BASE)
    g.check(z)
    for stride, bad_n in ((1024, 1025), (1024, -1), (1025, n), (n - 1, n), (0, 0), (1024, 1 << 30), (-5, -5)):
        invalid(S, g.eng.squelch_device, chan_t.data_ptr(), stride, bad_n, out_t.data_ptr() + GUARD,
                rec_t.data_ptr() + GUARD)
    L = S.load()
    nb = ctypes.c_int32(-7)
    h, c, o = g.eng._h, chan_t.data_ptr(), out_t.data_ptr() + GUARD
    assert L.sdrg_engine_squelch_device(h, None, 1024, n, o, None, ctypes.byref(nb)) == -1
    assert L.sdrg_engine_squelch_device(h, c, 1024, n, None, None, ctypes.byref(nb)) == -1
    assert L.sdrg_engine_squelch_device(h, c, 1024, n, o, None, None) == -1
    assert L.sdrg_engine_squelch_device(None, c, 1024, n, o, None, ctypes.byref(nb)) == -1
    assert nb.value == -7 and g.eng.squelch_config()["samples_consumed"] == n
    g.check(sq.keyed(B, n, 141, 64, PATTERN), "after refused calls")
    g.eng.set_squelch(off=True)
    invalid(S, g.eng.squelch_device, *args)
    g.eng.synchronize()
    assert np.all(out_t.cpu().numpy() == 0xAA) and np.all(rec_t.cpu().numpy() == 0xAA), "a refused call wrote"
    g.configure(**BASE)
    g.check(sq.keyed(B, n, 142, 64, PATTERN), "after off and on")
    g.close()


def test_host_path_equals_device_path(S, T):
    B, n = 5, 777
    dev = Gate(S, T, B, **dict(BASE, tau_blocks=1.0))
    host = engine(S, B)
    host.set_squelch(**dict(BASE, tau_blocks=1.0))
    z = sq.keyed(B, 3 * n, 150, 64, PATTERN)
    for f in range(3):
        part = z[:, f * n:(f + 1) * n - 100 * f]
        got, rec, nb = dev.check(part, f, in_stride=part.shape[1])
        h_out, h_rec, h_nb = host.squelch_host(part)
        assert h_out.dtype == np.complex64 and h_out.tobytes() == got.tobytes() and h_nb == nb
        assert h_rec.tobytes() == rec.tobytes()
    h_out, h_rec, h_nb = host.squelch_host(np.zeros((B, 0), np.complex64))
    assert h_out.shape == (B, 0) and h_nb == 0 and h_rec["level"].tobytes() == rec["level"].tobytes()
    h_out, none, _ = host.squelch_host(z[:, :64], want_records=False)
    assert none is None and h_out.shape == (B, 64)
    with pytest.raises(S.SdrgError):
        host.squelch_host(np.zeros((B, 1025), np.complex64))
    dev.close()
    host.close()


def test_process_device_and_demod_device_between_squelch_calls(S, T):
    """squelch, process_device, demod_device, squelch, ...: the gated rows are the restatement's, the audio its
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

    g = Gate(S, T, B, n, **BASE)
    g.eng.set_demod(**demod_cfg)
    d = g.eng.demod_config()
    demod_model = dm.Demod(B, d["mode"], d["kf"], d["alpha"], d["a"], d["taps"], 4, d["gain"], dm.OUT_F32, 1024)
    plain = engine(S, B, n)
    cap = g.eng.demod_max_out()
    chans = [sq.keyed(B, 900 + f, 160 + f, 64, PATTERN) for f in range(3)]
    held, outs, audio = [], [], []
    for f in range(3):
        chan_t = to_device(T, rows_bytes(chans[f], 1024))
        out_t, rec_t = out_buffer(T, B * 1024 * 8), out_buffer(T, B * 16)
        T.cuda.synchronize()
        nb = g.eng.squelch_device(chan_t.data_ptr(), 1024, chans[f].shape[1], out_t.data_ptr() + GUARD,
                                  rec_t.data_ptr() + GUARD)
        outs.append((out_t, rec_t, nb, chan_t))
        if f < 2:
            held.append((process(g.eng, f), process(plain, f)))
            a_t = T.full((B * cap * 4,), 0xAA, dtype=T.uint8, device="cuda:0")
            audio.append((a_t, g.eng.demod_device(chan_t.data_ptr(), chans[f].shape[1], a_t.data_ptr())))
    g.eng.synchronize()
    plain.synchronize()
    for f, (out_t, rec_t, nb, _) in enumerate(outs):
        want, want_rec, want_nb = g.model.call(chans[f], in_stride=1024)
        same(read_out(out_t, (B, 1024), np.complex64), nb, want, want_nb, f)
        same(read_out(rec_t, (B, 4), np.uint32), nb, want_rec.view(np.uint32).reshape(B, 4), want_nb, (f, "records"))
    for f, (a_t, n_out) in enumerate(audio):
        want, want_n = demod_model.call(chans[f])
        assert n_out == want_n and a_t.cpu().numpy().tobytes() == want.tobytes(), f
    for f, (a, b) in enumerate(held):
        for x, y, name in zip(a[1:], b[1:], ("spectra", "records", "pcm")):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), (f, name)
    assert held[0][0][1].cpu().numpy().max() > 0
    g.close()
    plain.close()


def test_scanner_finds_the_one_occupied_channel(S, T):
    """CS8 noise through an (M = 8, P = 8, O = 1) bank whose rows go, on the device, to a second engine of 8 B streams
    with the squelch set; half-way through, a carrier is keyed on at the centre of one row per stream.  Exactly those
    rows' records open, read from the records themselves; the bank's rows are within the channelizer's bound of its
    restatement (it is specified by a bound, not by bytes), and the squelch's bytes are its restatement's on those
    rows."""
    M, P, O, n, B, frames, block = 8, 8, 1, 8192, 2, 2, 64
    rows_with_carrier = {0: 5, 1: 2}
    rng = np.random.default_rng(11)
    t = np.arange(n * frames) / FS
    iq = np.empty((B, 2 * n * frames))
    for b in range(B):
        z = 0.03 * (rng.standard_normal(t.size) + 1j * rng.standard_normal(t.size))
        on = np.arange(t.size) >= n  # keyed on with the second frame
        z = z + on * 0.5 * np.exp(2j * np.pi * S.bin_offset_hz(M, FS, rows_with_carrier[b]) * t + 0.4j * b)
        iq[b, 0::2], iq[b, 1::2] = z.real, z.imag
    raw = np.round(iq * 128.0).clip(-128, 127).astype(np.int8)
    cfg = dict(cutoff_rel=0.4, channels=M, taps_per_channel=P, oversample=O, first_channel=0, n_channels=M)
    bank = engine(S, B, n)
    bank.set_channelizer(**cfg)
    bank_model = cc.Bank(B, S.channelizer_design(**cfg), M, P, O)
    cap = bank.channelizer_max_out()
    assert cap == n // M
    gates = engine(S, M * B, 1024)
    sq_cfg = dict(open_db=-12.0, close_db=-18.0, tau_blocks=1.0, block=block, hang_blocks=2, max_in=cap)
    gates.set_squelch(**sq_cfg)
    d = gates.squelch_config()
    model = sq.Squelch(M * B, d["open_thr"], d["close_thr"], d["beta"], block, 2)
    chan_t = T.zeros((M * B, cap, 2), dtype=T.float32, device="cuda:0")
    want_open = np.zeros(M * B, np.int32)
    for b, k in rows_with_carrier.items():
        want_open[b * M + k] = 1
    for f in range(frames):
        iq_t = to_device(T, raw[:, 2 * n * f:2 * n * (f + 1)])
        out_t, rec_t = out_buffer(T, M * B * cap * 8), out_buffer(T, M * B * 16)
        T.cuda.synchronize()
        n_out = bank.channelizer_device(iq_t.data_ptr(), dd.CS8, chan_t.data_ptr())
        bank.synchronize()
        nb = gates.squelch_device(chan_t.data_ptr(), cap, n_out, out_t.data_ptr() + GUARD, rec_t.data_ptr() + GUARD)
        gates.synchronize()
        rows = chan_t.cpu().numpy().view(np.complex64).reshape(M * B, cap)
        _, y64, bound, m0, want_n = bank_model.call(dd.CS8, raw[:, 2 * n * f:2 * n * (f + 1)], restate=False)
        assert n_out == want_n == cap
        cc.assert_within(rows.reshape(B, M, cap)[:, :, :n_out], y64, bound, m0, P, O, f)
        want, want_rec, want_nb = model.call(rows[:, :n_out], in_stride=cap)
        same(read_out(out_t, (M * B, cap), np.complex64), nb, want, want_nb, f)
        rec = read_out(rec_t, (M * B, 4), np.uint32)
        same(rec, nb, want_rec.view(np.uint32).reshape(M * B, 4), want_nb, (f, "records"))
        rec = rec.view(S.SquelchRecord)[:, 0]
        if f == 0:
            assert not rec["open"].any() and not rec["open_blocks"].any() and np.all(rec["level_db"] < -25.0)
        else:
            assert rec["open"].tolist() == want_open.tolist()
            assert np.all(rec["level_db"][want_open == 1] > -9.0) and np.all(rec["level_db"][want_open == 0] < -25.0)
            assert np.all(rec["open_blocks"][want_open == 1] >= nb - 3)
    bank.close()
    gates.close()


def test_listening_to_a_keyed_fm_carrier(S, T):
    """fs = 2 MHz, N = 16384, CS8 noise of 3 LSB rms; from the middle of the second frame an FM carrier at +250 kHz,
    deviated 50 kHz by a 1 kHz tone.  ddc_squelch_demod (D = 10, T = 127; S = 64; FM, R = 4, T2 = 63, float) gives zero
    bytes while the gate is closed and, throughout, the DDC, the squelch and the demodulator restated in sequence; the
    same frames through ddc_squelch_demod_resample_host (24 / 25 -> 48 kHz) equal the four restatements; and ddc_demod
    on the first engine afterwards ignores the squelch."""
    fs, n, B, frames = 2_000_000, 16384, 2, 4
    t = np.arange(frames * n, dtype=np.float64)
    rng = np.random.default_rng(3)
    raw = np.empty((B, 2 * frames * n), np.int8)
    key = n + n // 2
    for b in range(B):
        phi = 2 * np.pi * 250_000.0 * t / fs + 50.0 * np.sin(2 * np.pi * 1000.0 * t / fs + 0.7 * b) + 0.3 * b
        z = (t >= key) * 0.5 * np.exp(1j * phi) + (3 / 128) * (rng.standard_normal(t.size) + 1j * rng.standard_normal(t.size))
        raw[b, 0::2] = np.round(z.real * 128).clip(-128, 127).astype(np.int8)
        raw[b, 1::2] = np.round(z.imag * 128).clip(-128, 127).astype(np.int8)
    ddc_cfg = dict(offset_hz=250_000.0, cutoff_hz=100_000.0, decimation=10, taps=127)
    demod_cfg = dict(mode=dm.FM, channel_rate_hz=200_000.0, deviation_hz=75_000.0, dc_cutoff_hz=0.0, deemphasis_us=75.0,
                     audio_decimation=4, audio_taps=63, audio_cutoff_hz=15_000.0, gain=1.0, out_format=dm.OUT_F32,
                     max_in=1639)
    sq_cfg = dict(open_db=-12.0, close_db=-18.0, tau_blocks=1.0, block=64, hang_blocks=2, max_in=1639)
    rs_cfg = dict(interp=24, decim=25, taps_per_phase=8, cutoff_rel=0.9, components=1, out_format=rs.OUT_F32, gain=1.0,
                  max_in=410)
    first = raw[:, :2 * n]
    eng, eng48 = engine(S, B, n, fs), engine(S, B, n, fs)
    for e in (eng, eng48):
        e.set_ddc(**ddc_cfg)
        e.set_demod(**demod_cfg)
    eng48.set_resample(**rs_cfg)
    invalid(S, eng.ddc_squelch_demod, first, dd.CS8)  # the squelch off
    invalid(S, eng48.ddc_squelch_demod_resample_host, first, dd.CS8)
    eng.set_squelch(**dict(sq_cfg, max_in=1638))
    invalid(S, eng.ddc_squelch_demod, first, dd.CS8)  # max_in below the DDC's cap
    eng.set_squelch(**sq_cfg)
    eng.set_demod(off=True)
    invalid(S, eng.ddc_squelch_demod, first, dd.CS8)
    eng.set_demod(**demod_cfg)
    assert [eng.ddc_config()["samples_consumed"], eng.squelch_config()["samples_consumed"],
            eng.demod_config()["samples_consumed"]] == [0, 0, 0]
    eng48.set_squelch(**sq_cfg)

    d, q, c = eng.demod_config(), eng.squelch_config(), eng48.resample_config()
    taps, tab, inc = S.ddc_design(fs, **ddc_cfg), S.nco_tables(), eng.ddc_config()["nco_increment"]
    ddc_model = dd.Ddc(B, taps, tab, inc, 10)
    gate_model = sq.Squelch(B, q["open_thr"], q["close_thr"], q["beta"], 64, 2)
    demod_model = dm.Demod(B, d["mode"], d["kf"], d["alpha"], d["a"], d["taps"], 4, d["gain"], dm.OUT_F32, 1639)
    rs_model = rs.Resampler(B, 24, 25, c["taps"], c["gain"], rs.OUT_F32, 1, 410)
    opens = []
    for f in range(frames):
        part = raw[:, 2 * n * f:2 * n * (f + 1)]
        got, rec = eng.ddc_squelch_demod(part, dd.CS8)
        got48, rec48 = eng48.ddc_squelch_demod_resample_host(part, dd.CS8)
        chan, n_chan = ddc_model.call(dd.CS8, part)
        gated, want_rec, _ = gate_model.call(chan[:, :n_chan])
        want, want_n = demod_model.call(gated)
        assert got.dtype == np.float32 and got.shape == (B, want_n) and got.tobytes() == want[:, :want_n].tobytes(), f
        assert rec.tobytes() == want_rec.tobytes() and rec48.tobytes() == want_rec.tobytes(), f
        want48, want48_n = rs_model.call(want[:, :want_n])
        assert got48.shape == (B, want48_n) and got48.tobytes() == want48[:, :want48_n].tobytes(), f
        opens.append(rec["open"].tolist())
        if f == 0:  # no carrier yet: silence, in both detectors' sense +0, not noise at full scale
            assert not got.view(np.uint32).any() and not got48.view(np.uint32).any() and np.all(rec["level_db"] < -30.0)
        if f >= 2:
            assert np.abs(got).max() > 0.3 and np.all(rec["level_db"] > -9.0)
    assert opens == [[0] * B, [1] * B, [1] * B, [1] * B]
    assert eng.squelch_config()["samples_consumed"] == gate_model.g == eng48.squelch_config()["samples_consumed"]
    # the chain without the squelch, on the same engine: the squelch neither gates nor moves
    extra = raw[:, :2 * n]
    got = eng.ddc_demod(extra, dd.CS8)
    chan, n_chan = ddc_model.call(dd.CS8, extra)
    want, want_n = demod_model.call(chan[:, :n_chan])
    assert got.tobytes() == want[:, :want_n].tobytes() and np.abs(got).max() > 0.05  # noise alone, and loud
    assert eng.squelch_config()["samples_consumed"] == gate_model.g
    eng.set_squelch(off=True)
    invalid(S, eng.ddc_squelch_demod, extra, dd.CS8)
    eng.close()
    eng48.close()
