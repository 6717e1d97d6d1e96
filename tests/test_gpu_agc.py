"""GPU tests of the AGC stage (csrc/agc.hip, sdrg_engine_agc_*, sdrg_engine_listen_host): the levelled channel and the
records of each stream against the NumPy restatement in tests/agc_cases.py fed the library's own design values.  Every
comparison is of the bytes of the whole `out` and of the records (the stage is specified operation by operation: no
tolerances), except the behavioural case at the end, which holds the settled output level against
agc_cases.error_bound.  `out` and `records` are pre-filled with 0xAA between 64 guard bytes on either side, every stream
has its own data, and the input rows hold NaN past the call's n samples.

The power kernel works in tiles of `tile` positions counted from the start of the block in progress, the apply kernel in
tiles of `tile` samples of the call (sdrg.agc_geometry), blocks above 128 samples meet in LDS, and rows or offsets that
are not 16-byte aligned take 8-byte loads: the shapes below put data on each of these paths and seams."""
import ctypes
import math

import numpy as np
import pytest

import agc_cases as ag
import ddc_cases as dd
import demod_cases as dm
import resample_cases as rs
import squelch_cases as sq
from stage_harness import GUARD, BlockRig, engine, invalid, out_buffer, read_out, rows_bytes, same, to_device

pytestmark = pytest.mark.gpu

BASE = dict(target=0.25, max_gain_db=40.0, initial_gain_db=0.0, floor_db=-30.0, attack_blocks=0.0, decay_blocks=2.0,
            detector=ag.MEAN, block=64, hang_blocks=1, max_in=1024)
PATTERN = (1, 1, 0, 0, 0, 1, 0, 1, 1, 1, 0, 0)  # loud and quiet blocks: attacks, the hang used up and reloaded, decays
QUIET = 0.05  # the quiet blocks are 26 dB down: above BASE's floor


@pytest.fixture(scope="module")
def S():
    import sdrg
    return sdrg


@pytest.fixture(scope="module")
def T():
    import torch
    return torch


def levels(B, n, seed, block=64, pattern=PATTERN, quiet=QUIET):
    return ag.levels(B, n, seed, block, pattern, quiet=quiet)


class Leveller(BlockRig):
    """An engine with the AGC set, and the restatement that follows it call by call."""
    stage = "agc"
    record = "AGC_RECORD_DTYPE"

    def make_model(self, d):
        des = self.S.agc_design(**self.cfg)
        assert all(des[k].tobytes() == d[k].tobytes() for k in ag.DESIGN)
        return ag.Agc(self.B, d["target"], des, d["block"], d["hang_blocks"], d["detector"])

    def restart(self):
        self.eng.agc_reset()
        self.model.reset()


@pytest.mark.parametrize("B", [1, 9, 65, 130])
def test_stream_counts(S, T, B):
    """The step kernel takes 64 streams per wave: a wave in part, a wave and a stream, two waves and two streams."""
    n = 5 * 64 + 9
    g = Leveller(S, T, B, **BASE)
    z = levels(B, 3 * n, 20)
    attacks = 0
    for f in range(3):
        _, rec, nb = g.check(z[:, f * n:(f + 1) * n], (B, f))
        attacks += int(rec["attacks"].sum())
    assert attacks > B
    g.close()


@pytest.mark.parametrize("detector", [ag.MEAN, ag.PEAK])
@pytest.mark.parametrize("block", [16, 64, 256, 512, 1024])
def test_calls_around_the_block(S, T, block, detector):
    """n = 0, 1, S - 1, S, S + 1, 2 S - 1 in one stream, for every width of the butterfly, adding and taking the maximum:
    in a wave (S <= 128), across the waves through LDS (256, 512), and across the workgroup's two passes (1024)."""
    B = 3
    g = Leveller(S, T, B, **dict(BASE, block=block, max_in=2 * block, detector=detector))
    ns = (block + 1, 0, 1, block - 1, 0, block, block + 1, 2 * block - 1, 1, 2 * block, 0)
    z = levels(B, sum(ns), 30 + block, block, (1, 0, 1, 1, 0, 0))
    at, blocks = 0, 0
    for f, n in enumerate(ns):
        got, rec, nb = g.check(z[:, at:at + n], (block, f, n))
        at, blocks = at + n, blocks + nb
        if n == 0:
            assert nb == 0 and not got.view(np.uint32).any() and not rec["attacks"].any()
    assert blocks == sum(ns) // block and g.model.g == sum(ns)
    g.close()


def test_first_call_without_samples(S, T):
    B = 2
    g = Leveller(S, T, B, **dict(BASE, initial_gain_db=-6.0))
    got, rec, nb = g.check(np.zeros((B, 0), np.complex64))
    assert nb == 0 and got.shape == (B, 1024) and not got.view(np.uint32).any()
    assert np.all(rec["gain"] == g.model.init_gain) and not rec["attacks"].any()
    g.check(levels(B, 300, 35))
    g.close()


def test_a_stream_cut_at_every_offset_of_a_block(S, T):
    """S = 16: after a first call of `off` samples the next starts at every in-block offset, odd (8-byte loads in the
    power kernel) and even, and three calls share a block."""
    B, block = 3, 16
    g = Leveller(S, T, B, **dict(BASE, block=block, max_in=64))
    z = levels(B, 16 + 3 + 45, 40, block, (1, 0, 1, 0, 0, 1))
    for off in range(block):
        g.restart()
        at = 0
        for n in (off, 3, 45):
            g.check(z[:, at:at + n], (off, n))
            at += n
    g.close()


def test_five_calls_are_one_stream(S, T):
    B = 4
    cfg = dict(BASE, attack_blocks=0.5, hang_blocks=2)
    g = Leveller(S, T, B, **cfg)
    ns = (700, 64, 1, 1024, 333)
    z = levels(B, sum(ns), 50)
    outs, at = [], 0
    for f, n in enumerate(ns):
        got, rec, _ = g.check(z[:, at:at + n], f)
        outs.append(got[:, :n])
        at += n
    want, want_rec, _ = ag.one_call(z, cfg["target"], S.agc_design(**cfg), 64, 2)
    assert np.concatenate(outs, axis=1).tobytes() == want.tobytes()
    for k in ("gain", "gain_db", "level_db"):
        assert rec[k].tobytes() == want_rec[k].tobytes()
    g.close()


@pytest.mark.parametrize("block", [16, 256, 1024])
def test_every_workgroup_seam(S, T, block):
    """A call over three seams and a bit, started 5 samples (8-byte loads) and 6 samples (16-byte loads) into a block:
    the power kernel's tiles start at the multiples of `tile` counted from the block's start, the apply kernel's at the
    multiples of `tile` in the call."""
    B, tile = 2, S.agc_geometry(block)
    n = 3 * tile + 7
    g = Leveller(S, T, B, **dict(BASE, block=block, max_in=n + 1))
    for off in (5, 6):
        g.restart()
        z = levels(B, off + 2 * n, 60 + off, block, (1, 1, 0, 1, 0, 0, 0))
        g.check(z[:, :off], (block, off, "head"))
        got, _, _ = g.check(z[:, off:off + n], (block, off, "first"), in_stride=n + 1)
        assert np.abs(got[:, :n]).max() > 0.1
        g.check(z[:, off + n:], (block, off, "second"), in_stride=n)
    g.close()


def test_row_strides_and_alignments(S, T):
    """in_stride above n, even and odd (odd rows are not 16-byte aligned), and chan and out 8 bytes off alignment."""
    B, n = 3, 333
    g = Leveller(S, T, B, **BASE)
    z = levels(B, 6 * n, 70)
    for f, (stride, shift) in enumerate(((1024, 0), (n, 0), (n + 1, 0), (n + 4, 8), (1000, 8), (n, 8))):
        got, _, _ = g.check(z[:, f * n:(f + 1) * n], (stride, shift), in_stride=stride, shift=shift)
        assert not got[:, n:].view(np.uint32).any()
    g.close()


def test_in_place_equals_out_of_place(S, T):
    B, n = 5, 900
    a, b = Leveller(S, T, B, **BASE), Leveller(S, T, B, **BASE)
    z = levels(B, 3 * n, 80)
    for f, stride in enumerate((1024, n + 1, n)):
        part = z[:, f * n:(f + 1) * n]
        out_a, rec_a, _ = a.check(part, (f, "out of place"), in_stride=stride)
        out_b, rec_b, _ = b.check(part, (f, "in place"), in_stride=stride, in_place=True)
        assert out_a.tobytes() == out_b.tobytes() and rec_a.tobytes() == rec_b.tobytes()
    a.close()
    b.close()


@pytest.mark.parametrize("detector", [ag.MEAN, ag.PEAK])
@pytest.mark.parametrize("attack,decay", [(0.0, 0.0), (0.0, 3.0), (1.5, 0.0), (1.5, 3.0)])
def test_the_law_within_a_call_and_across_calls(S, T, detector, attack, decay):
    """Both detectors with alpha = 1 and alpha < 1 for each of attack and decay; the hang (2 blocks) within a call, and
    then, with the same stream in calls of one block, across calls: each call's record is the gain the block after the
    next will end on."""
    B, block, H = 2, 16, 2
    cfg = dict(BASE, block=block, hang_blocks=H, attack_blocks=attack, decay_blocks=decay, detector=detector, max_in=512)
    g = Leveller(S, T, B, **cfg)
    amps = [1, 1.25, 1.5] + [0.1] * 6 + [1, 2, 0.1, 3] + [0.1] * 6
    phase = np.random.default_rng(90).uniform(0, 2 * np.pi, (B, block * len(amps)))  # a constant envelope per block:
    z = (np.exp(1j * phase) * np.repeat(np.array(amps), block)[None, :]).astype(np.complex64)  # mean and peak are amp^2
    got, rec, nb = g.check(z, "one call")
    whole = got[:, :z.shape[1]].copy()
    gains = np.array(g.model.gains)  # [block][B]
    # each louder block attacks (0, 1, 2, 9, 10, 12), and at alpha_d = 1 a quiet block whose statistic is an ulp above the
    # one before it; the quiet blocks after a loud one hold for H blocks, then rise
    assert nb == len(amps) and np.all(rec["attacks"] >= 6)
    assert np.all(gains[3] == gains[2]) and np.all(gains[4] == gains[2]) and np.all(gains[5] > gains[4])
    g.restart()
    for j in range(len(amps)):
        got, rec, nb = g.check(z[:, j * block:(j + 1) * block], ("block", j))
        assert nb == 1 and got[:, :block].tobytes() == whole[:, j * block:(j + 1) * block].tobytes()
        assert rec["gain"].tobytes() == gains[j].astype(np.float32).tobytes()
    g.close()


def test_floor_held_blocks_across_a_call_boundary(S, T):
    """A loud stretch, then blocks under the floor (and blocks of zeros, as a closed squelch leaves them) that run over
    three calls, one of them inside a block: the gain stays where the loud stretch left it, and the first loud sample
    after the gap comes out at that gain, not at max_gain."""
    B, block = 3, 16
    g = Leveller(S, T, B, **dict(BASE, block=block, hang_blocks=0, decay_blocks=0.0, max_in=256))
    z = sq.noise(B, 14 * block, 95)
    z[:, 3 * block:7 * block] *= np.float32(0.01)  # 40 dB down: under the floor of -30 dB
    z[:, 7 * block:11 * block] = 0
    _, rec, _ = g.check(z[:, :3 * block], "loud")
    held = rec["gain"].copy()
    for a, b in ((3 * block, 5 * block + 7), (5 * block + 7, 5 * block + 9), (5 * block + 9, 11 * block)):
        _, rec, _ = g.check(z[:, a:b], ("held", a))
        assert rec["gain"].tobytes() == held.tobytes() and not rec["attacks"].any()
    assert np.all(rec["level_db"] < -199.0)
    got, rec, nb = g.check(z[:, 11 * block:], "loud again")
    w = np.abs(got[:, 0]) / np.abs(z[:, 11 * block])
    assert nb == 3 and np.all(np.abs(w / held - 1) < 1e-6) and np.all(held < 2.0) and g.model.max_gain == np.float32(100.0)
    g.close()


def test_max_gain_reached(S, T):
    B = 3
    g = Leveller(S, T, B, **dict(BASE, max_gain_db=20.0, floor_db=-math.inf, decay_blocks=0.0))
    z = (sq.noise(B, 1024, 97) * np.float32(1e-3)).astype(np.complex64)
    z[:, 512:576] = 0  # a block of zeros: a = 0 gives max_gain as well
    _, rec, _ = g.check(z)
    assert np.all(rec["gain"] == np.float32(10.0)) and np.all(np.abs(rec["gain_db"] - 20.0) < 2e-6)
    assert all(np.all(x == np.float32(10.0)) for x in g.model.gains)
    g.close()


def test_powers_down_to_denormal(S, T):
    """Amplitudes of 1e-21: every power is a denormal float, and so is the floor; a flushed power would read 0 and give
    max_gain, and a flushed floor would hold nothing."""
    B, block = 3, 64
    cfg = dict(BASE, target=1e-21, floor_db=-431.0, max_gain_db=40.0, decay_blocks=1.5, max_in=1024)
    g = Leveller(S, T, B, **cfg)
    assert 0 < g.model.floor_thr < np.float32(1.2e-38)
    z = (levels(B, 2048, 100, quiet=0.03).astype(np.complex128) * 1e-21).astype(np.complex64)
    attacks = 0
    for f in range(2):
        got, rec, _ = g.check(z[:, f * 1024:(f + 1) * 1024], f)
        assert np.all(g.model.Pl > 0) and np.all(g.model.Pl < np.float32(1.2e-38)) and np.all(rec["gain"] < 100.0)
        attacks += int(rec["attacks"].sum())
    assert attacks > B and np.abs(got).max() > 1e-22
    held = [k for k in range(1, len(g.model.gains)) if np.any(g.model.gains[k] == g.model.gains[k - 1])]
    assert held  # the quiet blocks (9e-46) are under the floor (7.9e-44)
    g.close()


def test_many_streams_long_rows(S, T):
    B, n = 64, 16384
    g = Leveller(S, T, B, **dict(BASE, attack_blocks=0.7, hang_blocks=1, max_in=n))
    z = levels(B, n + 100, 110)
    g.check(z[:, :100], "head")
    _, rec, nb = g.check(z[:, 100:], "64 x 16384")
    assert nb == 256 and 0 < rec["attacks"].min() and rec["attacks"].max() < 256
    g.close()


def test_the_most_blocks_a_call_completes(S, T):
    """S = 16 and a call that starts on a block's last sample: max_in / 16 + 1 blocks, the whole block scratch."""
    B, n = 2, 4096
    g = Leveller(S, T, B, **dict(BASE, block=16, max_in=n))
    z = levels(B, 15 + n, 115, 16)
    g.check(z[:, :15])
    _, _, nb = g.check(z[:, 15:], "starts on a block's last sample")
    assert nb == 256 == (15 + n) // 16
    g.close()


def test_without_records(S, T):
    B, n = 3, 500
    g = Leveller(S, T, B, **BASE)
    z = levels(B, 3 * n, 120)
    g.check(z[:, :n], "no records", records=False)
    g.check(np.zeros((B, 0), np.complex64), "no records, no samples", records=False)
    g.check(z[:, n:2 * n], "records again")
    g.check(z[:, 2 * n:], "no records, in place", records=False, in_place=True)
    g.close()


def test_reset_and_set_again_between_calls(S, T):
    B, n = 3, 700
    g = Leveller(S, T, B, **BASE)
    z = levels(B, n, 130, pattern=(1, 1, 1, 0))
    _, first, _ = g.check(z)
    g.check(z, "a second call goes on from the first")
    g.restart()
    assert g.eng.agc_config()["samples_consumed"] == 0
    _, again, _ = g.check(z, "after the reset")
    assert again.tobytes() == first.tobytes()
    g.configure(**dict(BASE, block=128, hang_blocks=0, decay_blocks=4.0, detector=ag.PEAK))
    g.check(z[:, :300], "another configuration")
    invalid(S, g.eng.set_agc, **dict(BASE, block=100))  # rejected: the configuration and the state stay
    assert g.eng.agc_config()["samples_consumed"] == 300 and g.eng.agc_config()["block"] == 128
    g.check(z[:, 300:], "after a rejected set_agc")
    g.configure(**BASE)  # the same configuration again restarts as well
    _, third, _ = g.check(z, "set again")
    assert third.tobytes() == first.tobytes()
    g.close()


def test_refusals_write_nothing_and_commit_nothing(S, T):
    B, n = 2, 300
    eng = engine(S, B)
    z = levels(B, n, 140)
    chan_t = to_device(T, rows_bytes(z, 1024))
    out_t, rec_t = out_buffer(T, B * 1024 * 8), out_buffer(T, B * 16)
    T.cuda.synchronize()
    args = (chan_t.data_ptr(), 1024, n, out_t.data_ptr() + GUARD, rec_t.data_ptr() + GUARD)
    invalid(S, eng.agc_device, *args)  # before any set_agc
    invalid(S, eng.agc_config)
    eng.close()

    g = Leveller(S, T, B, **BASE)
    g.check(z)
    for stride, bad_n in ((1024, 1025), (1024, -1), (1025, n), (n - 1, n), (0, 0), (1024, 1 << 30), (-5, -5)):
        invalid(S, g.eng.agc_device, chan_t.data_ptr(), stride, bad_n, out_t.data_ptr() + GUARD, rec_t.data_ptr() + GUARD)
    L = S.load()
    nb = ctypes.c_int32(-7)
    h, c, o = g.eng._h, chan_t.data_ptr(), out_t.data_ptr() + GUARD
    assert L.sdrg_engine_agc_device(h, None, 1024, n, o, None, ctypes.byref(nb)) == -1
    assert L.sdrg_engine_agc_device(h, c, 1024, n, None, None, ctypes.byref(nb)) == -1
    assert L.sdrg_engine_agc_device(h, c, 1024, n, o, None, None) == -1
    assert L.sdrg_engine_agc_device(None, c, 1024, n, o, None, ctypes.byref(nb)) == -1
    assert nb.value == -7 and g.eng.agc_config()["samples_consumed"] == n
    g.check(levels(B, n, 141), "after refused calls")
    g.eng.set_agc(off=True)
    invalid(S, g.eng.agc_device, *args)
    g.eng.synchronize()
    assert np.all(out_t.cpu().numpy() == 0xAA) and np.all(rec_t.cpu().numpy() == 0xAA), "a refused call wrote"
    g.configure(**BASE)
    g.check(levels(B, n, 142), "after off and on")
    g.close()


def test_host_path_equals_device_path(S, T):
    B, n = 5, 777
    dev = Leveller(S, T, B, **BASE)
    host = engine(S, B)
    host.set_agc(**BASE)
    z = levels(B, 3 * n, 150)
    for f in range(3):
        part = z[:, f * n:(f + 1) * n - 100 * f]
        got, rec, nb = dev.check(part, f, in_stride=part.shape[1])
        h_out, h_rec, h_nb = host.agc_host(part)
        assert h_out.dtype == np.complex64 and h_out.tobytes() == got.tobytes() and h_nb == nb
        assert h_rec.tobytes() == rec.tobytes()
    h_out, h_rec, h_nb = host.agc_host(np.zeros((B, 0), np.complex64))
    assert h_out.shape == (B, 0) and h_nb == 0 and h_rec["gain"].tobytes() == rec["gain"].tobytes()
    h_out, none, _ = host.agc_host(z[:, :64], want_records=False)
    assert none is None and h_out.shape == (B, 64)
    with pytest.raises(S.SdrgError):
        host.agc_host(np.zeros((B, 1025), np.complex64))
    dev.close()
    host.close()


def test_process_device_and_squelch_device_between_agc_calls(S, T):
    """agc, process_device, squelch_device, agc, ...: the levelled rows are the restatement's, the gated rows the
    squelch's restatement's, and the spectra, records and PCM are those of an engine that configured neither stage."""
    n, B, fmt = 16384, 4, dd.CS8
    stages = S.STAGE_SPECTRUM | S.STAGE_STATS | S.STAGE_SSB
    raws = [dd.tone(fmt, B, n, 0.01 + 0.001 * f, amp=0.4) for f in range(2)]
    sq_cfg = dict(open_db=-3.0, close_db=-9.0, tau_blocks=0.0, block=64, hang_blocks=1, max_in=1024)

    def process(eng, f):
        iq_t = T.from_numpy(raws[f]).to("cuda:0")
        spec = T.zeros((B, n), dtype=T.float32, device="cuda:0")
        rec = T.zeros((B * S.RECORD_DTYPE.itemsize,), dtype=T.uint8, device="cuda:0")
        pcm = T.zeros((B, max(eng.pcm_len, 1)), dtype=T.int16, device="cuda:0")
        T.cuda.synchronize()
        eng.process_device(iq_t.data_ptr(), fmt, stages, spec.data_ptr(), rec.data_ptr(), pcm.data_ptr(), 1000 + f)
        return iq_t, spec, rec, pcm

    g = Leveller(S, T, B, n, **BASE)
    g.eng.set_squelch(**sq_cfg)
    d = g.eng.squelch_config()
    gate_model = sq.Squelch(B, d["open_thr"], d["close_thr"], d["beta"], 64, 1)
    plain = engine(S, B, n)
    chans = [sq.keyed(B, 900 + f, 160 + f, 64, PATTERN, quiet=QUIET) for f in range(3)]
    held, outs, gated = [], [], []
    for f in range(3):
        chan_t = to_device(T, rows_bytes(chans[f], 1024))
        out_t, rec_t = out_buffer(T, B * 1024 * 8), out_buffer(T, B * 16)
        T.cuda.synchronize()
        nb = g.eng.agc_device(chan_t.data_ptr(), 1024, chans[f].shape[1], out_t.data_ptr() + GUARD,
                              rec_t.data_ptr() + GUARD)
        outs.append((out_t, rec_t, nb, chan_t))
        if f < 2:
            held.append((process(g.eng, f), process(plain, f)))
            q_t, qr_t = out_buffer(T, B * 1024 * 8), out_buffer(T, B * 16)
            T.cuda.synchronize()
            gated.append((q_t, qr_t, g.eng.squelch_device(chan_t.data_ptr(), 1024, chans[f].shape[1],
                                                          q_t.data_ptr() + GUARD, qr_t.data_ptr() + GUARD)))
    g.eng.synchronize()
    plain.synchronize()
    for f, (out_t, rec_t, nb, _) in enumerate(outs):
        want, want_rec, want_nb = g.model.call(chans[f], in_stride=1024)
        same(read_out(out_t, (B, 1024), np.complex64), nb, want, want_nb, f)
        same(read_out(rec_t, (B, 4), np.uint32), nb, want_rec.view(np.uint32).reshape(B, 4), want_nb, (f, "records"))
    for f, (q_t, qr_t, nb) in enumerate(gated):
        want, want_rec, want_nb = gate_model.call(chans[f], in_stride=1024)
        same(read_out(q_t, (B, 1024), np.complex64), nb, want, want_nb, (f, "squelch"))
        same(read_out(qr_t, (B, 4), np.uint32), nb, want_rec.view(np.uint32).reshape(B, 4), want_nb, (f, "squelch records"))
    for f, (a, b) in enumerate(held):
        for x, y, name in zip(a[1:], b[1:], ("spectra", "records", "pcm")):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), (f, name)
    assert held[0][0][1].cpu().numpy().max() > 0
    g.close()
    plain.close()


# ---- sdrg_engine_listen_host: fs = 2 MHz, N = 4096, CS8 noise of 3 LSB rms; from the middle of the second frame an AM
# carrier at +250 kHz, modulated 50 % by a 2 kHz tone.  DDC D = 10, T = 63 (cap 410); squelch and AGC S = 16; AM demodulator
# R = 4, T2 = 31, float; resampler 24 / 25.

LISTEN_FS, LISTEN_N, LISTEN_B, LISTEN_FRAMES, LISTEN_CAP = 2_000_000, 4096, 2, 4, 410
DDC_CFG = dict(offset_hz=250_000.0, cutoff_hz=60_000.0, decimation=10, taps=63)
DEMOD_CFG = dict(mode=dm.AM, channel_rate_hz=200_000.0, deviation_hz=0.0, dc_cutoff_hz=100.0, deemphasis_us=0.0,
                 audio_decimation=4, audio_taps=31, audio_cutoff_hz=15_000.0, gain=1.0, out_format=dm.OUT_F32,
                 max_in=LISTEN_CAP)
SQ_CFG = dict(open_db=-12.0, close_db=-18.0, tau_blocks=1.0, block=16, hang_blocks=2, max_in=LISTEN_CAP)
AGC_CFG = dict(target=0.5, max_gain_db=30.0, initial_gain_db=0.0, floor_db=-40.0, attack_blocks=0.0, decay_blocks=3.0,
               detector=ag.MEAN, block=16, hang_blocks=1, max_in=LISTEN_CAP)
RS_CFG = dict(interp=24, decim=25, taps_per_phase=8, cutoff_rel=0.9, components=1, out_format=rs.OUT_F32, gain=1.0,
              max_in=103)


@pytest.fixture(scope="module")
def keyed_am():
    """(raw CS8 [B][2 N frames], the DDC's restated channel of every frame [(chan, n_chan)]): computed once."""
    fs, n, B, frames = LISTEN_FS, LISTEN_N, LISTEN_B, LISTEN_FRAMES
    t = np.arange(frames * n, dtype=np.float64)
    rng = np.random.default_rng(3)
    raw = np.empty((B, 2 * frames * n), np.int8)
    key = n + n // 2
    for b in range(B):
        env = 0.3 * (1 + b) * (1.0 + 0.5 * np.cos(2 * np.pi * 2000.0 * t / fs + 0.7 * b))
        z = (t >= key) * env * np.exp(2j * np.pi * 250_000.0 * t / fs + 0.3j * b)
        z = z + (3 / 128) * (rng.standard_normal(t.size) + 1j * rng.standard_normal(t.size))
        raw[b, 0::2] = np.round(z.real * 128).clip(-128, 127).astype(np.int8)
        raw[b, 1::2] = np.round(z.imag * 128).clip(-128, 127).astype(np.int8)
    return raw


def listen_engine(S, steps, every_stage=False):
    eng = engine(S, LISTEN_B, LISTEN_N, LISTEN_FS)
    eng.set_ddc(**DDC_CFG)
    eng.set_demod(**DEMOD_CFG)
    if every_stage or steps & S.LISTEN_SQUELCH:
        eng.set_squelch(**SQ_CFG)
    if every_stage or steps & S.LISTEN_AGC:
        eng.set_agc(**AGC_CFG)
    if every_stage or steps & S.LISTEN_RESAMPLE:
        eng.set_resample(**RS_CFG)
    return eng


@pytest.fixture(scope="module")
def ddc_restated(S, T, keyed_am):
    """The DDC's restatement of every frame, which every mask shares: [(chan [B][cap], n_chan)]."""
    eng = listen_engine(S, 0)
    taps, tab, inc = S.ddc_design(LISTEN_FS, **DDC_CFG), S.nco_tables(), eng.ddc_config()["nco_increment"]
    assert eng.ddc_max_out() == LISTEN_CAP
    eng.close()
    model = dd.Ddc(LISTEN_B, taps, tab, inc, 10)
    n = LISTEN_N
    return [model.call(dd.CS8, keyed_am[:, 2 * n * f:2 * n * (f + 1)]) for f in range(LISTEN_FRAMES)]


@pytest.mark.parametrize("steps", range(8))
def test_listen_equals_the_restatements_chained(S, T, keyed_am, ddc_restated, steps):
    B, n = LISTEN_B, LISTEN_N
    eng = listen_engine(S, steps, every_stage=True)  # every stage set: the mask alone decides which run
    d, q, c = eng.demod_config(), eng.squelch_config(), eng.resample_config()
    gate = sq.Squelch(B, q["open_thr"], q["close_thr"], q["beta"], 16, 2)
    agc = ag.Agc(B, AGC_CFG["target"], S.agc_design(**AGC_CFG), 16, 1)
    demod = dm.Demod(B, d["mode"], d["kf"], d["alpha"], d["a"], d["taps"], 4, d["gain"], dm.OUT_F32, LISTEN_CAP)
    rsm = rs.Resampler(B, 24, 25, c["taps"], c["gain"], rs.OUT_F32, 1, 103)
    opened, gains = [], []
    for f in range(LISTEN_FRAMES):
        got, sq_rec, agc_rec = eng.listen(keyed_am[:, 2 * n * f:2 * n * (f + 1)], dd.CS8, steps)
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
        want, want_n = demod.call(chan)
        want = want[:, :want_n]
        if steps & S.LISTEN_RESAMPLE:
            want, want_n = rsm.call(want)
            want = want[:, :want_n]
        assert got.dtype == np.float32 and got.shape == want.shape and got.tobytes() == want.tobytes(), f
    g = [eng.ddc_config()["samples_consumed"], eng.squelch_config()["samples_consumed"],
         eng.agc_config()["samples_consumed"], eng.demod_config()["samples_consumed"]]
    assert g == [LISTEN_FRAMES * n, gate.g, agc.g, demod_consumed(ddc_restated)]
    if steps & S.LISTEN_SQUELCH:
        assert opened[0] == [0] * B and opened[-1] == [1] * B
    if steps & S.LISTEN_AGC:
        assert gains[-1][1] < gains[-1][0]  # the stronger carrier ends on the smaller gain
    eng.close()


def demod_consumed(ddc_restated):
    return sum(n_chan for _, n_chan in ddc_restated)


@pytest.mark.parametrize("steps", [0, 1, 4, 5])
def test_listen_without_the_agc_equals_the_existing_chain_calls(S, T, keyed_am, steps):
    n = LISTEN_N
    a, b = listen_engine(S, steps, every_stage=True), listen_engine(S, steps)
    old = {0: b.ddc_demod, 4: b.ddc_demod_resample_host, 1: b.ddc_squelch_demod, 5: b.ddc_squelch_demod_resample_host}
    for f in range(LISTEN_FRAMES):
        part = keyed_am[:, 2 * n * f:2 * n * (f + 1)]
        got, sq_rec, agc_rec = a.listen(part, dd.CS8, steps)
        want = old[steps](part, dd.CS8)
        if steps & S.LISTEN_SQUELCH:
            want, want_rec = want
            assert sq_rec.tobytes() == want_rec.tobytes(), f
        assert agc_rec is None and got.shape == want.shape and got.tobytes() == want.tobytes(), f
    assert a.agc_config()["samples_consumed"] == 0  # set, and not in the mask: it neither levels nor moves
    a.close()
    b.close()


def test_listen_refusals(S, T, keyed_am):
    """Each stage off while in the mask, each max_in below the DDC's cap, unknown bits, null pointers: SDRG_E_INVALID, and
    no stage has moved."""
    first = keyed_am[:, :2 * LISTEN_N]
    ALL = S.LISTEN_SQUELCH | S.LISTEN_AGC | S.LISTEN_RESAMPLE
    eng = listen_engine(S, ALL)
    sets = dict(ddc=(eng.set_ddc, DDC_CFG), demod=(eng.set_demod, DEMOD_CFG), squelch=(eng.set_squelch, SQ_CFG),
                agc=(eng.set_agc, AGC_CFG), resample=(eng.set_resample, RS_CFG))
    for name, (setter, cfg) in sets.items():
        setter(off=True)
        invalid(S, eng.listen, first, dd.CS8, ALL)
        setter(**cfg)
    for name in ("demod", "squelch", "agc"):
        setter, cfg = sets[name]
        setter(**dict(cfg, max_in=LISTEN_CAP - 1))
        invalid(S, eng.listen, first, dd.CS8, ALL)
        setter(**cfg)
    eng.set_resample(**dict(RS_CFG, max_in=102))
    invalid(S, eng.listen, first, dd.CS8, ALL)
    eng.set_resample(**RS_CFG)
    # a stage that is off and not in the mask does not matter
    eng.set_agc(off=True)
    got, sq_rec, agc_rec = eng.listen(first, dd.CS8, S.LISTEN_SQUELCH)
    assert agc_rec is None and sq_rec is not None
    eng.set_agc(**AGC_CFG)
    consumed = lambda: [eng.ddc_config()["samples_consumed"], eng.squelch_config()["samples_consumed"],  # noqa: E731
                        eng.agc_config()["samples_consumed"], eng.demod_config()["samples_consumed"],
                        eng.resample_config()["samples_consumed"]]
    before = consumed()
    L, n_out = S.load(), ctypes.c_int32(-7)
    out = np.full((LISTEN_B, 128), 7.0, np.float32)
    iq_p, out_p = first.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)
    for bad in (8, 16, -1, ALL | 64):
        assert L.sdrg_engine_listen_host(eng._h, bad, iq_p, dd.CS8, out_p, ctypes.byref(n_out), None, None) == -1
    assert L.sdrg_engine_listen_host(eng._h, ALL, None, dd.CS8, out_p, ctypes.byref(n_out), None, None) == -1
    assert L.sdrg_engine_listen_host(eng._h, ALL, iq_p, dd.CS8, None, ctypes.byref(n_out), None, None) == -1
    assert L.sdrg_engine_listen_host(eng._h, ALL, iq_p, dd.CS8, out_p, None, None, None) == -1
    assert L.sdrg_engine_listen_host(None, ALL, iq_p, dd.CS8, out_p, ctypes.byref(n_out), None, None) == -1
    assert L.sdrg_engine_listen_host(eng._h, ALL, iq_p, 99, out_p, ctypes.byref(n_out), None, None) == -1
    assert n_out.value == -7 and np.all(out == 7.0) and consumed() == before
    # records are optional, each on its own
    agc_only = np.zeros(LISTEN_B, S.AGC_RECORD_DTYPE)
    assert L.sdrg_engine_listen_host(eng._h, ALL, iq_p, dd.CS8, out_p, ctypes.byref(n_out), None,
                                     agc_only.ctypes.data_as(ctypes.c_void_p)) == 0
    assert n_out.value > 0 and np.all(agc_only["gain"] > 0)
    assert L.sdrg_engine_listen_host(eng._h, ALL, iq_p, dd.CS8, out_p, ctypes.byref(n_out), None, None) == 0
    eng.close()


def test_two_am_channels_30_db_apart_come_out_at_the_target(S, T):
    """The behavioural case of tests/test_agc_cases.py on the device: 2 streams x 64 blocks of S = 64, carriers 30 dB
    apart.  From the block agc_cases.settling_blocks names, each output block's RMS is within agc_cases.error_bound of
    the target (measured: 5.0e-5 against a bound of 2.5e-4, the bytes being the restatement's)."""
    z, d, first, bound = ag.am_case(S)
    g = Leveller(S, T, ag.AM["B"], **ag.AM["cfg"])
    got, rec, nb = g.check(z, "two AM channels")
    rms = ag.block_rms(got, ag.AM["S"])
    dist = np.abs(rms[:, first:] - ag.AM["target"]).max()
    print("settled from block", first, "distance", dist, "bound", bound)
    assert nb == ag.AM["blocks"] and dist <= bound, (dist, bound)
    rms_in = ag.block_rms(z, ag.AM["S"])
    assert rms_in[0, -1] / rms_in[1, -1] > 31.0 and abs(rms[0, -1] / rms[1, -1] - 1) < 1e-3
    g.close()
