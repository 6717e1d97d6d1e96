"""GPU tests of the AFC stage (csrc/afc.hip, sdrg_engine_afc_*, sdrg_engine_listen_afc_host): the corrected rows and the
records of each stream against the NumPy restatement in tests/afc_cases.py fed the library's own design values and NCO
tables.  Every comparison is of the bytes of the whole `out` and of the records (the stage is specified operation by
operation: no tolerances).  `out` and `records` are pre-filled with 0xAA between 64 guard bytes on either side, every
stream has its own data, and the input rows hold NaN past the call's n samples.

The moments kernel works in tiles of `tile` positions counted from the start of the block in progress, the pass kernel in
runs of four tiles of `tile` samples of the call (sdrg.afc_geometry); blocks up to 128 samples are summed inside a wave, larger ones
meet in LDS, and a block of 1024 takes a workgroup's two passes; a wave's first lane loads the sample before its own
where the other lanes take their neighbour's; rows or offsets that are not aligned to a pair of samples take one-sample
loads and stores: the shapes below put data on each of these paths."""
import ctypes

import numpy as np
import pytest

import afc_cases as af
import ddc_cases as dd
import demod_cases as dm
import resample_cases as rs
import squelch_cases as sq
from stage_harness import GUARD, engine, invalid, out_buffer, read_out, rows_bytes, same, to_device

pytestmark = pytest.mark.gpu

f32 = np.float32
RATE = 48000.0
BASE = dict(channel_rate=RATE, max_offset_hz=5000.0, tau_blocks=3.0, floor_db=-60.0, lock_threshold=0.25, mode=af.TRACK,
            block=64, max_in=2048)


@pytest.fixture(scope="module")
def S():
    import sdrg
    return sdrg


@pytest.fixture(scope="module")
def T():
    import torch
    return torch


def signal(B, n, seed, snr_db=15.0, amp=0.5):
    """Every stream its own carrier, from -4150 Hz up in steps of 700 Hz and around again, under its own noise."""
    rng = np.random.default_rng(seed)
    return np.stack([af.carrier(n, carrier_hz(b), RATE, amp, snr_db, rng, phase=0.3 * b) for b in range(B)])


def carrier_hz(b):
    return -4150.0 + 700.0 * (b % 13)


class Rig:
    """An engine with the stage set, and the restatement that follows it call by call."""

    def __init__(self, S, T, B, n=1024, **cfg):
        self.S, self.T, self.B = S, T, B
        self.eng = engine(S, B, n)
        self.tab = S.nco_tables()
        self.configure(**cfg)

    def configure(self, **cfg):
        self.cfg = cfg
        self.eng.set_afc(**cfg)
        self.remodel()

    def remodel(self):
        d = self.eng.afc_config()
        des = self.S.afc_design(**self.cfg)
        assert all(d[k] == v for k, v in self.cfg.items()), d
        assert all(des[k].tobytes() == d[k].tobytes() for k in des) and d["samples_consumed"] == 0
        self.model = af.Afc(self.B, d, d["block"], self.tab, d["mode"])

    def device_call(self, chan, in_stride=None, records=True, in_place=False, in_shift=0, out_shift=0):
        """afc_device into 0xAA-filled buffers between guard bytes: (out [B][stride] complex64 or None when measuring,
        records [B][8] as uint32 or None, n_blocks).  in_shift, out_shift: bytes by which chan and out are moved off a
        16-byte alignment."""
        T, B = self.T, self.B
        n = chan.shape[1]
        stride = self.cfg["max_in"] if in_stride is None else in_stride
        rows = rows_bytes(chan, stride).view(np.uint8).reshape(-1)
        nbytes = B * stride * 8
        track = self.cfg["mode"] == af.TRACK
        out_t = out_buffer(T, nbytes + out_shift)
        rec_t = out_buffer(T, B * 32)
        at = GUARD + out_shift
        if in_place:
            out_t[at:at + nbytes] = T.from_numpy(rows).to("cuda:0")
            chan_ptr = out_t.data_ptr() + at
        else:
            chan_t = T.zeros((rows.size + in_shift,), dtype=T.uint8, device="cuda:0")
            chan_t[in_shift:] = T.from_numpy(rows).to("cuda:0")
            chan_ptr = chan_t.data_ptr() + in_shift
        T.cuda.synchronize()
        nb = self.eng.afc_device(chan_ptr, stride, n, out_t.data_ptr() + at if track else None,
                                 rec_t.data_ptr() + GUARD if records else None)
        self.eng.synchronize()
        o = out_t.cpu().numpy()
        out = None
        if track:
            assert np.all(o[:at] == 0xAA) and np.all(o[at + nbytes:] == 0xAA), "bytes outside out"
            out = o[at:at + nbytes].copy().view(np.complex64).reshape(B, stride)
        else:
            assert np.all(o == 0xAA), "rows written while measuring"
        if not records:
            assert np.all(rec_t.cpu().numpy() == 0xAA), "records written without a pointer"
            return out, None, nb
        return out, read_out(rec_t, (B, 8), np.uint32), nb

    def check(self, chan, what=None, **kw):
        got, rec, nb = self.device_call(chan, **kw)
        stride = self.cfg["max_in"] if kw.get("in_stride") is None else kw["in_stride"]
        want, want_rec, want_nb = self.model.call(chan, in_stride=stride)
        if want is None:
            assert got is None and nb == want_nb, what
        else:
            same(got, nb, want, want_nb, what)
        if rec is not None:
            same(rec, nb, want_rec.view(np.uint32).reshape(self.B, 8), want_nb, (what, "records"))
            rec = rec.view(self.S.AfcRecord)[:, 0]
        assert self.eng.afc_config()["samples_consumed"] == self.model.g
        return got, rec, nb

    def restart(self):
        self.eng.afc_reset()
        self.model.reset()

    def close(self):
        self.eng.close()


@pytest.mark.parametrize("block", [16, 64, 256, 1024])
def test_stream_counts_and_blocks(S, T, block):
    """The step kernel takes 64 streams per workgroup: a wave in part, and a wave and a stream.  Blocks summed in a part
    of a wave (16), in a wave (64), across the waves (256) and over two passes (1024)."""
    ns = (700, 5, 1343)
    for B in (1, 3, 65):
        chan = signal(B, sum(ns), 100 + B)
        r = Rig(S, T, B, **dict(BASE, block=block))
        at = 0
        for f, n in enumerate(ns):
            _, rec, _ = r.check(chan[:, at:at + n], (B, block, f))
            at += n
        assert np.all(rec["flags"] == 3) and (rec["inc"] != 0).all()
        r.close()


@pytest.mark.parametrize("block", [16, 256, 1024])
def test_call_lengths_around_the_block_and_the_tile(S, T, block):
    """Every n as a call that follows whatever the others left, and as a fresh stream's first call: odd and even
    offsets, calls that end inside a block, on a seam, and one sample after it; the last two lie around the seam between
    two workgroups of the pass kernel, which take four tiles each."""
    B, tile = 3, S.afc_geometry(block)
    ns = (0, 1, block - 1, block, block + 1, tile - 1, tile, tile + 1, 2 * tile + 3, 4 * tile, 4 * tile + 1)
    r = Rig(S, T, B, **dict(BASE, block=block, max_in=4 * tile + 2))
    chan = signal(B, 2 * sum(ns), 200 + block)
    at, blocks = 0, 0
    for f, n in enumerate(ns):  # one stream
        got, rec, nb = r.check(chan[:, at:at + n], (block, f, n), in_stride=max(n, 1) + (f & 1))
        at, blocks = at + n, blocks + nb
        if n == 0:
            assert nb == 0 and not got.view(np.uint32).any()
    assert blocks == sum(ns) // block
    for n in ns:  # each the first call
        r.restart()
        r.check(chan[:, at:at + n], (block, "first", n), in_stride=max(n, 1))
        at += n
    r.close()


def test_odd_offsets_and_rows_that_are_not_aligned(S, T):
    """After a first call of 1, 2 or 3 samples the next starts at an odd or an even offset; in_stride odd and beyond n
    (the zero tail), chan and out moved by 8 bytes take the one-sample loads and the 8-byte stores."""
    B = 3
    r = Rig(S, T, B, **BASE)
    chan = signal(B, 4000, 300)
    at = 0
    for first in (1, 2, 3):
        for kw in (dict(), dict(in_stride=777), dict(in_shift=8), dict(out_shift=8), dict(in_stride=701, out_shift=8),
                   dict(in_shift=8, out_shift=8), dict(in_stride=1000)):
            r.restart()
            for n in (first, 700):
                r.check(chan[:, at:at + n], (first, n, kw), **(kw if n == 700 else {}))
                at = (at + n) % 3000
    r.close()


def test_five_calls_are_one_stream(S, T):
    """Calls of unequal lengths, some of which complete no block, against one call of the whole on the restatement."""
    B = 4
    r = Rig(S, T, B, **dict(BASE, block=256, max_in=2048))
    ns = (700, 10, 1, 2048, 333)
    chan = signal(B, sum(ns), 50)
    outs, at, blocks = [], 0, []
    for f, n in enumerate(ns):
        got, rec, nb = r.check(chan[:, at:at + n], f, records=f != 1)
        outs.append(got[:, :n])
        blocks.append(nb)
        at += n
    assert blocks == [2, 0, 0, 8, 2]
    want, want_rec, _, _ = af.one_call(chan, r.eng.afc_config(), 256, r.tab)
    assert np.concatenate(outs, axis=1).tobytes() == want.tobytes()
    assert rec["inc"].tobytes() == want_rec["inc"].tobytes() and rec["coherence"].tobytes() == want_rec["coherence"].tobytes()
    r.close()


def test_in_place(S, T):
    B = 5
    r = Rig(S, T, B, **BASE)
    chan = signal(B, 3000, 70)
    at = 0
    for f, (n, kw) in enumerate(((1000, {}), (33, {}), (900, dict(in_stride=901)), (1067, dict(out_shift=8)))):
        r.check(chan[:, at:at + n], (f, n), in_place=True, **kw)
        at += n
    r.close()


def test_measure_mode_writes_the_records_alone(S, T):
    """MEASURE: out is NULL, no row is written, and the records are those of TRACK on the same samples."""
    B = 3
    m, t = Rig(S, T, B, **dict(BASE, mode=af.MEASURE)), Rig(S, T, B, **BASE)
    chan = signal(B, 2000, 80)
    at = 0
    for f, n in enumerate((700, 0, 13, 1287)):
        got, rec, nb = m.check(chan[:, at:at + n], ("measure", f), in_stride=max(n, 1), records=f != 2)
        _, want, want_nb = t.check(chan[:, at:at + n], ("track", f), in_stride=max(n, 1))
        assert got is None and nb == want_nb and (rec is None or rec.tobytes() == want.tobytes())
        at += n
    buf = to_device(T, np.zeros(B * 2048 * 8, np.uint8))
    p = buf.data_ptr()
    invalid(S, m.eng.afc_device, p, 2048, 100, p)  # a non-NULL out while measuring
    invalid(S, t.eng.afc_device, p, 2048, 100, None)  # a NULL out while tracking
    assert m.eng.afc_config()["samples_consumed"] == t.eng.afc_config()["samples_consumed"] == 2000
    m.eng.synchronize()
    assert not buf.cpu().numpy().any(), "a refused call wrote"
    m.close()
    t.close()


@pytest.mark.parametrize("sign", [1, -1])
def test_the_phase_wraps_every_four_samples_at_the_clamp(S, T, sign):
    """max_offset_hz = channel_rate / 4 and a carrier beyond it: inc = +-2^30, Phi wraps every four samples, over 16
    blocks; and the exact quarter-rate carrier, whose estimate is the clamp itself."""
    B, block = 2, 64
    r = Rig(S, T, B, **dict(BASE, max_offset_hz=RATE / 4, tau_blocks=0.0))
    rng = np.random.default_rng(7)
    beyond = af.carrier(16 * block, sign * 0.3 * RATE, RATE, 0.5, 30.0, rng)
    exact = (0.5 * (1j * sign) ** np.arange(16 * block)).astype(np.complex64)
    chan = np.stack([beyond, exact])
    got, rec, nb = r.check(chan[:, :700], "head")
    got2, rec2, nb2 = r.check(chan[:, 700:], "tail")
    assert nb + nb2 == 16 and np.all(rec2["inc"] == sign * (1 << 30)) and np.all(rec2["flags"] == 3)
    assert np.all(rec2["offset_hz"] == f32(sign * RATE / 4))
    # the exact carrier stands still from block 1 on
    assert np.abs(got2[1, :324] - got2[1, 0]).max() < 1e-6
    r.close()


def test_the_lock_edge_and_a_block_under_the_floor(S, T):
    """A carrier, noise until the coherence has fallen under the threshold, a silent block, another carrier: the
    coherence crosses lock_threshold in both directions, and inc holds while unlocked and over the held block."""
    B, block = 2, 64
    cfg = dict(BASE, tau_blocks=2.0, lock_threshold=0.5)
    r = Rig(S, T, B, **dict(cfg, max_in=41 * block))
    rows = []
    for b in range(B):
        rng = np.random.default_rng(5 + b)
        rows.append(np.concatenate([af.carrier(8 * block, 2000.0, RATE, 0.5, 30.0, rng),
                                    af.white(rng, 24 * block, 0.25).astype(np.complex64), np.zeros(block, np.complex64),
                                    af.carrier(8 * block, -3000.0, RATE, 0.5, 30.0, rng)]))
    chan = np.stack(rows)
    _, rec, nb = r.check(chan[:, :1000], "head")
    _, rec2, nb2 = r.check(chan[:, 1000:], "tail")
    locked = r.model.traced("flags") & af.LOCKED
    assert nb + nb2 == 41 and locked[:8].all() and locked[-1].all() and (locked[8:33] == 0).any(axis=0).all()
    assert np.all(rec["held_blocks"] + rec2["held_blocks"] == 1) and np.all(rec2["inc"] < 0)
    r.close()


def test_amplitudes_down_to_1e_21(S, T):
    """Blocks of amplitude 1, 1e-7, 1e-14 and 1e-21 under a floor of -440 dB: the products are normal, then denormal,
    then zero, and the stage follows them as far as they are numbers."""
    B, block = 3, 64
    r = Rig(S, T, B, **dict(BASE, floor_db=-440.0, tau_blocks=0.0))
    amps = np.repeat(np.array([1.0, 1e-7, 1.0, 1e-14, 1e-21, 1e-21, 1.0, 1e-14]), 2 * block)
    chan = (signal(B, amps.size, 81, 30.0).astype(np.complex128) * amps[None, :]).astype(np.complex64)
    _, rec, nb = r.check(chan[:, :700], "head")
    _, rec2, nb2 = r.check(chan[:, 700:], "tail")
    assert nb + nb2 == 16 and np.all(rec2["flags"] & af.SEEDED)
    held, level = r.model.traced("held"), chan[:, 8 * block:12 * block]
    assert not held.any() and np.all(np.abs(level) < 1e-20) and np.all(rec2["level"] > 0)  # 1e-21: denormal powers count
    r.close()


def test_64_streams_of_16384(S, T):
    B, n = 64, 16384
    r = Rig(S, T, B, **dict(BASE, block=256, max_in=n, tau_blocks=16.0))
    _, rec, nb = r.check(signal(B, n, 90), "large")
    want = np.array([carrier_hz(b) for b in range(B)])
    assert nb == 64 and np.all(rec["flags"] == 3) and np.abs(rec["offset_hz"] - want).max() < 20.0
    r.close()


def test_reset_and_set_again_restart_the_streams(S, T):
    B = 3
    r = Rig(S, T, B, **BASE)
    chan = signal(B, 2000, 95)
    first, _, _ = r.check(chan[:, :900])
    r.check(chan[:, 900:])
    r.restart()
    again, _, _ = r.check(chan[:, :900])
    assert again.tobytes() == first.tobytes()
    r.check(chan[:, 900:950])
    invalid(S, r.eng.set_afc, **dict(BASE, block=48))  # a rejected set changes nothing
    invalid(S, r.eng.set_afc, **dict(BASE, mode=3))
    assert r.eng.afc_config()["samples_consumed"] == 950
    r.check(chan[:, 950:1000])
    r.configure(**dict(BASE, block=128))  # an accepted one restarts
    r.check(chan[:, :900])
    r.close()


def test_refusals_commit_nothing(S, T):
    B = 2
    r = Rig(S, T, B, **dict(BASE, max_in=512))
    chan = signal(B, 512, 96)
    r.check(chan[:, :100])
    buf = to_device(T, np.zeros(2 * B * 512 * 8, np.uint8))
    p = buf.data_ptr()
    L, h = S.load(), r.eng._h
    nb, ref = ctypes.c_int32(-7), ctypes.byref
    for args in ((p, 512, 513, p), (p, 513, 100, p), (p, 99, 100, p), (p, 512, -1, p), (p, 0, 0, p), (None, 512, 100, p),
                 (p, 512, 100, None)):
        assert L.sdrg_engine_afc_device(h, *args, None, ref(nb)) == -1, args
    assert L.sdrg_engine_afc_device(h, p, 512, 100, p, None, None) == -1
    assert L.sdrg_engine_afc_device(h, p + 4, 512, 100, p + 8192, None, ref(nb)) != 0  # chan off 8 bytes
    assert L.sdrg_engine_afc_device(h, p, 512, 100, p + 8196, None, ref(nb)) != 0  # out off 8 bytes
    assert L.sdrg_engine_afc_device(None, p, 512, 100, p, None, ref(nb)) == -1
    assert nb.value == -7 and r.eng.afc_config()["samples_consumed"] == 100
    r.eng.synchronize()
    assert not buf.cpu().numpy().any(), "a refused call wrote"
    r.check(chan[:, 100:])  # the stream goes on where it was
    r.eng.set_afc(off=True)
    invalid(S, r.eng.afc_config)
    invalid(S, r.eng.afc_device, p, 512, 100, p)
    invalid(S, r.eng.afc_host, chan)
    r.close()


@pytest.mark.parametrize("mode", [af.TRACK, af.MEASURE])
def test_host_path(S, T, mode):
    B = 3
    r = Rig(S, T, B, **dict(BASE, mode=mode))
    chan = signal(B, 1500, 97)
    at = 0
    for n, want_records in ((700, True), (0, True), (1, False), (799, True)):
        out, rec, nb = r.eng.afc_host(chan[:, at:at + n], want_records)
        want, want_rec, want_nb = r.model.call(chan[:, at:at + n])
        if mode == af.TRACK:
            same(out, nb, want, want_nb, n)
        else:
            assert out is None and want is None and nb == want_nb
        assert (rec is None) == (not want_records)
        if want_records:
            assert rec.tobytes() == want_rec.tobytes()
        at += n
    assert r.eng.afc_config()["samples_consumed"] == 1500
    r.close()


def test_other_stages_between_afc_calls(S, T):
    """process_device and squelch_device on the same engine between two AFC calls: the stream goes on as if they were not
    there, and the squelch gates the corrected rows in place."""
    B, n = 4, 1024
    r = Rig(S, T, B, n, **dict(BASE, max_in=n))
    sqc = dict(open_db=-20.0, close_db=-30.0, tau_blocks=0.0, block=64, hang_blocks=1, max_in=n)
    r.eng.set_squelch(**sqc)
    d = r.eng.squelch_config()
    gate = sq.Squelch(B, d["open_thr"], d["close_thr"], d["beta"], 64, 1)
    chan = signal(B, 3 * n, 98)
    raw = np.zeros((B, 2 * n), np.int8)
    spec = T.zeros((B, n), dtype=T.float32, device="cuda:0")
    for f in range(3):
        got, _, _ = r.check(chan[:, f * n:(f + 1) * n], f, in_stride=n)
        iq_t = to_device(T, raw)
        rc = S.load().sdrg_engine_process_device(r.eng._h, iq_t.data_ptr(), S.CS8, S.STAGE_SPECTRUM, spec.data_ptr(), None,
                                                 None, 0)
        assert rc == 0
        rows = to_device(T, got.view(np.float32))
        nb = r.eng.squelch_device(rows.data_ptr(), n, n, rows.data_ptr())
        r.eng.synchronize()
        want, _, want_nb = gate.call(got)
        same(rows.cpu().numpy().view(np.complex64).reshape(B, n), nb, want, want_nb, ("squelch", f))
    r.close()


# ---- sdrg_engine_listen_afc_host: fs = 2 MHz, N = 4096, a carrier 3 kHz above the DDC's tuning; DDC D = 10, T = 63 (cap
# 410, channel rate 200 kHz); AFC, squelch and AGC S = 16; AM demodulator R = 4, T2 = 31, float; resampler 24 / 25.

L_FS, L_N, L_B, L_FRAMES, L_CAP = 2_000_000, 4096, 2, 3, 410
DDC_CFG = dict(offset_hz=250_000.0, cutoff_hz=60_000.0, decimation=10, taps=63)
DEMOD_CFG = dict(mode=dm.AM, channel_rate_hz=200_000.0, deviation_hz=0.0, dc_cutoff_hz=100.0, deemphasis_us=0.0,
                 audio_decimation=4, audio_taps=31, audio_cutoff_hz=15_000.0, gain=1.0, out_format=dm.OUT_F32, max_in=L_CAP)
SQ_CFG = dict(open_db=-12.0, close_db=-18.0, tau_blocks=1.0, block=16, hang_blocks=2, max_in=L_CAP)
AGC_CFG = dict(target=0.5, max_gain_db=30.0, initial_gain_db=0.0, floor_db=-40.0, attack_blocks=0.0, decay_blocks=3.0,
               detector=0, block=16, hang_blocks=1, max_in=L_CAP)
RS_CFG = dict(interp=24, decim=25, taps_per_phase=8, cutoff_rel=0.9, components=1, out_format=rs.OUT_F32, gain=1.0,
              max_in=103)
AFC_CFG = dict(channel_rate=200_000.0, max_offset_hz=10_000.0, tau_blocks=2.0, floor_db=-40.0, lock_threshold=0.25,
               mode=af.TRACK, block=16, max_in=L_CAP)
ALL = 7


def listen_engine(S):
    eng = engine(S, L_B, L_N, L_FS)
    eng.set_ddc(**DDC_CFG)
    eng.set_demod(**DEMOD_CFG)
    eng.set_squelch(**SQ_CFG)
    eng.set_agc(**AGC_CFG)
    eng.set_resample(**RS_CFG)
    eng.set_afc(**AFC_CFG)
    return eng


@pytest.fixture(scope="module")
def off_tune():
    """CS8 [B][2 N frames]: an AM carrier 3 kHz (stream 0) and -4.5 kHz (stream 1) off the DDC's 250 kHz."""
    t = np.arange(L_FRAMES * L_N, dtype=np.float64)
    rng = np.random.default_rng(3)
    raw = np.empty((L_B, 2 * t.size), np.int8)
    for b, hz in enumerate((253_000.0, 245_500.0)):
        env = 0.4 * (1.0 + 0.5 * np.cos(2 * np.pi * 2000.0 * t / L_FS + 0.7 * b))
        z = env * np.exp(2j * np.pi * hz * t / L_FS) + (3 / 128) * (rng.standard_normal(t.size) + 1j * rng.standard_normal(t.size))
        raw[b, 0::2] = np.round(z.real * 128).clip(-128, 127).astype(np.int8)
        raw[b, 1::2] = np.round(z.imag * 128).clip(-128, 127).astype(np.int8)
    return raw


def consumed(eng, S=None):
    """samples_consumed of the six stages; with S, None for a stage that is off."""
    got = []
    for s in ("ddc", "afc", "squelch", "agc", "demod", "resample"):
        try:
            got.append(getattr(eng, s + "_config")()["samples_consumed"])
        except Exception as e:
            if S is None or not isinstance(e, S.SdrgError):
                raise
            got.append(None)
    return got


@pytest.mark.parametrize("steps", [0, ALL])
def test_listen_afc_equals_the_stages_one_by_one(S, T, off_tune, steps):
    a, b = listen_engine(S), listen_engine(S)
    for f in range(L_FRAMES):
        frame = off_tune[:, 2 * L_N * f:2 * L_N * (f + 1)]
        got, sq_rec, agc_rec, afc_rec = a.listen_afc(frame, dd.CS8, steps)
        chan = b.ddc(frame, dd.CS8)
        chan, want_afc, _ = b.afc_host(chan)
        assert afc_rec.tobytes() == want_afc.tobytes(), f
        if steps & S.LISTEN_SQUELCH:
            chan, want_rec, _ = b.squelch_host(chan)
            assert sq_rec.tobytes() == want_rec.tobytes(), f
        if steps & S.LISTEN_AGC:
            chan, want_rec, _ = b.agc_host(chan)
            assert agc_rec.tobytes() == want_rec.tobytes(), f
        want = b.demod(chan)
        if steps & S.LISTEN_RESAMPLE:
            want = b.resample_host(want)
        assert got.dtype == np.float32 and got.shape == want.shape and got.size and got.tobytes() == want.tobytes(), f
    assert np.all(afc_rec["flags"] == 3) and np.abs(afc_rec["offset_hz"] - np.array([3000.0, -4500.0])).max() < 150.0
    got = consumed(a)
    assert got[0] == L_FRAMES * L_N and got[1] == got[4] > 0 and got[2] == got[3] == (got[1] if steps else 0)
    # the other chain calls never run the AFC
    before = consumed(a)[1]
    a.listen(off_tune[:, :2 * L_N], dd.CS8, steps)
    assert consumed(a)[1] == before
    a.close()
    b.close()


def refused(S, eng, frame, steps, needle):
    """The call is refused for the reason that holds `needle`, and no stage has moved."""
    before = consumed(eng, S)
    with pytest.raises(S.SdrgError) as ei:
        eng.listen_afc(frame, dd.CS8, steps)
    assert "SDRG_E_INVALID" in str(ei.value) and needle in str(ei.value), (needle, str(ei.value))
    assert consumed(eng, S) == before


def test_listen_afc_refusals_in_their_order(S, T, off_tune):
    """listen_host's refusals in its order with the AFC's among them: off or measuring after the mask's stages' own, its
    max_in after the AGC's; and no stage has moved."""
    frame = off_tune[:, :2 * L_N]
    eng = listen_engine(S)
    eng.listen_afc(frame, dd.CS8, ALL)
    assert all(consumed(eng))
    refused(S, eng, frame, 8, "unknown bits")
    eng.set_afc(off=True)
    refused(S, eng, frame, ALL, "no afc configuration")
    refused(S, eng, frame, 8, "unknown bits")  # the mask comes first
    eng.set_agc(off=True)
    refused(S, eng, frame, ALL, "no agc configuration")  # the mask's stages come before the AFC
    refused(S, eng, frame, S.LISTEN_SQUELCH, "no afc configuration")
    eng.set_agc(**AGC_CFG)
    eng.set_afc(**dict(AFC_CFG, mode=af.MEASURE))
    refused(S, eng, frame, ALL, "SDRG_AFC_TRACK")
    eng.set_ddc(off=True)
    refused(S, eng, frame, ALL, "SDRG_AFC_TRACK")  # before the DDC's own
    eng.set_afc(**dict(AFC_CFG, max_in=L_CAP - 1))
    refused(S, eng, frame, ALL, "ddc")
    eng.set_ddc(**DDC_CFG)
    refused(S, eng, frame, ALL, "afc max_in")
    eng.set_agc(**dict(AGC_CFG, max_in=L_CAP - 1))
    refused(S, eng, frame, ALL, "agc max_in")  # the AGC's comes first
    refused(S, eng, frame, 0, "afc max_in")
    eng.set_resample(**dict(RS_CFG, max_in=102))
    refused(S, eng, frame, 0, "afc max_in")  # before the resampler's, which is not in the mask anyway
    eng.set_agc(**AGC_CFG)
    refused(S, eng, frame, ALL, "afc max_in")  # and before the resampler's when it is
    L, n_out = S.load(), ctypes.c_int32(-7)
    out = np.full((L_B, 128), 7.0, np.float32)
    iq_p, out_p = frame.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)
    before = consumed(eng)
    for args in ((None, out_p, ctypes.byref(n_out)), (iq_p, None, ctypes.byref(n_out)), (iq_p, out_p, None)):
        assert L.sdrg_engine_listen_afc_host(eng._h, ALL, args[0], dd.CS8, args[1], args[2], None, None, None) == -1
    assert L.sdrg_engine_listen_afc_host(None, ALL, iq_p, dd.CS8, out_p, ctypes.byref(n_out), None, None, None) == -1
    assert n_out.value == -7 and np.all(out == 7.0) and consumed(eng) == before
    # the records are optional
    eng.set_afc(**AFC_CFG)
    eng.set_resample(**RS_CFG)
    assert L.sdrg_engine_listen_afc_host(eng._h, ALL, iq_p, dd.CS8, out_p, ctypes.byref(n_out), None, None, None) == 0
    assert n_out.value > 0
    eng.close()


def test_fm_end_to_end(S, T):
    """The FM case of tests/test_afc_cases.py (a 1 kHz tone, 3 kHz deviation, the carrier at +1500 Hz, 20 dB SNR, 400
    blocks of 256) in one call: the restatement's bytes, and with them its figures."""
    n = 400 * 256
    r = Rig(S, T, 1, **dict(BASE, tau_blocks=16.0, block=256, max_in=n))
    z = af.fm(n, 1500.0, RATE, 1000.0, 3000.0, 0.5, 20.0, np.random.default_rng(1))
    got, rec, nb = r.check(z[None, :], "fm")
    step_out = af.mean_step_hz(got[0, 200 * 256:], RATE)
    hz = r.model.traced("inc")[200:, 0].astype(np.float32) * r.eng.afc_config()["hz_per_inc"]
    print("offset_hz mean %.2f; mean phase step of the output %.2f Hz" % (hz.mean(), step_out))
    assert nb == 400 and abs(hz.mean() - 1500.0) <= 2.0 and np.abs(hz - 1500.0).max() <= 25.0 and abs(step_out) < 5.0
    assert abs(rec["offset_hz"][0] - 1500.0) <= 25.0 and rec["flags"][0] == 3
    r.close()
