"""GPU tests of the tone detector stage (csrc/tones.hip, sdrg_engine_tones_*, sdrg_engine_listen_tones_host): the whole of
`powers` and the records are compared as bytes with the NumPy restatement (tests/tones_cases.py) fed the library's own
design.  Every buffer the stage writes is 0xAA-filled between guard bytes, and the rows carry NaN past n.  The shapes are
the smallest at which each mechanism can go wrong: one stream, a few, more than a wave of streams; one tone, two, 63 and
64; one sub-block per block, two, three and 256; calls around the sub-block and across every workgroup seam."""
import ctypes

import numpy as np
import pytest

import agc_cases as ag
import ddc_cases as dd
import demod_cases as dm
import resample_cases as rs
import squelch_cases as sq
import tones_cases as tc
from stage_harness import GUARD, engine, invalid, out_buffer, read_out, same

pytestmark = pytest.mark.gpu

FA = 8000.0
BASE = dict(rate_hz=FA, components=1, freq_hz=(700.0, 1000.0, 1750.0), sub_blocks=2, window=tc.HANN, min_db=-30.0,
            dominance_db=6.0, share=0.2, confirm_blocks=2, release_blocks=1, max_in=1024)


@pytest.fixture(scope="module")
def S():
    import sdrg
    return sdrg


@pytest.fixture(scope="module")
def T():
    import torch
    return torch


def freqs(K, fa=FA, components=1):
    """K distinct frequencies inside the band."""
    lo = 0.02 if components == 1 else -0.48
    return tuple(fa * (lo + 0.46 * (k + 0.5) / K * (1 if components == 1 else 2)) for k in range(K))


def signal(B, n, seed, cfg, amp=0.5, noise=0.05, hold=256):
    """Per stream a tone that moves through the configured frequencies every `hold` values (each stream starts on its
    own), with silences, in noise: candidates come, change and go."""
    rng = np.random.default_rng(seed)
    f, fa, comp = cfg["freq_hz"], cfg["rate_hz"], cfg.get("components", 1)
    t = np.arange(n, dtype=np.float64)
    x = np.empty((B, n), np.complex128)
    for b in range(B):
        step = (np.arange(n) // hold + b) % (len(f) + 1)
        fk = np.array(list(f) + [0.0])[step]
        on = step < len(f)
        x[b] = amp * on * np.exp(2j * np.pi * fk * t / fa)
    x = x + noise * (rng.standard_normal((B, n)) + 1j * rng.standard_normal((B, n)))
    return x.astype(np.complex64) if comp == 2 else np.ascontiguousarray(x.real).astype(np.float32)


class Detector:
    """An engine with the tone stage set, and the restatement that follows it call by call."""

    def __init__(self, S, T, B, **cfg):
        self.S, self.T, self.B = S, T, B
        self.eng = engine(S, B)
        self.configure(**cfg)

    def configure(self, **cfg):
        self.cfg = cfg
        self.eng.set_tones(**cfg)
        d = self.eng.tones_config()
        assert d["samples_consumed"] == 0 and d["n_tones"] == len(cfg["freq_hz"])
        des = self.S.tones_design(**cfg)
        assert all(des[k].tobytes() == d[k].tobytes() for k in tc.SCALARS)
        self.model = tc.model(self.B, des, **cfg)
        self.K, self.comp = d["n_tones"], cfg.get("components", 1)
        self.cap = self.eng.tones_max_blocks()
        assert self.cap == self.model.cap_blocks

    def device_call(self, x, in_stride=None, records=True, shift=0):
        """tones_device into 0xAA-filled buffers between guard bytes: (powers [B][cap][K], records [B][8] as uint32 or
        None, n_blocks).  shift: bytes by which the rows are moved off their 16-byte alignment."""
        T, B, comp = self.T, self.B, self.comp
        n = x.shape[1]
        stride = self.cfg["max_in"] if in_stride is None else in_stride
        rows = np.full((B, stride, comp), np.nan, np.float32)
        rows[:, :n] = np.ascontiguousarray(x).view(np.float32).reshape(B, n, comp)
        in_t = T.zeros((rows.nbytes + shift,), dtype=T.uint8, device="cuda:0")
        in_t[shift:] = T.from_numpy(rows.view(np.uint8).reshape(-1)).to("cuda:0")
        pw_t = out_buffer(T, B * self.cap * self.K * 4)
        rec_t = out_buffer(T, B * 32)
        T.cuda.synchronize()
        nb = self.eng.tones_device(in_t.data_ptr() + shift, stride, n, pw_t.data_ptr() + GUARD,
                                   rec_t.data_ptr() + GUARD if records else None)
        self.eng.synchronize()
        powers = read_out(pw_t, (B, self.cap, self.K), np.float32)
        if not records:
            assert np.all(rec_t.cpu().numpy() == 0xAA), "records written without a pointer"
            return powers, None, nb
        return powers, read_out(rec_t, (B, 8), np.uint32), nb

    def check(self, x, what=None, **kw):
        got, rec, nb = self.device_call(x, **kw)
        want, want_rec, want_nb = self.model.call(x)
        same(got, nb, want, want_nb, what)
        if rec is not None:
            same(rec, nb, want_rec.view(np.uint32).reshape(self.B, 8), want_nb, (what, "records"))
            rec = rec.view(self.S.TonesRecord)[:, 0]
        assert self.eng.tones_config()["samples_consumed"] == self.model.g
        return got, rec, nb

    def restart(self):
        self.eng.tones_reset()
        self.model.reset()

    def close(self):
        self.eng.close()


@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("components", [1, 2])
def test_stream_counts(S, T, B, components):
    cfg = dict(BASE, components=components)
    rig = Detector(S, T, B, **cfg)
    x = signal(B, 1000, B, cfg)
    _, rec, nb = rig.check(x[:, :600], "first")
    assert nb == 4
    _, rec, nb = rig.check(x[:, 600:], "second")
    assert nb == 3 and rec["tone"][0] == 2  # stream 0 ends on the third tone, one silent block into its release
    rig.close()


@pytest.mark.parametrize("K", [1, 2, 63, 64])
@pytest.mark.parametrize("components, window", [(1, tc.RECT), (2, tc.HANN)])
def test_tone_counts(S, T, K, components, window):
    cfg = dict(BASE, components=components, window=window, freq_hz=freqs(K, components=components), dominance_db=3.0)
    rig = Detector(S, T, 3, **cfg)
    x = signal(3, 900, K, cfg, hold=128)
    rig.check(x[:, :333], "first")
    _, rec, _ = rig.check(x[:, 333:], "second")
    if K == 1:  # P2 = +0: the dominance never refuses
        assert np.all(rec["power"] >= 0)
    rig.close()


@pytest.mark.parametrize("Q, B", [(1, 3), (2, 3), (3, 3), (256, 1)])
@pytest.mark.parametrize("components, window", [(1, tc.HANN), (2, tc.RECT)])
def test_sub_block_counts(S, T, Q, B, components, window):
    n = {1: 700, 2: 700, 3: 900, 256: 16384 + 300}[Q]
    cfg = dict(BASE, components=components, window=window, sub_blocks=Q, max_in=max(1024, 64 * Q + 1024), confirm_blocks=1)
    rig = Detector(S, T, B, **cfg)
    x = signal(B, 2 * n, Q, cfg, hold=64 * Q)
    _, _, nb0 = rig.check(x[:, :n], "first", in_stride=n)
    _, _, nb1 = rig.check(x[:, n:], "second", in_stride=n + 1)
    assert nb0 + nb1 == 2 * n // (64 * Q) and nb1 >= 1
    rig.close()


@pytest.mark.parametrize("components", [1, 2])
def test_calls_around_the_sub_block_and_every_seam(S, T, components):
    """n = 0, 1, 63, 64, 65 from a fresh stream and from inside a sub-block, and calls that end one value before, on and
    one value after every seam between two workgroups of the correlate kernel."""
    group = 64 * S.tones_geometry()
    cfg = dict(BASE, components=components, max_in=4 * group)
    rig = Detector(S, T, 3, **cfg)
    x = signal(3, 8 * group, 7, cfg, hold=192)
    for first in (0, 1, 63, 64, 65):
        rig.restart()
        at = 0
        for n in (first, 0, 1, 63, 64, 65, 0, 37):
            rig.check(x[:, at:at + n], (first, n))
            at += n
    for soff in (0, 1, 63):
        for seam in (group, 2 * group, 3 * group):
            for d in (-1, 0, 1):
                rig.restart()
                rig.check(x[:, :soff], ("lead", soff))
                n = seam - soff + d  # the call's positions end at seam + d
                rig.check(x[:, soff:soff + n], (soff, seam, d))
                rig.check(x[:, soff + n:soff + n + 200], (soff, seam, d, "after"))
    rig.close()


def test_odd_strides_and_rows_off_alignment(S, T):
    for components, shifts in ((1, (4, 8, 12)), (2, (8,))):
        cfg = dict(BASE, components=components)
        rig = Detector(S, T, 3, **cfg)
        x = signal(3, 1200, 9, cfg)
        at = 0
        for n, stride, shift in ((301, 301, 0), (300, 333, shifts[0]), (299, 1023, shifts[-1]), (300, 1024, 0)):
            rig.check(x[:, at:at + n], (n, stride, shift), in_stride=stride, shift=shift)
            at += n
        rig.close()


def test_five_calls_are_one_stream_and_many_calls_inside_a_sub_block(S, T):
    cfg = dict(BASE)
    rig, one = Detector(S, T, 3, **cfg), Detector(S, T, 3, **cfg)
    x = signal(3, 1000, 10, cfg)
    rows = []
    for a, b in zip((0, 130, 131, 500, 563), (130, 131, 500, 563, 1000)):
        got, rec, nb = rig.check(x[:, a:b], (a, b))
        rows.append(got[:, :nb])
    whole, whole_rec, nb = one.check(x[:, :1000], "one call")
    assert np.concatenate(rows, axis=1).tobytes() == whole[:, :nb].tobytes()
    for k in ("tone", "candidate", "power", "power_db", "share", "run"):
        assert rec[k].tobytes() == whole_rec[k].tobytes(), k
    rig.restart()
    rig.check(x[:, :100], "into a sub-block")  # 36 values in
    at = 100
    for n in (1, 2, 3, 5, 7, 9, 0, 1):  # 28 more: the sub-block completes on the last
        got, rec2, nb = rig.check(x[:, at:at + n], ("inside", n))
        at += n
    assert nb == 1 and at == 128
    got, rec3, nb = rig.check(x[:, at:at + 10], "no block")  # a call that completes no block: the records repeat
    assert nb == 0 and np.all(got == 0)
    for k in ("tone", "candidate", "power", "power_db", "share", "run"):
        assert rec3[k].tobytes() == rec2[k].tobytes(), k
    assert np.all(rec3["tone_blocks"] == 0) and np.all(rec3["changes"] == 0)
    rig.close()
    one.close()


def test_first_call_without_values(S, T):
    rig = Detector(S, T, 3, **BASE)
    got, rec, nb = rig.check(np.zeros((3, 0), np.float32), "fresh, n = 0", in_stride=5)
    assert nb == 0 and np.all(got == 0) and np.all(rec["tone"] == -1) and np.all(rec["candidate"] == -1)
    assert np.all(rec["power"] == 0) and np.all(rec["power_db"] == np.float32(-200.0))
    rig.check(signal(3, 300, 1, BASE), "then a stream")
    rig.close()


@pytest.mark.parametrize("components", [1, 2])
def test_amplitudes_down_to_1e_minus_21(S, T, components):
    """Products that are denormal and sums that leave the denormals: kept, not flushed."""
    cfg = dict(BASE, components=components, min_db=-600.0, share=0.0, dominance_db=0.0, confirm_blocks=1)
    rig = Detector(S, T, 3, **cfg)
    x = signal(3, 768, 12, cfg, amp=1.0, noise=0.01)
    scale = np.repeat(np.array([1e-21, 1e-19, 1e-10, 1e-21, 3e-20, 1.0], np.float32), 128)
    got, rec, nb = rig.check((x * scale[None, :]).astype(x.dtype), "tiny")
    assert nb == 6 and np.any((got > 0) & (got < np.float32(1.2e-38)))  # denormal powers among them
    rig.close()


def test_the_tie_and_the_tree(S, T):
    cfg = dict(BASE, freq_hz=(1750.0, 1000.0, 1000.0), dominance_db=0.0, confirm_blocks=1)
    rig = Detector(S, T, 1, **cfg)
    got, rec, nb = rig.check(tc.tone(256, 1000.0, FA, 0.7)[None, :], "tie")
    assert nb == 2 and np.all(got[0, :2, 1] == got[0, :2, 2]) and rec["tone"][0] == 1
    rig.configure(**dict(cfg, window=tc.RECT, sub_blocks=1))
    x = np.ones((1, 64), np.float32)
    x[0, 0] = 4096.0  # E is 2^24 + 62 by the tree, 2^24 by a running sum: the share tells them apart
    got, rec, nb = rig.check(x, "tree")
    assert nb == 1
    rig.close()


@pytest.mark.parametrize("confirm, release, cands, tones", [
    (1, 0, [0, 0, -1, 1, 1, -1, -1], [0, 0, -1, 1, 1, -1, -1]),
    (1, 2, [0, -1, -1, 0, -1, -1, -1, 0], [0, 0, 0, 0, 0, 0, -1, 0]),
    (3, 0, [0, 0, 0, 0, -1, 0, 0, 0], [-1, -1, 0, 0, -1, -1, -1, 0]),
    (3, 2, [0, 0, 1, 1, 1, -1, 0, -1, -1, -1], [-1, -1, -1, -1, 1, 1, 1, -1, -1, -1]),
])
def test_the_latch(S, T, confirm, release, cands, tones):
    cfg = dict(BASE, freq_hz=(1000.0, 1750.0), sub_blocks=1, window=tc.RECT, confirm_blocks=confirm,
               release_blocks=release)
    rig = Detector(S, T, 2, **cfg)
    x = np.concatenate([tc.tone(64, cfg["freq_hz"][c], FA, 0.5) if c >= 0 else np.zeros(64, np.float32) for c in cands])
    x = np.stack([x, np.roll(x, 64)])  # the second stream one block behind
    half = 64 * (len(cands) // 2) + 20  # one call boundary inside a block, the latch carried across it
    _, rec, _ = rig.check(x[:, :half], "first half")
    assert rec["tone"][0] == tones[len(cands) // 2 - 1]
    _, rec, _ = rig.check(x[:, half:], "second half")
    assert rec["tone"][0] == tones[-1] and rec["candidate"][0] == cands[-1]
    rig.restart()
    _, rec, nb = rig.check(x, "one call")
    assert nb == len(cands) and rec["tone_blocks"][0] == sum(t >= 0 for t in tones)
    assert rec["changes"][0] == sum(a != b for a, b in zip([-1] + tones[:-1], tones))
    rig.close()


def test_reset_and_set_again_between_calls(S, T):
    rig = Detector(S, T, 3, **BASE)
    x = signal(3, 900, 14, BASE)
    rig.check(x[:, :333], "before")
    rig.restart()
    rig.check(x[:, 333:600], "after the reset")
    cfg = dict(BASE, components=2, freq_hz=freqs(5, components=2), sub_blocks=3)
    rig.configure(**cfg)
    rig.check(signal(3, 777, 15, cfg), "after another configuration")
    rig.configure(**BASE)
    rig.check(x[:, :500], "and the first again")
    rig.close()


def test_without_records(S, T):
    rig = Detector(S, T, 3, **BASE)
    x = signal(3, 600, 16, BASE)
    _, rec, _ = rig.check(x[:, :300], "no records", records=False)
    assert rec is None
    rig.check(x[:, 300:], "with records")
    rig.close()


def test_refusals_write_nothing_and_commit_nothing(S, T):
    eng = engine(S, 2)
    buf = out_buffer(T, 4096)
    p = buf.data_ptr() + GUARD
    invalid(S, eng.tones_device, p, 64, 64, p)  # off
    invalid(S, eng.tones_max_blocks)
    invalid(S, eng.tones_config)
    eng.set_tones(**BASE)
    invalid(S, eng.set_tones, **dict(BASE, sub_blocks=0))  # a rejected set changes nothing
    assert eng.tones_config()["sub_blocks"] == 2
    x = T.zeros((2, 100), dtype=T.float32, device="cuda:0")
    pw = out_buffer(T, 2 * eng.tones_max_blocks() * 3 * 4)
    assert eng.tones_device(x.data_ptr(), 100, 100, pw.data_ptr() + GUARD) == 0
    eng.synchronize()
    before = pw.clone()
    for stride, n in ((100, -1), (100, 101), (0, 0), (1025, 10), (1024, 1025), (50, 51)):
        invalid(S, eng.tones_device, x.data_ptr(), stride, n, pw.data_ptr() + GUARD)
    L, nb = S.load(), ctypes.c_int32(7)
    assert L.sdrg_engine_tones_device(eng._h, None, 100, 100, pw.data_ptr() + GUARD, None, ctypes.byref(nb)) == -1
    assert L.sdrg_engine_tones_device(eng._h, x.data_ptr(), 100, 100, None, None, ctypes.byref(nb)) == -1
    assert L.sdrg_engine_tones_device(eng._h, x.data_ptr(), 100, 100, pw.data_ptr() + GUARD, None, None) == -1
    assert L.sdrg_engine_tones_device(None, x.data_ptr(), 100, 100, pw.data_ptr() + GUARD, None, ctypes.byref(nb)) == -1
    eng.synchronize()
    assert nb.value == 7 and T.equal(pw, before) and eng.tones_config()["samples_consumed"] == 100
    eng.set_tones(off=True)
    invalid(S, eng.tones_device, x.data_ptr(), 100, 100, pw.data_ptr() + GUARD)
    eng.close()


@pytest.mark.parametrize("components", [1, 2])
def test_host_path_equals_the_restatement(S, T, components):
    cfg = dict(BASE, components=components)
    eng = engine(S, 3)
    eng.set_tones(**cfg)
    m = tc.model(3, S.tones_design(**cfg), **cfg)
    x = signal(3, 900, 17, cfg)
    for a, b, want_rec in ((0, 333, True), (333, 333, True), (333, 700, False), (700, 900, True)):
        got, rec, nb = eng.tones_host(x[:, a:b], want_records=want_rec)
        want, w_rec, w_nb = m.call(x[:, a:b])
        assert nb == w_nb and got.tobytes() == want[:, :nb].tobytes(), (a, b)
        assert (rec is None) if not want_rec else rec.tobytes() == w_rec.tobytes(), (a, b)
    eng.close()


def test_other_stages_between_tones_calls(S, T):
    """squelch_device and demod_device between two tones calls: each keeps its own stream and scratch."""
    cfg = dict(BASE, components=2)
    rig = Detector(S, T, 2, **cfg)
    eng = rig.eng
    eng.set_squelch(open_db=-12.0, close_db=-18.0, tau_blocks=1.0, block=16, hang_blocks=2, max_in=1024)
    eng.set_demod(mode=dm.AM, channel_rate_hz=200_000.0, deviation_hz=0.0, dc_cutoff_hz=100.0, deemphasis_us=0.0,
                  audio_decimation=4, audio_taps=31, audio_cutoff_hz=15_000.0, gain=1.0, out_format=dm.OUT_F32, max_in=1024)
    x = signal(2, 900, 18, cfg)
    rig.check(x[:, :450], "before")
    chan = T.from_numpy(np.ascontiguousarray(x[:, :512])).to("cuda:0")
    out = T.empty_like(chan)
    audio = T.empty((2, eng.demod_max_out()), dtype=T.float32, device="cuda:0")
    eng.squelch_device(chan.data_ptr(), 512, 512, out.data_ptr())
    eng.demod_device(chan.data_ptr(), 512, audio.data_ptr())
    rig.check(x[:, 450:], "after")
    rig.close()


# ---- sdrg_engine_listen_tones_host: the listening chain of test_gpu_agc (fs = 2 MHz, N = 4096, an AM carrier at +250 kHz
# keyed on in the second frame, modulated by a 2 kHz tone; audio at 50 kHz, 102 or 103 values a frame), with the tone
# stage at 1, 2 and 3 kHz on the audio in blocks of 64.

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
TONES_CFG = dict(rate_hz=50_000.0, components=1, freq_hz=(1000.0, 2000.0, 3000.0), sub_blocks=1, window=tc.HANN,
                 min_db=-40.0, dominance_db=3.0, share=0.05, confirm_blocks=1, release_blocks=1, max_in=103)


@pytest.fixture(scope="module")
def keyed_am():
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


def listen_engine(S, tones=TONES_CFG):
    eng = engine(S, LISTEN_B, LISTEN_N, LISTEN_FS)
    eng.set_ddc(**DDC_CFG)
    eng.set_demod(**DEMOD_CFG)
    eng.set_squelch(**SQ_CFG)
    eng.set_agc(**AGC_CFG)
    eng.set_resample(**RS_CFG)
    if tones:
        eng.set_tones(**tones)
    return eng


@pytest.fixture(scope="module")
def ddc_restated(S, T, keyed_am):
    eng = listen_engine(S)
    taps, tab, inc = S.ddc_design(LISTEN_FS, **DDC_CFG), S.nco_tables(), eng.ddc_config()["nco_increment"]
    eng.close()
    model = dd.Ddc(LISTEN_B, taps, tab, inc, 10)
    n = LISTEN_N
    return [model.call(dd.CS8, keyed_am[:, 2 * n * f:2 * n * (f + 1)]) for f in range(LISTEN_FRAMES)]


@pytest.mark.parametrize("steps", range(8))
def test_listen_tones_equals_the_restatements_chained(S, T, keyed_am, ddc_restated, steps):
    B, n = LISTEN_B, LISTEN_N
    eng = listen_engine(S)
    d, q, c = eng.demod_config(), eng.squelch_config(), eng.resample_config()
    gate = sq.Squelch(B, q["open_thr"], q["close_thr"], q["beta"], 16, 2)
    agc = ag.Agc(B, AGC_CFG["target"], S.agc_design(**AGC_CFG), 16, 1)
    demod = dm.Demod(B, d["mode"], d["kf"], d["alpha"], d["a"], d["taps"], 4, d["gain"], dm.OUT_F32, LISTEN_CAP)
    rsm = rs.Resampler(B, 24, 25, c["taps"], c["gain"], rs.OUT_F32, 1, 103)
    det = tc.model(B, S.tones_design(**TONES_CFG), **TONES_CFG)
    heard = []
    for f in range(LISTEN_FRAMES):
        got, sq_rec, agc_rec, powers, t_rec, nb = eng.listen_tones(keyed_am[:, 2 * n * f:2 * n * (f + 1)], dd.CS8, steps)
        chan, n_chan = ddc_restated[f]
        chan = chan[:, :n_chan]
        if steps & S.LISTEN_SQUELCH:
            chan, want_rec, _ = gate.call(chan)
            assert sq_rec.tobytes() == want_rec.tobytes(), f
        else:
            assert sq_rec is None
        if steps & S.LISTEN_AGC:
            chan, want_rec, _ = agc.call(chan)
            assert agc_rec.tobytes() == want_rec.tobytes(), f
        else:
            assert agc_rec is None
        want, want_n = demod.call(chan)
        want = want[:, :want_n]
        w_pow, w_rec, w_nb = det.call(want)
        assert nb == w_nb and powers.tobytes() == w_pow[:, :w_nb].tobytes(), f
        assert t_rec.tobytes() == w_rec.tobytes(), f
        heard.append(t_rec["tone"].tolist())
        if steps & S.LISTEN_RESAMPLE:
            want, want_n = rsm.call(want)
            want = want[:, :want_n]
        assert got.dtype == np.float32 and got.shape == want.shape and got.tobytes() == want.tobytes(), f
    assert eng.tones_config()["samples_consumed"] == det.g == -(-eng.demod_config()["samples_consumed"] // 4)
    assert heard[-1] == [1] * B  # the carrier's 2 kHz modulation
    if not steps & S.LISTEN_AGC:  # and nothing before the carrier, unless the AGC has lifted the noise to its target
        assert heard[0] == [-1] * B
    eng.close()


def test_listen_tones_refusals_move_no_stage(S, T, keyed_am):
    first = keyed_am[:, :2 * LISTEN_N]
    ALL = S.LISTEN_SQUELCH | S.LISTEN_AGC | S.LISTEN_RESAMPLE

    def consumed(eng):
        return [eng.ddc_config()["samples_consumed"], eng.squelch_config()["samples_consumed"],
                eng.agc_config()["samples_consumed"], eng.demod_config()["samples_consumed"],
                eng.resample_config()["samples_consumed"]]

    eng = listen_engine(S, tones=None)
    invalid(S, eng.listen_tones, first, dd.CS8, ALL)  # the tone stage off (the mirror asks for its configuration)
    L, n_out, nb = S.load(), ctypes.c_int32(), ctypes.c_int32()
    out, pw = np.empty((LISTEN_B, 103), np.float32), np.empty((LISTEN_B, 2, 3), np.float32)
    args = (eng._h, ALL, first.ctypes.data_as(ctypes.c_void_p), dd.CS8, out.ctypes.data_as(ctypes.c_void_p),
            ctypes.byref(n_out), None, None)
    assert L.sdrg_engine_listen_tones_host(*args, pw.ctypes.data_as(ctypes.c_void_p), None, ctypes.byref(nb)) == -1
    for bad in (dict(TONES_CFG, components=2), dict(TONES_CFG, max_in=102)):
        eng.set_tones(**bad)
        invalid(S, eng.listen_tones, first, dd.CS8, ALL)
    eng.set_tones(**TONES_CFG)
    assert L.sdrg_engine_listen_tones_host(*args, None, None, ctypes.byref(nb)) == -1
    assert L.sdrg_engine_listen_tones_host(*args, pw.ctypes.data_as(ctypes.c_void_p), None, None) == -1
    eng.set_demod(**dict(DEMOD_CFG, out_format=dm.OUT_S16))
    invalid(S, eng.listen_tones, first, dd.CS8, 0)
    eng.set_demod(**DEMOD_CFG)
    eng.set_squelch(off=True)
    invalid(S, eng.listen_tones, first, dd.CS8, ALL)
    eng.set_squelch(**SQ_CFG)
    invalid(S, eng.listen_tones, first, dd.CS8, 8)
    assert consumed(eng) == [0] * 5 and eng.tones_config()["samples_consumed"] == 0
    assert L.sdrg_engine_listen_tones_host(*args, pw.ctypes.data_as(ctypes.c_void_p), None, ctypes.byref(nb)) == 0
    assert consumed(eng)[0] == LISTEN_N and eng.tones_config()["samples_consumed"] == 103
    eng.close()


def test_listen_and_listen_sideband_are_unchanged_by_a_set_tone_stage(S, T, keyed_am):
    n = LISTEN_N
    ALL = S.LISTEN_SQUELCH | S.LISTEN_AGC | S.LISTEN_RESAMPLE
    sb = dict(channel_rate_hz=200_000.0, low_hz=300.0, high_hz=20_000.0, mode=S.SIDEBAND_UPPER, audio_decimation=4, taps=63,
              out_format=S.SIDEBAND_OUT_F32, max_in=LISTEN_CAP, gain=1.0)
    a, b = listen_engine(S), listen_engine(S, tones=None)
    a.set_sideband(**sb)
    b.set_sideband(**sb)
    for f in range(2):
        part = keyed_am[:, 2 * n * f:2 * n * (f + 1)]
        for call in ("listen", "listen_sideband"):
            got, want = getattr(a, call)(part, dd.CS8, ALL), getattr(b, call)(part, dd.CS8, ALL)
            assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want)), (f, call)
    assert a.tones_config()["samples_consumed"] == 0  # set, and not asked for: it neither listens nor moves
    a.close()
    b.close()
