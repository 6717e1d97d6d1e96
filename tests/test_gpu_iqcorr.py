"""GPU tests of the IQ correction stage (csrc/iqcorr.hip, sdrg_engine_iqcorr_*): the corrected rows and the records of
each stream against the NumPy restatement in tests/iqcorr_cases.py fed the library's own design values.  Every comparison
is of the bytes of the whole `out` and of the records (the stage is specified operation by operation: no tolerances).
`out` and `records` are pre-filled with 0xAA between 64 guard bytes on either side, every stream has its own data, and
the input rows hold NaN (CF32) or a loud filler (the integer formats) past the call's n samples.

The moments kernel works in tiles of `tile` positions counted from the start of the block in progress, the pass kernel in
tiles of `tile` samples of the call (sdrg.iqcorr_geometry), blocks above 128 samples meet in LDS, and rows or offsets
that are not aligned to a pair of samples take one-sample loads: the shapes below put data on each of these paths."""
import ctypes

import numpy as np
import pytest

import iqcorr_cases as iq
import squelch_cases as sq
from stage_harness import GUARD, engine, invalid, out_buffer, read_out, same, to_device

pytestmark = pytest.mark.gpu

BASE = dict(dc_tau_blocks=3.0, balance_tau_blocks=2.0, floor_db=-60.0, mode=3, block=64, max_in=2048)
BPS = {iq.CS8: 2, iq.CU8: 2, iq.CS16: 4, iq.CF32: 8}
SCALE = {iq.CS8: 100.0, iq.CU8: 100.0, iq.CS16: 20000.0, iq.CF32: 1.0}
FORMATS = (iq.CS8, iq.CU8, iq.CS16, iq.CF32)


@pytest.fixture(scope="module")
def S():
    import sdrg
    return sdrg


@pytest.fixture(scope="module")
def T():
    import torch
    return torch


def signal(B, n, seed, fmt, amp=0.3):
    """Every stream its own impaired noise with its own offset, as raw [B][2 n] of fmt."""
    z = iq.impaired(iq.noise(B, n, seed, amp), dc=0.05 - 0.02j)
    z = z + (0.01 * np.arange(B))[:, None]
    return iq.to_raw(z, fmt, SCALE[fmt])


def rows_of(raw, fmt, stride):
    """raw [B][2 n] -> [B][2 stride] of the same type: NaN, or a loud filler, past n."""
    B = raw.shape[0]
    rows = np.full((B, 2 * stride), np.nan if fmt == iq.CF32 else 113, iq.RAW_DTYPE[fmt])
    rows[:, :raw.shape[1]] = raw
    return rows


class Rig:
    """An engine with the stage set, and the restatement that follows it call by call."""

    def __init__(self, S, T, B, n=1024, **cfg):
        self.S, self.T, self.B = S, T, B
        self.eng = engine(S, B, n)
        self.configure(**cfg)

    def configure(self, **cfg):
        self.cfg = cfg
        self.eng.set_iqcorr(**cfg)
        self.remodel()

    def remodel(self):
        d = self.eng.iqcorr_config()
        des = self.S.iqcorr_design(**self.cfg)
        assert all(d[k] == v for k, v in self.cfg.items()), d
        assert all(des[k].tobytes() == d[k].tobytes() for k in des) and d["samples_consumed"] == 0
        self.model = iq.Iqcorr(self.B, d["beta_dc"], d["beta_bal"], d["floor_thr"], d["mode"], d["block"])

    def device_call(self, raw, fmt, in_stride=None, records=True, in_place=False, in_shift=0, out_shift=0):
        """iqcorr_device into 0xAA-filled buffers between guard bytes: (out [B][stride] complex64, records [B][8] as
        uint32 or None, n_blocks).  in_shift, out_shift: bytes by which iq and out are moved off a 16-byte alignment."""
        T, B = self.T, self.B
        n = raw.shape[1] // 2
        stride = self.cfg["max_in"] if in_stride is None else in_stride
        rows = rows_of(raw, fmt, stride).view(np.uint8).reshape(-1)
        nbytes = B * stride * 8
        out_t = out_buffer(T, nbytes + out_shift)
        rec_t = out_buffer(T, B * 32)
        at = GUARD + out_shift
        if in_place:
            assert fmt == iq.CF32
            out_t[at:at + nbytes] = T.from_numpy(rows).to("cuda:0")
            iq_ptr = out_t.data_ptr() + at
        else:
            iq_t = T.zeros((rows.size + in_shift,), dtype=T.uint8, device="cuda:0")
            iq_t[in_shift:] = T.from_numpy(rows).to("cuda:0")
            iq_ptr = iq_t.data_ptr() + in_shift
        T.cuda.synchronize()
        nb = self.eng.iqcorr_device(iq_ptr, fmt, stride, n, out_t.data_ptr() + at, rec_t.data_ptr() + GUARD if records else None)
        self.eng.synchronize()
        o = out_t.cpu().numpy()
        assert np.all(o[:at] == 0xAA) and np.all(o[at + nbytes:] == 0xAA), "bytes outside out"
        out = o[at:at + nbytes].copy().view(np.complex64).reshape(B, stride)
        if not records:
            assert np.all(rec_t.cpu().numpy() == 0xAA), "records written without a pointer"
            return out, None, nb
        return out, read_out(rec_t, (B, 8), np.uint32), nb

    def check(self, raw, fmt, what=None, **kw):
        got, rec, nb = self.device_call(raw, fmt, **kw)
        want, want_rec, want_nb = self.model.call(raw, fmt, in_stride=got.shape[1])
        same(got, nb, want, want_nb, what)
        if rec is not None:
            same(rec, nb, want_rec.view(np.uint32).reshape(self.B, 8), want_nb, (what, "records"))
            rec = rec.view(self.S.IqcorrRecord)[:, 0]
        assert self.eng.iqcorr_config()["samples_consumed"] == self.model.g
        return got, rec, nb

    def restart(self):
        self.eng.iqcorr_reset()
        self.model.reset()

    def close(self):
        self.eng.close()


@pytest.mark.parametrize("fmt", FORMATS)
def test_formats_modes_and_stream_counts(S, T, fmt):
    """The step kernel takes 64 streams per wave: a wave in part, and a wave and a stream."""
    ns = (700, 5, 1343)
    for B in (1, 9, 65):
        raw = signal(B, sum(ns), 100 + B, fmt)
        r = Rig(S, T, B, **BASE)
        for mode in (iq.DC, iq.BALANCE, iq.DC | iq.BALANCE):
            r.configure(**dict(BASE, mode=mode))
            at = 0
            for f, n in enumerate(ns):
                _, rec, _ = r.check(raw[:, 2 * at:2 * (at + n)], fmt, (B, mode, f))
                at += n
            assert rec["seeded"].all() == bool(mode & iq.BALANCE) and (rec["dc_re"] != 0).all() == bool(mode & iq.DC)
        r.close()


@pytest.mark.parametrize("block", [64, 256, 1024])
def test_call_lengths_around_the_block_and_the_tile(S, T, block):
    """Every n as a fresh stream's first call and as a call that follows whatever the others left: odd and even offsets,
    in a wave (S = 64), across the waves through LDS (256), and across the workgroup's two passes (1024)."""
    B, tile = 3, S.iqcorr_geometry(block)
    ns = (0, 1, 2, 63, 64, 65, block - 1, block, block + 1, tile - 1, tile + 1, 3 * tile + 5)
    r = Rig(S, T, B, **dict(BASE, block=block, max_in=3 * tile + 6))
    for j, fmt in enumerate(FORMATS if block == 64 else (iq.CS8, iq.CF32)):
        raw = signal(B, 2 * sum(ns), 200 + block + j, fmt)
        r.restart()
        at, blocks = 0, 0
        for f, n in enumerate(ns):  # one stream
            got, rec, nb = r.check(raw[:, 2 * at:2 * (at + n)], fmt, (block, fmt, f, n), in_stride=max(n, 1) + (f & 1))
            at, blocks = at + n, blocks + nb
            if n == 0:
                assert nb == 0 and not got.view(np.uint32).any()
        assert blocks == sum(ns) // block
        for n in ns:  # each the first call
            r.restart()
            r.check(raw[:, 2 * at:2 * (at + n)], fmt, (block, fmt, "first", n), in_stride=max(n, 1))
            at += n
    r.close()


@pytest.mark.parametrize("fmt", FORMATS)
def test_odd_offsets_and_rows_that_are_not_aligned(S, T, fmt):
    """After a first call of 1, 2 or 3 samples the next starts at an odd or an even offset; in_stride odd, iq moved by
    one sample and out by 8 bytes take the one-sample loads and the 8-byte stores."""
    B = 3
    r = Rig(S, T, B, **BASE)
    raw = signal(B, 4000, 300 + fmt, fmt)
    at = 0
    for first in (1, 2, 3):
        for kw in (dict(), dict(in_stride=777), dict(in_shift=BPS[fmt]), dict(out_shift=8), dict(in_stride=701, out_shift=8)):
            r.restart()
            for n in (first, 700):
                r.check(raw[:, 2 * at:2 * (at + n)], fmt, (first, n, kw), **(kw if n == 700 else {}))
                at = (at + n) % 3000
    r.close()


def test_five_calls_are_one_stream_whatever_their_formats(S, T):
    B = 4
    r = Rig(S, T, B, **BASE)
    ns = (700, 64, 1, 2048, 333)
    fmts = (iq.CS8, iq.CF32, iq.CS16, iq.CU8, iq.CF32)
    z = iq.impaired(iq.noise(B, sum(ns), 50, 0.3), dc=0.04 + 0.03j)
    outs, zs, at = [], [], 0
    for f, (n, fmt) in enumerate(zip(ns, fmts)):
        raw = iq.to_raw(z[:, at:at + n], fmt, SCALE[fmt])
        got, rec, _ = r.check(raw, fmt, f)
        outs.append(got[:, :n])
        zr, zi = iq.sample(raw, fmt)
        zs.append(np.stack([zr, zi], axis=-1).reshape(B, -1))
        at += n
    d = r.eng.iqcorr_config()  # the scaled samples of the five calls, as one CF32 call
    want, want_rec, _ = iq.one_call(np.concatenate(zs, axis=1), iq.CF32, d["beta_dc"], d["beta_bal"], d["floor_thr"], 3, 64)
    assert np.concatenate(outs, axis=1).tobytes() == want.tobytes()
    assert rec["w_re"].tobytes() == want_rec["w_re"].tobytes() and rec["dc_im"].tobytes() == want_rec["dc_im"].tobytes()
    r.close()


def test_calls_that_complete_no_block(S, T):
    B = 2
    r = Rig(S, T, B, **dict(BASE, block=1024))
    raw = signal(B, 1100, 60, iq.CS16)
    at = 0
    for f, n in enumerate((10, 0, 21, 500, 1, 400, 92, 76)):  # the block completes in the seventh call
        got, rec, nb = r.check(raw[:, 2 * at:2 * (at + n)], iq.CS16, (f, n), records=f != 3)
        at += n
        assert nb == (1 if f == 6 else 0)
        if f < 6:  # nothing estimated yet: the scaled samples pass whole
            zr, zi = iq.sample(raw[:, 2 * (at - n):2 * at], iq.CS16)
            assert np.array_equal(got[:, :n].real, zr) and np.array_equal(got[:, :n].imag, zi)
    assert rec["seeded"].all()
    r.close()


def test_cf32_in_place(S, T):
    B = 5
    r = Rig(S, T, B, **BASE)
    raw = signal(B, 3000, 70, iq.CF32)
    at = 0
    for f, (n, kw) in enumerate(((1000, {}), (33, {}), (900, dict(in_stride=901)), (1067, dict(out_shift=8)))):
        r.check(raw[:, 2 * at:2 * (at + n)], iq.CF32, (f, n), in_place=True, **kw)
        at += n
    r.close()


@pytest.mark.parametrize("floor_db", [-60.0, -440.0])
def test_amplitudes_down_to_1e_21(S, T, floor_db):
    """Blocks of amplitude 1, 1e-7, 1e-14 and 1e-21: their powers are normal, then denormal, then zero.  Under a floor of
    -60 dB all but the loud blocks hold; under a denormal floor the balance follows the quiet ones as far as their
    powers are numbers."""
    B, block = 3, 64
    r = Rig(S, T, B, **dict(BASE, floor_db=floor_db, dc_tau_blocks=0.0))
    amps = np.repeat(np.array([1.0, 1e-7, 1.0, 1e-14, 1e-21, 1e-21, 1.0, 1e-14]), 2 * block)
    z = iq.impaired(iq.noise(B, amps.size, 80, 0.5), dc=0.1 + 0.1j) * amps[None, :]
    raw = iq.to_raw(z, iq.CF32)
    _, rec, nb = r.check(raw[:, :2 * 700], iq.CF32, "head")
    _, rec2, nb2 = r.check(raw[:, 2 * 700:], iq.CF32, "tail")
    assert nb + nb2 == 16 and rec2["seeded"].all()
    if floor_db == -60.0:  # the six loud blocks move the balance
        assert (rec["held_blocks"] + rec2["held_blocks"] == 10).all()
    r.close()


def test_64_streams_of_16384(S, T):
    B, n = 64, 16384
    r = Rig(S, T, B, **dict(BASE, block=256, max_in=n, dc_tau_blocks=16.0, balance_tau_blocks=16.0))
    _, rec, nb = r.check(signal(B, n, 90, iq.CS16), iq.CS16)
    assert nb == 64 and rec["seeded"].all() and (rec["image_db"] < -20).all()
    r.close()


def test_reset_and_set_again_restart_the_streams(S, T):
    B = 3
    r = Rig(S, T, B, **BASE)
    raw = signal(B, 2000, 95, iq.CU8)
    first, _, _ = r.check(raw[:, :2 * 900], iq.CU8)
    r.check(raw[:, 2 * 900:], iq.CU8)
    r.restart()
    again, _, _ = r.check(raw[:, :2 * 900], iq.CU8)
    assert again.tobytes() == first.tobytes()
    r.check(raw[:, 2 * 900:2 * 950], iq.CU8)
    invalid(S, r.eng.set_iqcorr, **dict(BASE, block=48))  # a rejected set changes nothing
    assert r.eng.iqcorr_config()["samples_consumed"] == 950
    r.check(raw[:, 2 * 950:2 * 1000], iq.CU8)
    r.configure(**dict(BASE, block=128))  # an accepted one restarts
    r.check(raw[:, :2 * 900], iq.CU8)
    r.close()


def test_refusals_commit_nothing(S, T):
    B = 2
    r = Rig(S, T, B, **dict(BASE, max_in=512))
    raw = signal(B, 512, 96, iq.CS8)
    r.check(raw[:, :2 * 100], iq.CS8)
    buf = to_device(T, np.zeros(2 * B * 512 * 8, np.uint8))
    p = buf.data_ptr()
    L, h = S.load(), r.eng._h
    nb, ref = ctypes.c_int32(-7), ctypes.byref
    for args in ((p, iq.CS8, 512, 513, p), (p, iq.CS8, 513, 100, p), (p, iq.CS8, 99, 100, p), (p, iq.CS8, 512, -1, p),
                 (p, 4, 512, 100, p), (p, -1, 512, 100, p), (p, iq.CS8, 0, 0, p), (None, iq.CS8, 512, 100, p),
                 (p, iq.CS8, 512, 100, None)):
        assert L.sdrg_engine_iqcorr_device(h, *args, None, ref(nb)) == -1, args
    assert L.sdrg_engine_iqcorr_device(h, p, iq.CS8, 512, 100, p, None, None) == -1
    assert L.sdrg_engine_iqcorr_device(h, p + 1, iq.CS16, 512, 100, p + 2048, None, ref(nb)) != 0  # a misaligned int16
    assert L.sdrg_engine_iqcorr_device(h, p, iq.CS8, 512, 100, p + 2052, None, ref(nb)) != 0  # out off 8 bytes
    assert L.sdrg_engine_iqcorr_device(None, p, iq.CS8, 512, 100, p, None, ref(nb)) == -1
    assert nb.value == -7 and r.eng.iqcorr_config()["samples_consumed"] == 100
    r.eng.synchronize()
    assert not buf.cpu().numpy().any(), "a refused call wrote"
    r.check(raw[:, 2 * 100:], iq.CS8)  # the stream goes on where it was
    r.eng.set_iqcorr(off=True)
    invalid(S, r.eng.iqcorr_config)
    invalid(S, r.eng.iqcorr_device, p, iq.CS8, 512, 100, p)
    invalid(S, r.eng.iqcorr_host, raw, iq.CS8)
    r.close()


@pytest.mark.parametrize("fmt", FORMATS)
def test_host_path(S, T, fmt):
    B = 3
    r = Rig(S, T, B, **BASE)
    raw = signal(B, 1500, 97, fmt)
    at = 0
    for n, want_records in ((700, True), (0, True), (1, False), (799, True)):
        out, rec, nb = r.eng.iqcorr_host(raw[:, 2 * at:2 * (at + n)], fmt, want_records)
        want, want_rec, want_nb = r.model.call(raw[:, 2 * at:2 * (at + n)], fmt)
        same(out, nb, want, want_nb, (fmt, n))
        assert (rec is None) == (not want_records)
        if want_records:
            assert rec.tobytes() == want_rec.tobytes()
        at += n
    assert r.eng.iqcorr_config()["samples_consumed"] == 1500
    r.close()


def test_other_stages_between_correction_calls(S, T):
    """process_device and squelch_device on the same engine between two correction calls: the stream goes on as if they
    were not there, and the squelch gates the corrected rows in place."""
    B, n = 4, 1024
    r = Rig(S, T, B, n, **dict(BASE, max_in=n))
    sqc = dict(open_db=-20.0, close_db=-30.0, tau_blocks=0.0, block=64, hang_blocks=1, max_in=n)
    r.eng.set_squelch(**sqc)
    d = r.eng.squelch_config()
    gate = sq.Squelch(B, d["open_thr"], d["close_thr"], d["beta"], 64, 1)
    raw = signal(B, 3 * n, 98, iq.CS8)
    spec = T.zeros((B, n), dtype=T.float32, device="cuda:0")
    for f in range(3):
        frame = raw[:, 2 * f * n:2 * (f + 1) * n]
        got, _, _ = r.check(frame, iq.CS8, f)
        iq_t = to_device(T, frame)
        rc = S.load().sdrg_engine_process_device(r.eng._h, iq_t.data_ptr(), iq.CS8, S.STAGE_SPECTRUM, spec.data_ptr(),
                                                 None, None, 0)
        assert rc == 0
        rows = to_device(T, got.view(np.float32))
        nb = r.eng.squelch_device(rows.data_ptr(), n, n, rows.data_ptr())
        r.eng.synchronize()
        want, _, want_nb = gate.call(got)
        same(rows.cpu().numpy().view(np.complex64).reshape(B, n), nb, want, want_nb, ("squelch", f))
    assert np.isfinite(spec.cpu().numpy()).all()
    r.close()


def test_chain_call_is_the_correction_then_process(S, T):
    """iqcorr_process_host against iqcorr_host followed by process_host on its rows as CF32, on a second engine."""
    B, n = 4, 4096
    cfg = dict(BASE, block=256, max_in=n)
    a, b = Rig(S, T, B, n, **cfg), Rig(S, T, B, n, **cfg)
    raw = signal(B, 2 * n, 99, iq.CS16)
    for f in range(2):
        frame = raw[:, 2 * f * n:2 * (f + 1) * n]
        spec, recs, pcm, iq_rec = a.eng.iqcorr_process(frame, iq.CS16, S.STAGE_ALL, now_ms=1000 + 10 * f)
        rows, want_iq_rec, _ = b.eng.iqcorr_host(frame, iq.CS16)
        want_spec, want_recs, want_pcm = b.eng.process(rows.view(np.float32), S.CF32, S.STAGE_ALL, now_ms=1000 + 10 * f)
        model_rows, model_rec, _ = a.model.call(frame, iq.CS16)
        assert rows.tobytes() == model_rows.tobytes() and iq_rec.tobytes() == model_rec.tobytes() == want_iq_rec.tobytes()
        assert spec.tobytes() == want_spec.tobytes() and recs.tobytes() == want_recs.tobytes(), f
        assert pcm.size > 0 and pcm.tobytes() == want_pcm.tobytes(), f
        assert a.eng.iqcorr_config()["samples_consumed"] == (f + 1) * n
    # its refusals move no stage: a bad mask, the stage's max_in under the frame, the stage off
    invalid(S, a.eng.iqcorr_process, raw[:, :2 * n], iq.CS16, 1 << 20)
    assert a.eng.iqcorr_config()["samples_consumed"] == 2 * n
    a.eng.set_iqcorr(**dict(cfg, max_in=n - 1))
    invalid(S, a.eng.iqcorr_process, raw[:, :2 * n], iq.CS16)
    assert a.eng.iqcorr_config()["samples_consumed"] == 0
    a.eng.set_iqcorr(off=True)
    invalid(S, a.eng.iqcorr_process, raw[:, :2 * n], iq.CS16)
    spec, _, _ = a.eng.process(raw[:, :2 * n], iq.CS16, S.STAGE_SPECTRUM)  # process_host itself goes on uncorrected
    want_spec, _, _ = b.eng.process(raw[:, :2 * n], iq.CS16, S.STAGE_SPECTRUM)
    assert spec.tobytes() == want_spec.tobytes()
    a.close()
    b.close()


def test_selectivity_cu8(S, T):
    """The CU8 receiver of tests/test_iqcorr_cases.py at S = 256 in one call: the restatement's bytes, and with them its
    image and offset at least 60 dB under the tone."""
    r = Rig(S, T, 1, **dict(BASE, dc_tau_blocks=16.0, balance_tau_blocks=16.0, block=256, max_in=iq.N_SEL))
    got, rec, nb = r.check(iq.receiver(iq.CU8), iq.CU8)
    image, dc = iq.levels_db(got[0])
    print("image %.1f dB and DC %.1f dB under the tone" % (image, dc))
    assert nb == iq.N_SEL // 256 and image >= 60.0 and dc >= 60.0
    r.close()
