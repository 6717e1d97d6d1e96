"""GPU tests of the noise blanker stage (csrc/blanker.hip, sdrg_engine_blanker_*, sdrg_engine_clean_process_host): the
blanked rows and the records of each stream against the NumPy restatement in tests/blanker_cases.py fed the library's own
design values.  Every comparison is of the bytes of the whole `out` and of the records (the stage is specified operation
by operation: no tolerances).  `out` and `records` are pre-filled with 0xAA between 64 guard bytes on either side, every
stream has its own data, and the input rows hold NaN (CF32) or a loud filler (the integer formats) past the call's n
samples.

The floor kernel works in tiles of floor_tile positions counted from the start of the block in progress, the pass kernel
in tiles of pass_tile outputs of the call (sdrg.blanker_geometry) with the lead + tail inputs before a tile decided a
second time, blocks above 128 samples meet in LDS, and rows or offsets that are not aligned to a pair of samples take
one-sample loads: the shapes below put data, and pulses, on each of these paths and seams.  `out` overlapping `iq` is
undefined and not detected (include/sdrg.h): it is not tested."""
import ctypes

import numpy as np
import pytest

import blanker_cases as bk
import iqcorr_cases as iq
from stage_harness import GUARD, engine, invalid, out_buffer, read_out, same, to_device

pytestmark = pytest.mark.gpu

BASE = dict(tau_blocks=3.0, threshold_db=10.0, floor_db=-60.0, block=64, lead=3, tail=7, max_in=2048)
BPS = {bk.CS8: 2, bk.CU8: 2, bk.CS16: 4, bk.CF32: 8}
SCALE = {bk.CS8: 100.0, bk.CU8: 100.0, bk.CS16: 20000.0, bk.CF32: 1.0}
FORMATS = (bk.CS8, bk.CU8, bk.CS16, bk.CF32)
WINDOWS = ((0, 0), (0, 64), (16, 0), (16, 64), (3, 7))


@pytest.fixture(scope="module")
def S():
    import sdrg
    return sdrg


@pytest.fixture(scope="module")
def T():
    import torch
    return torch


def signal(B, n, seed, fmt, at=(), every=97):
    """Every stream its own noise of amplitude 0.1 with its own pulses of 0.9: one every `every` samples from a start of
    its own, and at the indices `at` in every stream; as raw [B][2 n] of fmt."""
    z = bk.gaussian(B, n, seed, 0.1).astype(np.complex128)
    for b in range(B):
        z[b, (11 * b + 5) % every::every] += 0.9
    z[:, [a for a in at if a < n]] += 0.9j
    return bk.to_raw(z, fmt, SCALE[fmt])


def rows_of(raw, fmt, stride):
    """raw [B][2 n] -> [B][2 stride] of the same type: NaN, or a loud filler, past n."""
    B = raw.shape[0]
    rows = np.full((B, 2 * stride), np.nan if fmt == bk.CF32 else 113, bk.RAW_DTYPE[fmt])
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
        self.eng.set_blanker(**cfg)
        self.remodel()

    def remodel(self):
        d = self.eng.blanker_config()
        des = self.S.blanker_design(**self.cfg)
        assert all(d[k] == v for k, v in self.cfg.items()), d
        assert all(des[k].tobytes() == d[k].tobytes() for k in des) and d["samples_consumed"] == 0
        self.model = bk.Blanker(self.B, d["beta"], d["ratio"], d["floor_thr"], d["block"], d["lead"], d["tail"])

    def device_call(self, raw, fmt, in_stride=None, records=True, in_shift=0, out_shift=0):
        """blanker_device into 0xAA-filled buffers between guard bytes: (out [B][stride] complex64, records [B][4] as
        uint32 or None, n_blocks).  in_shift, out_shift: bytes by which iq and out are moved off a 16-byte alignment."""
        T, B = self.T, self.B
        n = raw.shape[1] // 2
        stride = self.cfg["max_in"] if in_stride is None else in_stride
        rows = rows_of(raw, fmt, stride).view(np.uint8).reshape(-1)
        nbytes = B * stride * 8
        out_t = out_buffer(T, nbytes + out_shift)
        rec_t = out_buffer(T, B * 16)
        at = GUARD + out_shift
        iq_t = T.zeros((rows.size + in_shift,), dtype=T.uint8, device="cuda:0")
        iq_t[in_shift:] = T.from_numpy(rows).to("cuda:0")
        T.cuda.synchronize()
        nb = self.eng.blanker_device(iq_t.data_ptr() + in_shift, fmt, stride, n, out_t.data_ptr() + at,
                                     rec_t.data_ptr() + GUARD if records else None)
        self.eng.synchronize()
        o = out_t.cpu().numpy()
        assert np.all(o[:at] == 0xAA) and np.all(o[at + nbytes:] == 0xAA), "bytes outside out"
        out = o[at:at + nbytes].copy().view(np.complex64).reshape(B, stride)
        if not records:
            assert np.all(rec_t.cpu().numpy() == 0xAA), "records written without a pointer"
            return out, None, nb
        return out, read_out(rec_t, (B, 4), np.uint32), nb

    def check(self, raw, fmt, what=None, **kw):
        got, rec, nb = self.device_call(raw, fmt, **kw)
        want, want_rec, want_nb = self.model.call(raw, fmt, in_stride=got.shape[1])
        same(got, nb, want, want_nb, what)
        if rec is not None:
            same(rec, nb, want_rec.view(np.uint32).reshape(self.B, 4), want_nb, (what, "records"))
            rec = rec.view(self.S.BlankerRecord)[:, 0]
        assert self.eng.blanker_config()["samples_consumed"] == self.model.g
        return got, rec, nb

    def stream(self, raw, fmt, ns, what=None, **kw):
        """The calls of ns samples one after the other: the records' hits and blanked outputs summed."""
        at, hits, blanked = 0, 0, 0
        for f, n in enumerate(ns):
            _, rec, _ = self.check(raw[:, 2 * at:2 * (at + n)], fmt, (what, f, n), in_stride=max(n, 1), **kw)
            at, hits, blanked = at + n, hits + rec["hits"], blanked + rec["blanked"]
        return hits, blanked

    def restart(self):
        self.eng.blanker_reset()
        self.model.reset()

    def close(self):
        self.eng.close()


@pytest.mark.parametrize("fmt", FORMATS)
def test_formats_blocks_and_stream_counts(S, T, fmt):
    """The step kernel takes 64 streams per wave: a wave in part, and a wave and a stream; every block length's way
    through the butterfly, LDS and the workgroup's two passes."""
    ns = (700, 5, 1343)
    for B in (1, 9, 65):
        raw = signal(B, sum(ns), 100 + B, fmt)
        r = Rig(S, T, B, **BASE)
        for block in (64, 128, 256, 512, 1024):
            r.configure(**dict(BASE, block=block))
            hits, blanked = r.stream(raw, fmt, ns, (B, block))
            assert (hits > 0).all() and (blanked > hits).all()
        r.close()


@pytest.mark.parametrize("block", [64, 256, 1024])
def test_call_lengths_around_the_window_the_block_and_the_tile(S, T, block):
    """Every n as a fresh stream's first call and as a call that follows whatever the others left, with the widest
    window: shorter than the halo, around a pass tile and around a floor tile."""
    B, lead, tail = 3, 16, 64
    floor_tile, tile = S.blanker_geometry(block)
    ns = [0, 1, 2, lead + tail - 1, lead + tail, tile - 1, tile, tile + 1, 2 * tile + 3]
    ns += [floor_tile - 1, floor_tile + 1] if floor_tile != tile else []
    r = Rig(S, T, B, **dict(BASE, block=block, lead=lead, tail=tail, max_in=2 * tile + 4))
    for j, fmt in enumerate(FORMATS if block == 64 else (bk.CS8, bk.CF32)):
        raw = signal(B, 2 * sum(ns), 200 + block + j, fmt, every=61)
        r.restart()
        at, blocks = 0, 0
        for f, n in enumerate(ns):  # one stream
            got, rec, nb = r.check(raw[:, 2 * at:2 * (at + n)], fmt, (block, fmt, f, n), in_stride=max(n, 1) + (f & 1),
                                   records=f != 3)
            at, blocks = at + n, blocks + nb
            if n == 0:
                assert nb == 0 and not got.view(np.uint32).any() and not rec["hits"].any()
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


@pytest.mark.parametrize("lead,tail", WINDOWS)
def test_pulses_on_every_seam(S, T, lead, tail):
    """Calls of 1300, 5, 7, 3, 40, 600 and 1045 samples.  Pulses at the call's indices 511 and 512 (the last input of a
    pass tile, its tail in the next; the first input of a tile, its lead in the one before), 1023 and 1024 (the same, and
    a block's last and first sample), at 127 and 128 (a block seam inside a tile), at 1299 and 1290 (in the last lead
    inputs of a call and within tail of its end: they blank outputs of the next calls), in the short calls (several in a
    row shorter than the halo), and at 1866 and 1867, the seam of the sixth call's first two tiles."""
    B = 3
    ns = (1300, 5, 7, 3, 40, 600, 1045)
    at = (127, 128, 511, 512, 1023, 1024, 1290, 1299, 1302, 1306, 1313, 1350, 1866, 1867, 2999)
    r = Rig(S, T, B, **dict(BASE, lead=lead, tail=tail, tau_blocks=0.0))
    for fmt in (bk.CS8, bk.CF32):
        r.restart()
        raw = signal(B, sum(ns), 400 + lead + tail, fmt, at, every=389)
        hits, blanked = r.stream(raw, fmt, ns, (lead, tail, fmt))
        assert (hits >= len(at)).all()
        assert np.array_equal(blanked, hits) if lead + tail == 0 else (blanked > hits).all()
    r.close()


def test_five_calls_are_one_stream_whatever_their_formats(S, T):
    B = 4
    r = Rig(S, T, B, **BASE)
    ns = (700, 64, 1, 2048, 333)
    fmts = (bk.CS8, bk.CF32, bk.CS16, bk.CU8, bk.CF32)
    z = bk.gaussian(B, sum(ns), 50, 0.1).astype(np.complex128)
    z[:, 70::131] += 0.9
    outs, zs, at, hits, blanked = [], [], 0, 0, 0
    for f, (n, fmt) in enumerate(zip(ns, fmts)):
        raw = bk.to_raw(z[:, at:at + n], fmt, SCALE[fmt])
        got, rec, _ = r.check(raw, fmt, f)
        outs.append(got[:, :n])
        zr, zi = bk.sample(raw, fmt)
        zs.append(zr + 1j * zi)
        at, hits, blanked = at + n, hits + rec["hits"], blanked + rec["blanked"]
    d = r.eng.blanker_config()  # the scaled samples of the five calls, as one stream under the second model
    got, zs = np.concatenate(outs, axis=1), np.concatenate(zs, axis=1)
    for b in range(B):
        want, L, h, k = bk.whole_stream(zs[b], d["beta"], d["ratio"], d["floor_thr"], 64, BASE["lead"], BASE["tail"])
        assert got[b].tobytes() == want.tobytes() and (L, h, k) == (rec["level"][b], hits[b], blanked[b])
    r.close()


def test_reset_and_set_again_restart_the_streams(S, T):
    B = 3
    r = Rig(S, T, B, **BASE)
    raw = signal(B, 2000, 95, bk.CU8)
    first, _, _ = r.check(raw[:, :2 * 900], bk.CU8)
    r.check(raw[:, 2 * 900:], bk.CU8)
    r.restart()
    again, _, _ = r.check(raw[:, :2 * 900], bk.CU8)
    assert again.tobytes() == first.tobytes()
    r.check(raw[:, 2 * 900:2 * 950], bk.CU8)
    invalid(S, r.eng.set_blanker, **dict(BASE, block=48))  # a rejected set changes nothing
    invalid(S, r.eng.set_blanker, **dict(BASE, lead=17))
    assert r.eng.blanker_config()["samples_consumed"] == 950
    r.check(raw[:, 2 * 950:2 * 1000], bk.CU8)
    r.configure(**dict(BASE, block=128, lead=0))  # an accepted one restarts
    r.check(raw[:, :2 * 900], bk.CU8)
    r.close()


def test_refusals_commit_nothing(S, T):
    B = 2
    r = Rig(S, T, B, **dict(BASE, max_in=512))
    raw = signal(B, 512, 96, bk.CS8)
    r.check(raw[:, :2 * 100], bk.CS8)
    buf = to_device(T, np.zeros(2 * B * 512 * 8, np.uint8))
    p = buf.data_ptr()
    q = p + B * 512 * 8  # out beside iq, not over it
    L, h = S.load(), r.eng._h
    nb, ref = ctypes.c_int32(-7), ctypes.byref
    for args in ((p, bk.CS8, 512, 513, q), (p, bk.CS8, 513, 100, q), (p, bk.CS8, 99, 100, q), (p, bk.CS8, 512, -1, q),
                 (p, 4, 512, 100, q), (p, -1, 512, 100, q), (p, bk.CS8, 0, 0, q), (None, bk.CS8, 512, 100, q),
                 (p, bk.CS8, 512, 100, None)):
        assert L.sdrg_engine_blanker_device(h, *args, None, ref(nb)) == -1, args
    assert L.sdrg_engine_blanker_device(h, p, bk.CS8, 512, 100, q, None, None) == -1
    assert L.sdrg_engine_blanker_device(h, p + 1, bk.CS16, 512, 100, q, None, ref(nb)) != 0  # a misaligned int16
    assert L.sdrg_engine_blanker_device(h, p, bk.CS8, 512, 100, q + 4, None, ref(nb)) != 0  # out off 8 bytes
    assert L.sdrg_engine_blanker_device(None, p, bk.CS8, 512, 100, q, None, ref(nb)) == -1
    assert nb.value == -7 and r.eng.blanker_config()["samples_consumed"] == 100
    r.eng.synchronize()
    assert not buf.cpu().numpy().any(), "a refused call wrote"
    r.check(raw[:, 2 * 100:], bk.CS8)  # the stream goes on where it was
    r.eng.set_blanker(off=True)
    invalid(S, r.eng.blanker_config)
    invalid(S, r.eng.blanker_device, p, bk.CS8, 512, 100, q)
    invalid(S, r.eng.blanker_host, raw, bk.CS8)
    r.close()


@pytest.mark.parametrize("fmt", FORMATS)
def test_host_path(S, T, fmt):
    B = 3
    r = Rig(S, T, B, **BASE)
    raw = signal(B, 1500, 97, fmt)
    at = 0
    for n, want_records in ((700, True), (0, True), (1, False), (799, True)):
        out, rec, nb = r.eng.blanker_host(raw[:, 2 * at:2 * (at + n)], fmt, want_records)
        want, want_rec, want_nb = r.model.call(raw[:, 2 * at:2 * (at + n)], fmt)
        same(out, nb, want, want_nb, (fmt, n))
        assert (rec is None) == (not want_records)
        if want_records:
            assert rec.tobytes() == want_rec.tobytes()
        at += n
    assert r.eng.blanker_config()["samples_consumed"] == 1500
    r.close()


def test_other_stages_between_blanker_calls(S, T):
    """iqcorr_device and process_device on the same engine between two blanker calls: the stream goes on as if they were
    not there, and the blanker takes the corrected rows as CF32."""
    B, n = 4, 1024
    r = Rig(S, T, B, n, **dict(BASE, max_in=n))
    icfg = dict(dc_tau_blocks=3.0, balance_tau_blocks=2.0, floor_db=-60.0, mode=3, block=64, max_in=n)
    r.eng.set_iqcorr(**icfg)
    d = r.eng.iqcorr_config()
    corr = iq.Iqcorr(B, d["beta_dc"], d["beta_bal"], d["floor_thr"], 3, 64)
    raw = signal(B, 3 * n, 98, bk.CS8)
    spec = T.zeros((B, n), dtype=T.float32, device="cuda:0")
    rows = T.zeros((B, n, 2), dtype=T.float32, device="cuda:0")
    for f in range(3):
        frame = raw[:, 2 * f * n:2 * (f + 1) * n]
        iq_t = to_device(T, frame)
        assert r.eng.iqcorr_device(iq_t.data_ptr(), bk.CS8, n, n, rows.data_ptr()) == n // 64
        rc = S.load().sdrg_engine_process_device(r.eng._h, iq_t.data_ptr(), bk.CS8, S.STAGE_SPECTRUM, spec.data_ptr(),
                                                 None, None, 0)
        assert rc == 0
        r.eng.synchronize()
        want, _, _ = corr.call(frame, bk.CS8)
        got = rows.cpu().numpy().view(np.complex64).reshape(B, n)
        assert got.tobytes() == want.tobytes()
        r.check(got.view(np.float32), bk.CF32, f)
    assert np.isfinite(spec.cpu().numpy()).all()
    r.close()


@pytest.mark.parametrize("mask", [0, 1])
def test_chain_call_is_the_cleaning_then_process(S, T, mask):
    """clean_process_host against [iqcorr_host,] blanker_host and process_host on the rows as CF32, on a second engine,
    and against the restatements chained."""
    B, n = 4, 4096
    cfg = dict(BASE, block=256, max_in=n)
    icfg = dict(dc_tau_blocks=3.0, balance_tau_blocks=2.0, floor_db=-60.0, mode=3, block=256, max_in=n)
    a, b = Rig(S, T, B, n, **cfg), Rig(S, T, B, n, **cfg)
    for e in (a.eng, b.eng):
        e.set_iqcorr(**icfg)
    d = a.eng.iqcorr_config()
    corr = iq.Iqcorr(B, d["beta_dc"], d["beta_bal"], d["floor_thr"], 3, 256)
    raw = signal(B, 2 * n, 99, bk.CS16)
    for f in range(2):
        frame = raw[:, 2 * f * n:2 * (f + 1) * n]
        spec, recs, pcm, iq_rec, blank_rec = a.eng.clean_process_host(frame, bk.CS16, mask, S.STAGE_ALL, now_ms=1000 + 10 * f)
        rows, fmt = frame, bk.CS16
        if mask:
            rows, want_iq_rec, _ = b.eng.iqcorr_host(frame, bk.CS16)
            model_rows, model_iq_rec, _ = corr.call(frame, bk.CS16)
            assert rows.tobytes() == model_rows.tobytes()
            assert iq_rec.tobytes() == want_iq_rec.tobytes() == model_iq_rec.tobytes()
            rows, fmt = rows.view(np.float32), bk.CF32
        else:
            assert iq_rec is None
        clean, want_blank_rec, _ = b.eng.blanker_host(rows, fmt)
        model_clean, model_rec, _ = a.model.call(rows, fmt)
        assert clean.tobytes() == model_clean.tobytes()
        assert blank_rec.tobytes() == want_blank_rec.tobytes() == model_rec.tobytes() and (blank_rec["hits"] > 0).all()
        want_spec, want_recs, want_pcm = b.eng.process(clean.view(np.float32), S.CF32, S.STAGE_ALL, now_ms=1000 + 10 * f)
        assert spec.tobytes() == want_spec.tobytes() and recs.tobytes() == want_recs.tobytes(), f
        assert pcm.size > 0 and pcm.tobytes() == want_pcm.tobytes(), f
        assert a.eng.blanker_config()["samples_consumed"] == (f + 1) * n
        assert a.eng.iqcorr_config()["samples_consumed"] == (f + 1) * n * mask
    a.close()
    b.close()


def test_chain_refusals_move_no_stage_and_the_other_chains_never_blank(S, T):
    B, n = 2, 4096
    cfg = dict(BASE, block=256, max_in=n)
    icfg = dict(dc_tau_blocks=3.0, balance_tau_blocks=2.0, floor_db=-60.0, mode=3, block=256, max_in=n)
    a, b = Rig(S, T, B, n, **cfg), engine(S, B, n)
    a.eng.set_iqcorr(**icfg)
    b.set_iqcorr(**icfg)
    raw = signal(B, 2 * n, 77, bk.CS16)
    frame = raw[:, :2 * n]
    a.eng.clean_process_host(frame, bk.CS16, 1, S.STAGE_SPECTRUM)
    moved = lambda: (a.eng.blanker_config()["samples_consumed"], a.eng.iqcorr_config()["samples_consumed"])  # noqa: E731
    assert moved() == (n, n)
    invalid(S, a.eng.clean_process_host, frame, bk.CS16, 2)  # a mask with other bits
    invalid(S, a.eng.clean_process_host, frame, bk.CS16, 3)
    invalid(S, a.eng.clean_process_host, frame, bk.CS16, 1, 1 << 20)  # process_host's own refusal
    host = np.ascontiguousarray(frame)
    for fmt, ptr in ((7, host.ctypes.data), (-1, host.ctypes.data), (bk.CS16, None)):  # an unknown format, a null iq
        assert S.load().sdrg_engine_clean_process_host(a.eng._h, ptr, fmt, 0, 1, None, None, None, 0, None, None) == -1
    assert moved() == (n, n)
    # process_host and iqcorr_process_host are what they are without a blanker
    b.iqcorr_process(frame, bk.CS16, S.STAGE_SPECTRUM)
    nxt = raw[:, 2 * n:]
    spec, _, _, _ = a.eng.iqcorr_process(nxt, bk.CS16, S.STAGE_SPECTRUM)
    want, _, _, _ = b.iqcorr_process(nxt, bk.CS16, S.STAGE_SPECTRUM)
    assert spec.tobytes() == want.tobytes() and moved() == (n, 2 * n)
    spec, _, _ = a.eng.process(nxt, bk.CS16, S.STAGE_SPECTRUM)
    want, _, _ = b.process(nxt, bk.CS16, S.STAGE_SPECTRUM)
    assert spec.tobytes() == want.tobytes() and moved() == (n, 2 * n)
    # a stage's max_in under the frame, a stage off
    a.eng.set_iqcorr(**dict(icfg, max_in=n - 1))
    invalid(S, a.eng.clean_process_host, frame, bk.CS16, 1)
    assert moved() == (n, 0)
    a.eng.clean_process_host(frame, bk.CS16, 0, S.STAGE_SPECTRUM)  # without the correction it goes on
    a.eng.set_iqcorr(off=True)
    invalid(S, a.eng.clean_process_host, frame, bk.CS16, 1)
    assert a.eng.blanker_config()["samples_consumed"] == 2 * n
    a.eng.set_blanker(**dict(cfg, max_in=n - 1))
    invalid(S, a.eng.clean_process_host, frame, bk.CS16, 0)
    assert a.eng.blanker_config()["samples_consumed"] == 0
    a.eng.set_blanker(off=True)
    invalid(S, a.eng.clean_process_host, frame, bk.CS16, 0)
    a.close()
    b.close()


def test_64_streams_of_16384(S, T):
    B, n = 64, 16384
    r = Rig(S, T, B, **dict(BASE, block=256, max_in=n, tau_blocks=16.0, lead=2, tail=8))
    _, rec, nb = r.check(signal(B, n, 90, bk.CS16), bk.CS16)
    assert nb == 64 and (rec["hits"] > 100).all() and (rec["level_db"] < -15).all()  # a pulse every 97 samples
    r.close()


def test_benefit_cs16(S, T):
    """The CS16 benefit case of tests/test_blanker_cases.py at S = 256 in one call: the restatement's bytes, and with
    them its floor and tone."""
    r = Rig(S, T, 1, **dict(bk.BENEFIT, block=256, max_in=bk.N_BEN))
    clean, dirty = (bk.to_raw(bk.pulsed(pulses=p)[None, :], bk.CS16, 20000.0) for p in (False, True))
    zr, zi = bk.sample(clean, bk.CS16)
    med_c, pk_c = bk.spectrum_levels(zr[0] + 1j * zi[0])
    got, rec, nb = r.check(dirty, bk.CS16)
    med, pk = bk.spectrum_levels(got[0])
    print("output %.2f dB over the clean median, tone %+.2f dB, %d hits, %d blanked" % (
        med - med_c, pk - pk_c, rec["hits"][0], rec["blanked"][0]))
    assert nb == bk.N_BEN // 256 and med - med_c <= 1.5 and abs(pk - pk_c) <= 0.3
    r.restart()
    _, rec, _ = r.check(clean, bk.CS16)
    assert rec["hits"][0] == 0 and rec["blanked"][0] == 0
    r.close()
