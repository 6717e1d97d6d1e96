"""GPU tests of the symbol stage (csrc/symbols.hip, sdrg_engine_symbols_*, sdrg_engine_listen_symbols_host): the whole of
`symbols`, zero tail included, and the records of each stream against the NumPy restatement in tests/symbols_cases.py fed
the library's own design values and table.  Every comparison is of bytes (the stage is specified operation by operation:
no tolerances).  `symbols` and `records` are pre-filled with 0xAA between 64 guard bytes on either side, every stream has
its own data, and the input rows hold NaN past the call's n values.

The moments kernel works in tiles of `tile` positions counted from the start of the block in progress, the pass kernel in
tiles of `pass_tile` symbols of a row (sdrg.symbols_geometry); blocks up to 128 values are summed inside a wave, larger
ones meet in LDS, and a block of 1024 takes a workgroup's two passes; a wave's first lane loads the value before its own
where the other lanes take their neighbour's; rows or offsets that are not aligned to a pair of values take one-value
loads; a symbol near a call's start reads its two values from the state: the shapes below put data on each of these
paths."""
import ctypes

import numpy as np
import pytest

import agc_cases as ag
import ddc_cases as dd
import demod_cases as dm
import resample_cases as rs
import symbols_cases as sc
from stage_harness import GUARD, engine, invalid, out_buffer, read_out

pytestmark = pytest.mark.gpu

f32 = np.float32
FS = 48000.0
RATES = {"2": FS / 2, "64": FS / 64, "10.4167": FS / 10.4167}  # inc = 2^31, 2^26, and 10.4167 samples per symbol
BASE = dict(sc.BASE, block=64, tau_blocks=3.0, tau_level_blocks=3.0, lock_threshold=0.05, fixed_centre=0.7,
            fixed_threshold=2.0, max_in=2048)
VARIANTS = [dict(levels=2, format=sc.HARD, level_mode=sc.LEVEL_TRACK), dict(levels=4, format=sc.HARD, level_mode=sc.LEVEL_TRACK),
            dict(levels=4, format=sc.SOFT, level_mode=sc.LEVEL_FIXED), dict(levels=2, format=sc.SOFT, level_mode=sc.LEVEL_TRACK),
            dict(levels=4, format=sc.HARD, level_mode=sc.LEVEL_FIXED), dict(levels=2, format=sc.HARD, level_mode=sc.LEVEL_FIXED)]


@pytest.fixture(scope="module")
def S():
    import sdrg
    return sdrg


@pytest.fixture(scope="module")
def T():
    import torch
    return torch


def same(got, n_sym, want, want_n, what=None):
    """stage_harness.same for rows of bytes as well."""
    assert n_sym == want_n and got.shape == want.shape and got.dtype == want.dtype, (what, n_sym, want_n, got.shape)
    bits = {1: np.uint8, 4: np.uint32}[got.dtype.itemsize]
    bad = np.argwhere(got.view(bits) != want.view(bits))
    assert got.tobytes() == want.tobytes(), (what, len(bad), [(tuple(i), got[tuple(i)], want[tuple(i)]) for i in bad[:4]])


def config(**kw):
    cfg = dict(BASE, **kw)
    if cfg["levels"] == 4 and "level_scale" not in kw:
        cfg["level_scale"] = 2 / np.sqrt(5)
    return cfg


def signal(B, n, seed, cfg, snr_db=20.0, ppm=0.0):
    """Every stream its own symbols, noise and start of the first cell."""
    Tc = cfg["sample_rate"] / cfg["symbol_rate"] * (1 + ppm * 1e-6)
    return np.stack([sc.signal(cfg["levels"], Tc, snr_db, n_symbols=int(n / Tc) + 2, seed=seed + b, start=0.37 + 0.11 * b)[0][:n]
                     for b in range(B)])


class Rig:
    """An engine with the stage set, and the restatement that follows it call by call."""

    def __init__(self, S, T, B, **cfg):
        self.S, self.T, self.B = S, T, B
        self.eng = engine(S, B)
        self.configure(**cfg)

    def configure(self, **cfg):
        self.cfg = cfg
        self.eng.set_symbols(**cfg)
        self.remodel()

    def remodel(self):
        d, des = self.eng.symbols_config(), self.S.symbols_design(**self.cfg)
        assert all(d[k] == v for k, v in self.cfg.items()), d
        assert all(np.asarray(des[k]).tobytes() == np.asarray(d[k]).tobytes() for k in sc.DESIGN) and d["samples_consumed"] == 0
        self.model = sc.make(self.B, des, self.cfg)
        self.cap = d["cap"]
        assert self.cap == self.model.cap == sc.cap(des["inc"], self.cfg["max_in"])
        self.dtype = np.float32 if self.cfg["format"] == sc.SOFT else np.uint8

    def device_call(self, x, in_stride=None, records=True, in_shift=0):
        """symbols_device into 0xAA-filled buffers between guard bytes: (symbols [B][cap], records [B][8] as uint32 or
        None, n_sym).  in_shift: bytes by which the rows are moved off an 8-byte alignment."""
        T, B = self.T, self.B
        n = x.shape[1]
        stride = self.cfg["max_in"] if in_stride is None else in_stride
        rows = np.full((B, stride), np.nan, np.float32)
        rows[:, :n] = x
        rows = rows.view(np.uint8).reshape(-1)
        in_t = T.zeros((rows.size + in_shift,), dtype=T.uint8, device="cuda:0")
        in_t[in_shift:] = T.from_numpy(rows).to("cuda:0")
        nbytes = B * self.cap * np.dtype(self.dtype).itemsize
        out_t, rec_t = out_buffer(T, nbytes), out_buffer(T, B * 32)
        T.cuda.synchronize()
        ns = self.eng.symbols_device(in_t.data_ptr() + in_shift, stride, n, out_t.data_ptr() + GUARD,
                                     rec_t.data_ptr() + GUARD if records else None)
        self.eng.synchronize()
        out = read_out(out_t, (B, self.cap), self.dtype)
        if not records:
            assert np.all(rec_t.cpu().numpy() == 0xAA), "records written without a pointer"
            return out, None, ns
        return out, read_out(rec_t, (B, 8), np.uint32), ns

    def check(self, x, what=None, **kw):
        got, rec, ns = self.device_call(x, **kw)
        want, want_rec, want_ns = self.model.call(x)
        same(got, ns, want, want_ns, what)
        if rec is not None:
            same(rec, ns, want_rec.view(np.uint32).reshape(self.B, 8), want_ns, (what, "records"))
            rec = rec.view(self.S.SymbolsRecord)[:, 0]
        assert self.eng.symbols_config()["samples_consumed"] == self.model.g
        return got, rec, ns

    def restart(self):
        self.eng.symbols_reset()
        self.model.reset()

    def close(self):
        self.eng.close()


@pytest.mark.parametrize("rate", list(RATES))
@pytest.mark.parametrize("block", [64, 256, 1024])
def test_stream_counts_blocks_and_rates(S, T, block, rate):
    """The step kernel takes 64 streams per workgroup: a wave in part, and a wave and a stream.  Blocks summed in a wave
    (64), across the waves (256) and over two passes (1024); cells of 2, 64 and 10.4167 samples; and each of the levels,
    formats and level modes in turn."""
    ns = (700, 5, 1343)
    for j, B in enumerate((1, 3, 65)):
        cfg = config(block=block, symbol_rate=RATES[rate], **VARIANTS[(j + block // 256 + len(rate)) % len(VARIANTS)])
        x = signal(B, sum(ns), 100 + B, cfg)
        r = Rig(S, T, B, **cfg)
        at = 0
        for f, n in enumerate(ns):
            _, rec, _ = r.check(x[:, at:at + n], (B, block, rate, f))
            at += n
        assert np.all(rec["flags"] & sc.SEEDED)
        if rate == "10.4167":  # 2 samples per cell carry no line at the symbol rate, and 2048 values are 32 cells of 64
            assert np.all(rec["flags"] == 3)
        r.close()


@pytest.mark.parametrize("variant", range(len(VARIANTS)))
def test_levels_formats_and_level_modes(S, T, variant):
    cfg = config(symbol_rate=4800.0, **VARIANTS[variant])
    r = Rig(S, T, 3, **cfg)
    x = signal(3, 2000, 40 + variant, cfg)
    got, rec, ns = r.check(x[:, :1500], variant)
    r.check(x[:, 1500:], variant)
    assert np.all(rec["flags"] == 3) and ns == 149
    if cfg["format"] == sc.HARD:
        assert set(np.unique(got[:, 20:ns] & 0x7F)) == set(range(cfg["levels"]))
    r.close()


@pytest.mark.parametrize("rate", list(RATES))
@pytest.mark.parametrize("block", [64, 256, 1024])
def test_call_lengths_around_the_block_and_the_tiles(S, T, block, rate):
    """Every n as a call that follows whatever the others left, and as a fresh stream's first call: odd and even offsets,
    calls that end inside a block, on a seam and one value after it, around the seam of two workgroups of the moments
    kernel, and (at 2 samples per symbol) around the seam of two workgroups of the pass kernel, whose tiles are counted
    in symbols.  in_stride is n or n + 1: odd and even rows."""
    B = 3
    tile, ptile = S.symbols_geometry(block)
    ns = [0, 1, block - 1, block, block + 1, tile - 1, tile, tile + 1, 2 * tile + 3]
    if rate == "2":
        ns += [2 * ptile - 2, 2 * ptile - 1, 2 * ptile, 2 * ptile + 1, 2 * ptile + 2, 4 * ptile + 1]
    cfg = config(block=block, symbol_rate=RATES[rate], max_in=max(ns) + 2, **VARIANTS[block // 256 % 3])
    r = Rig(S, T, B, **cfg)
    x = signal(B, 2 * sum(ns), 200 + block, cfg)
    at = 0
    for f, n in enumerate(ns):  # one stream
        got, rec, nsym = r.check(x[:, at:at + n], (block, f, n), in_stride=max(n, 1) + (f & 1))
        at += n
        if n == 0:
            assert nsym == 0 and not got.view(np.uint8).any()
    for n in ns:  # each the first call
        r.restart()
        r.check(x[:, at:at + n], (block, "first", n), in_stride=max(n, 1))
        at += n
    r.close()


def test_calls_without_a_symbol_and_calls_whose_first_value_emits(S, T):
    """At 64 samples per symbol c_i = 0 at every multiple of 64: a call that starts there writes a symbol for its first
    value (but not the stream's very first: i >= 1), and calls inside a cell write none."""
    cfg = config(symbol_rate=RATES["64"], block=64)
    r = Rig(S, T, 2, **cfg)
    x = signal(2, 1000, 7, cfg)
    at = 0
    for n, want in ((64, 0), (1, 1), (62, 0), (1, 0), (64, 1), (0, 0), (3, 1), (61, 0), (128, 2), (1, 1), (1, 0), (126, 1)):
        got, _, ns = r.check(x[:, at:at + n], (at, n))
        assert ns == want, (at, n)
        at += n
    r.close()


def test_odd_offsets_and_rows_that_are_not_aligned(S, T):
    """After a first call of 1, 2 or 3 values the next starts at an odd or an even offset; in_stride odd and beyond n,
    rows moved by 4 bytes: the one-value loads."""
    B = 3
    cfg = config(symbol_rate=4800.0, **VARIANTS[1])
    r = Rig(S, T, B, **cfg)
    x = signal(B, 4000, 300, cfg)
    at = 0
    for first in (1, 2, 3):
        for kw in (dict(), dict(in_stride=777), dict(in_shift=4), dict(in_stride=701, in_shift=4), dict(in_stride=1000),
                   dict(in_shift=8)):
            r.restart()
            for n in (first, 700):
                r.check(x[:, at:at + n], (first, n, kw), **(kw if n == 700 else {}))
                at = (at + n) % 3000
    r.close()


@pytest.mark.parametrize("rate", list(RATES))
def test_unequal_calls_are_one_stream(S, T, rate):
    """Calls of unequal lengths, some of which complete no block or write no symbol, against one call of the whole on the
    restatement; at 64 samples per symbol the two values of a symbol lie up to 66 back: in the call before, or the one
    before that."""
    B = 4
    cfg = config(block=256, symbol_rate=RATES[rate], **VARIANTS[3])
    r = Rig(S, T, B, **cfg)
    ns = (700, 10, 1, 2048, 0, 333, 40, 40, 2, 300)
    x = signal(B, sum(ns), 50, cfg)
    outs, at = [], 0
    for f, n in enumerate(ns):
        got, rec, nsym = r.check(x[:, at:at + n], f, records=f != 1)
        outs.append(got[:, :nsym])
        at += n
    whole = sc.make(B, S.symbols_design(**cfg), dict(cfg, max_in=1 << 16))
    want, want_rec, want_n = whole.call(x)
    got = np.concatenate(outs, axis=1)
    assert got.shape[1] == want_n and got.tobytes() == want[:, :want_n].tobytes()
    for k in ("tau", "coherence", "centre", "threshold", "slips", "flags"):
        assert rec[k].tobytes() == want_rec[k].tobytes(), k
    r.close()


def test_held_blocks_a_slip_and_amplitudes_down_to_1e_minus_21(S, T):
    B = 3
    cfg = config(symbol_rate=4800.0, block=256, floor_db=-30.0)
    r = Rig(S, T, B, **cfg)
    x = signal(B, 4096, 9, cfg)
    x[1, 512:1280] = 0  # a closed squelch: three blocks of zeros
    x[2, 256:512] *= f32(1e-3)
    got, rec, _ = r.check(x[:, :2048], "held")
    assert rec["held_blocks"].tolist() == [0, 3, 1]
    _, rec, _ = r.check(x[:, 2048:], "after")
    assert rec["held_blocks"].tolist() == [0, 0, 0] and np.all(rec["flags"] == 3)
    r.close()
    # a clock 2000 ppm fast over 1 000 symbols: the sampling point goes round the cell's edge twice
    cfg = config(symbol_rate=4800.0, block=64, tau_blocks=2.0, max_in=4096)
    r = Rig(S, T, B, **cfg)
    x = signal(B, 3 * 4096, 10, cfg, snr_db=30.0, ppm=2000.0)
    for f in range(3):
        _, rec, _ = r.check(x[:, 4096 * f:4096 * (f + 1)], ("slip", f))
    assert np.all(rec["slips"] >= 2) and np.all(rec["flags"] == 3)
    r.close()
    # x^2 and dx^2 are denormal or zero at 1e-21, and the floor lies under them
    for amp, floor_db in ((1e-10, -300.0), (1e-19, -440.0), (1e-21, -440.0)):
        cfg = config(symbol_rate=4800.0, block=64, floor_db=floor_db, **VARIANTS[2 if amp == 1e-19 else 1])
        r = Rig(S, T, B, **cfg)
        x = (signal(B, 1500, 11, cfg).astype(np.float64) * amp).astype(np.float32)
        r.check(x[:, :801], amp)
        _, rec, _ = r.check(x[:, 801:], amp)
        assert np.all(rec["flags"] & sc.SEEDED) if amp > 1e-20 else True
        r.close()


def test_reset_and_set_again_between_calls(S, T):
    B = 2
    cfg = config(symbol_rate=4800.0, **VARIANTS[0])
    r = Rig(S, T, B, **cfg)
    x = signal(B, 3000, 12, cfg)
    r.check(x[:, :700], "a")
    r.restart()
    r.check(x[:, 700:1400], "after reset")
    r.configure(**config(symbol_rate=RATES["10.4167"], block=256, **VARIANTS[2]))
    r.check(x[:, 1400:2100], "after set")
    bad = dict(r.cfg, levels=3)
    invalid(S, r.eng.set_symbols, **bad)  # a rejected set changes nothing: the stream goes on
    r.check(x[:, 2100:], "after a rejected set")
    r.eng.set_symbols(off=True)
    invalid(S, r.eng.symbols_config)
    r.close()


@pytest.mark.parametrize("variant", [0, 2])
def test_host_path_equals_the_restatement(S, T, variant):
    B = 3
    cfg = config(symbol_rate=4800.0, **VARIANTS[variant])
    eng = engine(S, B)
    eng.set_symbols(**cfg)
    model = sc.make(B, S.symbols_design(**cfg), cfg)
    x = signal(B, 2500, 13, cfg)
    for (a, b), want_rec in zip(((0, 900), (900, 900), (900, 901), (901, 2500)), (True, True, False, True)):
        got, rec, ns = eng.symbols_host(x[:, a:b], want_records=want_rec)
        want, w_rec, w_ns = model.call(x[:, a:b])
        assert ns == w_ns and got.dtype == want.dtype and got.tobytes() == want[:, :w_ns].tobytes(), (a, b)
        assert (rec is None) if not want_rec else rec.tobytes() == w_rec.tobytes(), (a, b)
    assert eng.symbols_config()["samples_consumed"] == 2500
    eng.close()


def test_other_stages_between_symbols_calls(S, T):
    """squelch_device and demod_device between two symbols calls: each keeps its own stream and scratch."""
    cfg = config(symbol_rate=4800.0)
    rig = Rig(S, T, 2, **cfg)
    eng = rig.eng
    eng.set_squelch(open_db=-12.0, close_db=-18.0, tau_blocks=1.0, block=16, hang_blocks=2, max_in=1024)
    eng.set_demod(mode=dm.AM, channel_rate_hz=200_000.0, deviation_hz=0.0, dc_cutoff_hz=100.0, deemphasis_us=0.0,
                  audio_decimation=4, audio_taps=31, audio_cutoff_hz=15_000.0, gain=1.0, out_format=dm.OUT_F32, max_in=1024)
    x = signal(2, 1800, 18, cfg)
    rig.check(x[:, :900], "before")
    chan = T.from_numpy(np.ascontiguousarray(x[:, :1024].astype(np.complex64))).to("cuda:0")
    out = T.empty_like(chan)
    audio = T.empty((2, eng.demod_max_out()), dtype=T.float32, device="cuda:0")
    eng.squelch_device(chan.data_ptr(), 512, 512, out.data_ptr())
    eng.demod_device(chan.data_ptr(), 512, audio.data_ptr())
    rig.check(x[:, 900:], "after")
    rig.close()


def test_refusals_write_nothing_and_commit_nothing(S, T):
    B = 2
    cfg = config(symbol_rate=4800.0, max_in=512)
    eng = engine(S, B)
    x = T.zeros((B, 512), dtype=T.float32, device="cuda:0")
    sym = T.full((B * 64,), 0xAA, dtype=T.uint8, device="cuda:0")
    before = sym.clone()
    invalid(S, eng.symbols_device, x.data_ptr(), 512, 100, sym.data_ptr())  # the stage off
    invalid(S, eng.symbols_max_out)
    eng.set_symbols(**cfg)
    assert eng.symbols_max_out() == 52
    assert eng.symbols_device(x.data_ptr(), 512, 100, sym.data_ptr()) == 9
    eng.synchronize()
    sym.copy_(before)
    for stride, n in ((512, -1), (512, 513), (513, 100), (99, 100), (0, 0)):
        invalid(S, eng.symbols_device, x.data_ptr(), stride, n, sym.data_ptr())
    L, ns = S.load(), ctypes.c_int32(7)
    assert L.sdrg_engine_symbols_device(eng._h, None, 512, 100, sym.data_ptr(), None, ctypes.byref(ns)) == -1
    assert L.sdrg_engine_symbols_device(eng._h, x.data_ptr(), 512, 100, None, None, ctypes.byref(ns)) == -1
    assert L.sdrg_engine_symbols_device(eng._h, x.data_ptr(), 512, 100, sym.data_ptr(), None, None) == -1
    eng.synchronize()
    assert ns.value == 7 and T.equal(sym, before) and eng.symbols_config()["samples_consumed"] == 100
    eng.close()


# ---- sdrg_engine_listen_symbols_host: the listening chain of test_gpu_agc (fs = 2 MHz, N = 4096, a carrier at +250 kHz,
# here FM by a 4-level signal of 4800 symbols/s; audio at 50 kHz, 102 or 103 values a frame), against the stages called
# one by one: listen() for the audio ahead of the resampler, then symbols_host on it.

LISTEN_FS, LISTEN_N, LISTEN_B, LISTEN_FRAMES, LISTEN_CAP = 2_000_000, 4096, 2, 6, 410
DDC_CFG = dict(offset_hz=250_000.0, cutoff_hz=60_000.0, decimation=10, taps=63)
DEMOD_CFG = dict(mode=dm.FM, channel_rate_hz=200_000.0, deviation_hz=5000.0, dc_cutoff_hz=0.0, deemphasis_us=0.0,
                 audio_decimation=4, audio_taps=31, audio_cutoff_hz=8_000.0, gain=1.0, out_format=dm.OUT_F32,
                 max_in=LISTEN_CAP)
SQ_CFG = dict(open_db=-12.0, close_db=-18.0, tau_blocks=1.0, block=16, hang_blocks=2, max_in=LISTEN_CAP)
AGC_CFG = dict(target=0.5, max_gain_db=30.0, initial_gain_db=0.0, floor_db=-40.0, attack_blocks=0.0, decay_blocks=3.0,
               detector=ag.MEAN, block=16, hang_blocks=1, max_in=LISTEN_CAP)
RS_CFG = dict(interp=24, decim=25, taps_per_phase=8, cutoff_rel=0.9, components=1, out_format=rs.OUT_F32, gain=1.0,
              max_in=103)
SYM_CFG = dict(sc.BASE, sample_rate=50_000.0, symbol_rate=4800.0, levels=4, level_scale=2 / np.sqrt(5), block=64,
               tau_blocks=2.0, tau_level_blocks=2.0, floor_db=-60.0, lock_threshold=0.05, max_in=103)
ALL = 7


@pytest.fixture(scope="module")
def fsk4():
    fs, n, B, frames = LISTEN_FS, LISTEN_N, LISTEN_B, LISTEN_FRAMES
    rng = np.random.default_rng(3)
    raw = np.empty((B, 2 * frames * n), np.int8)
    t = np.arange(frames * n)
    for b in range(B):
        sym = rng.integers(0, 4, frames * n * 4800 // fs + 2)
        dev = (2 * sym - 3)[(t * 4800 // fs)] * (5000.0 / 3)
        z = 0.4 * (1 + b) * np.exp(2j * np.pi * (250_000.0 * t / fs + np.cumsum(dev) / fs) + 0.3j * b)
        z = z + (2 / 128) * (rng.standard_normal(t.size) + 1j * rng.standard_normal(t.size))
        raw[b, 0::2] = np.round(z.real * 128).clip(-128, 127).astype(np.int8)
        raw[b, 1::2] = np.round(z.imag * 128).clip(-128, 127).astype(np.int8)
    return raw


def listen_engine(S, symbols=SYM_CFG):
    eng = engine(S, LISTEN_B, LISTEN_N, LISTEN_FS)
    eng.set_ddc(**DDC_CFG)
    eng.set_demod(**DEMOD_CFG)
    eng.set_squelch(**SQ_CFG)
    eng.set_agc(**AGC_CFG)
    eng.set_resample(**RS_CFG)
    if symbols:
        eng.set_symbols(**symbols)
    return eng


@pytest.mark.parametrize("steps", range(8))
def test_listen_symbols_equals_the_stages_one_by_one(S, T, fsk4, steps):
    n = LISTEN_N
    chain, plain, ahead = listen_engine(S), listen_engine(S, None), listen_engine(S)
    model = sc.make(LISTEN_B, S.symbols_design(**SYM_CFG), SYM_CFG)
    locked = False
    for f in range(LISTEN_FRAMES):
        part = fsk4[:, 2 * n * f:2 * n * (f + 1)]
        want_audio = f % 3 != 2  # every third call leaves the audio on the device
        got, sq_rec, agc_rec, sym, rec, ns = chain.listen_symbols(part, dd.CS8, steps, want_audio=want_audio)
        want, w_sq, w_agc = plain.listen(part, dd.CS8, steps)
        audio, _, _ = ahead.listen(part, dd.CS8, steps & ~S.LISTEN_RESAMPLE)  # what the symbol stage reads
        w_sym, w_rec, w_ns = ahead.symbols_host(audio)
        m_sym, m_rec, m_ns = model.call(audio)
        assert ns == w_ns == m_ns and sym.tobytes() == w_sym.tobytes() == m_sym[:, :m_ns].tobytes(), f
        assert rec.tobytes() == w_rec.tobytes() == m_rec.tobytes(), f
        assert (got is None) if not want_audio else got.tobytes() == want.tobytes(), f
        for a, b in ((sq_rec, w_sq), (agc_rec, w_agc)):
            assert (a is None and b is None) or a.tobytes() == b.tobytes(), f
        locked = bool(np.all(rec["flags"] == 3))
    assert locked
    assert chain.symbols_config()["samples_consumed"] == model.g == -(-chain.demod_config()["samples_consumed"] // 4)
    for e in (chain, plain, ahead):
        e.close()


def test_listen_symbols_refusals_move_no_stage(S, T, fsk4):
    first = fsk4[:, :2 * LISTEN_N]

    def consumed(eng):
        return [eng.ddc_config()["samples_consumed"], eng.squelch_config()["samples_consumed"],
                eng.agc_config()["samples_consumed"], eng.demod_config()["samples_consumed"],
                eng.resample_config()["samples_consumed"]]

    eng = listen_engine(S, None)
    invalid(S, eng.listen_symbols, first, dd.CS8, ALL)  # the symbol stage off (the mirror asks for its configuration)
    L, n_out, ns = S.load(), ctypes.c_int32(), ctypes.c_int32()
    out, sym = np.empty((LISTEN_B, 103), np.float32), np.empty((LISTEN_B, 16), np.uint8)
    P = ctypes.c_void_p
    args = (eng._h, ALL, first.ctypes.data_as(P), dd.CS8, out.ctypes.data_as(P), ctypes.byref(n_out), None, None)
    assert L.sdrg_engine_listen_symbols_host(*args, sym.ctypes.data_as(P), None, ctypes.byref(ns)) == -1
    eng.set_symbols(**dict(SYM_CFG, max_in=102))  # under the demodulator's row length
    invalid(S, eng.listen_symbols, first, dd.CS8, ALL)
    eng.set_symbols(**SYM_CFG)
    assert eng.symbols_max_out() == 10
    assert L.sdrg_engine_listen_symbols_host(*args, None, None, ctypes.byref(ns)) == -1
    assert L.sdrg_engine_listen_symbols_host(*args, sym.ctypes.data_as(P), None, None) == -1
    eng.set_demod(**dict(DEMOD_CFG, out_format=dm.OUT_S16))
    invalid(S, eng.listen_symbols, first, dd.CS8, 0)
    eng.set_demod(**DEMOD_CFG)
    eng.set_squelch(off=True)
    invalid(S, eng.listen_symbols, first, dd.CS8, ALL)
    eng.set_squelch(**SQ_CFG)
    invalid(S, eng.listen_symbols, first, dd.CS8, 8)
    assert consumed(eng) == [0] * 5 and eng.symbols_config()["samples_consumed"] == 0
    assert L.sdrg_engine_listen_symbols_host(*args, sym.ctypes.data_as(P), None, ctypes.byref(ns)) == 0
    assert consumed(eng)[0] == LISTEN_N and eng.symbols_config()["samples_consumed"] == 103 and ns.value == 9
    eng.close()


def test_the_other_chains_are_unchanged_by_a_set_symbol_stage(S, T, fsk4):
    n = LISTEN_N
    a, b = listen_engine(S), listen_engine(S, None)
    for f in range(2):
        part = fsk4[:, 2 * n * f:2 * n * (f + 1)]
        got, want = a.listen(part, dd.CS8, ALL), b.listen(part, dd.CS8, ALL)
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want)), f
    assert a.symbols_config()["samples_consumed"] == 0  # set, and not asked for: it neither listens nor moves
    a.close()
    b.close()
