"""GPU test of the staging the streaming stages' host calls share (sdrg_engine_ddc_host, _demod_host,
_channelizer_host, _resample_host, _ddc_demod_host, _ddc_demod_resample_host): a caller sees six independent calls.
One engine has all four stages set and makes the six calls in turn, so the shared input and output serve a smaller
call right after a larger one and a larger right after a smaller; every stage's history and cursor is carried across
the others' calls.  Every comparison is of bytes, against what the stages' own tests compare bytes with: the
restatements of ddc_cases, demod_cases and resample_cases fed the library's own designs, and for the channelizer the
device path of a second engine given the same calls."""
import numpy as np
import pytest

import ddc_cases as dd
import demod_cases as dm
import resample_cases as rs
from stage_harness import FS, GUARD, engine, out_buffer, read_out, same, to_device

pytestmark = pytest.mark.gpu

B, N = 2, 1024
DDC = dict(offset_hz=-123_456.0, cutoff_hz=60_000.0, decimation=5, taps=31)  # cap = 205
DEMOD = dict(mode=dm.FM, channel_rate_hz=FS / 5, deviation_hz=75_000.0, dc_cutoff_hz=300.0, deemphasis_us=75.0,
             audio_decimation=4, audio_taps=15, audio_cutoff_hz=15_000.0, gain=0.7, out_format=dm.OUT_F32, max_in=256)
CHAN = dict(cutoff_rel=0.5, channels=8, taps_per_channel=4, oversample=1, first_channel=2, n_channels=3)
RS = dict(interp=3, decim=2, taps_per_phase=8, cutoff_rel=0.9, components=1, out_format=rs.OUT_S16, gain=0.7,
          max_in=256)


def cut(model_out):
    """A restatement's (rows [B][cap], n_out) as the host calls return them: (rows [B][n_out], n_out)."""
    rows, n_out = model_out
    return rows[:, :n_out], n_out


def test_six_host_calls_share_one_staging_pair():
    import sdrg as S
    import torch as T
    eng, bank = engine(S, B, N), engine(S, B, N)
    eng.set_ddc(**DDC)
    eng.set_demod(**DEMOD)
    eng.set_resample(**RS)
    for e in (eng, bank):
        e.set_channelizer(**CHAN)
    assert eng.ddc_max_out() == 205
    d, c = eng.demod_config(), eng.resample_config()
    ddc = dd.Ddc(B, S.ddc_design(FS, **DDC), S.nco_tables(), eng.ddc_config()["nco_increment"], DDC["decimation"])
    demod = dm.Demod(B, d["mode"], d["kf"], d["alpha"], d["a"], d["taps"], d["audio_decimation"], d["gain"],
                     d["out_format"], d["max_in"])
    resampler = rs.Resampler(B, c["interp"], c["decim"], c["taps"], c["gain"], c["out_format"], 1, c["max_in"])
    chan_g = 0

    def check(got, want, what):
        """got: a host call's rows, cut to its n_out; want: (rows, n_out) of the reference."""
        same(np.ascontiguousarray(got), got.shape[-1], np.ascontiguousarray(want[0]), want[1], what)

    def channelizer(fmt, raw, what):
        """channelizer_host on eng against channelizer_device on bank."""
        nonlocal chan_g
        got = eng.channelizer(raw, fmt)
        cap = bank.channelizer_max_out()
        iq_t, out_t = to_device(T, raw), out_buffer(T, B * CHAN["n_channels"] * cap * 8)
        T.cuda.synchronize()
        n_out = bank.channelizer_device(iq_t.data_ptr(), fmt, out_t.data_ptr() + GUARD)
        bank.synchronize()
        want = read_out(out_t, (B, CHAN["n_channels"], cap), np.complex64)
        assert n_out > 0 and np.abs(want[:, :, :n_out]).max() > 0.01
        check(got, (want[:, :, :n_out], n_out), what)
        chan_g += raw.shape[1] // 2

    def ddc_call(fmt, raw, what):
        check(eng.ddc(raw, fmt), cut(ddc.call(fmt, raw)), what)

    for r in range(2):
        x = rs.noise(B, 100, seed=300 + r)
        check(eng.resample_host(x), cut(resampler.call(x)), (r, "resample_host"))
        channelizer(dd.CS16, dd.noise(dd.CS16, B, N, seed=310 + r), (r, "channelizer"))
        ddc_call(dd.CF32, dd.noise(dd.CF32, B, N, seed=320 + r), (r, "ddc"))
        z = dm.noise(B, 200, seed=330 + r)
        check(eng.demod(z), cut(demod.call(z)), (r, "demod"))
        raw = dd.noise(dd.CS8, B, N, seed=340 + r)
        chan = cut(ddc.call(dd.CS8, raw))[0]
        check(eng.ddc_demod(raw, dd.CS8), cut(demod.call(chan)), (r, "ddc_demod"))
        raw = dd.noise(dd.CS8, B, N, seed=350 + r)
        audio = cut(demod.call(cut(ddc.call(dd.CS8, raw))[0]))[0]
        check(eng.ddc_demod_resample_host(raw, dd.CS8), cut(resampler.call(audio)), (r, "ddc_demod_resample_host"))

    assert eng.ddc_config()["samples_consumed"] == ddc.g0 == 6 * N
    assert eng.demod_config()["samples_consumed"] == demod.g and demod.g > 2 * 200
    assert eng.resample_config()["samples_consumed"] == resampler.g and resampler.g > 2 * 100
    assert eng.channelizer_config()["samples_consumed"] == chan_g == 2 * N
    assert bank.channelizer_config()["samples_consumed"] == chan_g

    # a longer frame: the shared buffers grow between stages
    for e in (eng, bank):
        e.setSamplesPerReading(2 * N)
    ddc_call(dd.CS8, dd.noise(dd.CS8, B, 2 * N, seed=360), "ddc at 2048")
    channelizer(dd.CF32, dd.noise(dd.CF32, B, 2 * N, seed=361), "channelizer at 2048")
    assert eng.ddc_config()["samples_consumed"] == ddc.g0 == 8 * N
    assert eng.channelizer_config()["samples_consumed"] == chan_g == 4 * N
    eng.close()
    bank.close()
