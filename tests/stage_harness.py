"""What the GPU tests of the streaming stages share (test_gpu_ddc, test_gpu_demod, test_gpu_channelizer,
test_gpu_resample, test_gpu_squelch, test_gpu_agc, test_gpu_stream_staging): an engine, a refused call, and `out` as a
0xAA-filled device buffer between GUARD bytes on either side, read back with both guards checked and compared as bytes;
and BlockRig, the rig of the two block stages' tests.  S is the sdrg module, T torch."""
import numpy as np
import pytest

FS = 2_000_000
GUARD = 64


def engine(S, B, n=1024, fs=FS):
    return S.Engine(S.SDRConfig(centerFrequency=100_000_000, samplesPerReading=n, sampleRate=fs, freqFocusRangeKhz=5,
                                soundMode=1), B)


def invalid(S, fn, *a, **k):
    with pytest.raises(S.SdrgError) as ei:
        fn(*a, **k)
    assert "SDRG_E_INVALID" in str(ei.value)


def to_device(T, raw):
    return T.from_numpy(np.ascontiguousarray(raw)).to("cuda:0")


def out_buffer(T, nbytes):
    """A call's `out` of nbytes starts GUARD bytes into this buffer: out_buffer(...).data_ptr() + GUARD."""
    return T.full((GUARD + nbytes + GUARD,), 0xAA, dtype=T.uint8, device="cuda:0")


def read_out(out_t, shape, dtype):
    o = out_t.cpu().numpy()
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    assert np.all(o[:GUARD] == 0xAA) and np.all(o[GUARD + nbytes:] == 0xAA), "bytes written outside out"
    return o[GUARD:GUARD + nbytes].view(dtype).reshape(shape)


def same(got, n_out, want, want_n, what=None):
    assert n_out == want_n and got.shape == want.shape and got.dtype == want.dtype, (what, n_out, want_n, got.shape)
    bits = {2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    bad = np.argwhere(got.view(bits) != want.view(bits))
    assert got.tobytes() == want.tobytes(), (what, len(bad), [(tuple(i), got[tuple(i)], want[tuple(i)]) for i in bad[:4]])


def rows_bytes(chan, stride):
    """chan complex64 [B][n] -> float32 [B][stride][2], NaN past n."""
    B, n = chan.shape
    rows = np.full((B, stride, 2), np.nan, np.float32)
    rows[:, :n] = np.ascontiguousarray(chan).view(np.float32).reshape(B, n, 2)
    return rows


class BlockRig:
    """An engine with a block stage (the squelch, the AGC) set, and the restatement that follows it call by call.  A
    subclass names the stage (`stage`: the engine's set_<stage>, <stage>_config and <stage>_device), names its record
    dtype in S (`record`, 16 bytes) and makes the restatement: make_model(d), d the configuration in force with its
    design."""
    stage = record = None

    def __init__(self, S, T, B, n=1024, **cfg):
        self.S, self.T, self.B = S, T, B
        self.eng = engine(S, B, n)
        self.configure(**cfg)

    def config(self):
        return getattr(self.eng, self.stage + "_config")()

    def configure(self, **cfg):
        self.cfg = cfg
        getattr(self.eng, "set_" + self.stage)(**cfg)
        self.remodel()

    def remodel(self):
        """A fresh restatement from the library's design of the configuration in force."""
        d = self.config()
        assert all(d[k] == v for k, v in self.cfg.items()), d
        assert d["samples_consumed"] == 0
        self.model = self.make_model(d)

    def device_call(self, chan, in_stride=None, records=True, in_place=False, shift=0):
        """<stage>_device into 0xAA-filled buffers between guard bytes: (out [B][stride], records [B][4] as uint32 or
        None, n_blocks).  shift: bytes by which chan and out are moved off their 16-byte alignment."""
        T, B = self.T, self.B
        stride = self.cfg["max_in"] if in_stride is None else in_stride
        rows = rows_bytes(chan, stride)
        nbytes = B * stride * 8
        out_t = out_buffer(T, nbytes + shift)
        rec_t = out_buffer(T, B * 16)
        if in_place:
            out_t[GUARD + shift:GUARD + shift + nbytes] = T.from_numpy(rows.view(np.uint8).reshape(-1)).to("cuda:0")
            chan_ptr = out_t.data_ptr() + GUARD + shift
        else:
            chan_t = T.full((nbytes + shift,), 0, dtype=T.uint8, device="cuda:0")
            chan_t[shift:] = T.from_numpy(rows.view(np.uint8).reshape(-1)).to("cuda:0")
            chan_ptr = chan_t.data_ptr() + shift
        T.cuda.synchronize()
        device = getattr(self.eng, self.stage + "_device")
        nb = device(chan_ptr, stride, chan.shape[1], out_t.data_ptr() + GUARD + shift,
                    rec_t.data_ptr() + GUARD if records else None)
        self.eng.synchronize()
        o = out_t.cpu().numpy()
        assert np.all(o[:GUARD + shift] == 0xAA) and np.all(o[GUARD + shift + nbytes:] == 0xAA), "bytes outside out"
        out = o[GUARD + shift:GUARD + shift + nbytes].copy().view(np.complex64).reshape(B, stride)
        if not records:
            assert np.all(rec_t.cpu().numpy() == 0xAA), "records written without a pointer"
            return out, None, nb
        return out, read_out(rec_t, (B, 4), np.uint32), nb

    def check(self, chan, what=None, **kw):
        got, rec, nb = self.device_call(chan, **kw)
        want, want_rec, want_nb = self.model.call(chan, in_stride=got.shape[1])
        same(got, nb, want, want_nb, what)
        if rec is not None:
            same(rec, nb, want_rec.view(np.uint32).reshape(self.B, 4), want_nb, (what, "records"))
            rec = rec.view(getattr(self.S, self.record))[:, 0]
        assert self.config()["samples_consumed"] == self.model.g
        return got, rec, nb

    def close(self):
        self.eng.close()
