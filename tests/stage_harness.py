"""What the GPU tests of the four streaming stages share (test_gpu_ddc, test_gpu_demod, test_gpu_channelizer,
test_gpu_resample, test_gpu_stream_staging): an engine, a refused call, and `out` as a 0xAA-filled device buffer between
GUARD bytes on either side, read back with both guards checked and compared as bytes.  S is the sdrg module, T torch."""
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
