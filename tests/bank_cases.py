"""NumPy restatement of the DDC bank stage (include/sdrg.h, csrc/bank.hip): per stream the last T - 1 *unmixed* samples
are kept, and every call mixes the history and the frame again for each channel, then filters and decimates, operation by
operation in float32, so the GPU tests compare bytes.  Unpack, mix, taps and tables are ddc_cases': a row of the bank is
defined as the DDC's row at that offset, and test_bank_cases.py holds the two restatements against each other."""
import numpy as np

import ddc_cases as dd

MAX_CHANNELS, MAX_ROWS = 4096, 65535


def valid_config(fs, cutoff_hz, D, T, C, B, offsets_hz):
    o = np.asarray(offsets_hz, np.float64)
    return bool(dd.valid_config(fs, 0.0, cutoff_hz, D, T) and 1 <= C <= MAX_CHANNELS and B * C <= MAX_ROWS and
                o.shape == (B, C) and np.isfinite(o).all())


def increments(offsets_hz, fs):
    """nco_increment of every offset: uint32 of offsets_hz's shape."""
    o = np.asarray(offsets_hz, np.float64)
    return np.array([dd.nco_increment(v, fs) for v in o.reshape(-1)], np.uint32).reshape(o.shape)


class Bank:
    """One engine's bank state: g0 and, per stream, the last T - 1 unpacked, unmixed samples."""

    def __init__(self, B, taps, tab, incs, D):
        self.B, self.D = B, int(D)
        self.h = np.asarray(taps, np.float32).copy()
        self.T = self.h.size
        self.tab = np.asarray(tab, np.float32).copy()
        self.retune(incs)
        self.reset()

    def retune(self, incs):
        incs = np.asarray(incs, np.uint32)
        assert incs.ndim == 2 and incs.shape[0] == self.B
        self.incs, self.C = incs.copy(), incs.shape[1]

    def reset(self):
        self.g0 = 0
        self.xr = np.zeros((self.B, self.T - 1), np.float32)
        self.xi = np.zeros((self.B, self.T - 1), np.float32)

    def call(self, fmt, raw):
        """raw [B][2 N] -> (out complex64 [B][C][cap], zeros from n_out on; n_out)."""
        B, C, D, T, H = self.B, self.C, self.D, self.T, self.T - 1
        xr, xi = dd.unpack(fmt, np.asarray(raw).reshape(B, -1))
        n = xr.shape[1]
        xr = np.concatenate([self.xr, xr], axis=1)  # xr[:, H + t] = x at local index t, global index g0 + t
        xi = np.concatenate([self.xi, xi], axis=1)
        er = np.empty((B, C, H + n), np.float32)
        ei = np.empty((B, C, H + n), np.float32)
        for b in range(B):
            mixed = {}  # channels of equal increments are mixed once
            for c in range(C):
                inc = int(self.incs[b, c])
                if inc not in mixed:  # the phase at g < 0 multiplies a +0 sample
                    mixed[inc] = dd.mix(self.tab, inc, self.g0 - H, xr[b], xi[b])
                er[b, c], ei[b, c] = mixed[inc]
        cap = -(-n // D)
        n_out = dd.n_out_for(self.g0, n, D)
        first = (-self.g0) % D
        out = np.zeros((B, C, cap, 2), np.float32)
        if n_out > 0:
            at = H + first + D * np.arange(n_out)
            ar = np.zeros((B, C, n_out), np.float32)
            ai = np.zeros((B, C, n_out), np.float32)
            for k in range(T):
                ar = ar + self.h[k] * er[:, :, at - k]
                ai = ai + self.h[k] * ei[:, :, at - k]
            assert ar.dtype == np.float32
            out[:, :, :n_out, 0] = ar
            out[:, :, :n_out, 1] = ai
        if H:
            self.xr, self.xi = xr[:, -H:].copy(), xi[:, -H:].copy()
        self.g0 += n
        return out.view(np.complex64)[..., 0], n_out
