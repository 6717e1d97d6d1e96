"""Lab: the DDC bank stage (csrc/bank.hip) timed on resident CS8 frames, beside the DDC at the same rows and taps.
python tools/lab/bank_time.py [calls] [out.jsonl] [rounds]  (SDRG_LIB_PATH selects a variant library)

sdrg_engine_bank_device alone: HIP events around K calls on three rotating input buffers, us per call.  The shapes are
one stream of 16384 CS8 samples into 4096 channels at (T, D) = (255, 41), (127, 16) and (63, 8), the one-tap row (1, 41)
(staging and mix, next to no FIR), 64 streams x 64 channels and 1 stream x 16 channels at (255, 41).  The yardstick of the
first three is sdrg_engine_ddc_device at 4096 streams x 16384 CS8 with the same (T, D): the same number of output rows
and taps, which is the closest thing the DDC can do; the two are timed alternately, `rounds` times, and every reading is
kept.  A lab library (bank.o built with -DBANK_LAB_GROUP_NUM / _DEN, which scale channels_per_group, or
-DBANK_LAB_SKIP_MIX=1, which leaves the mix out) is timed by the same tool under SDRG_LIB_PATH; `library` says which."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "sdr-for-android-lib_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import sdrg  # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 40
OUT = sys.argv[2] if len(sys.argv) > 2 else None
ROUNDS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
N, FS = 16384, 2_000_000
LIBRARY = os.path.basename(os.environ.get("SDRG_LIB_PATH", "product"))
dev = torch.device("cuda", 0)
lib = sdrg.load()


def emit(r):
    line = json.dumps(r)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def timed(work, call):
    for k in range(6):
        call(k)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(work):
        a.record()
        for k in range(K):
            call(k)
        b.record()
    b.synchronize()
    return a.elapsed_time(b) / K * 1e3


class Stage:
    """An engine of B streams with the bank (C channels) or, at C == 0, the DDC set, on its own stream."""

    def __init__(self, B, C, T, D):
        self.B, self.C, self.T, self.D = B, C, T, D
        self.eng = sdrg.Engine(sdrg.SDRConfig(centerFrequency=100_000_000, samplesPerReading=N, sampleRate=FS,
                                              freqFocusRangeKhz=5, soundMode=1), B)
        cutoff = min(FS / 2, 0.4 * FS / D)
        if C:
            rng = np.random.default_rng(1)
            self.eng.set_bank(offsets_hz=(rng.random((B, C)) - 0.5) * FS, cutoff_hz=cutoff, decimation=D, taps=T)
            self.fn, cap = lib.sdrg_engine_bank_device, self.eng.bank_max_out()
        else:
            self.eng.set_ddc(offset_hz=-300_000.0, cutoff_hz=cutoff, decimation=D, taps=T)
            self.fn, cap = lib.sdrg_engine_ddc_device, self.eng.ddc_max_out()
        g = torch.Generator(device=dev)
        g.manual_seed(B + C)
        self.bufs = [torch.randint(-128, 128, (B, 2 * N), device=dev, generator=g, dtype=torch.int8) for _ in range(3)]
        self.out = torch.zeros((B * max(C, 1), cap, 2), dtype=torch.float32, device=dev)
        self.work = torch.cuda.Stream(dev)
        self.eng.set_stream(self.work.cuda_stream)
        self.n_out = ctypes.c_int32()
        torch.cuda.synchronize()

    def call(self, k):
        rc = self.fn(self.eng._h, ctypes.c_void_p(self.bufs[k % 3].data_ptr()), sdrg.CS8,
                     ctypes.c_void_p(self.out.data_ptr()), ctypes.byref(self.n_out))
        assert rc == 0, rc

    def time(self):
        return timed(self.work, self.call)

    def close(self):
        torch.cuda.synchronize()
        self.eng.set_stream(None)
        self.eng.close()


def shape(B, C, T, D, with_ddc):
    bank = Stage(B, C, T, D)
    ddc = Stage(B * C, 0, T, D) if with_ddc else None
    bank_us, ddc_us = [], []
    for _ in range(ROUNDS):
        if ddc:
            ddc_us.append(round(ddc.time(), 2))
        bank_us.append(round(bank.time(), 2))
    tile, group = sdrg.bank_geometry(D, T, C, B)
    r = dict(kind="bank", library=LIBRARY, streams=B, channels=C, n=N, taps=T, decimation=D, fmt="CS8", buffers=3,
             calls=K, tile_outputs=tile, channels_per_group=group, bank_us=bank_us, bank_us_median=float(np.median(bank_us)))
    if ddc:
        r.update(ddc_streams=B * C, ddc_us=ddc_us, ddc_us_median=float(np.median(ddc_us)),
                 ddc_spread_us=round(max(ddc_us) - min(ddc_us), 2),
                 over_ddc=round(float(np.median(bank_us)) / float(np.median(ddc_us)), 3))
        ddc.close()
    bank.close()
    emit(r)
    torch.cuda.empty_cache()


for T, D in ((255, 41), (127, 16), (63, 8)):
    shape(1, 4096, T, D, True)
shape(1, 4096, 1, 41, True)
shape(64, 64, 255, 41, False)
shape(1, 16, 255, 41, False)
