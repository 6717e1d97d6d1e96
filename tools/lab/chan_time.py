"""Lab: the channelizer stage (csrc/channelizer.hip) timed on resident raw IQ.
python tools/lab/chan_time.py [calls] [out.jsonl]  (SDRG_LIB_PATH selects a variant library)

sdrg_engine_channelizer_device alone: HIP events around K calls on three rotating input buffers, us per launch, beside
sdrg_measure_hbm_copy's read + write rate (a float4 streaming copy) before and after in the same run.  The yardstick of a
shape is its input read plus its output write at the copy's rate (the mean of the two measurements); `share` is
yardstick / measured.  The last rows time what the library offered for 16 channels before this stage, 16
sdrg_engine_ddc_device calls with T = 127 and D = 16 on the same input, alternating with the (16, 8, 1) bank in three
rounds.  Inputs: uniform noise over the format's whole range.  The lines go to stdout and, if named, to out.jsonl."""
import ctypes
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "sdr-for-android-lib_amd"))
import torch  # noqa: E402
import sdrg  # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 40
OUT = sys.argv[2] if len(sys.argv) > 2 else None
dev = torch.device("cuda", 0)
lib = sdrg.load()
TORCH_DTYPE = {sdrg.CS8: torch.int8, sdrg.CS16: torch.int16}
NAME = {sdrg.CS8: "CS8", sdrg.CS16: "CS16"}
LIBRARY = os.path.basename(os.environ.get("SDRG_LIB_PATH", "product"))
FS = 2_000_000
results = []


def sha256(t):
    """The hash of a device tensor's bytes once the work on it is done: two libraries that compute the same agree on it."""
    torch.cuda.synchronize()
    return hashlib.sha256(t.cpu().numpy()).hexdigest()


def emit(r):
    line = json.dumps(r)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def hbm():
    gbs = sdrg.measure_hbm_copy(0, 1 << 30, 10)
    emit(dict(kind="hbm_copy", read_plus_write_gb_s=round(gbs, 1), library=LIBRARY))
    return gbs


def timed(work, call, reps, warm):
    for k in range(warm):
        call(k)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(work):
        a.record()
        for k in range(reps):
            call(k)
        b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def inputs(B, n, fmt):
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    info = torch.iinfo(TORCH_DTYPE[fmt])
    return [torch.randint(info.min, info.max + 1, (B, 2 * n), device=dev, generator=g, dtype=torch.int32)
            .to(TORCH_DTYPE[fmt]) for _ in range(3)]


def engine(B, n):
    return sdrg.Engine(sdrg.SDRConfig(centerFrequency=100_000_000, samplesPerReading=n, sampleRate=FS,
                                      freqFocusRangeKhz=5, soundMode=1), B)


class BankRun:
    def __init__(self, B, n, fmt, M, P, O, first=0, rows=None, bufs=None):
        self.B, self.n, self.fmt, self.M, self.P, self.O = B, n, fmt, M, P, O
        self.rows = M - first if rows is None else rows
        self.cfg = dict(cutoff_rel=0.5, channels=M, taps_per_channel=P, oversample=O, first_channel=first,
                        n_channels=self.rows)
        self.eng = engine(B, n)
        self.eng.set_channelizer(**self.cfg)
        self.cap = self.eng.channelizer_max_out()
        self.bufs = bufs if bufs is not None else inputs(B, n, fmt)
        self.out = torch.zeros((B, self.rows, self.cap, 2), dtype=torch.float32, device=dev)
        self.n_out = ctypes.c_int32()
        self.work = torch.cuda.Stream(dev)
        self.eng.set_stream(self.work.cuda_stream)
        torch.cuda.synchronize()

    def call(self, k):
        rc = lib.sdrg_engine_channelizer_device(self.eng._h, ctypes.c_void_p(self.bufs[k % 3].data_ptr()), self.fmt,
                                                ctypes.c_void_p(self.out.data_ptr()), ctypes.byref(self.n_out))
        assert rc == 0, rc

    def time(self, note=None):
        us = timed(self.work, self.call, K, 6)
        in_bytes = self.B * self.n * sdrg.BYTES_PER_SAMPLE[self.fmt]
        out_bytes = self.B * self.rows * self.cap * 8
        r = dict(kind="channelizer", library=LIBRARY, streams=self.B, n=self.n, format=NAME[self.fmt], channels=self.M,
                 taps_per_channel=self.P, oversample=self.O, rows=self.rows, buffers=3, calls=K,
                 tile_outputs=sdrg.channelizer_tile_outputs(**self.cfg), us_per_launch=round(us, 2), in_bytes=in_bytes,
                 out_bytes=out_bytes, read_plus_write_gb_s=round((in_bytes + out_bytes) / (us * 1e-6) / 1e9, 1),
                 out_sha256=sha256(self.out))
        if note:
            r["note"] = note
        results.append(r)
        return us

    def close(self):
        self.eng.set_stream(None)
        self.eng.close()
        del self.bufs, self.out
        torch.cuda.empty_cache()


def bank_alone(*a, note=None, **k):
    run = BankRun(*a, **k)
    run.time(note)
    run.close()


def bank_against_16_ddc_calls(B, n, fmt):
    """The (16, 8, 1) bank and 16 ddc calls (T = 127, D = 16: the bank's taps and rate) on the same buffers, in turn."""
    bufs = inputs(B, n, fmt)
    bank = BankRun(B, n, fmt, 16, 8, 1, bufs=bufs)
    eng = engine(B, n)
    eng.set_ddc(offset_hz=125_000.0, cutoff_hz=0.5 * FS / 16, decimation=16, taps=127)
    out = torch.zeros((B, eng.ddc_max_out(), 2), dtype=torch.float32, device=dev)
    n_out = ctypes.c_int32()
    eng.set_stream(bank.work.cuda_stream)
    torch.cuda.synchronize()

    def sixteen(k):
        for _ in range(16):
            rc = lib.sdrg_engine_ddc_device(eng._h, ctypes.c_void_p(bufs[k % 3].data_ptr()), fmt,
                                            ctypes.c_void_p(out.data_ptr()), ctypes.byref(n_out))
            assert rc == 0, rc

    for rnd in range(3):
        us_bank = bank.time(note=f"round {rnd}, alternating with 16 ddc calls")
        us_ddc = timed(bank.work, sixteen, max(K // 8, 3), 2)
        results.append(dict(kind="ddc_x16", library=LIBRARY, streams=B, n=n, format=NAME[fmt], taps=127, decimation=16,
                            round=rnd, us_per_16_calls=round(us_ddc, 2), bank_us=round(us_bank, 2),
                            ratio=round(us_ddc / us_bank, 2), out_sha256=sha256(out)))
    eng.set_stream(None)
    eng.close()
    bank.close()


before = hbm()
bank_alone(4096, 16384, sdrg.CS8, 16, 8, 1)
bank_alone(4096, 16384, sdrg.CS8, 64, 8, 1)
bank_alone(4096, 16384, sdrg.CS8, 64, 8, 2)
bank_alone(4096, 16384, sdrg.CS8, 256, 16, 2)
bank_alone(4096, 16384, sdrg.CS8, 64, 8, 2, first=28, rows=8)
bank_alone(1024, 65536, sdrg.CS16, 256, 16, 2)
bank_alone(4096, 16384, sdrg.CS8, 64, 1, 1, note="attribution: staging, DFT and stores with one tap per branch")
bank_alone(4096, 16384, sdrg.CS8, 64, 1, 1, first=32, rows=1, note="attribution: staging and DFT, one row stored")
bank_alone(4096, 16384, sdrg.CS8, 64, 8, 1, first=32, rows=1, note="attribution: (64, 8, 1) with one row stored")
bank_against_16_ddc_calls(4096, 16384, sdrg.CS8)
after = hbm()
copy = (before + after) / 2
for r in results:
    if r["kind"] == "channelizer":
        floor_us = (r["in_bytes"] + r["out_bytes"]) / (copy * 1e9) * 1e6
        r.update(copy_gb_s=round(copy, 1), yardstick_us=round(floor_us, 2),
                 share=round(floor_us / r["us_per_launch"], 3))
    emit(r)
