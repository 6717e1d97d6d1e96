"""The SSB chain's case table: the shapes that reach every FIR slot layout, both kernel families and the chunk-table
edges of csrc/ssb.hip, and the input families that drive the chain's clamps, silences and number ranges.
tests/test_ssb_cases.py proves on the CPU (oracle + sdrg.ssb_layout, no device) that the table reaches what it
claims; tests/test_gpu_ssb_layouts.py and tests/test_gpu_ssb_inputs.py run it bit-exact against the oracle.

Layout of a shape (sdrg.ssb_layout, the launcher's own predicate): D = max(1, int(fs / 48000.0f)); the pipeline kernel
keeps ns = (64 + taps - 2) / D + 1 FIR accumulators per stream, rounded up to 4, 8, 16 or 32 slots; more than 32, or
more than 8 outputs completed per 64-sample chunk, goes to the lane-per-stream kernels.
"""
from __future__ import annotations

import numpy as np

FORMATS = ("CS8", "CU8", "CS16", "CF32")
B = 45          # a full 32-stream workgroup plus one of 13 (tests/test_gpu_ssb_schedule.py)
CALLS = 3
CHUNK = 64      # asserted against sdrg.ssb_layout()["chunk"]

# fs -> (D, layout with 255 taps, layout with 127 taps); a layout is a slot count or "lane" (lane-per-stream kernels).
# Checked row by row against sdrg.ssb_layout: the query is the authority.
RATES = {
    250_000: (5, "lane", "lane"),
    432_000: (9, "lane", 32),       # 127 taps: 8 outputs per chunk == MAX_DONE
    480_000: (10, 32, 32),          # 255 taps: all 32 slots live
    912_000: (19, 32, 16),          # 255 taps: 17 live
    1_024_000: (21, 16, 16),        # 255 taps: all 16 live
    1_440_000: (30, 16, 8),
    3_200_000: (66, 8, 4),          # D > chunk: chunks that complete no output
    3_840_000: (80, 4, 4),          # 255 taps: all 4 live
    10_000_000: (208, 4, 4),
    30_720_000: (640, 4, 4),        # D > chunk + taps: chunks inside no output window
}

# Frame lengths.  Whole chunks: 2048 (LDS-DMA loader for CS8, CU8, CS16: whole 256-B batches) and 1088 = 17 chunks (an
# odd chunk count: no DMA for the 8-bit formats, DMA for CS16).  Partial last chunk: 1500 and the odd 2005 (frames of
# the 8-bit formats then start at unaligned addresses).  CF32 never takes the DMA loader (64 samples are 512 B).
# 30.72 MHz needs 4096 samples for 7 outputs.
_WHOLE = (2048, 1088)
_PART = (1500, 2005)


def _shapes():
    out = []
    for r, fs in enumerate(RATES):
        for k, taps in enumerate((0, 127)):
            for part in (0, 1):
                n = (_PART if part else _WHOLE)[(r + k) % 2]
                if fs == 30_720_000:
                    n = 4000 if part else 4096
                # formats rotate so that every format meets every slot count (asserted in test_ssb_cases.py)
                fmt = FORMATS[(r + 3 * k + part + (r // 4)) % 4]
                out.append(dict(fs=fs, taps=taps, nco=0.0, fmt=fmt, n=n))
    # the NCO mixer (the loader's other role map) on a 32-, a 16- and a 4-slot layout and on the lane-per-stream path
    out += [dict(fs=480_000, taps=0, nco=40e3, fmt="CS16", n=2048),
            dict(fs=1_024_000, taps=0, nco=-100e3, fmt="CU8", n=1500),
            dict(fs=3_840_000, taps=127, nco=250e3 + 0.37, fmt="CF32", n=2005),
            dict(fs=432_000, taps=0, nco=-61e3, fmt="CS8", n=1088)]
    return out


SHAPES = _shapes()

# Output-count boundaries, 255 taps, at three slot counts: n = 254 (no output: the PL == 0 branches), 255 (one),
# 255 + D - 1 (still one), 255 + D (two)
BOUNDARY_RATES = (480_000, 1_024_000, 3_840_000)
BOUNDARIES = [dict(fs=fs, taps=0, nco=0.0, fmt=FORMATS[(i + j) % 4], n=n)
              for i, fs in enumerate(BOUNDARY_RATES)
              for j, n in enumerate((254, 255, 255 + RATES[fs][0] - 1, 255 + RATES[fs][0]))]

# short FIR switched off again (taps and chunk table re-derived), and the pipelined schedule, at 16 and 32 slots
SWITCH_BACK = [dict(fs=1_024_000, fmt="CS8", n=2048), dict(fs=480_000, fmt="CU8", n=1500)]
PIPELINED = [dict(fs=1_440_000, taps=0, nco=0.0, fmt="CS16", n=2048), dict(fs=912_000, taps=0, nco=0.0, fmt="CS8", n=1500)]

# Input-family shapes: one per slot count and the lane-per-stream path, 255 taps.  The last figure is the number of
# all-zero calls family 3 sends between its two tones: the smallest count after which the oracle's PCM is all zero for
# a whole call for every stream, format, mode schedule and sideband below (counted in test_ssb_cases.py).  The
# oracle's low-pass state itself never returns to exactly zero: it parks on a subnormal fixed point of the biquad
# (|z| between 4e-45 and 1e-42 here), so "silence" is measured where it is observable, in the PCM.
INPUT_SHAPES = [dict(fs=250_000, n=2048, silence=2), dict(fs=480_000, n=2005, silence=2),
                dict(fs=1_024_000, n=2048, silence=3), dict(fs=3_200_000, n=4000, silence=4),
                dict(fs=3_840_000, n=4096, silence=5)]
SILENCE_CALLS = {(s["fs"], s["n"]): s["silence"] for s in INPUT_SHAPES}  # any other shape: 1
MODE_SCHEDULES = {"mode0": (0,), "mode1": (1,), "mode2": (2,), "switch": (1, 2, 0)}  # cycled over the calls


def _input_cases():
    out = []
    for s, sh in enumerate(INPUT_SHAPES):
        calls = sh["silence"] + 2
        for k, sched in enumerate(MODE_SCHEDULES):
            out.append(dict(fs=sh["fs"], n=sh["n"], fmt=FORMATS[(s + k) % 4], sched=sched, upper=True, calls=calls))
        out.append(dict(fs=sh["fs"], n=sh["n"], fmt=FORMATS[(s + 3) % 4], sched="switch", upper=False, calls=calls))
        out.append(dict(fs=sh["fs"], n=sh["n"], fmt=FORMATS[s % 4], sched="mode0", upper=False, calls=3))
    return out


INPUT_CASES = _input_cases()

# fixtures from the reference build at the rates above (tests/golden/make_golden.py make_ssb_layout_fixtures)
GOLDEN_SSB_CASES = ["golden_ssb_cs8_2048_fs250k", "golden_ssb_cu8_2005_fs480k", "golden_ssb_cs16_2048_fs1024k",
                    "golden_ssb_cf32_2048_fs10m", "golden_ssb_cf32_range_2048_fs1024k"]
GOLDEN_SSB_DESIGN = "golden_ssb_layout_design"


def modes_of(sched: str, calls: int):
    m = MODE_SCHEDULES[sched]
    return [m[f % len(m)] for f in range(calls)]


def case_id(c: dict) -> str:
    s = f"{c['fmt']}-fs{c['fs']}-n{c['n']}"
    if c.get("taps"):
        s += f"-t{c['taps']}"
    if c.get("nco"):
        s += "-nco"
    if "sched" in c:
        s += f"-{c['sched']}-{'usb' if c['upper'] else 'lsb'}"
    return s


# ---------------------------------------------------------------------------------------------------------
# Input families: (fmt name, stream, call, n, fs, seed) -> the raw frame, 2n codes of the format's type
# ---------------------------------------------------------------------------------------------------------
_DTYPE = {"CS8": np.int8, "CU8": np.uint8, "CS16": np.int16, "CF32": np.float32}
_HI = {"CS8": 127, "CU8": 255, "CS16": 32767, "CF32": 1.0}
_LO = {"CS8": -128, "CU8": 0, "CS16": -32768, "CF32": -1.0}
_ZERO = {"CS8": 0, "CU8": 127, "CS16": 0, "CF32": 0.0}  # CU8 has no exact zero: 127 is -0.4 / 128


def _blank(fmt, n):
    return np.full(2 * n, _ZERO[fmt], dtype=_DTYPE[fmt])


def _rng(seed, stream, call, fam):
    return np.random.default_rng([seed, stream, call, fam])


def fam_uniform(fmt, stream, call, n, fs, seed):
    """1: uniform random codes over the format's whole range (CF32: [-1, 1)), the extreme codes and zero included;
    every call different."""
    rng = _rng(seed, stream, call, 1)
    if fmt == "CF32":
        raw = rng.uniform(-1.0, 1.0, 2 * n).astype(np.float32)
    else:
        raw = rng.integers(_LO[fmt], _HI[fmt] + 1, 2 * n).astype(_DTYPE[fmt])
    pos = rng.permutation(2 * n)[:6]
    raw[pos[0::3]] = _LO[fmt]
    raw[pos[1::3]] = _HI[fmt]
    raw[pos[2::3]] = 0
    return raw


def fam_square(fmt, stream, call, n, fs, seed):
    """2: a full-scale square wave in the passband (1 to 2 kHz) on I, zero on Q; phase runs on across calls."""
    period = max(2, int(round(fs / (1000.0 + 61.0 * (stream % 17)))))
    t = np.arange(n, dtype=np.int64) + call * n + 7 * stream + seed
    raw = _blank(fmt, n)
    raw[0::2] = np.where((t % period) < period // 2, _HI[fmt], _LO[fmt]).astype(_DTYPE[fmt])
    return raw


def fam_silence(fmt, stream, call, n, fs, seed):
    """3: a tone for one call, all-zero frames for SILENCE_CALLS[fs, n] calls (1 for a shape not listed), the tone
    again from then on."""
    z = SILENCE_CALLS.get((fs, n), 1)
    if 1 <= call <= z:
        return _blank(fmt, n)
    t = np.arange(n, dtype=np.float64) + call * n
    ph = 2 * np.pi * (1000.0 + 37.0 * (stream % 27)) * t / fs + 0.1 * (stream + seed % 7)
    iq = 0.47 * np.stack([np.cos(ph), np.sin(ph)], axis=1).reshape(-1)
    if fmt == "CF32":
        return iq.astype(np.float32)
    if fmt == "CU8":
        return np.clip(np.round(iq * 128.0 + 127.4), 0, 255).astype(np.uint8)
    return np.round(iq * (_HI[fmt] + 1)).astype(_DTYPE[fmt])


def impulse_positions(n):
    """0, the last sample of the first chunk, the first of the second, n - 1, the first sample of the last chunk
    (the partial one when n is no multiple of the chunk)"""
    last = ((n - 1) // CHUNK) * CHUNK
    return [min(p, n - 1) for p in (0, CHUNK - 1, CHUNK, n - 1, last)]


def fam_impulse(fmt, stream, call, n, fs, seed):
    """4: one full-scale sample on I at one of impulse_positions(n), everything else zero."""
    pos = impulse_positions(n)
    k = stream // len(families_for(fmt)) + call + seed  # 5 positions x 2 signs: distinct over a batch's 9 streams
    raw = _blank(fmt, n)
    raw[2 * pos[k % len(pos)]] = _HI[fmt] if (k // len(pos)) % 2 == 0 else _LO[fmt]
    return raw


def fam_step(fmt, stream, call, n, fs, seed):
    """5: the first half of the frame at full-scale DC, the second half at the opposite full scale (the switch a few
    samples past the middle, by stream, so that no two streams of a batch agree)."""
    j = stream // len(families_for(fmt))
    a, b = (_HI[fmt], _LO[fmt]) if (j + call + seed) % 2 == 0 else (_LO[fmt], _HI[fmt])
    raw = np.empty(2 * n, dtype=_DTYPE[fmt])
    raw[: 2 * (n // 2 + j)] = a
    raw[2 * (n // 2 + j):] = b
    return raw


def fam_range(fmt, stream, call, n, fs, seed):
    """6 (CF32 only): magnitudes log-uniform over 2^0 .. 2^100 (call % 3 == 0), over 2^-149 .. 2^0 (1) or each
    sample from one of the two ranges (2); random signs; +0 and -0 sprinkled in."""
    assert fmt == "CF32"
    rng = _rng(seed, stream, call, 6)
    big = np.exp2(rng.uniform(0.0, 100.0, 2 * n))
    small = np.exp2(rng.uniform(-149.0, 0.0, 2 * n))
    pick = (np.zeros(2 * n, bool), np.ones(2 * n, bool), rng.random(2 * n) < 0.5)[call % 3]
    mag = np.where(pick, small, big)
    raw = (mag * rng.choice([-1.0, 1.0], 2 * n)).astype(np.float32)
    zeros = rng.permutation(2 * n)[: max(2, n // 16)]
    raw[zeros[0::2]] = 0.0
    raw[zeros[1::2]] = -0.0
    return raw


FAMILIES = (fam_uniform, fam_square, fam_silence, fam_impulse, fam_step, fam_range)


def families_for(fmt: str):
    return FAMILIES if fmt == "CF32" else FAMILIES[:5]


def family_of(fmt: str, stream: int) -> int:
    """Stream b of a batch runs family b % K: neighbours in one 16-stream workgroup never share a trajectory."""
    return stream % len(families_for(fmt))


def batch(fmt: str, n_streams: int, calls: int, n: int, fs: int, seed: int = 0x55B) -> np.ndarray:
    """raw[stream][call][2n] of the format's type, stream b from family b % K"""
    fams = families_for(fmt)
    return np.stack([np.stack([fams[b % len(fams)](fmt, b, f, n, fs, seed) for f in range(calls)])
                     for b in range(n_streams)])


def oracle_pcm(O, raw, fmt, n, fs, modes, upper=True, taps=0, nco=0.0, stages=False, streams=None):
    """want[call][stream] (with stages: (pcm, stage taps)) of the oracle's processSSB_opt restatement, one fresh
    state per stream; modes[call] and upper may change per call (upper: a bool or one per call)."""
    fmt_id = getattr(O, fmt)
    calls = raw.shape[1]
    ups = [upper] * calls if isinstance(upper, bool) else list(upper)
    streams = range(raw.shape[0]) if streams is None else streams
    want = [dict() for _ in range(calls)]
    for b in streams:
        st = O.SsbState()
        if taps or nco:
            st.set_variant(nco, fs, taps)
        for f in range(calls):
            want[f][b] = st.process(O.unpack(fmt_id, raw[b, f], n), fs, modes[f], ups[f], stages=stages)
    return want
