"""The statistics launcher's arithmetic restated for the tests, the case table tied to it and the spectra the GPU
test feeds ("Statistics variants").

launch_stats (csrc/stats.hip) picks one of six kernels from the window geometry alone, and the kernels branch further
on it.  Nothing here touches a GPU:

  geometry(fs, n, focus_khz) -> dict    csrc/design.cpp stats_geometry in float32 arithmetic
  plan(geometry)             -> label   the launcher's choice, naming everything that selects code:
        narrow-nofocus                        an empty focus window (the kernels write the stale record)
        narrow-R{8,24,0}-nref{k}              stats_narrow_kernel<R>: the pool in 8 or 24 registers per lane, or in LDS
        multi<true|false>-lg{l}-nref{k}       stats_wide_multi_kernel<want_db>, chunks of 2^lg bins per window
        wide1-nref{k}-nb{n_bottom}[-poolreg|-poolglob]
                                              stats_wide_kernel; one bottom window (scan_wide<true>, the dB rows) with
                                              its gaps in registers or in HBM scratch; several (scan_wide<false>)
  CASES                                 (n, fs, focus_khz, label): tests/test_gpu_stats_variants.py runs every row,
                                        tests/test_stats_cases.py checks the labels and that no label a sweep of
                                        geometries produces is missing from it
  COVERED_ELSEWHERE                     labels of the sweep that an older GPU test's own geometry list already runs
  case_spectra(...)                     the input kinds, chosen per (stream, call)
  WALK, E2E, walk_spectra(...)          one engine reconfigured across the variants; the end-to-end geometries
  design_table()                        the variant -> covering test table of DESIGN.md

tests/test_stats_cases.py compares every constant below with the sources, geometry() with the oracle's, and asserts
the input conditions that keep the GPU test from going blind."""
from __future__ import annotations

import numpy as np

f32 = np.float32

# csrc/stats.hip (tests/test_stats_cases.py parses the file for each)
WAVE = 64                   # :29
STAGE_MAX = 8192            # :30   bins the narrow kernel stages into LDS
WIDE_WG = 256               # :135  threads of stats_wide_kernel
WIDE_RING = 9216            # :137  floats of scan_wide's ring (SDRG_WIDE_RING)
REG_POOL = 64               # :683  pooled gaps per thread of stats_wide_kernel held in registers
NARROW_REG_POOL = 24        # :684  the narrow kernel's pool in registers up to 24 x 64 values
MW_T = 1024                 # :1246 threads per multi-frame workgroup (SDRG_MW_T)
MW_F = 4                    # :1258 frames per workgroup
SDRG_MW_WREF = 2            # :1260 producer lanes per reference-window lane per focus lane
MW_P0 = 1 + MW_F            # :1276 first producer wave (1 + MW_RECW, MW_RECW = MW_F)
MW_PROD = MW_T - 64 * MW_P0  # :1277 producer lanes
MW_PR = 12                  # :1278 bins per producer lane per chunk at most
MW_RING_FLOATS = 28672      # :1279
MW_POOL = 13312             # :1280 pooled gaps per frame held in registers
MW_K = 4                    # :1281 focus candidates per producer lane


# --------------------------------------------------------------------------------------------------
# csrc/design.cpp stats_geometry (:106-178)
# --------------------------------------------------------------------------------------------------
def _off_to_bin(offset_hz, nyquist, freq_per_bin) -> int:
    return int((f32(offset_hz) + nyquist) / freq_per_bin)  # a C cast: towards zero


def geometry(fs: int, n: int, focus_khz: int) -> dict:
    fpb = f32(fs) / f32(n)
    x_hz = f32(focus_khz) * f32(1000.0)
    nyq = f32(fs) / f32(2.0)
    lo = _off_to_bin(-x_hz, nyq, fpb)
    hi = _off_to_bin(x_hz, nyq, fpb) - 1
    g = {"n": n, "fs": fs, "focus_khz": focus_khz, "focus_lo": max(lo, 0), "focus_hi": min(hi, n - 1)}
    g["focus_len"] = g["focus_hi"] - g["focus_lo"] + 1
    g["win_bins_1k"] = max(int(np.ceil(f32(1000.0) / fpb)), 1)
    wins = []
    for k in range(1, 6):
        near, far = f32(4 * k - 2) * x_hz, f32(4 * k) * x_hz
        if far >= nyq:
            break
        for l, h in ((_off_to_bin(near, nyq, fpb), _off_to_bin(far, nyq, fpb) - 1),
                     (_off_to_bin(-far, nyq, fpb), _off_to_bin(-near, nyq, fpb) - 1)):
            l, h = max(l, 0), min(h, n - 1)
            if h <= l:
                continue
            wins.append((l, h))
    g["wins"], g["n_ref"] = wins, len(wins)
    lens = sorted((h - l + 1 for l, h in wins), reverse=True)
    g["n_bottom"] = max(int(f32(len(wins)) * f32(0.4)), 1)
    g["max_pool"] = sum(lens[:g["n_bottom"]])
    return g


# --------------------------------------------------------------------------------------------------
# csrc/stats.hip launch_stats (:1874-2005)
# --------------------------------------------------------------------------------------------------
def stage_bins(g: dict) -> int:
    return max(0, g["focus_len"]) + sum(max(0, h - l + 1) for l, h in g["wins"][:10])


def spec_pool(g: dict) -> bool:
    """One bottom window: its dB sum and its dB values come out of the scan."""
    return g["n_ref"] >= 2 and g["n_bottom"] == 1


def mw_lanes(n_ref: int, want_db: bool):
    if want_db and n_ref > 0:
        pgf = MW_PROD // (SDRG_MW_WREF * MW_F * n_ref + MW_F)
        return pgf, (MW_PROD - MW_F * pgf) // (MW_F * n_ref)
    return (MW_PROD // (MW_F * (n_ref + 1)),) * 2


def multi_for(g: dict):
    """(ok, want_db, lg) of stats.hip multi_for."""
    n_ref, nwin, sp = g["n_ref"], g["n_ref"] + 1, spec_pool(g)
    if g["focus_len"] <= 0 or n_ref > 10 or (n_ref >= 2 and not sp) or g["max_pool"] > MW_POOL:
        return False, False, 0
    chains = 2 * nwin + (nwin - 1 if sp else 0)
    if chains > WAVE // MW_F or WAVE // (MW_F * nwin) < 1:
        return False, False, 0
    pg = min(mw_lanes(n_ref, sp))
    if pg < 1:
        return False, False, 0
    lg = 0
    for l in range(6, 11):
        if MW_F * nwin * 8 * ((1 << l) + 4) <= MW_RING_FLOATS and (1 << l) <= MW_PR * pg:
            lg = l
    return lg > 0, sp, lg


def narrow_r(g: dict) -> int:
    pool16 = (g["max_pool"] + 15) & ~15
    return 8 if pool16 <= 8 * WAVE else NARROW_REG_POOL if pool16 <= NARROW_REG_POOL * WAVE else 0


def wide_scan_lg(nwin: int) -> int:
    """scan_wide's chunk (:226-227): the largest 2^lg bins per window whose two slots fit the ring."""
    lg = 6
    while 8 * nwin * ((2 << lg) + 4) <= WIDE_RING and lg < 12:
        lg += 1
    return lg


def chunk_lg(g: dict) -> int:
    """log2 of the bins per window a scan takes at a time, counted from the window's first bin: the multi-frame
    kernel's lg, scan_wide's for the single-frame wide kernel, 8 for the narrow kernel (which has no chunks; 256 bins
    are four trips of its wave).  The generators put their edges there."""
    if stage_bins(g) <= STAGE_MAX:
        return 8
    ok, _, lg = multi_for(g)
    return lg if ok else wide_scan_lg(g["n_ref"] + 1)


def plan(g: dict) -> str:
    if g["focus_len"] <= 0:
        assert g["n_ref"] == 0  # focus 0 kHz: every window is empty too, so nothing is wide
        return "narrow-nofocus"
    if stage_bins(g) <= STAGE_MAX:
        return f"narrow-R{narrow_r(g)}-nref{g['n_ref']}"
    ok, want_db, lg = multi_for(g)
    if ok:
        return f"multi<{'true' if want_db else 'false'}>-lg{lg}-nref{g['n_ref']}"
    label = f"wide1-nref{g['n_ref']}-nb{g['n_bottom']}"
    if spec_pool(g):  # the kernel's `cnt <= REG_POOL * WG` on the bottom window, whichever it is
        lens = {h - l + 1 for l, h in g["wins"]}
        reg = {c <= REG_POOL * WIDE_WG for c in lens}
        label += "-poolreg" if reg == {True} else "-poolglob" if reg == {False} else "-poolmixed"
    return label


# --------------------------------------------------------------------------------------------------
# the case table: (n, fs, focus kHz, label)
# --------------------------------------------------------------------------------------------------
CASES = (
    (65536, 2_000_000, 400, "multi<false>-lg9-nref0"),        # focus 26215 bins
    (16384, 2_000_000, 1000, "multi<false>-lg9-nref0"),       # focus = whole spectrum, both ends clipped
    (12288, 2_000_000, 667, "multi<false>-lg9-nref0"),        # stage_bins 8197, just wide; N no power of two
    (32768, 2_000_000, 250, "narrow-R8-nref0"),               # stage_bins == STAGE_MAX exactly
    (16384, 2_400_000, 200, "multi<true>-lg8-nref2"),         # stage_bins STAGE_MAX + 1
    (65536, 2_048_000, 208, "multi<true>-lg8-nref2"),         # max_pool == MW_POOL exactly
    (131072, 2_048_000, 104, "multi<true>-lg7-nref4"),        # max_pool == MW_POOL, four windows
    (65536, 2_500_000, 254, "wide1-nref2-nb1-poolreg"),       # max_pool MW_POOL + 5
    (65536, 2_000_000, 225, "wide1-nref2-nb1-poolreg"),       # next to the benchmark geometry (200 kHz)
    (131072, 2_000_000, 125, "wide1-nref2-nb1-poolreg"),      # max_pool == REG_POOL * WIDE_WG exactly
    (98304, 2_000_000, 167, "wide1-nref2-nb1-poolglob"),      # max_pool 16417
    (131072, 2_000_000, 150, "wide1-nref2-nb1-poolglob"),
    (131072, 2_000_000, 105, "wide1-nref4-nb1-poolreg"),
    (262144, 2_000_000, 85, "wide1-nref4-nb1-poolglob"),
    (131072, 2_000_000, 65, "wide1-nref6-nb2"),               # pool 17040 in HBM
    (98304, 2_000_000, 60, "wide1-nref8-nb3"),                # pool 17694
    (98304, 2_000_000, 45, "wide1-nref10-nb4"),               # pool 17696
    (12288, 2_000_000, 65, "narrow-R0-nref6"),
    (8192, 2_048_000, 16, "narrow-R8-nref10"),                # pool 512, the R = 8 bound
    (4096, 2_000_000, 129, "narrow-R24-nref2"),               # pool 528, one 16-value step past it
    (8192, 2_400_000, 223, "narrow-R24-nref2"),               # pool 1522 -> 1536, the R = 24 bound
    (8192, 2_048_000, 194, "narrow-R0-nref2"),                # pool 1552, one step past it
    (1024, 2_000_000, 200, "narrow-R8-nref2"),
    (64, 2_000_000, 85, "narrow-R8-nref4"),                   # windows of 5 bins
    (4096, 2_400_000, 75, "narrow-R8-nref6"),                 # pool 512 again, two bottom windows
    (64, 2_000_000, 55, "narrow-R8-nref8"),
    (100, 2_000_000, 11, "narrow-R8-nref1"),                  # the reference's `h <= l` skip leaves odd counts;
    (100, 2_000_000, 13, "narrow-R8-nref3"),                  # one window alone is an invalid frame
    (100, 2_000_000, 15, "narrow-R8-nref5"),
    (100, 2_000_000, 17, "narrow-R8-nref7"),
    (100, 2_000_000, 19, "narrow-R8-nref9"),
    (1024, 2_000_000, 0, "narrow-nofocus"),
)

# labels the sweep of tests/test_stats_cases.py produces that an older GPU test already runs:
# label -> (test, (n, fs, focus kHz)), the geometry taken from that test's own parameter list
COVERED_ELSEWHERE = {
    "narrow-R0-nref10": ("test_gpu_stats_geometry.py::test_stats_geometry_vs_oracle", (65536, 2_000_000, 10)),
    "narrow-R0-nref4": ("test_gpu_stats_geometry.py::test_stats_geometry_vs_oracle", (16384, 2_000_000, 100)),
    "narrow-R0-nref8": ("test_gpu_stats_geometry.py::test_stats_geometry_vs_oracle", (16384, 2_000_000, 50)),
    "narrow-R24-nref10": ("test_gpu_stats_geometry.py::test_stats_geometry_vs_oracle", (8192, 2_000_000, 20)),
    "narrow-R24-nref4": ("test_gpu_stats_geometry.py::test_stats_geometry_vs_oracle", (8192, 2_000_000, 100)),
    "narrow-R24-nref6": ("test_gpu_stats_geometry.py::test_stats_geometry_vs_oracle", (8192, 2_500_000, 100)),
    "narrow-R24-nref8": ("test_gpu_stats_geometry.py::test_stats_geometry_vs_oracle", (8192, 2_000_000, 50)),
}

SWEEP_N = (64, 100, 1000, 4096, 8192, 12288, 16384, 20000, 32768, 65536, 65537, 98304, 131072, 262144, 1048576)
SWEEP_FS = (250_000, 1_000_000, 2_000_000, 2_048_000, 2_400_000, 2_500_000, 3_200_000, 10_000_000)
SWEEP_FOCUS = tuple(range(0, 31)) + tuple(range(35, 201, 5)) + tuple(range(225, 1001, 25))


def design_table():
    """The rows of DESIGN.md's "Statistics variants" table (variant -> covering test and geometries);
    tests/test_stats_cases.py compares the document with them."""
    rows = {}
    for n, fs, focus, label in CASES:
        rows.setdefault(label, []).append(f"{n} / {fs / 1e6:g} M / {focus}")
    out = []
    for label in sorted(set(rows) | set(COVERED_ELSEWHERE)):
        if label in rows:
            where = "`test_gpu_stats_variants.py`: " + ", ".join(rows[label])
        else:
            test, (n, fs, focus) = COVERED_ELSEWHERE[label]
            where = f"`{test.split('::')[0]}`: {n} / {fs / 1e6:g} M / {focus}"
        out.append(f"| `{label}` | {where} |")
    return out


def case_id(row) -> str:
    return f"{row[0]}-{row[1] // 1000}k-{row[2]}kHz"


def case_streams(label: str):
    """Stream counts of a row: the multi-frame kernel takes four frames per workgroup, so 9 streams are two full
    groups and one of a single frame; the others run 5."""
    return 9 if label.startswith("multi") else 5


# one <true> and one <false> row also run with a single stream (one workgroup of one frame)
SINGLE_STREAM_ROWS = ((65536, 2_048_000, 208, "multi<true>-lg8-nref2"),
                      (12288, 2_000_000, 667, "multi<false>-lg9-nref0"))

CALLS = 3


# --------------------------------------------------------------------------------------------------
# input kinds: stream b of call c takes KINDS[(b + c) % len(KINDS)]
# --------------------------------------------------------------------------------------------------
# With 5 streams and 3 calls b + c runs over 0..6: position k is taken 1, 2, 3, 3, 3, 2, 1, 0 times; with 9 streams
# (0..10) 4, 4, 4, 3, 3, 3, 3, 3 times.  So "peak" comes at least twice (both focus edges) and four times for the
# multi-frame kernel (both chunk edges as well), "bottom" three or four times (it rotates the bottom window), and the
# plateaus, which aim at the multi-frame kernel's candidate lists, sit where only its rows reach.
KINDS = ("noise", "peak", "bottom", "crafted", "bump", "tiny", "const", "plateau")


def kind_of(b: int, call: int) -> str:
    return KINDS[(b + call) % len(KINDS)]


def occurrence(b: int, call: int, B: int) -> int:
    """How many frames of the same kind the run has had before stream b of this call (calls in order, streams in
    order within a call): the generators rotate their variants by it."""
    k = (b + call) % len(KINDS)
    return sum(1 for c in range(call + 1) for s in range(B)
               if (s + c) % len(KINDS) == k and (c, s) < (call, b))


class _Geo:
    """What tests/test_gpu_stats_exact.py crafted() asks of the oracle module, answered from geometry() (crafted
    passes its own 2 MHz sample rate; the windows here are the row's)."""

    def __init__(self, g):
        self.g = g

    def window_geometry(self, fs, n, focus):
        g = self.g
        assert (n, focus) == (g["n"], g["focus_khz"])
        return g["focus_lo"], g["focus_hi"], g["win_bins_1k"], list(g["wins"])


def peak_positions(g: dict):
    """kind "peak": the focus edges, then the last bin of the first scan chunk and the first of the second."""
    lo, hi, sc = g["focus_lo"], g["focus_hi"], 1 << chunk_lg(g)
    pos = [lo, hi]
    if lo + sc <= hi:
        pos += [lo + sc - 1, lo + sc]
    return pos


def bump_start(lo: int, hi: int, w: int, lg: int, variant: int) -> int:
    """kind "bump": first bin of a w-bin bump in [lo, hi]: at lo, ending at hi, or across the first chunk edge."""
    if hi - lo + 1 <= w:
        return lo
    if variant == 0:
        return lo
    if variant == 1:
        return hi - w + 1
    s = lo + (1 << lg) - w // 2
    return s if lo <= s and s + w - 1 <= hi else lo + (hi - lo + 1 - w) // 2


def bottom_index(n_ref: int, occ: int) -> int:
    """kind "bottom": the window scaled down, from the last window towards the first.  Three frames of a 5-stream run
    reach windows 3, 2, 1 of four; a "const" frame, whose order falls to the window index, makes window 0 the bottom
    one, so every window is the single-frame kernel's scratch row `wb` at least once."""
    return (n_ref - 1 - occ) % n_ref


def frame(g: dict, row_index: int, B: int, b: int, call: int, rng) -> np.ndarray:
    """The spectrum of stream b at this call, float32 [n]."""
    n, lo, hi, wins = g["n"], g["focus_lo"], g["focus_hi"], g["wins"]
    kind, occ = kind_of(b, call), occurrence(b, call, B)
    if kind == "const":  # every window mean equal: the order falls to the window index
        return np.full(n, f32(0.37 * (1 + b) * (1 + call)), f32)
    if kind == "tiny":  # denormals of growing size and exact zeros (the 1e-20 floor dominates)
        level = (3 * occ + 2 * row_index + call) % 8
        if level == 0:
            return np.zeros(n, f32)
        p = rng.integers(1, 1 << (3 * level), n).astype(np.uint32).view(f32).copy()
        if level == 7:
            p[::7] = 0.0
        return p
    if kind == "crafted":  # ulp ties in the focus and between the windows' means
        from test_gpu_stats_exact import P0S, crafted
        sub = (occ + row_index) % (4 if wins else 2)  # its kinds 2 and 3 are about reference windows
        p0 = P0S[(5 * row_index + 3 * occ + b) % len(P0S)]
        return crafted(_Geo(g), n, g["focus_khz"], sub + 1, rng, [p0])[sub]
    if kind == "bottom":  # reference window `w` 6 dB down: the bottom window, whichever index it has
        p = rng.uniform(0.75, 1.25, n).astype(f32)  # no window mean strays more than 2.2 dB, whatever its length
        if wins:
            l, h = wins[bottom_index(len(wins), occ)]
            p[l:h + 1] *= f32(0.25)
        return p
    p = rng.exponential(1.0, n).astype(f32)
    if kind == "peak" and hi >= lo:
        pos = peak_positions(g)
        p[pos[occ % len(pos)]] = f32(1e4 * (1 + call))
    elif kind == "plateau" and hi >= lo:  # 40 equal maxima, or 400: more than the multi-frame kernel's lanes keep
        width, mid = (40, 400)[occ % 2], (lo + hi + 1) // 2
        p[max(lo, mid - width // 2):min(hi + 1, mid + width // 2)] = f32(55.0 + call)
    elif kind == "bump":  # the running 1 kHz sum's best start at a window's ends and across a chunk edge
        w, lg = g["win_bins_1k"], chunk_lg(g)
        for q, (l, h) in enumerate(list(wins) + ([(lo, hi)] if hi >= lo else [])):
            s = bump_start(l, h, w, lg, (occ + q) % 3)
            p[s:min(s + w, h + 1)] *= f32(8.0)
    return p


def case_spectra(row, row_index: int, B: int, call: int) -> np.ndarray:
    """[B][n] float32: call `call` of the row's run."""
    n, fs, focus, _ = row
    g = geometry(fs, n, focus)
    rng = np.random.default_rng([n, fs, focus, B, call])
    return np.stack([frame(g, row_index, B, b, call, rng) for b in range(B)])


# --------------------------------------------------------------------------------------------------
# one engine walked across the variants with setFrequencyFocusRange, and the end-to-end cases
# --------------------------------------------------------------------------------------------------
WALK_N, WALK_FS, WALK_STREAMS, WALK_CALLS = 65536, 2_000_000, 6, 2
WALK = ((5, "narrow-R24-nref10"), (200, "multi<true>-lg8-nref2"), (225, "wide1-nref2-nb1-poolreg"),
        (400, "multi<false>-lg9-nref0"), (60, "wide1-nref8-nb3"), (5, "narrow-R24-nref10"))
E2E_N, E2E_FS, E2E_STREAMS, E2E_CALLS = 65536, 2_000_000, 6, 3
E2E = ((225, "wide1-nref2-nb1-poolreg"), (400, "multi<false>-lg9-nref0"))


def walk_spectra(step: int, k: int) -> np.ndarray:
    """[WALK_STREAMS][WALK_N]: call k at step `step` of the walk; the kinds go on rotating over the whole walk."""
    g = geometry(WALK_FS, WALK_N, WALK[step][0])
    call = WALK_CALLS * step + k
    rng = np.random.default_rng([WALK_N, step, k])
    return np.stack([frame(g, step, WALK_STREAMS, b, call, rng) for b in range(WALK_STREAMS)])
