"""tests/stats_cases.py kept honest on the CPU: its constants against csrc/stats.hip, its geometry against the oracle's,
its labels against the case table, the table against a sweep of geometries (a launcher change that adds or moves a
variant fails here until a case exists), the two statistics restatements against each other on the very spectra the
GPU test feeds, and the conditions on those spectra that keep the GPU test from going blind."""
import functools
import os
import re

import numpy as np
import pytest

import stats_cases as sc
import stats_np
from conftest import ROOT
from test_stats_restatements import compare

CSRC = os.path.join(ROOT, "sdr-for-android-lib_amd", "csrc")
CF = 100_000_000
ROWS = list(enumerate(sc.CASES))
ROW_IDS = [sc.case_id(r) for r in sc.CASES]


# --------------------------------------------------------------------------------------------------
# constants and expressions
# --------------------------------------------------------------------------------------------------
def test_restated_constants_match_the_source():
    with open(os.path.join(CSRC, "stats.hip")) as f:
        st = f.read()

    def const(name):
        return int(re.search(r"constexpr int %s = (\d+);" % name, st).group(1))

    def define(name):
        return int(re.search(r"#ifndef %s\b[^\n]*\n#define %s (\d+)" % (name, name), st).group(1))

    for name in ("WAVE", "STAGE_MAX", "WIDE_WG", "REG_POOL", "NARROW_REG_POOL", "MW_F", "MW_PR", "MW_RING_FLOATS",
                 "MW_POOL", "MW_K"):
        assert const(name) == getattr(sc, name), name
    assert define("SDRG_MW_T") == sc.MW_T and re.search(r"constexpr int MW_T = SDRG_MW_T;", st)
    assert define("SDRG_MW_WREF") == sc.SDRG_MW_WREF
    assert define("SDRG_WIDE_RING") == sc.WIDE_RING and re.search(r"constexpr int RING_FLOATS = SDRG_WIDE_RING;", st)
    assert define("SDRG_WIDE_DBPOOL") == 2 and define("SDRG_MW_DBPOOL") == 1  # the dB rows the labels speak of
    assert re.search(r"constexpr int MW_RECW = MW_F;", st) and re.search(r"constexpr int MW_P0 = 1 \+ MW_RECW;", st)
    assert re.search(r"constexpr int MW_PROD = MW_T - 64 \* MW_P0;", st)
    assert sc.MW_P0 == 1 + sc.MW_F and sc.MW_PROD == sc.MW_T - 64 * sc.MW_P0
    # the expressions plan() restates
    for pattern in (
            r"return stage_bins\(geo\) > STAGE_MAX;",
            r"geo\.n_ref > 10 \|\| \(geo\.n_ref >= 2 && !spec_pool\) \|\| geo\.max_pool > MW_POOL\) return mp;",
            r"const int chains = 2 \* nwin \+ \(spec_pool \? nwin - 1 : 0\);",
            r"if \(chains > WAVE / MW_F \|\| WAVE / \(MW_F \* nwin\) < 1\) return mp;",
            r"if \(MW_F \* nwin \* 8 \* \(\(1 << l\) \+ 4\) <= MW_RING_FLOATS && \(1 << l\) <= MW_PR \* pg\) "
            r"mp\.lg = l;",
            r"\*pgf = MW_PROD / \(SDRG_MW_WREF \* MW_F \* fq \+ MW_F\);",
            r"\*pgr = \(MW_PROD - MW_F \* \*pgf\) / \(MW_F \* fq\);",
            r"\*pgf = \*pgr = MW_PROD / \(MW_F \* nwin\);",
            r"const int R = pool16 <= 8 \* WAVE \? 8 : pool16 <= NARROW_REG_POOL \* WAVE \? NARROW_REG_POOL : 0;",
            r"pool16 = \(geo\.max_pool \+ 15\) & ~15;",
            r"if \(cnt <= REG_POOL \* WG\) \{",
            r"while \(8 \* nwin \* \(\(2 << lg\) \+ 4\) <= RING_FLOATS && lg < 12\) lg\+\+;",
            r"const dim3 grid\(\(n_frames \+ MW_F - 1\) / MW_F\);"):
        assert re.search(pattern, st), pattern


# --------------------------------------------------------------------------------------------------
# geometry, labels, coverage
# --------------------------------------------------------------------------------------------------
def same_geometry(O, fs, n, focus):
    g = sc.geometry(fs, n, focus)
    lo, hi, w, wins = O.window_geometry(fs, n, focus)
    assert (lo, hi, w, wins) == (g["focus_lo"], g["focus_hi"], g["win_bins_1k"], g["wins"]), (fs, n, focus)
    return g


@functools.lru_cache(maxsize=None)
def sweep_labels():
    import oracle as O
    labels = {}
    for n in sc.SWEEP_N:
        for fs in sc.SWEEP_FS:
            for focus in sc.SWEEP_FOCUS:
                labels.setdefault(sc.plan(same_geometry(O, fs, n, focus)), (n, fs, focus))
    return labels


def test_geometry_equals_the_oracles(oracle_mod):
    for n, fs, focus, _ in sc.CASES:
        same_geometry(oracle_mod, fs, n, focus)
    assert len(sweep_labels()) >= 30  # every geometry of the sweep was compared on the way


@pytest.mark.parametrize("row", sc.CASES, ids=ROW_IDS)
def test_labels(row):
    n, fs, focus, label = row
    assert sc.plan(sc.geometry(fs, n, focus)) == label


def uncovered(cases, elsewhere):
    have = {row[3] for row in cases} | set(elsewhere)
    return {label: where for label, where in sweep_labels().items() if label not in have}


def test_every_variant_of_the_sweep_has_a_case(oracle_mod):
    assert uncovered(sc.CASES, sc.COVERED_ELSEWHERE) == {}
    # the check does bite: without the <false> rows, or without the map, it names what is missing
    fewer = [r for r in sc.CASES if not r[3].startswith("multi<false>")]
    assert set(uncovered(fewer, sc.COVERED_ELSEWHERE)) == {"multi<false>-lg9-nref0"}
    assert set(uncovered(sc.CASES, {})) == set(sc.COVERED_ELSEWHERE)
    # all six kernels, and both pools of the single-frame kernel with one bottom window
    labels = {r[3] for r in sc.CASES} | set(sc.COVERED_ELSEWHERE)
    for part in ("narrow-R8-", "narrow-R24-", "narrow-R0-", "multi<true>", "multi<false>", "wide1-", "-nb1-poolreg",
                 "-nb1-poolglob", "-nb2", "-nb3", "-nb4"):
        assert any(part in label for label in labels), part


def test_cases_covered_elsewhere_are_run_there():
    import test_gpu_stats_geometry as tg
    for label, (test, (n, fs, focus)) in sc.COVERED_ELSEWHERE.items():
        assert sc.plan(sc.geometry(fs, n, focus)) == label
        module, name = test.split("::")
        assert module == "test_gpu_stats_geometry.py" and callable(getattr(tg, name))
        assert (n, fs, focus) in tg.GEOMETRIES, label


def test_design_table_lists_every_variant():
    """DESIGN.md section 4, "Statistics variants": the variant -> covering test table is stats_cases.design_table()."""
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        lines = f.read().splitlines()
    head = lines.index("| variant | covered by: N / sample rate / focus kHz |")
    table = []
    for line in lines[head + 2:]:
        if not line.startswith("|"):
            break
        table.append(line)
    assert table == sc.design_table()


def test_thresholds_have_a_case_on_each_side():
    g = {row[:3]: sc.geometry(row[1], row[0], row[2]) for row in sc.CASES}
    stage = {sc.stage_bins(x) for x in g.values()}
    assert sc.STAGE_MAX in stage and sc.STAGE_MAX + 1 in stage
    one = [x["max_pool"] for x in g.values() if sc.stage_bins(x) > sc.STAGE_MAX and sc.spec_pool(x)]
    assert sc.MW_POOL in one and any(sc.MW_POOL < p <= sc.MW_POOL + 8 for p in one)
    top = sc.REG_POOL * sc.WIDE_WG
    assert top in one and any(top < p <= top + 64 for p in one)
    pool16 = {(x["max_pool"] + 15) & ~15 for x in g.values() if sc.stage_bins(x) <= sc.STAGE_MAX}
    for bound in (8 * sc.WAVE, sc.NARROW_REG_POOL * sc.WAVE):
        assert bound in pool16 and bound + 16 in pool16, bound


# --------------------------------------------------------------------------------------------------
# the run of every row: both restatements, and the conditions on its spectra
# --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def run(index):
    """Every frame of the row's GPU run (its stream count, three calls, one state per stream) through the C oracle:
    [(call, b, kind, occurrence, spectrum, record)], and the numpy restatement compared on the way."""
    import oracle as O
    n, fs, focus, label = sc.CASES[index]
    B = sc.case_streams(label)
    c_state = [O.FftState(CF, fs, n, focus) for _ in range(B)]
    np_state = [stats_np.SignalStrength(CF, fs, focus) for _ in range(B)]
    out = []
    for call in range(sc.CALLS):
        spec = sc.case_spectra(sc.CASES[index], index, B, call)
        now = 1000 + 333 * call
        for b in range(B):
            want = c_state[b].signal_strength(spec[b], now)
            compare(np_state[b].evaluate(spec[b], now), want, (sc.CASES[index], call, b, sc.kind_of(b, call)))
            out.append((call, b, sc.kind_of(b, call), sc.occurrence(b, call, B), spec[b], want))
    return out


def window_db(p, wins):
    """Each window's mean power in dB, float64."""
    return np.array([10.0 * np.log10(np.mean(p[l:h + 1].astype(np.float64)) + 1e-20) for l, h in wins])


@pytest.mark.parametrize("index,row", ROWS, ids=ROW_IDS)
def test_restatements_agree_and_inputs_hold_their_conditions(oracle_mod, index, row):
    n, fs, focus, label = row
    g = sc.geometry(fs, n, focus)
    B = sc.case_streams(label)
    frames = run(index)  # raises where the C oracle and oracle/stats_np.py differ in a bit
    assert len(frames) == sc.CALLS * B >= 6
    kinds = {k for _, _, k, _, _, _ in frames}
    assert kinds >= set(sc.KINDS) - ({"plateau"} if B < 9 else set()), kinds
    # the oracle alone: frames are valid exactly when two reference windows exist
    for call, b, kind, _, _, rec in frames:
        assert int(rec["valid"]) == (1 if g["n_ref"] >= 2 and g["focus_len"] > 0 else 0), (call, b, kind)
        assert int(rec["n_ref_windows"]) == (g["n_ref"] if g["focus_len"] > 0 else 0), (call, b, kind)
    if g["focus_len"] <= 0:
        return
    # "peak": the oracle's peak sits on both focus edges (and, where the run has four such frames, on both sides
    # of the first chunk edge)
    want = sc.peak_positions(g)[:4 if B >= 9 else 2]
    got = [int(rec["peak_bin"]) for _, _, kind, _, _, rec in frames if kind == "peak"]
    assert set(want) <= set(got), (want, got)
    assert g["focus_lo"] in got and g["focus_hi"] in got
    if label.startswith("multi"):
        assert g["focus_lo"] + (1 << sc.chunk_lg(g)) in got  # a second chunk exists in every such row
    # "plateau": the 400 equal maxima exceed what the multi-frame kernel's lanes keep (MW_K each, whatever the
    # split of a chunk among them), and the peak is the plateau's first bin
    for _, _, kind, occ, p, rec in frames:
        if kind == "plateau":
            focus = p[g["focus_lo"]:g["focus_hi"] + 1]
            top = np.flatnonzero(focus == focus.max())
            assert top.size == min((40, 400)[occ % 2], g["focus_len"])
            assert int(rec["peak_bin"]) == g["focus_lo"] + top[0]
    # "bottom": the scaled window is the lowest by 1 dB at least
    bottoms = set()
    for _, _, kind, occ, p, _ in frames:
        if kind == "bottom" and g["n_ref"] >= 2:
            db = window_db(p, g["wins"])
            wb = sc.bottom_index(g["n_ref"], occ)
            assert int(np.argmin(db)) == wb and np.sort(db)[1] - db[wb] >= 1.0, (occ, db)
            bottoms.add(wb)
        elif kind == "const" and g["n_ref"] >= 2:
            assert p.min() == p.max()  # equal means: the stable sort leaves window 0 first
            bottoms.add(0)
    if sc.spec_pool(g):  # one bottom window (n_ref 2..4): each is it at least once
        assert bottoms == set(range(g["n_ref"])), bottoms
    elif g["n_ref"] >= 2:
        assert len(bottoms) >= 3
    # "bump": a w-bin bump at each window's start, at its end and, where the window is long enough, across the
    # first chunk edge
    w, lg = g["win_bins_1k"], sc.chunk_lg(g)
    for l, h in g["wins"] + [(g["focus_lo"], g["focus_hi"])]:
        starts = {sc.bump_start(l, h, w, lg, v) for v in range(3)}
        if h - l + 1 > w:
            assert l in starts and h - w + 1 in starts
        if h - l + 1 > (1 << lg) + w and w >= 2:
            s = l + (1 << lg) - w // 2
            assert s in starts and s < l + (1 << lg) <= s + w - 1


def test_walk_and_end_to_end_labels_and_restatements(oracle_mod):
    """The reconfiguration walk of the GPU test crosses the variants it names, and both restatements carry a
    stream's state across it alike."""
    O = oracle_mod
    n, fs, B = sc.WALK_N, sc.WALK_FS, sc.WALK_STREAMS
    assert [sc.plan(sc.geometry(fs, n, focus)) for focus, _ in sc.WALK] == [label for _, label in sc.WALK]
    assert [sc.plan(sc.geometry(sc.E2E_FS, sc.E2E_N, focus)) for focus, _ in sc.E2E] == [label for _, label in sc.E2E]
    c_state = [O.FftState(CF, fs, n, sc.WALK[0][0]) for _ in range(B)]
    np_state = [stats_np.SignalStrength(CF, fs, sc.WALK[0][0]) for _ in range(B)]
    kinds, valid = set(), []
    for step, (focus, _) in enumerate(sc.WALK):
        for b in range(B):
            c_state[b].configure(CF, fs, n, focus)
            np_state[b].configure(CF, fs, focus)
        for k in range(sc.WALK_CALLS):
            spec = sc.walk_spectra(step, k)
            now = 1000 + 150 * (sc.WALK_CALLS * step + k)
            for b in range(B):
                want = c_state[b].signal_strength(spec[b], now)
                compare(np_state[b].evaluate(spec[b], now), want, ("walk", step, k, b))
                kinds.add(sc.kind_of(b, sc.WALK_CALLS * step + k))
            valid.append(int(want["valid"]))
    assert kinds == set(sc.KINDS)
    assert valid == [1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1]  # the invalid stretch at 400 kHz in the middle


def test_single_stream_rows_are_rows():
    assert {r[3][:11] for r in sc.SINGLE_STREAM_ROWS} == {"multi<true>", "multi<false"}
    assert all(r in sc.CASES for r in sc.SINGLE_STREAM_ROWS)
    for label in {r[3] for r in sc.CASES}:  # 9 streams: two full workgroups and one of a single frame
        B = sc.case_streams(label)
        assert (B == 9 and B % sc.MW_F == 1 and B // sc.MW_F == 2) if label.startswith("multi") else B == 5
