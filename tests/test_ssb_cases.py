"""CPU proof that tests/ssb_cases.py reaches what it claims, with the layout query (sdrg.ssb_layout, the launcher's
own predicate) and the oracle's stage taps alone: every FIR slot layout and both kernel families, the chunk-table
edges, both loaders per format, and inputs that drive the AGC clamp, the PCM clamp, silence and the lower sideband
with every stage value finite.  No device."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden

import sdrg
import ssb_cases as C


@pytest.fixture(scope="module")
def layouts():
    return [(s, sdrg.ssb_layout(s["fs"], s["n"], s["taps"])) for s in C.SHAPES]


@pytest.fixture(scope="module")
def staged(oracle_mod):
    """per input case: (case, want[call][stream] = (pcm, stage taps)), computed once"""
    out = []
    for c in C.INPUT_CASES:
        raw = C.batch(c["fmt"], C.B, c["calls"], c["n"], c["fs"])
        out.append((c, C.oracle_pcm(oracle_mod, raw, c["fmt"], c["n"], c["fs"], C.modes_of(c["sched"], c["calls"]),
                                    c["upper"], stages=True)))
    return out


def test_query_agrees_with_the_oracle_and_rejects_bad_arguments(oracle_mod):
    O = oracle_mod
    for fs in list(C.RATES) + [2_000_000, 2_400_000, 2_500_000, 47_999, 1]:
        for n in (1, 64, 100, 254, 255, 256, 1500, 4096, 16384):
            for taps in (0, 3, 91, 127, 255):
                L = sdrg.ssb_layout(fs, n, taps)
                assert L["decimation"] == O.ssb_decim(fs)
                assert L["pcm_len"] == O.ssb_pcm_len(n, fs, taps), (fs, n, taps)
                assert L["taps"] == min(taps or 255, n | 1)
                assert L["chunk"] == C.CHUNK and L["chunk_outputs"] == -(-C.CHUNK // L["decimation"])
                assert L["slots"] in ((4, 8, 16, 32) if L["pipeline"] else (0,))
                if taps == 0:
                    assert L["pcm_len"] == sdrg.ssb_pcm_len(n, fs)
    # the shapes every earlier GPU test of the 255-tap chain ran: always 8 slots
    for fs in (2_000_000, 2_400_000, 2_500_000):
        assert sdrg.ssb_layout(fs, 16384)["slots"] == 8 and sdrg.ssb_layout(fs, 16384)["pipeline"]
    for bad in ((0, 1024, 0), (2_000_000, 0, 0), (2_000_000, 1024, 2), (2_000_000, 1024, 257), (2**32, 1024, 0),
                (2_000_000, 1024, 1), (-5, 1024, 0)):
        with pytest.raises(sdrg.SdrgError):
            sdrg.ssb_layout(*bad)
    assert sdrg.load().sdrg_ssb_layout(2_000_000, 1024, 0, ctypes.POINTER(sdrg.SsbLayout)()) != 0


def test_rate_table_is_the_launchers(layouts):
    """every row of RATES, by the query (the authority)"""
    for s, L in layouts:
        d, lay255, lay127 = C.RATES[s["fs"]]
        want = lay127 if s["taps"] else lay255
        assert L["decimation"] == d, s
        assert (L["slots"] if L["pipeline"] else "lane") == want, (s, L)
        assert L["taps"] == (s["taps"] or 255) and L["pcm_len"] >= 5, (s, L)
        assert 1024 <= s["n"] <= 4096


def test_table_reaches_every_layout(layouts):
    plain = [(s, L) for s, L in layouts if not s["nco"]]
    assert {L["pipeline"] for _, L in plain} == {True, False}
    for taps in (0, 127):
        assert {L["slots"] for s, L in plain if s["taps"] == taps} == {0, 4, 8, 16, 32}, taps
    # the plain reference chain through the lane-per-stream kernels, and the 255-tap chain in the 4-slot layout
    assert any(not L["pipeline"] and s["taps"] == 0 for s, L in plain)
    assert any(L["slots"] == 4 and s["taps"] == 0 for s, L in plain)
    # all slots live: (chunk + taps - 2) / D + 1 equals the slot count
    live = {L["slots"] for s, L in plain if L["pipeline"] and (C.CHUNK + L["taps"] - 2) // L["decimation"] + 1 == L["slots"]}
    assert live >= {4, 16, 32}
    assert any(L["pipeline"] and L["chunk_outputs"] == L["max_chunk_outputs"] for _, L in plain)
    assert any(L["pipeline"] and L["decimation"] > C.CHUNK for _, L in plain)
    assert any(L["pipeline"] and L["decimation"] > C.CHUNK + L["taps"] for _, L in plain)
    # the mixer on both kernel families
    assert {L["pipeline"] for s, L in layouts if s["nco"]} == {True, False}


def test_each_rate_has_whole_and_partial_frames_and_each_format_meets_each_layout(layouts):
    for fs in C.RATES:
        for taps in (0, 127):
            ns = [s["n"] for s, _ in layouts if s["fs"] == fs and s["taps"] == taps and not s["nco"]]
            assert any(n % C.CHUNK == 0 for n in ns) and any(n % C.CHUNK for n in ns), (fs, taps)
    for slots in (0, 4, 8, 16, 32):
        assert {s["fmt"] for s, L in layouts if L["slots"] == slots} == set(C.FORMATS), slots


def test_each_format_takes_both_loaders(layouts):
    """launch_ssb's dma: 64 samples fit a 256-byte batch, the frame is whole batches and whole 16-byte pieces (the
    engine's buffers are 16-byte aligned).  CF32 (512 bytes per chunk) never takes the LDS-DMA loader."""
    def dma(fmt, n):
        bps = {"CS8": 2, "CU8": 2, "CS16": 4, "CF32": 8}[fmt]
        return 64 * bps <= 256 and n % (max(256 // (64 * bps), 1) * 64) == 0 and (n * bps) % 16 == 0

    for fmt in ("CS8", "CU8", "CS16"):
        took = {dma(fmt, s["n"]) for s, L in layouts if s["fmt"] == fmt and L["pipeline"]}
        assert took == {True, False}, fmt
    assert {dma("CF32", s["n"]) for s, _ in layouts if s["fmt"] == "CF32"} == {False}


def test_boundaries_give_zero_one_one_two_outputs():
    got = {}
    for c in C.BOUNDARIES:
        L = sdrg.ssb_layout(c["fs"], c["n"], 0)
        got.setdefault(c["fs"], []).append(L["pcm_len"])
        assert L["pipeline"]
    assert got == {fs: [0, 1, 1, 2] for fs in C.BOUNDARY_RATES}
    assert {sdrg.ssb_layout(fs, 2048)["slots"] for fs in C.BOUNDARY_RATES} == {4, 16, 32}
    for c, slots in zip(C.SWITCH_BACK, (16, 32)):
        assert sdrg.ssb_layout(c["fs"], c["n"], 0)["slots"] == slots
        assert sdrg.ssb_layout(c["fs"], c["n"], 127)["pcm_len"] != sdrg.ssb_layout(c["fs"], c["n"], 0)["pcm_len"]
    assert [sdrg.ssb_layout(c["fs"], c["n"], 0)["slots"] for c in C.PIPELINED] == [16, 32]


def test_input_shapes_cover_each_slot_count_and_the_lane_path():
    got = [sdrg.ssb_layout(s["fs"], s["n"])["slots"] for s in C.INPUT_SHAPES]
    assert sorted(got) == [0, 4, 8, 16, 32]
    # every family under every mode schedule and both sidebands, at every input shape
    for s in C.INPUT_SHAPES:
        mine = [c for c in C.INPUT_CASES if (c["fs"], c["n"]) == (s["fs"], s["n"])]
        assert {c["sched"] for c in mine if c["upper"]} == set(C.MODE_SCHEDULES)
        assert any(not c["upper"] for c in mine)
        assert any(c["fmt"] == "CF32" for c in mine)  # family 6
    assert {c["sched"] for c in C.INPUT_CASES if c["fmt"] == "CF32" and c["upper"]} == set(C.MODE_SCHEDULES)
    assert len(set(C.modes_of("switch", 3))) == 3


def test_families_are_distinct_per_stream_and_hit_the_codes():
    for fmt in C.FORMATS:
        raw = C.batch(fmt, C.B, 3, 1500, 1_024_000)
        assert raw.dtype == C._DTYPE[fmt] and raw.shape == (C.B, 3, 3000)
        for f in (0, 2):  # call 1 is family 3's silence
            assert len({raw[b, f].tobytes() for b in range(C.B)}) == C.B
        u = raw[0]  # family 1
        for f in range(3):
            assert (u[f] == C._LO[fmt]).any() and (u[f] == C._HI[fmt]).any() and (u[f] == 0).any()
        assert u[0].tobytes() != u[1].tobytes()
        sq = raw[1]  # family 2: full scale on I, zero on Q
        assert set(np.unique(sq[:, 0::2])) == {C._LO[fmt], C._HI[fmt]} and (sq[:, 1::2] == C._ZERO[fmt]).all()
        assert (raw[2, 1] == C._ZERO[fmt]).all() and not (raw[2, 0] == C._ZERO[fmt]).all()
        st = raw[4, 0]  # family 5
        assert (st[:1500] == st[0]).all() and (st[1500:] == st[-1]).all() and {st[0], st[-1]} == {C._LO[fmt], C._HI[fmt]}
    # family 4 over a batch and three calls: every position
    n = 1500
    hit = set()
    for b in range(3, C.B, 5):
        for f in range(3):
            i = C.fam_impulse("CS16", b, f, n, 1_024_000, 0x55B)[0::2]
            (p,) = np.nonzero(i)
            assert p.size == 1 and i[p[0]] in (32767, -32768)
            hit.add(int(p[0]))
    assert hit == {0, 63, 64, n - 1, 1472} == set(C.impulse_positions(n))
    r = np.stack([C.fam_range("CF32", 5, f, 4096, 2_000_000, 1) for f in range(3)])
    assert np.isfinite(r).all() and np.abs(r[0]).max() > 2.0**90 and 0 < np.abs(r[1][r[1] != 0]).min() < 2.0**-140
    assert (r == 0).any() and np.signbit(r[r == 0]).any() and not np.signbit(r[r == 0]).all()


def test_every_stage_tap_is_finite_for_every_family(staged):
    for c, want in staged:
        for f, per_stream in enumerate(want):
            for b, (pcm, taps) in per_stream.items():
                for k, a in taps.items():
                    assert np.isfinite(a).all(), (C.case_id(c), "family", C.family_of(c["fmt"], b) + 1, "call", f, k)


def test_agc_clamp_engages_on_both_sides(staged):
    hi = sum(int((t["agc"] == 1.0).sum()) for _, want in staged for w in want for _, t in w.values())
    lo = sum(int((t["agc"] == -1.0).sum()) for _, want in staged for w in want for _, t in w.values())
    assert hi > 0 and lo > 0
    # family 6 alone, and at every input shape
    for c, want in staged:
        if c["fmt"] == "CF32" and c["upper"]:
            agc = np.concatenate([t["agc"] for w in want for b, (_, t) in w.items() if C.family_of("CF32", b) == 5])
            assert (agc == 1.0).any() and (agc == -1.0).any(), C.case_id(c)


def test_pcm_clamp_engages_on_both_sides_in_modes_0_and_2(staged):
    for c, want in staged:
        if not c["upper"] or c["sched"] not in ("mode0", "mode2"):
            continue
        pcm = np.concatenate([p for w in want for p, _ in w.values()])
        assert (pcm == 32767).any() and (pcm == -32767).any(), C.case_id(c)
        assert pcm.min() >= -32767  # floatToPCM's clamp is symmetric


def test_silence_gives_an_all_zero_pcm_call_after_a_loud_one(staged):
    """family 3, formats with an exact zero code: the tone's call is loud, the last silent call's PCM is all zero,
    the tone is back afterwards; and the count in the table is the smallest that holds at every case"""
    needed = {}
    for c, want in staged:
        if not c["upper"] or c["fmt"] == "CU8" or c["calls"] < 4:
            continue
        z = C.SILENCE_CALLS[c["fs"], c["n"]]
        for b in range(2, C.B, len(C.families_for(c["fmt"]))):
            loud = [bool(want[f][b][0].any()) for f in range(c["calls"])]
            assert loud[0] and not loud[z] and loud[z + 1], (C.case_id(c), b, loud)
            assert np.abs(want[z][b][1]["lpf"]).max() > 0  # the low-pass is not at rest: a subnormal tail
            first = next(f for f in range(1, z + 1) if not loud[f])
            needed[c["fs"], c["n"]] = max(needed.get((c["fs"], c["n"]), 0), first)
    assert needed == C.SILENCE_CALLS


def test_lower_sideband_is_all_zero_pcm_over_a_live_low_pass(staged):
    seen = 0
    for c, want in staged:
        if c["upper"]:
            continue
        for w in want:
            for pcm, taps in w.values():
                assert not pcm.any() and not taps["agc"].any()
                seen += bool(taps["lpf"].any())
    assert seen > 0


# ---------------------------------------------------------------------------------------------------------
# the oracle (and the engine's host design code) against the reference build at the new rates
# ---------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("case", C.GOLDEN_SSB_CASES)
def test_oracle_ssb_matches_reference_fixtures_at_the_new_rates(oracle_mod, case):
    """D = 5, 10, 21 and 208, mixed sound modes, a lower-sideband stream, magnitudes up to 2^100: the oracle's
    restatement is the reference's own ssb_demod_opt.cpp there too, bit for bit"""
    O = oracle_mod
    g = load_golden(case)
    n, fs, fmt = int(g["n"]), int(g["fs"]), int(g["fmt"])
    assert g["raw"].shape[:2] == (2, 3) and n <= 2048 and sorted(g["upper"]) == [0, 1]
    assert sdrg.ssb_layout(fs, n)["slots"] != 8  # not the layout the older fixtures pin
    for s in range(2):
        st = O.SsbState()
        for f in range(3):
            pcm = st.process(O.unpack(fmt, g["raw"][s, f], n), fs, int(g["modes"][s, f]), bool(g["upper"][s]))
            np.testing.assert_array_equal(pcm, g["pcm"][s, f], err_msg=f"{case} stream {s} frame {f}")
        assert g["pcm"][s].any() == bool(g["upper"][s])  # the reference's lower sideband is silence


def test_filter_design_matches_reference_at_the_new_rates(oracle_mod):
    O = oracle_mod
    d = load_golden(C.GOLDEN_SSB_DESIGN)
    for fs in (250_000, 480_000, 1_024_000, 10_000_000):
        for mode, fc, q in ((1, 3200.0, 0.9), (2, 2200.0, 1.2), (0, 2200.0, 1.2)):
            want = d[f"lpf_{fs}_{int(fc)}"]
            np.testing.assert_array_equal(_bits(O.lpf_coefs(float(fs), fc, q)), _bits(want))
            np.testing.assert_array_equal(_bits(sdrg.ssb_design(2048, fs, mode)["lpf"]), _bits(want))
    keys = [k for k in d if k.startswith("taps_")]
    assert len(keys) == 4
    for key in keys:
        size, dec = (int(x) for x in key.split("_")[1:])
        fs = {5: 250_000, 10: 480_000, 21: 1_024_000, 208: 10_000_000}[dec]
        want = d[key]
        nz = want != 0  # read back from the reference as impulse responses, which maps -0 to +0
        for got in (O.fir_taps(size, dec), sdrg.ssb_design(size, fs, 1)["taps"]):
            np.testing.assert_array_equal(got == 0, ~nz, err_msg=key)
            np.testing.assert_array_equal(_bits(got[nz]), _bits(want[nz]), err_msg=key)
