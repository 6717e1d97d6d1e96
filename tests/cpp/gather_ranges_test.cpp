// gather_ranges_test.cpp — GatherRanges of csrc/gather_ranges.h against a byte map (tests/test_gather_ranges.py builds
// and runs it).
//
// The model knows no intervals.  Each gather is the set of bytes it reads in a 256-byte arena; the byte map holds, per
// byte, the latest seq among the gathers still pending; a query is the largest seq under its bytes; a write retires a
// gather that has no byte outside it.  Two sweeps over every pair of ranges with ends on the 16-byte grid (136 ranges):
//   gather A, gather B       then every grid range queried
//   two gathers, a write W   the wait W needs, then the write, then every grid range queried and the entries counted
// and the cases by name below.  Slots are seq % GRING, as the engine assigns them.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "gather_ranges.h"

using sdrg::GatherRanges;

static const int ARENA = 256, GRID = 16, GRING = 8;
alignas(16) static unsigned char arena[ARENA];
static long failures = 0, checks = 0;

#define CHECK(cond)                                                              \
    do {                                                                         \
        checks++;                                                                \
        if (!(cond) && failures++ < 10) printf("line %d: %s\n", __LINE__, #cond); \
    } while (0)

struct Model {
    struct Gather {
        bool reads[ARENA];
        int slot;
        int64_t seq;
        bool pending;
    };
    std::vector<Gather> gathers;
    int64_t map[ARENA];  // the latest seq per byte, -1: none
    std::vector<int> slot_of;

    void record(int lo, int hi, int slot, int64_t seq) {
        Gather g{};
        for (int x = lo; x < hi; x++) g.reads[x] = true;
        g.slot = slot, g.seq = seq, g.pending = lo < hi;
        gathers.push_back(g);
        if ((size_t)seq >= slot_of.size()) slot_of.resize((size_t)seq + 1, -1);
        slot_of[(size_t)seq] = slot;
        paint();
    }
    void retire(int lo, int hi) {
        for (Gather &g : gathers) {
            bool outside = false;
            for (int x = 0; x < ARENA; x++) outside |= g.reads[x] && (x < lo || x >= hi);
            if (!outside) g.pending = false;
        }
        paint();
    }
    void paint() {
        std::fill(map, map + ARENA, (int64_t)-1);
        for (const Gather &g : gathers)
            for (int x = 0; x < ARENA; x++)
                if (g.pending && g.reads[x]) map[x] = std::max(map[x], g.seq);
    }
    int latest(int lo, int hi) const {
        int64_t best = -1;
        for (int x = lo; x < hi; x++) best = std::max(best, map[x]);
        return best < 0 ? -1 : slot_of[(size_t)best];
    }
    int distinct_pending() const {  // gathers of one byte set share an entry
        int k = 0;
        for (size_t i = 0; i < gathers.size(); i++) {
            bool first = gathers[i].pending;
            for (size_t j = 0; j < i && first; j++)
                first = !(gathers[j].pending && std::equal(gathers[i].reads, gathers[i].reads + ARENA, gathers[j].reads));
            k += first;
        }
        return k;
    }
};

struct Pair {
    GatherRanges r;
    Model m;
    void record(int lo, int hi, int64_t seq) {
        r.record(arena + lo, (size_t)(hi - lo), (int)(seq % GRING), seq);
        m.record(lo, hi, (int)(seq % GRING), seq);
    }
    void retire(int lo, int hi) {
        r.retire(arena + lo, (size_t)(hi - lo));
        m.retire(lo, hi);
    }
    int latest(int lo, int hi) const { return r.latest(arena + lo, (size_t)(hi - lo)); }
    void check_every_grid_range() const {
        for (int lo = 0; lo < ARENA; lo += GRID) {
            int64_t best = -1;  // the model's answer, grown a byte at a time
            for (int x = lo; x < ARENA; x++) {
                best = std::max(best, m.map[x]);
                if ((x + 1) % GRID == 0) CHECK(latest(lo, x + 1) == (best < 0 ? -1 : m.slot_of[(size_t)best]));
            }
        }
        CHECK((int)r.entries.size() == m.distinct_pending());
    }
};

static void sweeps() {
    for (int a0 = 0; a0 < ARENA; a0 += GRID)
        for (int a1 = a0 + GRID; a1 <= ARENA; a1 += GRID)
            for (int b0 = 0; b0 < ARENA; b0 += GRID)
                for (int b1 = b0 + GRID; b1 <= ARENA; b1 += GRID) {
                    {  // gather A, gather B
                        Pair p;
                        p.record(a0, a1, 6);
                        p.record(b0, b1, 7);
                        p.check_every_grid_range();
                    }
                    {  // gathers [96, 160) and A, then the write B
                        Pair p;
                        p.record(96, 160, 3);
                        p.record(a0, a1, 5);
                        CHECK(p.latest(b0, b1) == p.m.latest(b0, b1));
                        p.retire(b0, b1);
                        p.check_every_grid_range();
                    }
                }
}

static void a_write_at_an_offset_into_a_gathered_range_waits() {
    Pair p;
    p.record(32, 160, 0);
    CHECK(p.latest(100, 104) == 0 && p.latest(100, 200) == 0 && p.latest(159, 160) == 0);
}

static void a_slice_of_a_gathered_range_waits() {
    Pair p;
    p.record(32, 160, 2);
    CHECK(p.latest(32, 64) == 2 && p.latest(64, 96) == 2 && p.latest(128, 160) == 2);
}

static void a_write_adjacent_to_a_gathered_range_does_not_wait() {
    Pair p;
    p.record(32, 160, 1);
    CHECK(p.latest(0, 32) == -1);     // its hi is the entry's lo
    CHECK(p.latest(160, 256) == -1);  // its lo is the entry's hi
    CHECK(p.latest(0, 33) == 1 && p.latest(159, 256) == 1);
}

static void a_null_or_zero_length_range_never_waits() {
    GatherRanges r;
    r.record(arena, ARENA, 0, 0);
    CHECK(r.latest(nullptr, 16) == -1 && r.latest(nullptr, 0) == -1 && r.latest(arena + 8, 0) == -1);
    r.record(nullptr, 16, 1, 1);  // nor is one recorded
    r.record(arena, 0, 1, 1);
    CHECK(r.entries.size() == 1 && r.latest(arena, 1) == 0);
    r.retire(nullptr, ARENA);  // nor does one retire anything
    r.retire(arena + 8, 0);
    CHECK(r.entries.size() == 1);
}

static void two_gathers_over_one_byte_resolve_to_the_later_one() {
    Pair p;
    p.record(0, 100, 4);
    p.record(99, 200, 5);
    CHECK(p.latest(99, 100) == 5 && p.latest(0, 99) == 4 && p.latest(0, 256) == 5);
    Pair q;  // whichever was recorded first
    q.record(99, 200, 5);
    q.record(0, 100, 4);
    CHECK(q.latest(99, 100) == 5 && q.latest(0, 99) == 4);
}

static void the_same_range_gathered_again_updates_its_entry_and_adds_none() {
    Pair p;
    p.record(16, 48, 0);
    p.record(64, 80, 1);
    p.record(16, 48, 2);
    CHECK(p.r.entries.size() == 2 && p.latest(16, 48) == 2 && p.latest(64, 80) == 1);
    p.record(16, 47, 3);  // another range: another entry
    CHECK(p.r.entries.size() == 3 && p.latest(47, 48) == 2 && p.latest(16, 17) == 3);
}

static void a_partial_overwrite_leaves_the_entry_pending() {
    Pair p;
    p.record(32, 96, 1);
    p.retire(32, 95);
    p.retire(33, 96);
    p.retire(0, 64);
    p.retire(64, 256);
    CHECK(p.r.entries.size() == 1 && p.latest(32, 33) == 1 && p.latest(95, 96) == 1);
    p.check_every_grid_range();
}

static void a_whole_overwrite_retires_it() {
    Pair p;
    p.record(32, 96, 1);
    p.retire(32, 96);
    CHECK(p.r.entries.empty() && p.latest(0, 256) == -1);
    p.record(32, 96, 2);
    p.retire(16, 112);  // a wider write
    CHECK(p.r.entries.empty());
}

static void a_written_range_covering_two_entries_retires_both() {
    Pair p;
    p.record(32, 64, 1);
    p.record(64, 128, 2);
    p.record(120, 136, 3);
    p.retire(32, 128);
    CHECK(p.r.entries.size() == 1 && p.latest(32, 120) == -1 && p.latest(120, 128) == 3);
    p.check_every_grid_range();
}

static void slot_reuse_after_GRING_gathers_still_resolves_by_seq() {
    Pair p;
    for (int k = 0; k < GRING; k++) p.record(16 * k, 16 * k + 16, k);  // slots 0 .. 7
    p.record(8, 40, GRING);                                             // slot 0 again, over gathers 0, 1 and 2
    CHECK(p.r.entries.size() == (size_t)GRING + 1);
    CHECK(p.latest(16, 32) == 0);  // seq 8 in slot 0 beats seq 1 in slot 1
    CHECK(p.latest(40, 48) == 2 && p.latest(0, 8) == 0 && p.latest(112, 128) == 7);
    p.retire(0, 16);  // gather 0's range whole: gather 8, which has its slot now, stays
    CHECK(p.r.entries.size() == (size_t)GRING && p.latest(0, 8) == -1 && p.latest(8, 16) == 0);
    p.check_every_grid_range();
}

int main() {
    sweeps();
    a_write_at_an_offset_into_a_gathered_range_waits();
    a_slice_of_a_gathered_range_waits();
    a_write_adjacent_to_a_gathered_range_does_not_wait();
    a_null_or_zero_length_range_never_waits();
    two_gathers_over_one_byte_resolve_to_the_later_one();
    the_same_range_gathered_again_updates_its_entry_and_adds_none();
    a_partial_overwrite_leaves_the_entry_pending();
    a_whole_overwrite_retires_it();
    a_written_range_covering_two_entries_retires_both();
    slot_reuse_after_GRING_gathers_still_resolves_by_seq();
    printf("gather_ranges: %ld checks, %ld failures\n", checks, failures);
    return failures != 0;
}
