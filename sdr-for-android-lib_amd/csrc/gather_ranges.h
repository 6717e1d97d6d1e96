// gather_ranges.h — the byte ranges that gathers still read (engine.cpp: Gathers, sdrg_engine_gather and enqueue).
// A gather reads its caller's buffers on a stream of its own choosing and ends in an event, kept in a ring of slots; a
// later call that writes into such a buffer waits for that event first.  What is tracked are ranges, not base pointers:
// an output written at an offset into, or as a slice of, a gathered allocation still waits.  Gathers run in call order,
// so the latest gather over a byte covers the earlier ones, and a slot re-recorded by a later gather still covers the
// gather that had it before.  Host only: no HIP (tests/cpp/gather_ranges_test.cpp).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace sdrg {

struct GatherRanges {
    struct Entry {
        uintptr_t lo, hi;  // the byte range [lo, hi) a gather reads
        int slot;          // that gather's slot in the ring of end events
        int64_t seq;       // that gather's number among all gathers
    };
    std::vector<Entry> entries;  // ranges read by gathers that no later call has yet written whole

    // the slot of the latest gather (the larger seq) that reads any byte of [p, p + bytes), or -1; an empty or null
    // range never matches
    int latest(const void *p, size_t bytes) const {
        if (!p || !bytes) return -1;
        const uintptr_t lo = reinterpret_cast<uintptr_t>(p), hi = lo + bytes;
        const Entry *best = nullptr;
        for (const Entry &g : entries)
            if (g.lo < hi && lo < g.hi && (!best || g.seq > best->seq)) best = &g;
        return best ? best->slot : -1;
    }

    // gather `seq`, whose end is slot's event, reads [p, p + bytes): the same range gathered again updates its entry
    void record(const void *p, size_t bytes, int slot, int64_t seq) {
        if (!p || !bytes) return;
        const uintptr_t lo = reinterpret_cast<uintptr_t>(p), hi = lo + bytes;
        for (Entry &g : entries)
            if (g.lo == lo && g.hi == hi) {
                g.slot = slot, g.seq = seq;
                return;
            }
        entries.push_back({lo, hi, slot, seq});
    }

    // A call wrote [p, p + bytes) after waiting for latest(p, bytes), on a stream ordered after the gathers: a range
    // that lies wholly inside is no longer pending.  One written only in part stays, until a call writes it whole.
    void retire(const void *p, size_t bytes) {
        if (!p) return;
        const uintptr_t lo = reinterpret_cast<uintptr_t>(p), hi = lo + bytes;
        entries.erase(std::remove_if(entries.begin(), entries.end(),
                                     [lo, hi](const Entry &g) { return lo <= g.lo && g.hi <= hi; }),
                      entries.end());
    }
};

}  // namespace sdrg
