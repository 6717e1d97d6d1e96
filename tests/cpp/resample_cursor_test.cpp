// resample_cursor_test.cpp — csrc/decim_cursor.h's ResampleCursor against a direct count
// (tests/test_resample_cursor.py builds and runs it).
//
// For (L, M) in {(1,1), (3,2), (2,3), (123,125), (512,511), (8,1), (1,8)} a stream of S samples is cut into three calls
// at the points 0 <= a <= b <= S (zero-length calls included; every cut into fewer calls is a prefix of one of these,
// and the checks are made call by call), then restarted.  Each call is checked against the outputs m with
// g <= floor(m M / L) < g + n, counted one by one: m runs up from 0 and every q = floor(m M / L) is computed by that
// division.  S = 3 max(L, M) + 5 where that is at most 100, so every phase of the ratio starts a call; the two long
// ratios take S = 260 (every a, b), which still passes through 260 of their phases at each cut.
// The same walk is then made with the stream's start placed at g = 2^62 + small offsets (the counts there by 128-bit
// divisions m = ceil(x L / M), checked against the definition of q on both sides of every boundary).
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "decim_cursor.h"

using sdrg::ResampleCursor;
typedef unsigned __int128 u128;

static long failures = 0, calls = 0;

#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        if (!(cond) && failures++ < 10)                                                                      \
            printf("line %d: %s (L %d M %d g %llu n %d)\n", __LINE__, #cond, L, M, (unsigned long long)g, n); \
    } while (0)

// The outputs before global sample x, by the definition alone: the first m whose q = floor(m M / L) is at least x.
// Near 0 they are counted one by one; far out the candidate ceil(x L / M) is checked on both sides.
static std::vector<uint64_t> before_x;  // counted one by one for the ratio under test, x in [0, S]

static void count_directly(int L, int M, int S) {
    before_x.assign((size_t)S + 1, 0);
    uint64_t m = 0;
    for (int x = 0; x <= S; x++) {
        while (m * (uint64_t)M / (uint64_t)L < (uint64_t)x) m++;
        before_x[(size_t)x] = m;
    }
}

static u128 outputs_before(uint64_t x, int L, int M, bool count) {
    if (count) return before_x[(size_t)x];
    const u128 m = ((u128)x * (unsigned)L + (unsigned)M - 1) / (unsigned)M;
    const bool at_or_after = m * (unsigned)M / (unsigned)L >= x;
    const bool one_less_is_before = m == 0 || (m - 1) * (unsigned)M / (unsigned)L < x;
    if (!(at_or_after && one_less_is_before)) {
        if (failures++ < 10) printf("outputs_before(%llu, %d, %d) is not the boundary\n", (unsigned long long)x, L, M);
    }
    return m;
}

// one call of n samples from `cur`, which has consumed g samples, `moved` calls with n > 0 since the restart
static int call(ResampleCursor &cur, int L, int M, uint64_t g, int n, int moved, bool count) {
    calls++;
    const u128 m0 = outputs_before(g, L, M, count), m1 = outputs_before(g + (uint64_t)n, L, M, count);
    const int want_n_out = (int)(m1 - m0);
    const u128 t0 = m0 * (unsigned)M;  // the first output at or after g, whether or not this call holds it
    const uint64_t want_q = (uint64_t)(t0 / (unsigned)L);
    const int want_phi = (int)(t0 % (unsigned)L);
    CHECK(cur.g == g);
    CHECK(cur.fresh == (moved == 0));
    CHECK(cur.half == (moved & 1));
    CHECK(cur.old_half() == cur.half && cur.new_half() == (cur.half ^ 1));
    CHECK(cur.first_output(L, M) == m0);
    CHECK(cur.n_out(n, L, M) == want_n_out);
    CHECK(cur.n_out(n, L, M) <= ResampleCursor::cap(n, L, M));
    CHECK(want_q >= g && (uint64_t)cur.q0(L, M) == want_q - g);
    CHECK(cur.phi0(L, M) == want_phi);
    CHECK(cur.phi0(L, M) >= 0 && cur.phi0(L, M) < L);
    if (want_n_out > 0) {  // the last output's newest sample is in the call: q0 + (phi0 + (n_out - 1) M) / L < n
        const int64_t q_last = (int64_t)cur.q0(L, M) + ((int64_t)cur.phi0(L, M) + (int64_t)(want_n_out - 1) * M) / L;
        CHECK(q_last < n);
        CHECK((u128)g + (u128)q_last == (m1 - 1) * (unsigned)M / (unsigned)L);
    }
    const int n_out = cur.n_out(n, L, M);
    const ResampleCursor before = cur;
    cur.advance(n);
    CHECK(cur.g == g + (uint64_t)n);
    if (n == 0)
        CHECK(cur.fresh == before.fresh && cur.half == before.half);
    else
        CHECK(!cur.fresh && cur.half == (before.half ^ 1));
    return n_out;
}

static void cut(int L, int M, uint64_t base, int a, int b, int S) {
    const int at[4] = {0, a, b, S};
    const bool count = base == 0;
    ResampleCursor cur;
    int moved = 0;
    if (base != 0) cur.g = base, cur.fresh = false, moved = 2;  // placed there directly: an even number of calls ago
    long sum = 0;
    for (int i = 0; i < 3; i++) {
        const int n = at[i + 1] - at[i];
        sum += call(cur, L, M, base + (uint64_t)at[i], n, moved, count);
        moved += n > 0;
    }
    const uint64_t g = base + (uint64_t)S;
    const int n = 0;
    CHECK((u128)sum == outputs_before(g, L, M, count) - outputs_before(base, L, M, count));
    if (base == 0) CHECK(sum == ((long)S * L + M - 1) / M);
    cur.restart();
    CHECK(cur.g == 0 && cur.fresh && cur.half == 0 && cur.q0(L, M) == 0 && cur.phi0(L, M) == 0);
}

int main() {
    const int ratios[][2] = {{1, 1}, {3, 2}, {2, 3}, {123, 125}, {512, 511}, {8, 1}, {1, 8}};
    for (const auto &r : ratios) {
        const int L = r[0], M = r[1];
        const int big = L > M ? L : M;
        const int S = 3 * big + 5 <= 100 ? 3 * big + 5 : 260;
        count_directly(L, M, S);
        for (int a = 0; a <= S; a++)
            for (int b = a; b <= S; b++) cut(L, M, 0, a, b, S);
        // g placed directly at 2^62 + small offsets: every residue of g mod M for the short ratios, a spread for the long
        const int S2 = 3 * big + 5 <= 100 ? 3 * big + 5 : 40;
        for (uint64_t off = 0; off < 130; off += (off < 10 ? 1 : 7)) {
            const uint64_t base = ((uint64_t)1 << 62) + off;
            for (int a = 0; a <= S2; a++)
                for (int b = a; b <= S2; b++) cut(L, M, base, a, b, S2);
        }
    }
    {  // cap
        const int L = 123, M = 125, n = 0;
        const uint64_t g = 0;
        CHECK(ResampleCursor::cap(0, L, M) == 0 && ResampleCursor::cap(1, L, M) == 1 && ResampleCursor::cap(125, L, M) == 123);
        CHECK(ResampleCursor::cap(126, L, M) == 124 && ResampleCursor::cap(1639, L, M) == 1613);
        CHECK(ResampleCursor::cap(1 << 20, 8, 1) == 1 << 23 && ResampleCursor::cap(1 << 20, 1, 8) == 1 << 17);
        CHECK(ResampleCursor::cap(1 << 20, 512, 511) == (int)(((int64_t)(1 << 20) * 512 + 510) / 511));
    }
    printf("resample_cursor: %ld calls, %ld failures\n", calls, failures);
    return failures != 0;
}
