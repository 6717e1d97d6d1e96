// decim_cursor_test.cpp — csrc/decim_cursor.h against a direct count (tests/test_decim_cursor.py builds and runs it).
//
// For D in {1, 2, 3, 41, 64, 512} a stream of S = 3 D + 5 samples is cut into four calls at the points
// 0 <= a <= b <= c <= S (zero-length calls included; every shorter stream and every cut into fewer calls is a prefix
// of one of these, and the checks are made call by call), then restarted.  Each call is checked against the multiples of
// D in [g, g + n), counted one by one over [0, S] beforehand.  D <= 64: every (a, b, c).  D = 512 has 6.1e8 of them,
// minutes of work, so there every (a, b) is walked with c = b (all cuts into three calls) and the cuts into four take
// their points from the indices within 2 of a multiple of D, the multiples of 61 (coprime to D: the phases in between)
// and the last three.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "decim_cursor.h"

using sdrg::DecimCursor;

static long failures = 0, calls = 0;
// counted one by one for the D under test: before_x[x] multiples of D in [0, x), next_x[x] the first multiple at or after x
static std::vector<int> before_x, next_x;

static void count_directly(int D, int S) {
    before_x.assign((size_t)S + 1, 0);
    next_x.assign((size_t)S + 1, 0);
    for (int x = 1; x <= S; x++) before_x[x] = before_x[x - 1] + ((x - 1) % D == 0);
    int nx = S;
    while (nx % D != 0) nx++;
    for (int x = S; x >= 0; x--) next_x[x] = nx = (x % D == 0 ? x : nx);
}

#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond) && failures++ < 10) printf("line %d: %s (D %d g %llu n %d)\n", __LINE__, #cond, D, (unsigned long long)g, n); \
    } while (0)

// one call of n samples from `cur`, which has consumed g samples in `moved` calls with n > 0; returns its n_out
static int call(DecimCursor &cur, int D, uint64_t g, int n, int moved) {
    calls++;
    const int multiples = before_x[g + (uint64_t)n] - before_x[g];  // multiples of D in [g, g + n)
    const int first = next_x[g] - (int)g;  // local index of the first multiple of D at or after g
    CHECK(cur.g == g);
    CHECK(cur.fresh == (moved == 0));
    CHECK(cur.half == (moved & 1));
    CHECK(cur.old_half() == cur.half && cur.new_half() == (cur.half ^ 1));
    CHECK(cur.first(D) == first);
    CHECK(cur.first(D) >= 0 && cur.first(D) < D);
    CHECK(cur.n_out(n, D) == multiples);
    CHECK(cur.n_out(n, D) <= DecimCursor::cap(n, D));
    CHECK(n == 0 || cur.first(D) + (int64_t)(multiples - 1) * D < n);  // the last output's newest sample is in the call
    const int n_out = cur.n_out(n, D);
    const DecimCursor before = cur;
    cur.advance(n);
    CHECK(cur.g == g + (uint64_t)n);
    if (n == 0)
        CHECK(cur.fresh == before.fresh && cur.half == before.half);
    else
        CHECK(!cur.fresh && cur.half == (before.half ^ 1));
    return n_out;
}

static void cut(int D, int a, int b, int c, int S) {
    const int at[5] = {0, a, b, c, S};
    DecimCursor cur;
    int moved = 0, sum = 0;
    for (int i = 0; i < 4; i++) {
        const int n = at[i + 1] - at[i];
        sum += call(cur, D, (uint64_t)at[i], n, moved);
        moved += n > 0;
    }
    const uint64_t g = (uint64_t)S;
    const int n = 0;
    CHECK(sum == (S + D - 1) / D);  // the multiples of D in [0, S)
    cur.restart();
    CHECK(cur.g == 0 && cur.fresh && cur.half == 0 && cur.first(D) == 0);
}

int main() {
    const int Ds[] = {1, 2, 3, 41, 64, 512};
    for (int D : Ds) {
        const int S = 3 * D + 5;
        count_directly(D, S);
        if (D <= 64) {
            for (int a = 0; a <= S; a++)
                for (int b = a; b <= S; b++)
                    for (int c = b; c <= S; c++) cut(D, a, b, c, S);
            continue;
        }
        for (int a = 0; a <= S; a++)
            for (int b = a; b <= S; b++) cut(D, a, b, b, S);
        std::vector<int> pts;
        for (int t = 0; t <= S; t++)
            if (t % D <= 2 || t % D >= D - 2 || t % 61 == 0 || t >= S - 2) pts.push_back(t);
        for (size_t i = 0; i < pts.size(); i++)
            for (size_t j = i; j < pts.size(); j++)
                for (size_t k = j; k < pts.size(); k++) cut(D, pts[i], pts[j], pts[k], S);
    }
    {  // cap, and a position past 2^32 samples
        const int D = 41, n = 100;
        const uint64_t g = ((uint64_t)1 << 40) + 7;
        CHECK(DecimCursor::cap(0, D) == 0 && DecimCursor::cap(1, D) == 1 && DecimCursor::cap(41, D) == 1 && DecimCursor::cap(42, D) == 2);
        DecimCursor cur;
        cur.g = g, cur.fresh = false;
        CHECK(cur.first(D) == (int)((41 - g % 41) % 41));
        CHECK(cur.n_out(n, D) == (int)((g + 100 + 40) / 41 - (g + 40) / 41));
        CHECK(cur.first_output(D) == (g + 40) / 41);
    }
    printf("decim_cursor: %ld calls, %ld failures\n", calls, failures);
    return failures != 0;
}
