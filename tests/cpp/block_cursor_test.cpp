// block_cursor_test.cpp — BlockCursor of csrc/decim_cursor.h against a direct count (tests/test_block_cursor.py builds
// and runs it).
//
// For S in {16, 64, 1024} a stream of 3 S + 5 samples is cut into four calls at the points 0 <= a <= b <= c <= 3 S + 5
// (zero-length calls and several calls inside one block included); S <= 64 takes every (a, b, c), S = 1024 the points
// within 2 of a multiple of S, the multiples of 61 and the last three.  Each call is checked against the block ends in
// (g, g + n], counted one by one beforehand, then the cursor is restarted.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "decim_cursor.h"

using sdrg::BlockCursor;

static long failures = 0, calls = 0;
static std::vector<int> ends_x;  // ends_x[x]: blocks of S that end at or before x, i.e. lie whole in [0, x)

#define CHECK(cond)                                                                                                  \
    do {                                                                                                             \
        if (!(cond) && failures++ < 10)                                                                              \
            printf("line %d: %s (S %d g %llu n %d)\n", __LINE__, #cond, S, (unsigned long long)g, n);                \
    } while (0)

static int call(BlockCursor &cur, int S, uint64_t g, int n, int moved) {
    calls++;
    const int completed = ends_x[g + (uint64_t)n] - ends_x[g];
    int into = 0;  // samples since the last block start, counted down from g
    for (uint64_t x = g; x % (uint64_t)S != 0; x--) into++;
    CHECK(cur.g == g);
    CHECK(cur.fresh == (moved == 0));
    CHECK(cur.half == (moved & 1));
    CHECK(cur.offset(S) == into);
    CHECK(cur.offset(S) >= 0 && cur.offset(S) < S);
    CHECK(cur.blocks(n, S) == completed);
    CHECK(cur.blocks(n, S) == (cur.offset(S) + n) / S);  // what the launcher is handed
    CHECK(cur.blocks(n, S) <= BlockCursor::cap(n, S));
    const int blocks = cur.blocks(n, S);
    const BlockCursor before = cur;
    cur.advance(n);
    CHECK(cur.g == g + (uint64_t)n);
    if (n == 0)
        CHECK(cur.fresh == before.fresh && cur.half == before.half);
    else
        CHECK(!cur.fresh && cur.half == (before.half ^ 1));
    return blocks;
}

static void cut(int S, int a, int b, int c, int len) {
    const int at[5] = {0, a, b, c, len};
    BlockCursor cur;
    int moved = 0, sum = 0;
    for (int i = 0; i < 4; i++) {
        const int n = at[i + 1] - at[i];
        sum += call(cur, S, (uint64_t)at[i], n, moved);
        moved += n > 0;
    }
    const uint64_t g = (uint64_t)len;
    const int n = 0;
    CHECK(sum == len / S);
    cur.restart();
    CHECK(cur.g == 0 && cur.fresh && cur.half == 0 && cur.offset(S) == 0);
}

int main() {
    const int Ss[] = {16, 64, 1024};
    for (int S : Ss) {
        const int len = 3 * S + 5;
        ends_x.assign((size_t)len + 1, 0);
        for (int x = 1; x <= len; x++) ends_x[x] = ends_x[x - 1] + (x % S == 0);
        if (S <= 64) {
            for (int a = 0; a <= len; a++)
                for (int b = a; b <= len; b++)
                    for (int c = b; c <= len; c++) cut(S, a, b, c, len);
            continue;
        }
        std::vector<int> pts;
        for (int t = 0; t <= len; t++)
            if (t % S <= 2 || t % S >= S - 2 || t % 61 == 0 || t >= len - 2) pts.push_back(t);
        for (size_t i = 0; i < pts.size(); i++)
            for (size_t j = i; j < pts.size(); j++)
                for (size_t k = j; k < pts.size(); k++) cut(S, pts[i], pts[j], pts[k], len);
    }
    {  // cap (the call that starts one sample before a block end completes the most), and a position past 2^32 samples
        const int S = 16, n = 100;
        const uint64_t g = ((uint64_t)1 << 40) + 7;
        CHECK(BlockCursor::cap(0, S) == 0 && BlockCursor::cap(1, S) == 1 && BlockCursor::cap(16, S) == 1 &&
              BlockCursor::cap(17, S) == 2 && BlockCursor::cap(1 << 20, 16) == 65536);
        BlockCursor cur;
        cur.g = g, cur.fresh = false;
        CHECK(cur.offset(S) == 7);
        CHECK(cur.blocks(n, S) == 6);  // 7 + 100 = 107 = 6 * 16 + 11
        cur.g = 15;
        CHECK(cur.blocks(1, S) == 1 && cur.blocks(17, S) == 2 && cur.blocks(0, S) == 0);
    }
    printf("block_cursor: %ld calls, %ld failures\n", calls, failures);
    return failures != 0;
}
