// decim_cursor.h — the host's side of a streaming stage's stream position (engine.cpp: DDC, demodulator, channelizer,
// resampler, squelch, AGC, sideband; fir_tile.h and block_stage.h have the device's side).  A stage decimates by D from
// the first sample after a restart: the outputs sit on the global sample indices that are multiples of D
// (DecimCursor); the resampler's output m sits on the input index floor(m M / L) with the filter phase (m M) mod L
// (ResampleCursor); the block stages' blocks start on the multiples of S (BlockCursor).  What a call reads of the
// stream before it comes from one half of a PingPong; the five FIR stages get PingPong::old, which is nullptr after a
// restart: no old history, zeros.  Host only: no HIP.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace sdrg {

// What every stage's position holds, whatever its rate: the arithmetic is the derived cursors'.
struct StreamCursor {
    uint64_t g = 0;     // samples every stream has consumed since the last restart
    bool fresh = true;  // the next call starts from a history of zeros
    int half = 0;       // the half of the stage's ping-pong buffer the next call reads

    int old_half() const { return half; }
    int new_half() const { return half ^ 1; }
    // after a call of n samples; one without samples wrote no history: the state stays where it is
    void advance(int n) {
        if (n == 0) return;
        g += (uint64_t)n;
        fresh = false;
        half ^= 1;
    }
    void restart() { *this = StreamCursor{}; }
};

struct DecimCursor : StreamCursor {
    // outputs before global sample x: the multiples of D in [0, x)
    static uint64_t outputs_before(uint64_t x, int D) { return (x + (uint64_t)D - 1) / (uint64_t)D; }
    // global time of the next call's first output
    uint64_t first_output(int D) const { return outputs_before(g, D); }
    // local index of the next call's first output
    int first(int D) const { return (int)(((uint64_t)D - g % (uint64_t)D) % (uint64_t)D); }
    // outputs of a call of n samples
    int n_out(int n, int D) const { return (int)(outputs_before(g + (uint64_t)n, D) - outputs_before(g, D)); }
    // the most outputs any call of n samples has: the row length of `out`
    static int cap(int n, int D) { return (n + D - 1) / D; }
};

// The resampler's position (resample.hip): the rate changes by L / M, gcd(L, M) = 1, both in [1, 512].  Output m reads
// the inputs up to q = floor(m M / L) with the phase phi = (m M) mod L, so the outputs before global sample x are the
// m with m M < x L: ceil(x L / M) of them.  With d = (M - (g L) mod M) mod M the next output m0 = ceil(g L / M) has
// m0 M = g L + d, hence q = g + d / L and phi = d mod L: everything a call needs follows from g mod M, in 64 bits and
// exactly for every g < 2^63; only m0 itself needs more (g L / M passes 2^64 at L / M = 8).
struct ResampleCursor : StreamCursor {
    // m0 M - g L of the next call's first output m0, in [0, M)
    int ahead(int L, int M) const {
        const uint64_t r = (g % (uint64_t)M) * (uint64_t)L % (uint64_t)M;
        return (int)(((uint64_t)M - r) % (uint64_t)M);
    }
    // global index of the next call's first output: ceil(g L / M)
    unsigned __int128 first_output(int L, int M) const {
        return ((unsigned __int128)g * (unsigned)L + (unsigned)M - 1) / (unsigned)M;
    }
    // local input index (q - g) and filter phase of the next call's first output
    int q0(int L, int M) const { return ahead(L, M) / L; }
    int phi0(int L, int M) const { return ahead(L, M) % L; }
    // outputs of a call of n samples: ceil((g + n) L / M) - ceil(g L / M) = ceil((n L - d) / M), 0 for n L <= d
    int n_out(int n, int L, int M) const {
        return (int)(((int64_t)n * L - ahead(L, M) + M - 1) / M);
    }
    // the most outputs any call of n samples has (d = 0): the row length of `out`
    static int cap(int n, int L, int M) { return (int)(((int64_t)n * L + M - 1) / M); }
};

// The position of a block stage (the skeleton of block_stage.h: the squelch and the AGC): the stream is cut into blocks
// of S samples (a power of two) at the global indices that are multiples of S.  A call of n samples takes the
// positions [offset, offset + n) counted from the start of the block in progress, and completes the blocks that end
// at or before g + n.
struct BlockCursor : StreamCursor {
    // samples of the block in progress that earlier calls consumed: g mod S
    int offset(int S) const { return (int)(g % (uint64_t)S); }
    // blocks a call of n samples completes: floor((g + n) / S) - floor(g / S)
    int blocks(int n, int S) const { return (int)((g + (uint64_t)n) / (uint64_t)S - g / (uint64_t)S); }
    // the most blocks any call of n samples completes (offset S - 1): the rows of the block scratch
    static int cap(int n, int S) { return (int)(((int64_t)n + S - 1) / S); }
};

// A device buffer of two halves of half_elems values each: a call reads what the previous one wrote into one half and
// writes the other (no workgroup reads what another writes in the same launch).  p and n are the allocation's (the
// engine allocates); a restart needs no fill, since a fresh cursor reads no half.
template <typename T>
struct PingPong {
    T *p = nullptr;
    size_t n = 0;
    T *half(int h, size_t half_elems) const { return p + (size_t)h * half_elems; }
    // the history the next call reads; nullptr: zeros
    template <typename Cursor>
    const T *old(const Cursor &c, size_t half_elems) const {
        return c.fresh ? nullptr : half(c.old_half(), half_elems);
    }
    template <typename Cursor>
    T *next(const Cursor &c, size_t half_elems) const {
        return half(c.new_half(), half_elems);
    }
};

}  // namespace sdrg
