// decim_cursor.h — the host's side of a decimating stage's stream position (engine.cpp: DDC, demodulator, channelizer;
// fir_tile.h has the device's side).  A stage decimates by D from the first sample after a restart: the outputs sit on
// the global sample indices that are multiples of D.  Host only: no HIP.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace sdrg {

struct DecimCursor {
    uint64_t g = 0;     // samples every stream has consumed since the last restart
    bool fresh = true;  // the next call starts from a history of zeros
    int half = 0;       // the half of the stage's ping-pong buffer the next call reads

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
    int old_half() const { return half; }
    int new_half() const { return half ^ 1; }
    // after a call of n samples; one without samples wrote no history: the state stays where it is
    void advance(int n) {
        if (n == 0) return;
        g += (uint64_t)n;
        fresh = false;
        half ^= 1;
    }
    void restart() { *this = DecimCursor{}; }
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
    const T *old(const DecimCursor &c, size_t half_elems) const {
        return c.fresh ? nullptr : half(c.old_half(), half_elems);
    }
    T *next(const DecimCursor &c, size_t half_elems) const { return half(c.new_half(), half_elems); }
};

}  // namespace sdrg
