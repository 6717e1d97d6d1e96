// block_power.h — what the squelch and the AGC (squelch.hip, agc.hip) share on the device: a sample's power and the
// reduction of a block's powers across the lanes of a wave, two positions per lane.  The sum is the adjacent-pair tree
// of include/sdrg.h (q'[i] = q[2 i] + q[2 i + 1] until one value is left); the maximum does not depend on the order.
// Device only; compile with -ffp-contract=off.
#pragma once

#include <hip/hip_runtime.h>

namespace sdrg {

constexpr int SQ_THREADS = 256;
constexpr int SQ_PASS = 2 * SQ_THREADS;  // positions a workgroup takes at a time
constexpr int SQ_WAVE = 64;
constexpr int SQ_AHEAD = 8;  // blocks the step kernels load ahead of the chain

// the value of the lane at distance 1, 2 (quad permutes), 4 (mirror of 8) or 8 (mirror of 16): the mirrors serve as
// xor once the lanes of every group of 4, or of 8, hold the same value
template <int CTRL>
__device__ __forceinline__ float sq_dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}

template <bool MAX>
__device__ __forceinline__ float sq_join(float a, float b) {
    return MAX ? fmaxf(a, b) : a + b;
}

// the sum (the maximum) over the `width` lanes (a power of two in [8, 64]) around this one, as the adjacent-pair tree
template <bool MAX>
__device__ __forceinline__ float sq_reduce(float v, int width) {
    v = sq_join<MAX>(v, sq_dpp<0xB1>(v));   // quad_perm [1, 0, 3, 2]
    v = sq_join<MAX>(v, sq_dpp<0x4E>(v));   // quad_perm [2, 3, 0, 1]
    v = sq_join<MAX>(v, sq_dpp<0x141>(v));  // row_half_mirror
    if (width >= 16) v = sq_join<MAX>(v, sq_dpp<0x140>(v));  // row_mirror
    if (width >= 32) v = sq_join<MAX>(v, __shfl_xor(v, 16));
    if (width >= 64) v = sq_join<MAX>(v, __shfl_xor(v, 32));
    return v;
}

__device__ __forceinline__ float sq_butterfly(float v, int width) { return sq_reduce<false>(v, width); }

__device__ __forceinline__ float sq_power(float2 z) {
    const float a = z.x * z.x, b = z.y * z.y;
    return a + b;
}

}  // namespace sdrg
