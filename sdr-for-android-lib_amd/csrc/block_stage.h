// block_stage.h — the block-stage skeleton: what the squelch and the AGC (squelch.hip, agc.hip) are on the device apart
// from their laws.  Per stream the CF32 channel is cut into blocks of S samples at the global indices
// that are multiples of S.  A call's samples sit at the positions u = off + i, off = g mod S: position 0 is the first
// sample of the block in progress, whose off leading powers the previous calls left in the state (BlockParams,
// sdrg_internal.h).  Three launches:
//   power   grid (tiles of block_tile(S) positions, streams), 256 lanes.  A lane takes the positions 2 t and 2 t + 1: one
//           16-byte load of two complex samples (two 8-byte loads when off is odd or the rows are not 16-byte aligned),
//           or the state's powers below off.  It joins its own two powers (adds them, or at MAX takes the larger), and
//           an xor butterfly joins across the min(S / 2, 64) lanes of a block: DPP moves for the distances 1, 2, 4 and
//           8, bpermute for 16 and 32.  Float addition is commutative, so every lane of the butterfly holds the bits of
//           the adjacent-pair tree of include/sdrg.h (q'[i] = q[2 i] + q[2 i + 1] until one value is left); the maximum
//           does not depend on the order.  Above a wave (S >= 256) the waves' values meet in LDS, and at S = 1024 a
//           workgroup's two halves of 512.  Writes one float per completed block, the mean or the peak power, to
//           blk[block][stream], and the powers of the block the call leaves in progress to the new state (those below
//           off among them: a call inside a block carries them over).
//   step    one lane per stream, serial in the block index: the stage's law, eight blocks' statistics loaded ahead of
//           the chain.  blk is [block][stream], so the 64 lanes of a wave read and write 256 contiguous bytes; each
//           statistic is overwritten with what the pass kernel needs of its block.  Writes the law's four state words
//           to the new state if n > 0, and the record if a pointer was given (glibc's log10f, its table in LDS).
//   pass    grid (tiles of block_tile(S) samples of the call, streams): two samples per lane, each multiplied by what
//           the law makes of its block's entry of blk (for the call's first blocks, of the old state), one fetch for
//           both when they fall in the same block, and the zero tail up to in_stride.
// No workgroup reads what another writes in the same launch, and the pass kernel's lanes read the samples they write:
// out may be chan.
//
// A stage is a law, a struct with
//   Params                      its parameters, derived from BlockParams, with a typed `records`
//   Law(p)                      the constants and the state of a fresh stream;  unpack(float4) / pack() the state words
//   float step(P)               one block's statistic into the state; returns what blk keeps of the block
//   record(tab)                 the record, from the state after the call's last block
//   Old, old(p, state)          what a stream's lanes of the pass kernel read of its old state (not at all if p.fresh)
//   Weight, fetch(k, old, col, B)   what the samples of the call's block k are multiplied by, from blk's column
//   apply(z, i, w, p)           the sample at in-block index i under w
// and launch_block_stage<Law, MAX> is its launcher.  The kernels have internal linkage: each of the two translation
// units has its own.  Device only; compile with -ffp-contract=off.
#pragma once

#include <hip/hip_runtime.h>

#include "glibc_logf.h"
#include "sdrg_internal.h"

namespace sdrg {
namespace {

constexpr int BLOCK_THREADS = BLOCK_PASS / 2;  // a lane takes two positions
constexpr int BLOCK_WAVE = 64;
constexpr int BLOCK_AHEAD = 8;  // blocks the step kernel loads ahead of the chain

// the value of the lane at distance 1, 2 (quad permutes), 4 (mirror of 8) or 8 (mirror of 16): the mirrors serve as
// xor once the lanes of every group of 4, or of 8, hold the same value
template <int CTRL>
__device__ __forceinline__ float block_dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}

template <bool MAX>
__device__ __forceinline__ float block_join(float a, float b) {
    return MAX ? fmaxf(a, b) : a + b;
}

// the sum (the maximum) over the `width` lanes (a power of two in [8, 64]) around this one, as the adjacent-pair tree
template <bool MAX>
__device__ __forceinline__ float block_reduce(float v, int width) {
    v = block_join<MAX>(v, block_dpp<0xB1>(v));   // quad_perm [1, 0, 3, 2]
    v = block_join<MAX>(v, block_dpp<0x4E>(v));   // quad_perm [2, 3, 0, 1]
    v = block_join<MAX>(v, block_dpp<0x141>(v));  // row_half_mirror
    if (width >= 16) v = block_join<MAX>(v, block_dpp<0x140>(v));  // row_mirror
    if (width >= 32) v = block_join<MAX>(v, __shfl_xor(v, 16));
    if (width >= 64) v = block_join<MAX>(v, __shfl_xor(v, 32));
    return v;
}

__device__ __forceinline__ float block_power(float2 z) {
    const float a = z.x * z.x, b = z.y * z.y;
    return a + b;
}

template <bool MAX, bool VEC>
__global__ __launch_bounds__(BLOCK_THREADS) void block_power_kernel(const float2 *chan, BlockParams p) {
    __shared__ float wsum[BLOCK_THREADS / BLOCK_WAVE];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int S = p.block, off = p.off, end = p.off + p.n;  // the call's positions are [off, end)
    const int tail = p.n_blocks << p.log2_block;            // the first position of the block left in progress
    const size_t st = (size_t)b * (size_t)(S + BLOCK_STATE_HEAD);
    const float2 *row = chan + (size_t)b * (size_t)p.in_stride;
    const float *old_pw = p.state_old + st + BLOCK_STATE_HEAD;  // read below off only, and off is 0 in a fresh stream
    float *new_pw = p.state_new + st + BLOCK_STATE_HEAD;
    const int width = min(S / 2, BLOCK_WAVE);
    const int passes = p.tile / BLOCK_PASS;
    const float scale = MAX ? 1.0f : p.inv_block;  // x * 1.0f is x
    float half0 = 0.0f;
    for (int pass = 0; pass < passes; pass++) {
        const int u = (int)blockIdx.x * p.tile + pass * BLOCK_PASS + 2 * tid;
        float q0 = 0.0f, q1 = 0.0f;
        if (VEC && u >= off && u + 1 < end) {
            const float4 zz = *reinterpret_cast<const float4 *>(row + (u - off));
            q0 = block_power(make_float2(zz.x, zz.y));
            q1 = block_power(make_float2(zz.z, zz.w));
        } else {
            if (u < off)
                q0 = old_pw[u];
            else if (u < end)
                q0 = block_power(row[u - off]);
            if (u + 1 < off)
                q1 = old_pw[u + 1];
            else if (u + 1 < end)
                q1 = block_power(row[u + 1 - off]);
        }
        if (u >= tail && u < end) new_pw[u - tail] = q0;  // u - tail < S - 1: the block is not complete
        if (u + 1 >= tail && u + 1 < end) new_pw[u + 1 - tail] = q1;
        const float v = block_reduce<MAX>(block_join<MAX>(q0, q1), width);
        const int k = u >> p.log2_block;  // the block of this lane's pair
        if (S <= 2 * BLOCK_WAVE) {
            if ((u & (S - 1)) == 0 && k < p.n_blocks) p.blk[(size_t)k * (size_t)p.n_streams + b] = v * scale;
        } else {
            if ((tid & (BLOCK_WAVE - 1)) == 0) wsum[tid / BLOCK_WAVE] = v;
            __syncthreads();
            if (tid == 0) {
                const float lo = block_join<MAX>(wsum[0], wsum[1]), hi = block_join<MAX>(wsum[2], wsum[3]);
                float *to = p.blk + (size_t)k * (size_t)p.n_streams + b;
                if (S == 4 * BLOCK_WAVE) {  // two blocks of 256 per pass
                    if (k < p.n_blocks) to[0] = lo * scale;
                    if (k + 1 < p.n_blocks) to[p.n_streams] = hi * scale;
                } else if (S == BLOCK_PASS) {
                    if (k < p.n_blocks) to[0] = block_join<MAX>(lo, hi) * scale;
                } else if (pass == 0) {  // S = 1024: the block's first half
                    half0 = block_join<MAX>(lo, hi);
                } else if (k < p.n_blocks) {
                    to[0] = block_join<MAX>(half0, block_join<MAX>(lo, hi)) * scale;
                }
            }
            __syncthreads();
        }
    }
}

template <class Law>
__global__ __launch_bounds__(BLOCK_WAVE) void block_step_kernel(typename Law::Params p) {
    __shared__ glibc::LogfEntry tab[16];
    if (threadIdx.x < 16) tab[threadIdx.x] = glibc::logf_table()[threadIdx.x];
    __syncthreads();
    const int b = (int)blockIdx.x * BLOCK_WAVE + (int)threadIdx.x;
    if (b >= p.n_streams) return;
    const size_t st = (size_t)b * (size_t)(p.block + BLOCK_STATE_HEAD), B = (size_t)p.n_streams;
    Law law(p);
    if (!p.fresh) law.unpack(*reinterpret_cast<const float4 *>(p.state_old + st));
    float *col = p.blk + b;
    int k = 0;
    for (; k + BLOCK_AHEAD <= p.n_blocks; k += BLOCK_AHEAD) {
        float P[BLOCK_AHEAD];
#pragma unroll
        for (int j = 0; j < BLOCK_AHEAD; j++) P[j] = col[(size_t)(k + j) * B];
#pragma unroll
        for (int j = 0; j < BLOCK_AHEAD; j++) col[(size_t)(k + j) * B] = law.step(P[j]);
    }
    for (; k < p.n_blocks; k++) col[(size_t)k * B] = law.step(col[(size_t)k * B]);
    if (p.n > 0) *reinterpret_cast<float4 *>(p.state_new + st) = law.pack();
    if (p.records) p.records[b] = law.record(tab);  // the caller's pointer: aligned as its int32 members, no more
}

template <class Law, bool VEC>
__global__ __launch_bounds__(BLOCK_THREADS) void block_pass_kernel(const float2 *chan, typename Law::Params p,
                                                                   float2 *out) {
    const int tid = threadIdx.x, b = blockIdx.y;
    const float2 *row = chan + (size_t)b * (size_t)p.in_stride;
    float2 *orow = out + (size_t)b * (size_t)p.in_stride;
    const float *col = p.blk + b;
    const size_t B = (size_t)p.n_streams;
    const typename Law::Old old = Law::old(p, p.state_old + (size_t)b * (size_t)(p.block + BLOCK_STATE_HEAD));
    const int passes = p.tile / BLOCK_PASS, mask = p.block - 1;
    for (int pass = 0; pass < passes; pass++) {
        const int i = (int)blockIdx.x * p.tile + pass * BLOCK_PASS + 2 * tid;
        if (i >= p.in_stride) return;
        const int u = p.off + i, k0 = u >> p.log2_block, k1 = (u + 1) >> p.log2_block;
        typename Law::Weight g{}, h{};
        if (i < p.n) g = Law::fetch(k0, old, col, B);
        if (i + 1 < p.n) h = k1 == k0 ? g : Law::fetch(k1, old, col, B);
        float2 a = make_float2(0.0f, 0.0f), c = a;
        if (VEC) {  // in_stride is even: i + 1 < in_stride
            if (i + 1 < p.n) {
                const float4 zz = *reinterpret_cast<const float4 *>(row + i);
                a = Law::apply(make_float2(zz.x, zz.y), u & mask, g, p);
                c = Law::apply(make_float2(zz.z, zz.w), (u + 1) & mask, h, p);
            } else if (i < p.n) {
                a = Law::apply(row[i], u & mask, g, p);
            }
            *reinterpret_cast<float4 *>(orow + i) = make_float4(a.x, a.y, c.x, c.y);
        } else {
            if (i < p.n) a = Law::apply(row[i], u & mask, g, p);
            if (i + 1 < p.n) c = Law::apply(row[i + 1], (u + 1) & mask, h, p);
            orow[i] = a;
            if (i + 1 < p.in_stride) orow[i + 1] = c;
        }
    }
}

// What launch_squelch and launch_agc are after their own clauses: the shared refusals, the launcher's fields of p, and
// the three launches, each only if it has work.  MAX: the power kernel takes the maximum (the AGC's peak detector).
template <class Law, bool MAX>
hipError_t launch_block_stage(const float *chan, int n_streams, typename Law::Params p, float *out, hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    const int S = p.block;
    if (!chan || !out || S < BLOCK_MIN || S > BLOCK_MAX || (S & (S - 1)) != 0 || p.n < 0 || p.n > BLOCK_MAX_IN ||
        p.in_stride < p.n || p.in_stride > BLOCK_MAX_IN || p.off < 0 || p.off >= S || p.n_blocks != (p.off + p.n) / S ||
        p.hang < 0 || n_streams > 65535 || !p.blk || !p.state_old || !p.state_new || (p.fresh && p.off != 0))
        return hipErrorInvalidValue;
    p.n_streams = n_streams;
    p.log2_block = __builtin_ctz((unsigned)S);
    p.inv_block = 1.0f / (float)S;
    p.tile = block_tile(S);
    const bool rows16 = (p.in_stride & 1) == 0 && (reinterpret_cast<uintptr_t>(chan) & 15) == 0;
    const float2 *z = reinterpret_cast<const float2 *>(chan);
    hipError_t er;
    if (p.n > 0) {
        const dim3 grid((unsigned)((p.off + p.n + p.tile - 1) / p.tile), (unsigned)n_streams);
        const BlockParams &bp = p;
        if (rows16 && (p.off & 1) == 0)
            hipLaunchKernelGGL((block_power_kernel<MAX, true>), grid, dim3(BLOCK_THREADS), 0, stream, z, bp);
        else
            hipLaunchKernelGGL((block_power_kernel<MAX, false>), grid, dim3(BLOCK_THREADS), 0, stream, z, bp);
        if ((er = hipGetLastError()) != hipSuccess) return er;
    }
    if (p.n > 0 || p.records) {
        hipLaunchKernelGGL(block_step_kernel<Law>, dim3((unsigned)((n_streams + BLOCK_WAVE - 1) / BLOCK_WAVE)),
                           dim3(BLOCK_WAVE), 0, stream, p);
        if ((er = hipGetLastError()) != hipSuccess) return er;
    }
    if (p.in_stride > 0) {
        const dim3 grid((unsigned)((p.in_stride + p.tile - 1) / p.tile), (unsigned)n_streams);
        float2 *o = reinterpret_cast<float2 *>(out);
        if (rows16 && (reinterpret_cast<uintptr_t>(out) & 15) == 0)
            hipLaunchKernelGGL((block_pass_kernel<Law, true>), grid, dim3(BLOCK_THREADS), 0, stream, z, p, o);
        else
            hipLaunchKernelGGL((block_pass_kernel<Law, false>), grid, dim3(BLOCK_THREADS), 0, stream, z, p, o);
        if ((er = hipGetLastError()) != hipSuccess) return er;
    }
    return hipSuccess;
}

}  // namespace
}  // namespace sdrg
