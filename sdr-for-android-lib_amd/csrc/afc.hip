// afc.hip — the AFC stage (sdrg_engine_afc_*): the carrier offset of a CF32 channel estimated block by block from the
// lag-1 product sum and removed by a phase-continuous NCO per stream (include/sdrg.h).  A sibling of
// iqcorr.hip, not a third law of block_stage.h: a block's statistic is three sums instead of one power, two of them over
// products of neighbouring samples, so the state keeps the block in progress as samples (a sample's product needs the
// one before it), and a sample is not scaled by its block's entry but turned by a phase that runs on from block to
// block.  What it takes from block_stage.h is the positions (u = off + i, off = g mod S), the xor butterfly
// (block_reduce) and the shape of the three launches:
//   moments grid (tiles of block_tile(S) positions, streams), 256 lanes.  A lane takes the positions 2 t and 2 t + 1: one
//           16-byte load of two samples (two 8-byte loads when off is odd or the rows are not 16-byte aligned), or the
//           state's samples below off.  The sample before the lane's second is its first; the one before its first is
//           the neighbouring lane's second, moved by DPP within a wave and loaded again (8 bytes, a cache hit) at a
//           wave's first lane; a block's first position takes none: its products are +0.  Per sample pr, pi and q; the
//           lane adds its own two, the butterfly joins the lanes of a block, LDS the waves of a block (S >= 256), so
//           each value is the adjacent-pair tree of include/sdrg.h.  Writes three floats per completed block, each
//           times 1 / S, to mom[block][3][stream], and the samples of the block the call leaves in progress to the new
//           state.
//   step    one lane per stream, serial in the block index: the smoothed sums, the coherence, the lock and the
//           increment, four blocks' moments loaded ahead of the chain.  Writes blk[j][2][stream] = (Phi, inc) for the
//           call's blocks j = 0 .. n_blocks (the last is the block the call leaves in progress): the phase at the
//           block's first sample and the increment it is mixed by; the eight words of the new state if n > 0, and the
//           record if a pointer was given.
//   pass    (TRACK only) grid (runs of AFC_PASS_TILES tiles of block_tile(S) samples of the call, streams): the NCO's
//           two tables staged in 16 KiB of LDS once per workgroup (every stream has its own phase, so the phasors cannot
//           be shared as the DDC shares them; staging them per tile of 512 samples moved four times the samples' bytes
//           and measured 12 % slower at 16384 samples a row, lookups from global memory slower still: DESIGN.md
//           §3.22), then two samples per lane: ph = Phi + inc * i of the first from its block's entry of blk, the
//           second's is ph + inc whichever block it lies in (the phase runs on over a seam: Phi_(k+1) = Phi_k + inc S),
//           each sample turned by hi[ph >> 22] * lo[(ph >> 12) & 1023], and the zero tail up to in_stride; 16-byte
//           stores where the rows allow.
// No workgroup reads what another writes in the same launch, and the pass kernel's lanes read the samples they write:
// out may be chan.  Compiled with -ffp-contract=off: every product, sum, quotient and root is rounded on its own (`/`
// and sqrtf are the compiler's correctly rounded sequences: tests/cpp/demod_math.hip).
#include "block_stage.h"

namespace sdrg {
namespace {

constexpr int AFC_MOMENTS = 3;
constexpr int AFC_AHEAD = 4;        // blocks the step kernel loads ahead of the chain
constexpr int AFC_TAB = 2048;       // float2 entries of nco_tables(): hi[1024] then lo[1024]
// The pass kernel's phasor lookups: from the tables staged in LDS, or (1) from global memory; and how many tiles a
// workgroup takes one after the other under one staging (a lab build may override either: DESIGN.md §3.22)
#ifndef AFC_LAB_GLOBAL_TABLE
#define AFC_LAB_GLOBAL_TABLE 0
#endif
#ifndef AFC_LAB_PASS_TILES
#define AFC_LAB_PASS_TILES 4
#endif
constexpr bool AFC_GLOBAL_TABLE = AFC_LAB_GLOBAL_TABLE != 0;
constexpr int AFC_PASS_TILES = AFC_LAB_PASS_TILES;

// the value of the lane before this one in the wave (wave_shr:1); the wave's first lane keeps its own
__device__ __forceinline__ float afc_lane_before(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), 0x138, 0xf, 0xf, false));
}

// sdrg_atan2f of sdrg.h, operation by operation (demod.hip's)
__device__ __forceinline__ float afc_atan2f(float y, float x) {
    const float ax = fabsf(x), ay = fabsf(y);
    const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
    const float q = mx > 0.0f ? mn / mx : 0.0f;
    const float s = q * q;
    float p = -0x1.0bce58p-8f;
    p = p * s + 0x1.68671ep-6f;
    p = p * s + -0x1.cbe51p-5f;
    p = p * s + 0x1.8bc022p-4f;
    p = p * s + -0x1.1d09a6p-3f;
    p = p * s + 0x1.988d5p-3f;
    p = p * s + -0x1.554ce6p-2f;
    p = p * s + 0x1.ffffecp-1f;
    float r = p * q;
    if (ay > ax) r = 0x1.921fb6p+0f - r;
    if (__float_as_uint(x) >> 31) r = 0x1.921fb6p+1f - r;
    return copysignf(r, y);
}

// the three values of the two samples of a lane, each pair added: level 0 of the tree.  w is the sample before z0;
// none: z0 is its block's first
__device__ __forceinline__ void afc_products(float2 w, float2 z0, float2 z1, bool none, float (&v)[AFC_MOMENTS]) {
    const float a0 = z0.x * w.x, b0 = z0.y * w.y, c0 = z0.y * w.x, d0 = z0.x * w.y;
    const float a1 = z1.x * z0.x, b1 = z1.y * z0.y, c1 = z1.y * z0.x, d1 = z1.x * z0.y;
    const float pr0 = none ? 0.0f : a0 + b0, pi0 = none ? 0.0f : c0 - d0;
    const float pr1 = a1 + b1, pi1 = c1 - d1;
    v[0] = pr0 + pr1;
    v[1] = pi0 + pi1;
    v[2] = block_power(z0) + block_power(z1);
}

template <bool VEC>
__global__ __launch_bounds__(BLOCK_THREADS) void afc_moments_kernel(const float2 *chan, AfcParams p) {
    __shared__ float wsum[AFC_MOMENTS][BLOCK_THREADS / BLOCK_WAVE];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int S = p.block, off = p.off, end = p.off + p.n;  // the call's positions are [off, end)
    const int tail = p.n_blocks << p.log2_block;            // the first position of the block left in progress
    const size_t st = (size_t)b * (size_t)(2 * S + AFC_STATE_HEAD);
    const float2 *row = chan + (size_t)b * (size_t)p.in_stride;
    // read below off only, and off is 0 in a fresh stream
    const float2 *old_z = reinterpret_cast<const float2 *>(p.state_old + st + AFC_STATE_HEAD);
    float2 *new_z = reinterpret_cast<float2 *>(p.state_new + st + AFC_STATE_HEAD);
    const int width = min(S / 2, BLOCK_WAVE);
    const int passes = p.tile / BLOCK_PASS;
    const size_t B = (size_t)p.n_streams;
    float half0 = 0.0f;  // of the lanes below AFC_MOMENTS, each its own moment's
    for (int pass = 0; pass < passes; pass++) {
        const int u = (int)blockIdx.x * p.tile + pass * BLOCK_PASS + 2 * tid;
        float2 z0 = make_float2(0.0f, 0.0f), z1 = z0;
        if (VEC && u >= off && u + 1 < end) {
            const float4 zz = *reinterpret_cast<const float4 *>(row + (u - off));
            z0 = make_float2(zz.x, zz.y);
            z1 = make_float2(zz.z, zz.w);
        } else {
            if (u < off)
                z0 = old_z[u];
            else if (u < end)
                z0 = row[u - off];
            if (u + 1 < off)
                z1 = old_z[u + 1];
            else if (u + 1 < end)
                z1 = row[u + 1 - off];
        }
        if (u >= tail && u < end) new_z[u - tail] = z0;  // u - tail < S - 1: the block is not complete
        if (u + 1 >= tail && u + 1 < end) new_z[u + 1 - tail] = z1;
        const bool none = (u & (S - 1)) == 0;  // u + 1 is odd: never a block's first
        float2 w = make_float2(afc_lane_before(z1.x), afc_lane_before(z1.y));
        if ((tid & (BLOCK_WAVE - 1)) == 0 && !none && u < end) w = u - 1 < off ? old_z[u - 1] : row[u - 1 - off];
        float v[AFC_MOMENTS];
        afc_products(w, z0, z1, none, v);
#pragma unroll
        for (int j = 0; j < AFC_MOMENTS; j++) v[j] = block_reduce<false>(v[j], width);
        const int k = u >> p.log2_block;  // the block of this lane's pair
        if (S <= 2 * BLOCK_WAVE) {
            if (none && k < p.n_blocks) {
                float *to = p.mom + (size_t)k * AFC_MOMENTS * B + b;
#pragma unroll
                for (int j = 0; j < AFC_MOMENTS; j++) to[(size_t)j * B] = v[j] * p.inv_block;
            }
        } else {
            if ((tid & (BLOCK_WAVE - 1)) == 0) {
#pragma unroll
                for (int j = 0; j < AFC_MOMENTS; j++) wsum[j][tid / BLOCK_WAVE] = v[j];
            }
            __syncthreads();
            if (tid < AFC_MOMENTS) {  // lane j joins moment j across the waves
                const float lo = wsum[tid][0] + wsum[tid][1], hi = wsum[tid][2] + wsum[tid][3];
                float *to = p.mom + ((size_t)k * AFC_MOMENTS + (size_t)tid) * B + b;
                if (S == 4 * BLOCK_WAVE) {  // two blocks of 256 per pass
                    if (k < p.n_blocks) to[0] = lo * p.inv_block;
                    if (k + 1 < p.n_blocks) to[AFC_MOMENTS * B] = hi * p.inv_block;
                } else if (S == BLOCK_PASS) {
                    if (k < p.n_blocks) to[0] = (lo + hi) * p.inv_block;
                } else if (pass == 0) {  // S = 1024: the block's first half
                    half0 = lo + hi;
                } else if (k < p.n_blocks) {
                    to[0] = (half0 + (lo + hi)) * p.inv_block;
                }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(BLOCK_WAVE) void afc_step_kernel(AfcParams p) {
    __shared__ glibc::LogfEntry tab[16];
    if (threadIdx.x < 16) tab[threadIdx.x] = glibc::logf_table()[threadIdx.x];
    __syncthreads();
    const int b = (int)blockIdx.x * BLOCK_WAVE + (int)threadIdx.x;
    if (b >= p.n_streams) return;
    const size_t st = (size_t)b * (size_t)(2 * p.block + AFC_STATE_HEAD), B = (size_t)p.n_streams;
    float A = 0.0f, Bm = 0.0f, P = 0.0f, coh = 0.0f;
    int inc = 0, flags = 0, held = 0;
    uint32_t phi = 0;  // of the first sample of the block in progress
    if (!p.fresh) {
        const float4 *s = reinterpret_cast<const float4 *>(p.state_old + st);
        const float4 m = s[0], c = s[1];
        A = m.x, Bm = m.y, P = m.z, coh = m.w;
        inc = __float_as_int(c.x), phi = __float_as_uint(c.y), flags = __float_as_int(c.z);
    }
    const float *mom = p.mom + b;
    uint32_t *blk = p.blk + b;
    blk[0] = phi, blk[B] = (uint32_t)inc;
    auto step = [&](const float (&q)[AFC_MOMENTS], int k) {
        phi += (uint32_t)inc << p.log2_block;  // the block was mixed by the increment before its own step
        if (q[2] < p.floor_thr) {
            held++;
        } else {
            if (!(flags & SDRG_AFC_SEEDED)) {
                A = q[0], Bm = q[1], P = q[2];
            } else {
                const float da = q[0] - A, db = q[1] - Bm, dp = q[2] - P;
                A = A + p.beta * da;
                Bm = Bm + p.beta * db;
                P = P + p.beta * dp;
            }
            const float aa = A * A, bb = Bm * Bm;
            coh = sqrtf(aa + bb) / P;
            flags = SDRG_AFC_SEEDED;
            if (coh >= p.lock_thr) {
                flags |= SDRG_AFC_LOCKED;
                float s = afc_atan2f(Bm, A) * p.K;
                s = fminf(fmaxf(s, -p.max_s), p.max_s);
                inc = (int)rintf(s);
            }
        }
        uint32_t *to = blk + (size_t)(k + 1) * 2 * B;
        to[0] = phi, to[B] = (uint32_t)inc;
    };
    int k = 0;
    for (; k + AFC_AHEAD <= p.n_blocks; k += AFC_AHEAD) {
        float q[AFC_AHEAD][AFC_MOMENTS];
#pragma unroll
        for (int j = 0; j < AFC_AHEAD; j++)
#pragma unroll
            for (int c = 0; c < AFC_MOMENTS; c++) q[j][c] = mom[((size_t)(k + j) * AFC_MOMENTS + c) * B];
#pragma unroll
        for (int j = 0; j < AFC_AHEAD; j++) step(q[j], k + j);
    }
    for (; k < p.n_blocks; k++) {
        float q[AFC_MOMENTS];
#pragma unroll
        for (int c = 0; c < AFC_MOMENTS; c++) q[c] = mom[((size_t)k * AFC_MOMENTS + c) * B];
        step(q, k);
    }
    if (p.n > 0) {
        float4 *s = reinterpret_cast<float4 *>(p.state_new + st);
        s[0] = make_float4(A, Bm, P, coh);
        s[1] = make_float4(__int_as_float(inc), __uint_as_float(phi), __int_as_float(flags), 0.0f);
    }
    if (p.records) {  // the caller's pointer: aligned as its members, no more
        sdrg_afc_record r;
        r.offset_hz = (float)inc * p.hz_per_inc;
        r.step = (float)inc * p.rad_per_inc;
        r.inc = inc;
        r.coherence = coh;
        r.level = P;
        r.level_db = 10.0f * glibc::log10f_fast(P + 1e-20f, tab);
        r.held_blocks = held;
        r.flags = flags;
        p.records[b] = r;
    }
}

// z * hi[ph >> 22] * lo[(ph >> 12) & 1023]: the DDC's phasor and mix, in their products and order
__device__ __forceinline__ float2 afc_mix(float2 z, uint32_t ph, const float2 *tab) {
    const float2 h = tab[ph >> 22], l = tab[1024 + ((ph >> 12) & 1023)];
    const float wr = h.x * l.x - h.y * l.y, wi = h.x * l.y + h.y * l.x;
    return make_float2(z.x * wr - z.y * wi, z.x * wi + z.y * wr);
}

// VEC: the rows of chan are 16-byte aligned; WIDE: in_stride is even and out is 16-byte aligned
template <bool VEC, bool WIDE>
__global__ __launch_bounds__(BLOCK_THREADS) void afc_pass_kernel(const float2 *chan, AfcParams p, float2 *out) {
    __shared__ __attribute__((aligned(16))) float2 lds_tab[AFC_GLOBAL_TABLE ? 1 : AFC_TAB];
    const int tid = threadIdx.x, b = blockIdx.y;
    const float2 *tab = reinterpret_cast<const float2 *>(p.nco_tab);
    if (!AFC_GLOBAL_TABLE) {
        const float4 *from = reinterpret_cast<const float4 *>(p.nco_tab);  // a hipMalloc'ed table: aligned
        float4 *to = reinterpret_cast<float4 *>(lds_tab);
#pragma unroll
        for (int j = 0; j < AFC_TAB / 2 / BLOCK_THREADS; j++) to[j * BLOCK_THREADS + tid] = from[j * BLOCK_THREADS + tid];
        __syncthreads();
        tab = lds_tab;
    }
    const float2 *row = chan + (size_t)b * (size_t)p.in_stride;
    float2 *orow = out + (size_t)b * (size_t)p.in_stride;
    const uint32_t *col = p.blk + b;
    const size_t B = (size_t)p.n_streams;
    const int passes = AFC_PASS_TILES * (p.tile / BLOCK_PASS), mask = p.block - 1;
    for (int pass = 0; pass < passes; pass++) {
        const int i = (int)blockIdx.x * AFC_PASS_TILES * p.tile + pass * BLOCK_PASS + 2 * tid;
        if (i >= p.in_stride) return;
        float2 a = make_float2(0.0f, 0.0f), c = a;
        if (i < p.n) {
            const int u = p.off + i;
            const uint32_t *at = col + (size_t)(u >> p.log2_block) * 2 * B;
            const uint32_t inc = at[B];
            const uint32_t ph = at[0] + inc * (uint32_t)(u & mask);
            if (i + 1 < p.n) {  // the next sample's phase is ph + inc in this block and as the next block's first
                float2 z0, z1;
                if (VEC) {
                    const float4 zz = *reinterpret_cast<const float4 *>(row + i);
                    z0 = make_float2(zz.x, zz.y);
                    z1 = make_float2(zz.z, zz.w);
                } else {
                    z0 = row[i];
                    z1 = row[i + 1];
                }
                a = afc_mix(z0, ph, tab);
                c = afc_mix(z1, ph + inc, tab);
            } else {
                a = afc_mix(row[i], ph, tab);
            }
        }
        if (WIDE) {  // in_stride is even: i + 1 < in_stride
            *reinterpret_cast<float4 *>(orow + i) = make_float4(a.x, a.y, c.x, c.y);
        } else {
            orow[i] = a;
            if (i + 1 < p.in_stride) orow[i + 1] = c;
        }
    }
}

}  // namespace

hipError_t launch_afc(const float *chan, int n_streams, AfcParams p, float *out, hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    const int S = p.block;
    const uintptr_t at = reinterpret_cast<uintptr_t>(chan), to = reinterpret_cast<uintptr_t>(out);
    if (!chan || (p.track != 0) != (out != nullptr) || S < BLOCK_MIN || S > BLOCK_MAX || (S & (S - 1)) != 0 || p.n < 0 ||
        p.n > BLOCK_MAX_IN || p.in_stride < p.n || p.in_stride > BLOCK_MAX_IN || p.off < 0 || p.off >= S ||
        p.n_blocks != (p.off + p.n) / S || n_streams > 65535 || !p.mom || !p.blk || !p.state_old || !p.state_new ||
        (p.fresh && p.off != 0) || (p.track && !p.nco_tab) || (at & 7) != 0 || (to & 7) != 0)
        return hipErrorInvalidValue;
    p.n_streams = n_streams;
    p.log2_block = __builtin_ctz((unsigned)S);
    p.inv_block = 1.0f / (float)S;
    p.tile = block_tile(S);
    const bool even = (p.in_stride & 1) == 0, rows16 = even && (at & 15) == 0;
    const float2 *z = reinterpret_cast<const float2 *>(chan);
    const dim3 lanes(BLOCK_THREADS);
    hipError_t er;
    if (p.n > 0) {
        const dim3 grid((unsigned)((p.off + p.n + p.tile - 1) / p.tile), (unsigned)n_streams);
        if (rows16 && (p.off & 1) == 0)
            hipLaunchKernelGGL((afc_moments_kernel<true>), grid, lanes, 0, stream, z, p);
        else
            hipLaunchKernelGGL((afc_moments_kernel<false>), grid, lanes, 0, stream, z, p);
        if ((er = hipGetLastError()) != hipSuccess) return er;
    }
    if (p.n > 0 || p.records) {
        hipLaunchKernelGGL(afc_step_kernel, dim3((unsigned)((n_streams + BLOCK_WAVE - 1) / BLOCK_WAVE)), dim3(BLOCK_WAVE),
                           0, stream, p);
        if ((er = hipGetLastError()) != hipSuccess) return er;
    }
    if (p.track && p.in_stride > 0) {
        const int span = AFC_PASS_TILES * p.tile;  // samples per workgroup
        const dim3 grid((unsigned)((p.in_stride + span - 1) / span), (unsigned)n_streams);
        float2 *o = reinterpret_cast<float2 *>(out);
        const bool wide = even && (to & 15) == 0;
        if (rows16 && wide)
            hipLaunchKernelGGL((afc_pass_kernel<true, true>), grid, lanes, 0, stream, z, p, o);
        else if (rows16)
            hipLaunchKernelGGL((afc_pass_kernel<true, false>), grid, lanes, 0, stream, z, p, o);
        else if (wide)
            hipLaunchKernelGGL((afc_pass_kernel<false, true>), grid, lanes, 0, stream, z, p, o);
        else
            hipLaunchKernelGGL((afc_pass_kernel<false, false>), grid, lanes, 0, stream, z, p, o);
        if ((er = hipGetLastError()) != hipSuccess) return er;
    }
    return hipSuccess;
}

}  // namespace sdrg
