// symbols.hip — the symbol stage (sdrg_engine_symbols_*): the symbol clock of real float audio recovered block by block
// and the audio sliced to 2 or 4 levels per stream, one byte or one float per symbol (include/sdrg.h).
// A sibling of afc.hip on block_stage.h: a block's statistic is five sums, three of them over the squared difference
// of neighbouring values (two of those against the clock's phasor), so the state keeps the block in progress as values,
// and below it the SYM_HISTORY values before the block, which a symbol sampled near a call's or a block's start reaches
// back into.  What it takes from block_stage.h is the positions (u = off + i, off = g mod S), the xor butterfly
// (block_reduce) and the shape of the three launches:
//   moments grid (tiles of block_tile(S) positions, streams), 256 lanes, the clock's table staged in 8 KiB of LDS once
//           per workgroup (or read from global memory: SYM_LAB_GLOBAL_TABLE).  A lane takes the positions 2 t and
//           2 t + 1: one 8-byte load of two values (two 4-byte loads when off is odd or the rows are not 8-byte aligned),
//           or the state's values below off.  The value before the lane's second is its first; the one before its first
//           is the neighbouring lane's second, moved by DPP within a wave and loaded again (a cache hit) at a wave's
//           first lane; a block's first position takes none: its u, a and b are +0.  c of a position is cpos0 + inc u
//           in 32 bits.  The lane adds its own two of each sum, the butterfly joins the lanes of a block, LDS the waves
//           of a block (S >= 256), so each value is the adjacent-pair tree of include/sdrg.h.  Writes five floats per
//           completed block, each times 1 / S, to mom[block][5][stream], and to the new state the SYM_HISTORY values
//           before the block the call leaves in progress and that block's values.
//   step    one lane per stream, serial in the block index: the smoothed sums, the coherence, the lock, tau, the slips
//           and the levels, four blocks' moments loaded ahead of the chain.  Writes blk[j][4][stream] = (tau, centre,
//           thr, locked) for the call's blocks j = 0 .. n_blocks (the last is the block the call leaves in progress),
//           the words of the new state if n > 0, and the record if a pointer was given.
//   pass    grid (runs of SYM_PASS_TILE symbols of a row, streams), one lane per *symbol*: the call's value that emits
//           the symbol in place m is t = ceil(((m + 1) 2^32 - emit0) / inc), a 64-bit division; its block's entry of
//           blk, the two values around the sampling point from the row or from the old state below the call's start,
//           the decision, and one dense store of a byte or a float; the lanes from n_sym to cap write the zero tail.
// No workgroup reads what another writes in the same launch.  Compiled with -ffp-contract=off: every product, sum,
// quotient and root is rounded on its own (`/` and sqrtf are the compiler's correctly rounded sequences:
// tests/cpp/demod_math.hip).
#include "block_stage.h"

namespace sdrg {
namespace {

constexpr int SYM_MOMENTS = 5;
constexpr int SYM_AHEAD = 4;  // blocks the step kernel loads ahead of the chain
// The moments kernel's table lookups: from the table staged in LDS, or (1) from global memory (a lab build may
// override it: DESIGN.md §3.24)
#ifndef SYM_LAB_GLOBAL_TABLE
#define SYM_LAB_GLOBAL_TABLE 0
#endif
constexpr bool SYM_GLOBAL_TABLE = SYM_LAB_GLOBAL_TABLE != 0;

// the value of the lane before this one in the wave (wave_shr:1); the wave's first lane keeps its own
__device__ __forceinline__ float sym_lane_before(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), 0x138, 0xf, 0xf, false));
}

// sdrg_atan2f of sdrg.h, operation by operation (demod.hip's)
__device__ __forceinline__ float sym_atan2f(float y, float x) {
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

// the five values of the two positions of a lane, each pair added: level 0 of the tree.  w is the value before x0;
// none: x0 is its block's first.  c is the clock at x0's position.
__device__ __forceinline__ void sym_products(float w, float x0, float x1, bool none, uint32_t c, uint32_t inc,
                                             const float2 *tab, float (&v)[SYM_MOMENTS]) {
    const float2 t0 = tab[c >> 22], t1 = tab[(c + inc) >> 22];
    const float d0 = x0 - w, d1 = x1 - x0;
    const float e0 = d0 * d0, e1 = d1 * d1;
    const float a0 = e0 * t0.x, b0 = e0 * t0.y, a1 = e1 * t1.x, b1 = e1 * t1.y;
    v[0] = (none ? 0.0f : a0) + a1;
    v[1] = (none ? 0.0f : b0) + b1;
    v[2] = (none ? 0.0f : e0) + e1;
    v[3] = x0 + x1;
    v[4] = x0 * x0 + x1 * x1;
}

template <bool VEC>
__global__ __launch_bounds__(BLOCK_THREADS) void sym_moments_kernel(const float *in, SymParams p) {
    __shared__ float wsum[SYM_MOMENTS][BLOCK_THREADS / BLOCK_WAVE];
    __shared__ __attribute__((aligned(16))) float2 lds_tab[SYM_GLOBAL_TABLE ? 1 : SDRG_SYM_TABLE];
    const int tid = threadIdx.x, b = blockIdx.y;
    const float2 *tab = reinterpret_cast<const float2 *>(p.tab);
    if (!SYM_GLOBAL_TABLE) {
        const float4 *from = reinterpret_cast<const float4 *>(p.tab);  // a hipMalloc'ed table: aligned
        float4 *to = reinterpret_cast<float4 *>(lds_tab);
#pragma unroll
        for (int j = 0; j < SDRG_SYM_TABLE / 2 / BLOCK_THREADS; j++) to[j * BLOCK_THREADS + tid] = from[j * BLOCK_THREADS + tid];
        __syncthreads();
        tab = lds_tab;
    }
    const int S = p.block, off = p.off, end = p.off + p.n;  // the call's positions are [off, end)
    const int tail = p.n_blocks << p.log2_block;            // the first position of the block left in progress
    const size_t st = (size_t)b * (size_t)sym_state_words(S) + SYM_STATE_HEAD + SYM_HISTORY;
    const float *row = in + (size_t)b * (size_t)p.in_stride;
    // by position, [-SYM_HISTORY, off): read only if the stream is not fresh
    const float *old_v = p.state_old + st;
    float *new_v = p.state_new + st;  // by position - tail, [-SYM_HISTORY, S - 1)
    // the history that lies below position 0 (tail is 0, or S = 64 and tail = 64) is carried over
    if (blockIdx.x == 0 && tid < SYM_HISTORY) {
        const int h = tail - SYM_HISTORY + tid;
        if (h < 0) new_v[h - tail] = p.fresh ? 0.0f : old_v[h];
    }
    const int width = min(S / 2, BLOCK_WAVE);
    const int passes = p.tile / BLOCK_PASS;
    const size_t B = (size_t)p.n_streams;
    float half0 = 0.0f;  // of the lanes below SYM_MOMENTS, each its own moment's
    for (int pass = 0; pass < passes; pass++) {
        const int u = (int)blockIdx.x * p.tile + pass * BLOCK_PASS + 2 * tid;
        float x0 = 0.0f, x1 = 0.0f;
        if (VEC && u >= off && u + 1 < end) {
            const float2 xx = *reinterpret_cast<const float2 *>(row + (u - off));
            x0 = xx.x, x1 = xx.y;
        } else {
            if (u < off)
                x0 = old_v[u];
            else if (u < end)
                x0 = row[u - off];
            if (u + 1 < off)
                x1 = old_v[u + 1];
            else if (u + 1 < end)
                x1 = row[u + 1 - off];
        }
        if (u >= tail - SYM_HISTORY && u < end) new_v[u - tail] = x0;  // u - tail < S - 1: the block is not complete
        if (u + 1 >= tail - SYM_HISTORY && u + 1 < end) new_v[u + 1 - tail] = x1;
        const bool none = (u & (S - 1)) == 0;  // u + 1 is odd: never a block's first
        float w = sym_lane_before(x1);
        if ((tid & (BLOCK_WAVE - 1)) == 0 && !none && u < end) w = u - 1 < off ? old_v[u - 1] : row[u - 1 - off];
        float v[SYM_MOMENTS];
        sym_products(w, x0, x1, none, p.cpos0 + p.inc * (uint32_t)u, p.inc, tab, v);
#pragma unroll
        for (int j = 0; j < SYM_MOMENTS; j++) v[j] = block_reduce<false>(v[j], width);
        const int k = u >> p.log2_block;  // the block of this lane's pair
        if (S <= 2 * BLOCK_WAVE) {
            if (none && k < p.n_blocks) {
                float *to = p.mom + (size_t)k * SYM_MOMENTS * B + b;
#pragma unroll
                for (int j = 0; j < SYM_MOMENTS; j++) to[(size_t)j * B] = v[j] * p.rs;
            }
        } else {
            if ((tid & (BLOCK_WAVE - 1)) == 0) {
#pragma unroll
                for (int j = 0; j < SYM_MOMENTS; j++) wsum[j][tid / BLOCK_WAVE] = v[j];
            }
            __syncthreads();
            if (tid < SYM_MOMENTS) {  // lane j joins moment j across the waves
                const float lo = wsum[tid][0] + wsum[tid][1], hi = wsum[tid][2] + wsum[tid][3];
                float *to = p.mom + ((size_t)k * SYM_MOMENTS + (size_t)tid) * B + b;
                if (S == 4 * BLOCK_WAVE) {  // two blocks of 256 per pass
                    if (k < p.n_blocks) to[0] = lo * p.rs;
                    if (k + 1 < p.n_blocks) to[SYM_MOMENTS * B] = hi * p.rs;
                } else if (S == BLOCK_PASS) {
                    if (k < p.n_blocks) to[0] = (lo + hi) * p.rs;
                } else if (pass == 0) {  // S = 1024: the block's first half
                    half0 = lo + hi;
                } else if (k < p.n_blocks) {
                    to[0] = (half0 + (lo + hi)) * p.rs;
                }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(BLOCK_WAVE) void sym_step_kernel(SymParams p) {
    const int b = (int)blockIdx.x * BLOCK_WAVE + (int)threadIdx.x;
    if (b >= p.n_streams) return;
    const size_t st = (size_t)b * (size_t)sym_state_words(p.block), B = (size_t)p.n_streams;
    float A = 0.0f, Bm = 0.0f, U = 0.0f, M = 0.0f, Q = 0.0f, coh = 0.0f;
    float centre = p.track ? 0.0f : p.fixed_centre, thr = p.track ? 1.0f : p.fixed_thr;
    uint32_t tau = p.tau0;
    int flags = 0, slips = 0, held = 0;
    if (!p.fresh) {
        const float4 *s = reinterpret_cast<const float4 *>(p.state_old + st);
        const float4 m = s[0], c = s[1], l = s[2];
        A = m.x, Bm = m.y, U = m.z, M = m.w;
        Q = c.x, coh = c.y, tau = __float_as_uint(c.z), flags = __float_as_int(c.w);
        slips = __float_as_int(l.x), centre = l.y, thr = l.z;
    }
    const float *mom = p.mom + b;
    uint32_t *blk = p.blk + b;
    auto put = [&](int j) {
        uint32_t *to = blk + (size_t)j * 4 * B;
        to[0] = tau, to[B] = __float_as_uint(centre), to[2 * B] = __float_as_uint(thr);
        to[3 * B] = (uint32_t)(flags & SDRG_SYM_LOCKED);
    };
    if (p.n > 0) put(0);
    auto step = [&](const float (&q)[SYM_MOMENTS], int k) {
        if (q[4] < p.floor_thr) {
            held++;
        } else {
            if (!(flags & SDRG_SYM_SEEDED)) {
                A = q[0], Bm = q[1], U = q[2], M = q[3], Q = q[4];
            } else {
                const float da = q[0] - A, db = q[1] - Bm, du = q[2] - U, dm = q[3] - M, dq = q[4] - Q;
                A = A + p.beta * da;
                Bm = Bm + p.beta * db;
                U = U + p.beta * du;
                M = M + p.beta_level * dm;
                Q = Q + p.beta_level * dq;
            }
            const float aa = A * A, bb = Bm * Bm;
            const float len = sqrtf(aa + bb);
            coh = U == 0.0f ? 0.0f : len / U;
            flags = SDRG_SYM_SEEDED;
            if (coh >= p.lock_thr) {
                flags |= SDRG_SYM_LOCKED;
                const int64_t ang = (int64_t)rintf(sym_atan2f(Bm, A) * p.K);
                const uint32_t next = (uint32_t)(uint64_t)(ang - (int64_t)(p.inc >> 1) + 2147483648ll + p.trim);
                const int32_t d = (int32_t)(next - tau);
                if ((d >= 0 && next < tau) || (d < 0 && next > tau)) slips++;
                tau = next;
            }
            if (p.track) {
                const float mm = M * M;
                const float w = Q - mm;
                centre = M;
                thr = p.level_scale * sqrtf(fmaxf(w, 0.0f));
            }
        }
        put(k + 1);
    };
    int k = 0;
    for (; k + SYM_AHEAD <= p.n_blocks; k += SYM_AHEAD) {
        float q[SYM_AHEAD][SYM_MOMENTS];
#pragma unroll
        for (int j = 0; j < SYM_AHEAD; j++)
#pragma unroll
            for (int c = 0; c < SYM_MOMENTS; c++) q[j][c] = mom[((size_t)(k + j) * SYM_MOMENTS + c) * B];
#pragma unroll
        for (int j = 0; j < SYM_AHEAD; j++) step(q[j], k + j);
    }
    for (; k < p.n_blocks; k++) {
        float q[SYM_MOMENTS];
#pragma unroll
        for (int c = 0; c < SYM_MOMENTS; c++) q[c] = mom[((size_t)k * SYM_MOMENTS + c) * B];
        step(q, k);
    }
    if (p.n > 0) {
        float4 *s = reinterpret_cast<float4 *>(p.state_new + st);
        s[0] = make_float4(A, Bm, U, M);
        s[1] = make_float4(Q, coh, __uint_as_float(tau), __int_as_float(flags));
        s[2] = make_float4(__int_as_float(slips), centre, thr, 0.0f);
    }
    if (p.records) {  // the caller's pointer: aligned as its members, no more
        sdrg_symbols_record r;
        r.tau_frac = (float)tau * 0x1p-32f;
        r.tau = tau;
        r.coherence = coh;
        r.centre = centre;
        r.threshold = thr;
        r.slips = slips;
        r.held_blocks = held;
        r.flags = flags;
        p.records[b] = r;
    }
}

template <bool SOFT>
__global__ __launch_bounds__(SYM_PASS_TILE) void sym_pass_kernel(const float *in, SymParams p, void *symbols) {
    const int m = (int)blockIdx.x * SYM_PASS_TILE + (int)threadIdx.x, b = blockIdx.y;
    if (m >= p.cap) return;
    float soft = 0.0f;
    uint32_t hard = 0;
    if (m < p.n_sym) {
        // the call's value that ends the symbol in place m: the smallest t with emit0 + inc t >= (m + 1) 2^32
        const int64_t need = (int64_t)((uint64_t)(m + 1) << 32) - (int64_t)p.emit0;
        int t = need <= 0 ? 0 : (int)(((uint64_t)need + p.inc - 1) / p.inc);
        t = min(t, p.n - 1);  // the count's arithmetic keeps t under n: no read past the row whatever the caller passed
        const uint32_t c = p.c0 + p.inc * (uint32_t)t;
        const int u = p.off + t;
        const size_t B = (size_t)p.n_streams;
        const uint32_t *at = p.blk + b + (size_t)(u >> p.log2_block) * 4 * B;
        const uint32_t tau = at[0];
        const float centre = __uint_as_float(at[B]), thr = __uint_as_float(at[2 * B]);
        const bool locked = at[3 * B] != 0;
        const uint64_t num = (uint64_t)c + (0x100000000ull - (uint64_t)tau);
        const uint32_t qd = min((uint32_t)(num / p.inc), (uint32_t)(SYM_HISTORY - 1));  // c < inc: at most 65
        const uint32_t r = (uint32_t)(num - (uint64_t)qd * p.inc);
        const float nu = (float)r * p.rinc;
        const float *row = in + (size_t)b * (size_t)p.in_stride;
        const float *old_v = p.state_old + (size_t)b * (size_t)sym_state_words(p.block) + SYM_STATE_HEAD + SYM_HISTORY;
        const int p0 = u - (int)qd, p1 = p0 - 1;  // positions, at least off - SYM_HISTORY
        const float x0 = p0 >= p.off ? row[p0 - p.off] : p.fresh ? 0.0f : old_v[p0];
        const float x1 = p1 >= p.off ? row[p1 - p.off] : p.fresh ? 0.0f : old_v[p1];
        const float dx = x0 - x1;
        const float nd = nu * dx;
        const float y = x0 - nd;
        const float v = y - centre;
        if (SOFT) {
            soft = thr > 0.0f ? v / thr : 0.0f;
        } else {
            const uint32_t s = p.levels == 2 ? (v >= 0.0f ? 1u : 0u) : v < -thr ? 0u : v < 0.0f ? 1u : v < thr ? 2u : 3u;
            hard = s | (locked ? 0u : (uint32_t)SDRG_SYM_UNLOCKED);
        }
    }
    const size_t to = (size_t)b * (size_t)p.cap + (size_t)m;
    if (SOFT)
        static_cast<float *>(symbols)[to] = soft;
    else
        static_cast<uint8_t *>(symbols)[to] = (uint8_t)hard;
}

}  // namespace

hipError_t launch_symbols(const float *in, int n_streams, SymParams p, void *symbols, hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    const int S = p.block;
    const uintptr_t at = reinterpret_cast<uintptr_t>(in), to = reinterpret_cast<uintptr_t>(symbols);
    if (!in || !symbols || S < SDRG_SYM_MIN_BLOCK || S > BLOCK_MAX || (S & (S - 1)) != 0 || p.n < 0 || p.n > BLOCK_MAX_IN ||
        p.in_stride < p.n || p.in_stride > BLOCK_MAX_IN || p.off < 0 || p.off >= S || p.n_blocks != (p.off + p.n) / S ||
        n_streams > 65535 || !p.mom || !p.blk || !p.state_old || !p.state_new || !p.tab || (p.fresh && p.off != 0) ||
        p.inc < (1u << 26) || p.inc > (1u << 31) || p.cap < 1 || p.n_sym < 0 || p.n_sym > p.cap || p.n_sym > p.n ||
        (at & 3) != 0 || (p.soft && (to & 3) != 0))
        return hipErrorInvalidValue;
    p.n_streams = n_streams;
    p.log2_block = __builtin_ctz((unsigned)S);
    p.tile = block_tile(S);
    hipError_t er;
    if (p.n > 0) {
        const dim3 grid((unsigned)((p.off + p.n + p.tile - 1) / p.tile), (unsigned)n_streams);
        const bool pairs = (p.in_stride & 1) == 0 && (at & 7) == 0 && (p.off & 1) == 0;
        if (pairs)
            hipLaunchKernelGGL((sym_moments_kernel<true>), grid, dim3(BLOCK_THREADS), 0, stream, in, p);
        else
            hipLaunchKernelGGL((sym_moments_kernel<false>), grid, dim3(BLOCK_THREADS), 0, stream, in, p);
        if ((er = hipGetLastError()) != hipSuccess) return er;
    }
    if (p.n > 0 || p.records) {
        hipLaunchKernelGGL(sym_step_kernel, dim3((unsigned)((n_streams + BLOCK_WAVE - 1) / BLOCK_WAVE)), dim3(BLOCK_WAVE),
                           0, stream, p);
        if ((er = hipGetLastError()) != hipSuccess) return er;
    }
    const dim3 grid((unsigned)((p.cap + SYM_PASS_TILE - 1) / SYM_PASS_TILE), (unsigned)n_streams);
    if (p.soft)
        hipLaunchKernelGGL((sym_pass_kernel<true>), grid, dim3(SYM_PASS_TILE), 0, stream, in, p, symbols);
    else
        hipLaunchKernelGGL((sym_pass_kernel<false>), grid, dim3(SYM_PASS_TILE), 0, stream, in, p, symbols);
    return hipGetLastError();
}

}  // namespace sdrg
