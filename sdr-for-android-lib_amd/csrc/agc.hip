// agc.hip — the AGC stage (sdrg_engine_agc_*): per stream, the CF32 channel cut into blocks of S samples at the global
// indices that are multiples of S; each completed block's statistic (its mean power by the squelch's adjacent-pair tree,
// or its peak power) moves one gain per stream by an attack / hang / decay law, and block b is multiplied by a ramp from
// gain[b - 2] to gain[b - 1], so the gain is continuous across the seams and no decision reaches back into the block
// that produced it (include/sdrg.h).  A call's samples sit at the positions u = off + i, off = g mod S,
// as the squelch's do (squelch.hip).  Three launches:
//   power   the squelch power kernel's shape: grid (tiles of AGC_TILE(S) positions, streams), 256 lanes, a lane takes the
//           positions 2 t and 2 t + 1 with one 16-byte load (two 8-byte loads when off is odd or the rows are not 16-byte
//           aligned) or the state's powers below off; the butterfly of block_power.h adds (MEAN) or takes the maximum
//           (PEAK).  Writes one float per completed block to blk[block][stream] and the powers of the block left in
//           progress to the new state.
//   step    one lane per stream, serial in the block index: G, the hang counter and the attack count, eight blocks'
//           statistics loaded ahead of the chain.  blk is [block][stream]: a wave reads and writes 256 contiguous bytes;
//           each statistic is overwritten with gain[k], the gain after its block.  Writes {G, G_prev, hang, P_last} to the
//           new state and the record (both dB with glibc's log10f, its table in LDS).
//   apply   grid (tiles of AGC_TILE(S) samples of the call, streams): two samples per lane, each under the ramp of its
//           block (g1 = blk[k - 1], g0 = blk[k - 2], or the old state's G and G_prev for the call's first two blocks),
//           and the zero tail up to in_stride.
// No workgroup reads what another writes in the same launch, and the apply kernel's lanes read the samples they write:
// out may be chan.  Compiled with -ffp-contract=off: every product, sum, quotient and root is rounded on its own (`/` and
// sqrtf are the compiler's correctly rounded sequences: tests/cpp/demod_math.hip).
#include "block_power.h"
#include "glibc_logf.h"
#include "sdrg_internal.h"

namespace sdrg {
namespace {

template <bool MAX, bool VEC>
__global__ __launch_bounds__(SQ_THREADS) void agc_power_kernel(const float2 *chan, AgcParams p) {
    __shared__ float wsum[SQ_THREADS / SQ_WAVE];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int S = p.block, off = p.off, end = p.off + p.n;  // the call's positions are [off, end)
    const int tail = p.n_blocks << p.log2_block;            // the first position of the block left in progress
    const size_t st = (size_t)b * (size_t)(S + AGC_STATE_HEAD);
    const float2 *row = chan + (size_t)b * (size_t)p.in_stride;
    const float *old_pw = p.state_old + st + AGC_STATE_HEAD;  // read below off only, and off is 0 in a fresh stream
    float *new_pw = p.state_new + st + AGC_STATE_HEAD;
    const int width = min(S / 2, SQ_WAVE);
    const int passes = p.tile / SQ_PASS;
    const float scale = MAX ? 1.0f : p.inv_block;  // x * 1.0f is x
    float half0 = 0.0f;
    for (int pass = 0; pass < passes; pass++) {
        const int u = (int)blockIdx.x * p.tile + pass * SQ_PASS + 2 * tid;
        float q0 = 0.0f, q1 = 0.0f;
        if (VEC && u >= off && u + 1 < end) {
            const float4 zz = *reinterpret_cast<const float4 *>(row + (u - off));
            q0 = sq_power(make_float2(zz.x, zz.y));
            q1 = sq_power(make_float2(zz.z, zz.w));
        } else {
            if (u < off)
                q0 = old_pw[u];
            else if (u < end)
                q0 = sq_power(row[u - off]);
            if (u + 1 < off)
                q1 = old_pw[u + 1];
            else if (u + 1 < end)
                q1 = sq_power(row[u + 1 - off]);
        }
        if (u >= tail && u < end) new_pw[u - tail] = q0;  // u - tail < S - 1: the block is not complete
        if (u + 1 >= tail && u + 1 < end) new_pw[u + 1 - tail] = q1;
        const float v = sq_reduce<MAX>(sq_join<MAX>(q0, q1), width);
        const int k = u >> p.log2_block;  // the block of this lane's pair
        if (S <= 2 * SQ_WAVE) {
            if ((u & (S - 1)) == 0 && k < p.n_blocks) p.blk[(size_t)k * (size_t)p.n_streams + b] = v * scale;
        } else {
            if ((tid & (SQ_WAVE - 1)) == 0) wsum[tid / SQ_WAVE] = v;
            __syncthreads();
            if (tid == 0) {
                const float lo = sq_join<MAX>(wsum[0], wsum[1]), hi = sq_join<MAX>(wsum[2], wsum[3]);
                float *to = p.blk + (size_t)k * (size_t)p.n_streams + b;
                if (S == 4 * SQ_WAVE) {  // two blocks of 256 per pass
                    if (k < p.n_blocks) to[0] = lo * scale;
                    if (k + 1 < p.n_blocks) to[p.n_streams] = hi * scale;
                } else if (S == SQ_PASS) {
                    if (k < p.n_blocks) to[0] = sq_join<MAX>(lo, hi) * scale;
                } else if (pass == 0) {  // S = 1024: the block's first half
                    half0 = sq_join<MAX>(lo, hi);
                } else if (k < p.n_blocks) {
                    to[0] = sq_join<MAX>(half0, sq_join<MAX>(lo, hi)) * scale;
                }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(SQ_WAVE) void agc_step_kernel(AgcParams p) {
    __shared__ glibc::LogfEntry tab[16];
    if (threadIdx.x < 16) tab[threadIdx.x] = glibc::logf_table()[threadIdx.x];
    __syncthreads();
    const int b = (int)blockIdx.x * SQ_WAVE + (int)threadIdx.x;
    if (b >= p.n_streams) return;
    const size_t st = (size_t)b * (size_t)(p.block + AGC_STATE_HEAD), B = (size_t)p.n_streams;
    float G = p.init_gain, Gp = p.init_gain, Pl = 0.0f;
    int hang = 0, attacks = 0;
    if (!p.fresh) {
        const float4 s = *reinterpret_cast<const float4 *>(p.state_old + st);
        G = s.x, Gp = s.y, hang = __float_as_int(s.z), Pl = s.w;
    }
    const float target = p.target, max_gain = p.max_gain, floor_thr = p.floor_thr, aa = p.alpha_a, ad = p.alpha_d;
    const bool whole_a = aa == 1.0f, whole_d = ad == 1.0f;
    const int H = p.hang;
    auto step = [&](float P) {
        Gp = G;
        Pl = P;
        if (P < floor_thr) return;  // the hold: neither the gain nor the hang counter moves
        const float a = sqrtf(P);
        const float want = fminf(target / a, max_gain);
        const float d = want - G;
        if (want < G) {
            G = whole_a ? want : G + aa * d;
            hang = H;
            attacks++;
        } else if (hang > 0) {
            hang = hang - 1;
        } else {
            G = whole_d ? want : G + ad * d;
        }
    };
    float *col = p.blk + b;
    int k = 0;
    for (; k + SQ_AHEAD <= p.n_blocks; k += SQ_AHEAD) {
        float P[SQ_AHEAD];
#pragma unroll
        for (int j = 0; j < SQ_AHEAD; j++) P[j] = col[(size_t)(k + j) * B];
#pragma unroll
        for (int j = 0; j < SQ_AHEAD; j++) {
            step(P[j]);
            col[(size_t)(k + j) * B] = G;
        }
    }
    for (; k < p.n_blocks; k++) {
        step(col[(size_t)k * B]);
        col[(size_t)k * B] = G;
    }
    if (p.n > 0) *reinterpret_cast<float4 *>(p.state_new + st) = make_float4(G, Gp, __int_as_float(hang), Pl);
    if (p.records) {
        sdrg_agc_record r;
        r.gain = G;
        r.gain_db = 20.0f * glibc::log10f_fast(G, tab);
        r.level_db = 10.0f * glibc::log10f_fast(Pl + 1e-20f, tab);
        r.attacks = attacks;
        p.records[b] = r;  // the caller's pointer: aligned as its int32 members, no more
    }
}

// the gains at the two ends of the ramp of the call's block k: {gain[-2], gain[-1]} counted from that block
__device__ __forceinline__ float2 agc_ends(int k, float2 old, const float *col, size_t B) {
    const float g1 = k >= 1 ? col[(size_t)(k - 1) * B] : old.x;
    const float g0 = k >= 2 ? col[(size_t)(k - 2) * B] : (k == 1 ? old.x : old.y);
    return make_float2(g0, g1);
}

// the sample at in-block index i under the ramp from g.x to g.y
__device__ __forceinline__ float2 agc_ramp(float2 z, int i, float2 g, float r) {
    const float t = (float)(i + 1) * r;
    const float d = g.y - g.x;
    const float w = g.x + d * t;
    return make_float2(z.x * w, z.y * w);
}

template <bool VEC>
__global__ __launch_bounds__(SQ_THREADS) void agc_apply_kernel(const float2 *chan, AgcParams p, float2 *out) {
    const int tid = threadIdx.x, b = blockIdx.y;
    const float2 *row = chan + (size_t)b * (size_t)p.in_stride;
    float2 *orow = out + (size_t)b * (size_t)p.in_stride;
    const float *col = p.blk + b;
    const size_t B = (size_t)p.n_streams;
    float2 old = make_float2(p.init_gain, p.init_gain);  // {G, G_prev} before the call
    if (!p.fresh) old = *reinterpret_cast<const float2 *>(p.state_old + (size_t)b * (size_t)(p.block + AGC_STATE_HEAD));
    const int passes = p.tile / SQ_PASS, mask = p.block - 1;
    for (int pass = 0; pass < passes; pass++) {
        const int i = (int)blockIdx.x * p.tile + pass * SQ_PASS + 2 * tid;
        if (i >= p.in_stride) return;
        const int u = p.off + i, k0 = u >> p.log2_block, k1 = (u + 1) >> p.log2_block;
        float2 g = make_float2(0.0f, 0.0f), h = g;
        if (i < p.n) g = agc_ends(k0, old, col, B);
        if (i + 1 < p.n) h = k1 == k0 ? g : agc_ends(k1, old, col, B);
        float2 a = make_float2(0.0f, 0.0f), c = a;
        if (VEC) {  // in_stride is even: i + 1 < in_stride
            if (i + 1 < p.n) {
                const float4 zz = *reinterpret_cast<const float4 *>(row + i);
                a = agc_ramp(make_float2(zz.x, zz.y), u & mask, g, p.inv_block);
                c = agc_ramp(make_float2(zz.z, zz.w), (u + 1) & mask, h, p.inv_block);
            } else if (i < p.n) {
                a = agc_ramp(row[i], u & mask, g, p.inv_block);
            }
            *reinterpret_cast<float4 *>(orow + i) = make_float4(a.x, a.y, c.x, c.y);
        } else {
            if (i < p.n) a = agc_ramp(row[i], u & mask, g, p.inv_block);
            if (i + 1 < p.n) c = agc_ramp(row[i + 1], (u + 1) & mask, h, p.inv_block);
            orow[i] = a;
            if (i + 1 < p.in_stride) orow[i + 1] = c;
        }
    }
}

template <bool MAX>
void agc_launch_power(bool vec, dim3 grid, hipStream_t stream, const float2 *z, const AgcParams &p) {
    if (vec)
        hipLaunchKernelGGL((agc_power_kernel<MAX, true>), grid, dim3(SQ_THREADS), 0, stream, z, p);
    else
        hipLaunchKernelGGL((agc_power_kernel<MAX, false>), grid, dim3(SQ_THREADS), 0, stream, z, p);
}

}  // namespace

int agc_tile(int block) { return block > SQ_PASS ? block : SQ_PASS; }

hipError_t launch_agc(const float *chan, int n_streams, const AgcParams &p0, float *out, hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    AgcParams p = p0;
    const int S = p.block;
    if (!chan || !out || S < SDRG_AGC_MIN_BLOCK || S > SDRG_AGC_MAX_BLOCK || (S & (S - 1)) != 0 || p.n < 0 ||
        p.n > SDRG_AGC_MAX_IN || p.in_stride < p.n || p.in_stride > SDRG_AGC_MAX_IN || p.off < 0 || p.off >= S ||
        p.n_blocks != (p.off + p.n) / S || p.hang < 0 || n_streams > 65535 || !p.blk || !p.state_old || !p.state_new ||
        (p.fresh && p.off != 0) || (p.detector != SDRG_AGC_DET_MEAN && p.detector != SDRG_AGC_DET_PEAK))
        return hipErrorInvalidValue;
    p.n_streams = n_streams;
    p.log2_block = __builtin_ctz((unsigned)S);
    p.inv_block = 1.0f / (float)S;
    p.tile = agc_tile(S);
    const bool rows16 = (p.in_stride & 1) == 0 && (reinterpret_cast<uintptr_t>(chan) & 15) == 0;
    const float2 *z = reinterpret_cast<const float2 *>(chan);
    hipError_t er;
    if (p.n > 0) {
        const dim3 grid((unsigned)((p.off + p.n + p.tile - 1) / p.tile), (unsigned)n_streams);
        const bool vec = rows16 && (p.off & 1) == 0;
        if (p.detector == SDRG_AGC_DET_PEAK)
            agc_launch_power<true>(vec, grid, stream, z, p);
        else
            agc_launch_power<false>(vec, grid, stream, z, p);
        if ((er = hipGetLastError()) != hipSuccess) return er;
    }
    if (p.n > 0 || p.records) {
        hipLaunchKernelGGL(agc_step_kernel, dim3((unsigned)((n_streams + SQ_WAVE - 1) / SQ_WAVE)), dim3(SQ_WAVE), 0,
                           stream, p);
        if ((er = hipGetLastError()) != hipSuccess) return er;
    }
    if (p.in_stride > 0) {
        const dim3 grid((unsigned)((p.in_stride + p.tile - 1) / p.tile), (unsigned)n_streams);
        float2 *o = reinterpret_cast<float2 *>(out);
        if (rows16 && (reinterpret_cast<uintptr_t>(out) & 15) == 0)
            hipLaunchKernelGGL(agc_apply_kernel<true>, grid, dim3(SQ_THREADS), 0, stream, z, p, o);
        else
            hipLaunchKernelGGL(agc_apply_kernel<false>, grid, dim3(SQ_THREADS), 0, stream, z, p, o);
        if ((er = hipGetLastError()) != hipSuccess) return er;
    }
    return hipSuccess;
}

}  // namespace sdrg
