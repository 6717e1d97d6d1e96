// iqcorr.hip — the IQ correction stage (sdrg_engine_iqcorr_*): the DC offset and the gain / phase imbalance of a raw IQ
// stream estimated block by block and removed, CF32 out (include/sdrg.h).  A sibling of block_stage.h,
// not a third law of it: the input is raw words of any of the four formats, a block's statistic is five moments instead
// of one power, the state keeps the block in progress as scaled samples (its moments are centred on the block's own
// mean, which is known only once the block is complete), and a sample is corrected by four ramped parameters.  What it
// takes from block_stage.h is the positions (u = off + i, off = g mod S), the xor butterfly (block_reduce) and the shape
// of the three launches:
//   moments grid (tiles of block_tile(S) positions, streams), 256 lanes.  A lane takes the positions 2 t and 2 t + 1: one
//           load of two raw samples (two loads of one when off is odd or the rows are not aligned to a pair), or the
//           state's samples below off.  Per sample zr, zi, zr zr - zi zi, zr zr + zi zi and zr zi; the lane adds its own
//           two, the butterfly joins the lanes of a block, LDS the waves of a block (S >= 256), so each value is the
//           adjacent-pair tree of include/sdrg.h.  Writes five floats per completed block, each times 1 / S, to
//           mom[block][5][stream], and the scaled samples of the block the call leaves in progress to the new state.
//   step    one lane per stream, serial in the block index: the moments centred, the DC and the balance estimates, four
//           blocks' moments loaded ahead of the chain.  Writes theta[block][4][stream] (dr, di, wr, wi after the block),
//           the twelve words of the new state if n > 0, and the record if a pointer was given.
//   pass    grid (tiles of block_tile(S) samples of the call, streams): two samples per lane read from the raw words
//           again, each corrected under the ramp from theta[k - 2] to theta[k - 1] of its block k (for the call's first
//           two blocks, the old state's), one fetch for both when they fall in the same block, and the zero tail up to
//           in_stride; 16-byte stores where the rows allow.
// No workgroup reads what another writes in the same launch, and the pass kernel's lanes read the samples they write:
// out may be iq when the format is CF32.  Compiled with -ffp-contract=off: every product, sum, quotient and root is
// rounded on its own (`/` and sqrtf are the compiler's correctly rounded sequences: tests/cpp/demod_math.hip).
#include "block_stage.h"
#include "ssb_common.h"

namespace sdrg {
namespace {

constexpr int IQC_MOMENTS = 5;
constexpr int IQC_AHEAD = 4;  // blocks the step kernel loads ahead of the chain

// sample i of a row of raw words, scaled (the DDC's unpack: ssb_common.h)
template <int FMT>
__device__ __forceinline__ float2 iqc_load(const char *row, int i) {
    return make_float2(load_i1<FMT>(row, i), load_q1<FMT>(row, i));
}

// samples i and i + 1, i even, of a row aligned to two samples: one load
template <int FMT>
__device__ __forceinline__ void iqc_load_pair(const char *row, int i, float2 &a, float2 &c) {
    if constexpr (FMT == SDRG_IQ_CF32) {
        const float4 v = *reinterpret_cast<const float4 *>(row + 8 * (size_t)i);
        a = make_float2(v.x, v.y);
        c = make_float2(v.z, v.w);
    } else if constexpr (FMT == SDRG_IQ_CS16) {
        const uint2 v = *reinterpret_cast<const uint2 *>(row + 4 * (size_t)i);
        a = make_float2((float)(int16_t)(v.x & 0xffff) * (1.0f / 32768.0f), (float)(int16_t)(v.x >> 16) * (1.0f / 32768.0f));
        c = make_float2((float)(int16_t)(v.y & 0xffff) * (1.0f / 32768.0f), (float)(int16_t)(v.y >> 16) * (1.0f / 32768.0f));
    } else {
        const uint32_t w = *reinterpret_cast<const uint32_t *>(row + 2 * (size_t)i);
        if constexpr (FMT == SDRG_IQ_CS8) {
            a = make_float2((float)(int8_t)(w & 0xff) * (1.0f / 128.0f), (float)(int8_t)((w >> 8) & 0xff) * (1.0f / 128.0f));
            c = make_float2((float)(int8_t)((w >> 16) & 0xff) * (1.0f / 128.0f), (float)(int8_t)(w >> 24) * (1.0f / 128.0f));
        } else {
            a = make_float2(((float)(w & 0xff) - 127.4f) * (1.0f / 128.0f), ((float)((w >> 8) & 0xff) - 127.4f) * (1.0f / 128.0f));
            c = make_float2(((float)((w >> 16) & 0xff) - 127.4f) * (1.0f / 128.0f), ((float)(w >> 24) - 127.4f) * (1.0f / 128.0f));
        }
    }
}

// the five values of the two samples of a lane, each pair added: level 0 of the tree
__device__ __forceinline__ void iqc_products(float2 z0, float2 z1, float (&v)[IQC_MOMENTS]) {
    const float a0 = z0.x * z0.x, b0 = z0.y * z0.y, a1 = z1.x * z1.x, b1 = z1.y * z1.y;
    const float e0 = a0 - b0, e1 = a1 - b1, s0 = a0 + b0, s1 = a1 + b1;
    const float c0 = z0.x * z0.y, c1 = z1.x * z1.y;
    v[0] = z0.x + z1.x;
    v[1] = z0.y + z1.y;
    v[2] = e0 + e1;
    v[3] = s0 + s1;
    v[4] = c0 + c1;
}

template <int FMT, bool VEC>
__global__ __launch_bounds__(BLOCK_THREADS) void iqcorr_moments_kernel(const char *iq, IqcorrParams p) {
    __shared__ float wsum[IQC_MOMENTS][BLOCK_THREADS / BLOCK_WAVE];
    constexpr int BPS = bytes_per_sample<FMT>();
    const int tid = threadIdx.x, b = blockIdx.y;
    const int S = p.block, off = p.off, end = p.off + p.n;  // the call's positions are [off, end)
    const int tail = p.n_blocks << p.log2_block;            // the first position of the block left in progress
    const size_t st = (size_t)b * (size_t)(2 * S + IQCORR_STATE_HEAD);
    const char *row = iq + (size_t)b * (size_t)p.in_stride * BPS;
    // read below off only, and off is 0 in a fresh stream
    const float2 *old_z = reinterpret_cast<const float2 *>(p.state_old + st + IQCORR_STATE_HEAD);
    float2 *new_z = reinterpret_cast<float2 *>(p.state_new + st + IQCORR_STATE_HEAD);
    const int width = min(S / 2, BLOCK_WAVE);
    const int passes = p.tile / BLOCK_PASS;
    const size_t B = (size_t)p.n_streams;
    float half0 = 0.0f;  // of the lanes below IQC_MOMENTS, each its own moment's
    for (int pass = 0; pass < passes; pass++) {
        const int u = (int)blockIdx.x * p.tile + pass * BLOCK_PASS + 2 * tid;
        float2 z0 = make_float2(0.0f, 0.0f), z1 = z0;
        if (VEC && u >= off && u + 1 < end) {
            iqc_load_pair<FMT>(row, u - off, z0, z1);
        } else {
            if (u < off)
                z0 = old_z[u];
            else if (u < end)
                z0 = iqc_load<FMT>(row, u - off);
            if (u + 1 < off)
                z1 = old_z[u + 1];
            else if (u + 1 < end)
                z1 = iqc_load<FMT>(row, u + 1 - off);
        }
        if (u >= tail && u < end) new_z[u - tail] = z0;  // u - tail < S - 1: the block is not complete
        if (u + 1 >= tail && u + 1 < end) new_z[u + 1 - tail] = z1;
        float v[IQC_MOMENTS];
        iqc_products(z0, z1, v);
#pragma unroll
        for (int j = 0; j < IQC_MOMENTS; j++) v[j] = block_reduce<false>(v[j], width);
        const int k = u >> p.log2_block;  // the block of this lane's pair
        if (S <= 2 * BLOCK_WAVE) {
            if ((u & (S - 1)) == 0 && k < p.n_blocks) {
                float *to = p.mom + (size_t)k * IQC_MOMENTS * B + b;
#pragma unroll
                for (int j = 0; j < IQC_MOMENTS; j++) to[(size_t)j * B] = v[j] * p.inv_block;
            }
        } else {
            if ((tid & (BLOCK_WAVE - 1)) == 0) {
#pragma unroll
                for (int j = 0; j < IQC_MOMENTS; j++) wsum[j][tid / BLOCK_WAVE] = v[j];
            }
            __syncthreads();
            if (tid < IQC_MOMENTS) {  // lane j joins moment j across the waves
                const float lo = wsum[tid][0] + wsum[tid][1], hi = wsum[tid][2] + wsum[tid][3];
                float *to = p.mom + ((size_t)k * IQC_MOMENTS + (size_t)tid) * B + b;
                if (S == 4 * BLOCK_WAVE) {  // two blocks of 256 per pass
                    if (k < p.n_blocks) to[0] = lo * p.inv_block;
                    if (k + 1 < p.n_blocks) to[IQC_MOMENTS * B] = hi * p.inv_block;
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

__global__ __launch_bounds__(BLOCK_WAVE) void iqcorr_step_kernel(IqcorrParams p) {
    __shared__ glibc::LogfEntry tab[16];
    if (threadIdx.x < 16) tab[threadIdx.x] = glibc::logf_table()[threadIdx.x];
    __syncthreads();
    const int b = (int)blockIdx.x * BLOCK_WAVE + (int)threadIdx.x;
    if (b >= p.n_streams) return;
    const size_t st = (size_t)b * (size_t)(2 * p.block + IQCORR_STATE_HEAD), B = (size_t)p.n_streams;
    float4 cur = make_float4(0.0f, 0.0f, 0.0f, 0.0f), prev = cur;  // theta after the last block, and the one before
    float A = 0.0f, Bm = 0.0f, P = 0.0f;
    int seeded = 0, held = 0;
    if (!p.fresh) {
        const float4 *s = reinterpret_cast<const float4 *>(p.state_old + st);
        cur = s[0], prev = s[1];
        const float4 m = s[2];
        A = m.x, Bm = m.y, P = m.z, seeded = __float_as_int(m.w);
    }
    const bool dc = p.mode & SDRG_IQCORR_DC, bal = p.mode & SDRG_IQCORR_BALANCE, whole = p.beta_dc == 1.0f;
    const float *mom = p.mom + b;
    float *theta = p.theta + b;
    auto step = [&](const float (&q)[IQC_MOMENTS], int k) {
        const float mr = q[0], mi = q[1];
        prev = cur;
        if (dc) {
            if (whole) {
                cur.x = mr, cur.y = mi;
            } else {
                const float er = mr - cur.x, ei = mi - cur.y;
                cur.x = cur.x + p.beta_dc * er;
                cur.y = cur.y + p.beta_dc * ei;
            }
        }
        if (bal) {
            const float rr = mr * mr, ii = mi * mi;
            const float a = q[2] - (rr - ii);
            const float c = q[4] - mr * mi;
            const float pw = q[3] - (rr + ii);
            if (pw < p.floor_thr) {
                held++;
            } else {
                if (!seeded) {
                    A = a, Bm = c, P = pw, seeded = 1;
                } else {
                    const float da = a - A, db = c - Bm, dp = pw - P;
                    A = A + p.beta_bal * da;
                    Bm = Bm + p.beta_bal * db;
                    P = P + p.beta_bal * dp;
                }
                const float cr = A / P, ci = (2.0f * Bm) / P;
                const float m = cr * cr + ci * ci;
                if (m <= 0.25f) {
                    const float d = 1.0f + sqrtf(1.0f - m);
                    cur.z = cr / d;
                    cur.w = ci / d;
                } else {
                    held++;
                }
            }
        }
        float *to = theta + (size_t)k * 4 * B;
        to[0] = cur.x, to[B] = cur.y, to[2 * B] = cur.z, to[3 * B] = cur.w;
    };
    int k = 0;
    for (; k + IQC_AHEAD <= p.n_blocks; k += IQC_AHEAD) {
        float q[IQC_AHEAD][IQC_MOMENTS];
#pragma unroll
        for (int j = 0; j < IQC_AHEAD; j++)
#pragma unroll
            for (int c = 0; c < IQC_MOMENTS; c++) q[j][c] = mom[((size_t)(k + j) * IQC_MOMENTS + c) * B];
#pragma unroll
        for (int j = 0; j < IQC_AHEAD; j++) step(q[j], k + j);
    }
    for (; k < p.n_blocks; k++) {
        float q[IQC_MOMENTS];
#pragma unroll
        for (int c = 0; c < IQC_MOMENTS; c++) q[c] = mom[((size_t)k * IQC_MOMENTS + c) * B];
        step(q, k);
    }
    if (p.n > 0) {
        float4 *s = reinterpret_cast<float4 *>(p.state_new + st);
        s[0] = cur, s[1] = prev, s[2] = make_float4(A, Bm, P, __int_as_float(seeded));
    }
    if (p.records) {  // the caller's pointer: aligned as its members, no more
        sdrg_iqcorr_record r;
        r.dc_re = cur.x, r.dc_im = cur.y, r.w_re = cur.z, r.w_im = cur.w;
        r.power = P;
        const float wr2 = cur.z * cur.z, wi2 = cur.w * cur.w;
        r.image_db = 10.0f * glibc::log10f_fast(wr2 + wi2 + 1e-20f, tab);
        r.held_blocks = held;
        r.seeded = seeded;
        p.records[b] = r;
    }
}

__device__ __forceinline__ float4 iqc_theta(const float *col, int j, size_t B) {
    const float *at = col + (size_t)j * 4 * B;
    return make_float4(at[0], at[B], at[2 * B], at[3 * B]);
}

// t0, t1 = theta[k - 2], theta[k - 1] counted from the call's block k: the two ends of the block's ramp; cur and prev
// are the old state's, theta[-1] and theta[-2]
__device__ __forceinline__ void iqc_fetch(int k, float4 cur, float4 prev, const float *col, size_t B, float4 &t0,
                                          float4 &t1) {
    t0 = prev, t1 = cur;
    if (k >= 1) t0 = cur, t1 = iqc_theta(col, k - 1, B);
    if (k >= 2) t0 = iqc_theta(col, k - 2, B);
}

__device__ __forceinline__ float iqc_ramp(float x0, float x1, float t) {
    const float d = x1 - x0;
    return x0 + d * t;
}

// the sample at in-block index i under its block's ramp
__device__ __forceinline__ float2 iqc_apply(float2 z, int i, float4 t0, float4 t1, float inv_block) {
    const float t = (float)(i + 1) * inv_block;
    const float dr = iqc_ramp(t0.x, t1.x, t), di = iqc_ramp(t0.y, t1.y, t);
    const float wr = iqc_ramp(t0.z, t1.z, t), wi = iqc_ramp(t0.w, t1.w, t);
    const float ur = z.x - dr, ui = z.y - di;
    const float a = wr * ur, c = wi * ui, d = wi * ur, e = wr * ui;
    return make_float2(ur - (a + c), ui - (d - e));
}

// VEC: the rows of iq are aligned to two samples; WIDE: in_stride is even and out is 16-byte aligned
template <int FMT, bool VEC, bool WIDE>
__global__ __launch_bounds__(BLOCK_THREADS) void iqcorr_pass_kernel(const char *iq, IqcorrParams p, float2 *out) {
    constexpr int BPS = bytes_per_sample<FMT>();
    const int tid = threadIdx.x, b = blockIdx.y;
    const char *row = iq + (size_t)b * (size_t)p.in_stride * BPS;
    float2 *orow = out + (size_t)b * (size_t)p.in_stride;
    const float *col = p.theta + b;
    const size_t B = (size_t)p.n_streams;
    float4 cur = make_float4(0.0f, 0.0f, 0.0f, 0.0f), prev = cur;
    if (!p.fresh) {
        const float4 *s = reinterpret_cast<const float4 *>(p.state_old + (size_t)b * (size_t)(2 * p.block + IQCORR_STATE_HEAD));
        cur = s[0], prev = s[1];
    }
    const int passes = p.tile / BLOCK_PASS, mask = p.block - 1;
    for (int pass = 0; pass < passes; pass++) {
        const int i = (int)blockIdx.x * p.tile + pass * BLOCK_PASS + 2 * tid;
        if (i >= p.in_stride) return;
        const int u = p.off + i, k0 = u >> p.log2_block, k1 = (u + 1) >> p.log2_block;
        float4 g0 = prev, g1 = cur, h0 = prev, h1 = cur;
        if (i < p.n) iqc_fetch(k0, cur, prev, col, B, g0, g1);
        h0 = g0, h1 = g1;
        if (i + 1 < p.n && k1 != k0) iqc_fetch(k1, cur, prev, col, B, h0, h1);
        float2 a = make_float2(0.0f, 0.0f), c = a;
        if (i + 1 < p.n) {
            float2 z0, z1;
            if (VEC) {
                iqc_load_pair<FMT>(row, i, z0, z1);
            } else {
                z0 = iqc_load<FMT>(row, i);
                z1 = iqc_load<FMT>(row, i + 1);
            }
            a = iqc_apply(z0, u & mask, g0, g1, p.inv_block);
            c = iqc_apply(z1, (u + 1) & mask, h0, h1, p.inv_block);
        } else if (i < p.n) {
            a = iqc_apply(iqc_load<FMT>(row, i), u & mask, g0, g1, p.inv_block);
        }
        if (WIDE) {  // in_stride is even: i + 1 < in_stride
            *reinterpret_cast<float4 *>(orow + i) = make_float4(a.x, a.y, c.x, c.y);
        } else {
            orow[i] = a;
            if (i + 1 < p.in_stride) orow[i + 1] = c;
        }
    }
}

template <int FMT>
hipError_t iqcorr_launch(const char *iq, const IqcorrParams &p, float2 *out, hipStream_t stream) {
    constexpr int BPS = bytes_per_sample<FMT>();
    const uintptr_t at = reinterpret_cast<uintptr_t>(iq);
    if ((at & (uintptr_t)(BPS / 2 - 1)) != 0) return hipErrorInvalidValue;  // a component's own alignment
    const bool rows2 = (p.in_stride & 1) == 0 && (at & (uintptr_t)(2 * BPS - 1)) == 0;
    const dim3 lanes(BLOCK_THREADS);
    hipError_t er;
    if (p.n > 0) {
        const dim3 grid((unsigned)((p.off + p.n + p.tile - 1) / p.tile), (unsigned)p.n_streams);
        if (rows2 && (p.off & 1) == 0)
            hipLaunchKernelGGL((iqcorr_moments_kernel<FMT, true>), grid, lanes, 0, stream, iq, p);
        else
            hipLaunchKernelGGL((iqcorr_moments_kernel<FMT, false>), grid, lanes, 0, stream, iq, p);
        if ((er = hipGetLastError()) != hipSuccess) return er;
    }
    if (p.n > 0 || p.records) {
        hipLaunchKernelGGL(iqcorr_step_kernel, dim3((unsigned)((p.n_streams + BLOCK_WAVE - 1) / BLOCK_WAVE)),
                           dim3(BLOCK_WAVE), 0, stream, p);
        if ((er = hipGetLastError()) != hipSuccess) return er;
    }
    if (p.in_stride > 0) {
        const dim3 grid((unsigned)((p.in_stride + p.tile - 1) / p.tile), (unsigned)p.n_streams);
        const bool wide = (p.in_stride & 1) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
        if (rows2 && wide)
            hipLaunchKernelGGL((iqcorr_pass_kernel<FMT, true, true>), grid, lanes, 0, stream, iq, p, out);
        else if (rows2)
            hipLaunchKernelGGL((iqcorr_pass_kernel<FMT, true, false>), grid, lanes, 0, stream, iq, p, out);
        else if (wide)
            hipLaunchKernelGGL((iqcorr_pass_kernel<FMT, false, true>), grid, lanes, 0, stream, iq, p, out);
        else
            hipLaunchKernelGGL((iqcorr_pass_kernel<FMT, false, false>), grid, lanes, 0, stream, iq, p, out);
        if ((er = hipGetLastError()) != hipSuccess) return er;
    }
    return hipSuccess;
}

}  // namespace

hipError_t launch_iqcorr(const void *iq, int fmt, int n_streams, IqcorrParams p, float *out, hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    const int S = p.block;
    if (!iq || !out || S < IQCORR_MIN_BLOCK || S > BLOCK_MAX || (S & (S - 1)) != 0 || p.n < 0 || p.n > BLOCK_MAX_IN ||
        p.in_stride < p.n || p.in_stride > BLOCK_MAX_IN || p.off < 0 || p.off >= S || p.n_blocks != (p.off + p.n) / S ||
        n_streams > 65535 || !p.mom || !p.theta || !p.state_old || !p.state_new || (p.fresh && p.off != 0) ||
        (p.mode & ~(SDRG_IQCORR_DC | SDRG_IQCORR_BALANCE)) != 0 || p.mode == 0 ||
        (reinterpret_cast<uintptr_t>(out) & 7) != 0)
        return hipErrorInvalidValue;
    p.n_streams = n_streams;
    p.log2_block = __builtin_ctz((unsigned)S);
    p.inv_block = 1.0f / (float)S;
    p.tile = block_tile(S);
    const char *raw = static_cast<const char *>(iq);
    float2 *o = reinterpret_cast<float2 *>(out);
    switch (fmt) {
    case SDRG_IQ_CS8: return iqcorr_launch<SDRG_IQ_CS8>(raw, p, o, stream);
    case SDRG_IQ_CU8: return iqcorr_launch<SDRG_IQ_CU8>(raw, p, o, stream);
    case SDRG_IQ_CS16: return iqcorr_launch<SDRG_IQ_CS16>(raw, p, o, stream);
    case SDRG_IQ_CF32: return iqcorr_launch<SDRG_IQ_CF32>(raw, p, o, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace sdrg
