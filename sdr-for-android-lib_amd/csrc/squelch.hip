// squelch.hip — the squelch stage (sdrg_engine_squelch_*): per stream, the CF32 channel cut into blocks of S samples at
// the global indices that are multiples of S; each completed block's mean power updates a smoothed level, a hysteresis
// gate with a hang time decides from it how the next block passes, and a record reports level and gate (DESIGN.md
// §3.16, include/sdrg.h).  A call's samples sit at the positions u = off + i, off = g mod S: position 0 is the first
// sample of the block in progress, whose off leading powers the previous calls left in the state.  Three launches:
//   power   grid (tiles of SQ_TILE(S) positions, streams), 256 lanes.  A lane takes the positions 2 t and 2 t + 1: one
//           16-byte load of two complex samples (two 8-byte loads when off is odd or the rows are not 16-byte aligned),
//           or the state's powers below off.  It adds its own two powers, and an xor butterfly adds across the
//           min(S / 2, 64) lanes of a block: DPP moves for the distances 1, 2, 4 and 8, bpermute for 16 and 32.  Float
//           addition is commutative, so every lane of the butterfly holds the adjacent-pair tree's bits.  Above a wave
//           (S >= 256) the waves' sums meet in LDS, and at S = 1024 a workgroup's two halves of 512.  Writes one float,
//           the mean power, per completed block to blk[block][stream], and the powers of the block the call leaves in
//           progress to the new state (those below off among them: a call inside a block carries them over).
//   step    one lane per stream, serial in the block index: the level, the gate and the hang counter, eight blocks'
//           powers loaded ahead of the chain.  blk is [block][stream], so the 64 lanes of a wave read and write 256
//           contiguous bytes; each power is overwritten with the code of the block after it.  Writes {L, open, hang,
//           code} to the new state and the record (the dB with the display stage's glibc log10f, its table in LDS).
//   gate    grid (tiles of SQ_TILE(S) samples of the call, streams): two samples per lane, each under the code of its
//           block (block 0 of the call: the state's; block k: blk[k - 1]), and the zero tail up to in_stride.
// No workgroup reads what another writes in the same launch, and the gate kernel's lanes read the samples they write: out
// may be chan.  Compiled with -ffp-contract=off: every product and sum is rounded on its own.
#include "block_power.h"
#include "glibc_logf.h"
#include "sdrg_internal.h"

namespace sdrg {
namespace {

// SQ_THREADS, SQ_PASS, SQ_WAVE, SQ_AHEAD, sq_power and sq_butterfly (the DPP and bpermute tree) are block_power.h's

template <bool VEC>
__global__ __launch_bounds__(SQ_THREADS) void squelch_power_kernel(const float2 *chan, SquelchParams p) {
    __shared__ float wsum[SQ_THREADS / SQ_WAVE];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int S = p.block, off = p.off, end = p.off + p.n;  // the call's positions are [off, end)
    const int tail = p.n_blocks << p.log2_block;            // the first position of the block left in progress
    const size_t st = (size_t)b * (size_t)(S + SQ_STATE_HEAD);
    const float2 *row = chan + (size_t)b * (size_t)p.in_stride;
    const float *old_pw = p.state_old + st + SQ_STATE_HEAD;  // read below off only, and off is 0 in a fresh stream
    float *new_pw = p.state_new + st + SQ_STATE_HEAD;
    const int width = min(S / 2, SQ_WAVE);
    const int passes = p.tile / SQ_PASS;
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
        const float v = sq_butterfly(q0 + q1, width);
        const int k = u >> p.log2_block;  // the block of this lane's pair
        if (S <= 2 * SQ_WAVE) {
            if ((u & (S - 1)) == 0 && k < p.n_blocks) p.blk[(size_t)k * (size_t)p.n_streams + b] = v * p.inv_block;
        } else {
            if ((tid & (SQ_WAVE - 1)) == 0) wsum[tid / SQ_WAVE] = v;
            __syncthreads();
            if (tid == 0) {
                const float lo = wsum[0] + wsum[1], hi = wsum[2] + wsum[3];
                float *to = p.blk + (size_t)k * (size_t)p.n_streams + b;
                if (S == 4 * SQ_WAVE) {  // two blocks of 256 per pass
                    if (k < p.n_blocks) to[0] = lo * p.inv_block;
                    if (k + 1 < p.n_blocks) to[p.n_streams] = hi * p.inv_block;
                } else if (S == SQ_PASS) {
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

__global__ __launch_bounds__(SQ_WAVE) void squelch_step_kernel(SquelchParams p) {
    __shared__ glibc::LogfEntry tab[16];
    if (threadIdx.x < 16) tab[threadIdx.x] = glibc::logf_table()[threadIdx.x];
    __syncthreads();
    const int b = (int)blockIdx.x * SQ_WAVE + (int)threadIdx.x;
    if (b >= p.n_streams) return;
    const size_t st = (size_t)b * (size_t)(p.block + SQ_STATE_HEAD), B = (size_t)p.n_streams;
    float L = 0.0f;
    int open = 0, hang = 0, code = 0, open_blocks = 0;
    if (!p.fresh) {
        const float4 s = *reinterpret_cast<const float4 *>(p.state_old + st);
        L = s.x, open = __float_as_int(s.y), hang = __float_as_int(s.z), code = __float_as_int(s.w);
    }
    const float beta = p.beta, open_thr = p.open_thr, close_thr = p.close_thr;
    const bool whole = beta == 1.0f;
    const int H = p.hang;
    auto step = [&](float P) {
        if (whole) {
            L = P;
        } else {
            const float d = P - L;
            L = L + beta * d;
        }
        const int was = open;
        if (open) {
            if (L >= close_thr)
                hang = H;
            else if (hang > 0)
                hang = hang - 1;
            else
                open = 0;
        } else if (L >= open_thr) {
            open = 1, hang = H;
        }
        code = 2 * was + open;
        open_blocks += open;
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
            col[(size_t)(k + j) * B] = __int_as_float(code);
        }
    }
    for (; k < p.n_blocks; k++) {
        step(col[(size_t)k * B]);
        col[(size_t)k * B] = __int_as_float(code);
    }
    if (p.n > 0)
        *reinterpret_cast<float4 *>(p.state_new + st) =
            make_float4(L, __int_as_float(open), __int_as_float(hang), __int_as_float(code));
    if (p.records) {
        sdrg_squelch_record r;
        r.level = L;
        r.level_db = 10.0f * glibc::log10f_fast(L + 1e-20f, tab);
        r.open = open;
        r.open_blocks = open_blocks;
        p.records[b] = r;  // the caller's pointer: aligned as its int32 members, no more
    }
}

// the sample at position u of the call (in-block index u mod S) under its block's code
__device__ __forceinline__ float2 sq_gate(float2 z, int u, int code0, const float *col, const SquelchParams &p) {
    const int k = u >> p.log2_block, i = u & (p.block - 1);
    const int code = k == 0 ? code0 : __float_as_int(col[(size_t)(k - 1) * (size_t)p.n_streams]);
    if (code == 3) return z;
    if (code == 0) return make_float2(0.0f, 0.0f);
    const float w = (float)(code == 1 ? i + 1 : p.block - 1 - i) * p.inv_block;
    return make_float2(z.x * w, z.y * w);
}

template <bool VEC>
__global__ __launch_bounds__(SQ_THREADS) void squelch_gate_kernel(const float2 *chan, SquelchParams p, float2 *out) {
    const int tid = threadIdx.x, b = blockIdx.y;
    const float2 *row = chan + (size_t)b * (size_t)p.in_stride;
    float2 *orow = out + (size_t)b * (size_t)p.in_stride;
    const float *col = p.blk + b;
    const int code0 =
        p.fresh ? 0 : __float_as_int(p.state_old[(size_t)b * (size_t)(p.block + SQ_STATE_HEAD) + SQ_STATE_HEAD - 1]);
    const int passes = p.tile / SQ_PASS;
    for (int pass = 0; pass < passes; pass++) {
        const int i = (int)blockIdx.x * p.tile + pass * SQ_PASS + 2 * tid;
        if (i >= p.in_stride) return;
        if (VEC) {  // in_stride is even: i + 1 < in_stride
            float4 zz = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (i + 1 < p.n) {
                zz = *reinterpret_cast<const float4 *>(row + i);
            } else if (i < p.n) {
                const float2 z = row[i];
                zz.x = z.x, zz.y = z.y;
            }
            float2 a = make_float2(0.0f, 0.0f), c = a;
            if (i < p.n) a = sq_gate(make_float2(zz.x, zz.y), p.off + i, code0, col, p);
            if (i + 1 < p.n) c = sq_gate(make_float2(zz.z, zz.w), p.off + i + 1, code0, col, p);
            *reinterpret_cast<float4 *>(orow + i) = make_float4(a.x, a.y, c.x, c.y);
        } else {
            float2 a = make_float2(0.0f, 0.0f), c = a;
            if (i < p.n) a = sq_gate(row[i], p.off + i, code0, col, p);
            if (i + 1 < p.n) c = sq_gate(row[i + 1], p.off + i + 1, code0, col, p);
            orow[i] = a;
            if (i + 1 < p.in_stride) orow[i + 1] = c;
        }
    }
}

}  // namespace

int squelch_tile(int block) { return block > SQ_PASS ? block : SQ_PASS; }

hipError_t launch_squelch(const float *chan, int n_streams, const SquelchParams &p0, float *out, hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    SquelchParams p = p0;
    const int S = p.block;
    if (!chan || !out || S < SDRG_SQUELCH_MIN_BLOCK || S > SDRG_SQUELCH_MAX_BLOCK || (S & (S - 1)) != 0 || p.n < 0 ||
        p.n > SDRG_SQUELCH_MAX_IN || p.in_stride < p.n || p.in_stride > SDRG_SQUELCH_MAX_IN || p.off < 0 || p.off >= S ||
        p.n_blocks != (p.off + p.n) / S || p.hang < 0 || n_streams > 65535 || !p.blk || !p.state_old || !p.state_new ||
        (p.fresh && p.off != 0))
        return hipErrorInvalidValue;
    p.n_streams = n_streams;
    p.log2_block = __builtin_ctz((unsigned)S);
    p.inv_block = 1.0f / (float)S;
    p.tile = squelch_tile(S);
    const bool rows16 = (p.in_stride & 1) == 0 && (reinterpret_cast<uintptr_t>(chan) & 15) == 0;
    const float2 *z = reinterpret_cast<const float2 *>(chan);
    hipError_t er;
    if (p.n > 0) {
        const dim3 grid((unsigned)((p.off + p.n + p.tile - 1) / p.tile), (unsigned)n_streams);
        if (rows16 && (p.off & 1) == 0)
            hipLaunchKernelGGL(squelch_power_kernel<true>, grid, dim3(SQ_THREADS), 0, stream, z, p);
        else
            hipLaunchKernelGGL(squelch_power_kernel<false>, grid, dim3(SQ_THREADS), 0, stream, z, p);
        if ((er = hipGetLastError()) != hipSuccess) return er;
    }
    if (p.n > 0 || p.records) {
        hipLaunchKernelGGL(squelch_step_kernel, dim3((unsigned)((n_streams + SQ_WAVE - 1) / SQ_WAVE)), dim3(SQ_WAVE), 0,
                           stream, p);
        if ((er = hipGetLastError()) != hipSuccess) return er;
    }
    if (p.in_stride > 0) {
        const dim3 grid((unsigned)((p.in_stride + p.tile - 1) / p.tile), (unsigned)n_streams);
        float2 *o = reinterpret_cast<float2 *>(out);
        if (rows16 && (reinterpret_cast<uintptr_t>(out) & 15) == 0)
            hipLaunchKernelGGL(squelch_gate_kernel<true>, grid, dim3(SQ_THREADS), 0, stream, z, p, o);
        else
            hipLaunchKernelGGL(squelch_gate_kernel<false>, grid, dim3(SQ_THREADS), 0, stream, z, p, o);
        if ((er = hipGetLastError()) != hipSuccess) return er;
    }
    return hipSuccess;
}

}  // namespace sdrg
