// blanker.hip — the noise blanker stage (sdrg_engine_blanker_*): impulse noise zeroed per stream in the raw IQ, CF32 out
// (include/sdrg.h).  A sibling of iqcorr.hip, not a third law of block_stage.h: the decision is per
// sample, each hit blanks a window of its neighbours, so a workgroup of the pass kernel needs the decisions of the lead +
// tail inputs before its tile, the stage delays the stream by lead samples, and part of the state is samples and hit
// flags instead of powers.  What it takes from block_stage.h is the positions (u = off + i, off = g mod S), the first
// three steps of the xor butterfly and the shape of the three launches:
//   floor   grid (tiles of block_tile(S) positions, streams), 256 lanes.  A lane takes the positions 2 t and 2 t + 1: one
//           load of two raw samples (two loads of one when off is odd or the rows are not aligned to a pair), or the
//           state's powers below off.  The lane adds its two powers and the butterfly adds over the distances 1, 2 and 4
//           lanes: every lane of a group of 8 holds f_j, the adjacent-pair tree over its sub-block of 16.  From there on
//           the butterfly takes fminf: DPP to 8 lanes, bpermute to 16 and 32, LDS across the waves of a block (S >=
//           256).  Writes F = min_j(f_j) * 0.0625f of each completed block to flo[block][stream], and the powers of the
//           block the call leaves in progress to the new state.
//   step    one lane per stream, serial in the block index: L, eight blocks' F loaded ahead of the chain.  Writes
//           thr[block][stream] (the threshold after the block), the state's head if n > 0, and the record, its two
//           counts at 0, if a pointer was given.
//   pass    grid (tiles of BLANKER_TILE outputs of the call, streams), 256 lanes.  A lane scales the inputs t0 + 2 t and
//           t0 + 2 t + 1 of its tile and tests each power against the threshold of the block before its own; wave 0 does
//           the same for the 128 inputs before the tile (in the call's first tile: the old state's flags and samples).
//           The decisions are wave ballots, the even inputs' and the odd inputs' apart (a lane holds one of each), kept
//           as 64-bit words in LDS with the scaled samples.  After the barrier a lane takes the outputs t0 + 2 t and
//           t0 + 2 t + 1: the bits of its window [j - lead - tail, j] are a run of at most 41 in each of the two arrays.
//           Writes the delayed sample or zero, the zero tail up to in_stride (16-byte stores where the rows allow), the
//           new state's flags and last samples, and adds the tile's counts to the record with integer atomics.
// No workgroup reads what another writes in the same launch; the pass kernel's halo reads raw samples of the tile before
// it, so out must not overlap iq.  Compiled with -ffp-contract=off: every product and sum is rounded on its own.
#include <math.h>

#include "block_stage.h"
#include "ssb_common.h"

namespace sdrg {
namespace {

constexpr int BLK_FLAGS = BLANKER_FLAGS, BLK_LEAD = BLANKER_MAX_LEAD;
constexpr int BLK_HALO = 128;  // inputs before the tile that wave 0 decides: two per lane, >= BLK_FLAGS
static_assert(BLANKER_TILE == 2 * BLOCK_THREADS && BLK_HALO == 2 * BLOCK_WAVE && BLK_HALO >= BLK_FLAGS &&
                  BLK_FLAGS == BLANKER_MAX_LEAD + BLANKER_MAX_TAIL,
              "a lane takes two inputs and two outputs; wave 0 takes the halo");

// sample i of a row of raw words, scaled (the DDC's unpack: ssb_common.h)
template <int FMT>
__device__ __forceinline__ float2 blk_load(const char *row, int i) {
    return make_float2(load_i1<FMT>(row, i), load_q1<FMT>(row, i));
}

// samples i and i + 1, i even, of a row aligned to two samples: one load (the expressions of iqcorr.hip's)
template <int FMT>
__device__ __forceinline__ void blk_load_pair(const char *row, int i, float2 &a, float2 &c) {
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

__device__ __forceinline__ size_t blk_state_at(int b, int S) { return (size_t)b * (size_t)blanker_state_words(S); }

template <int FMT, bool VEC>
__global__ __launch_bounds__(BLOCK_THREADS) void blanker_floor_kernel(const char *iq, BlankerParams p) {
    __shared__ float wmin[BLOCK_THREADS / BLOCK_WAVE];
    constexpr int BPS = bytes_per_sample<FMT>();
    const int tid = threadIdx.x, b = blockIdx.y;
    const int S = p.block, off = p.off, end = p.off + p.n;  // the call's positions are [off, end)
    const int tail = p.n_blocks << p.log2_block;            // the first position of the block left in progress
    const size_t st = blk_state_at(b, S);
    const char *row = iq + (size_t)b * (size_t)p.in_stride * BPS;
    const float *old_pw = p.state_old + st + BLANKER_STATE_HEAD;  // read below off only, and off is 0 in a fresh stream
    float *new_pw = p.state_new + st + BLANKER_STATE_HEAD;
    const int width = min(S / 2, BLOCK_WAVE);
    const int passes = p.tile / BLOCK_PASS;
    float half0 = 0.0f;
    for (int pass = 0; pass < passes; pass++) {
        const int u = (int)blockIdx.x * p.tile + pass * BLOCK_PASS + 2 * tid;
        float q0 = 0.0f, q1 = 0.0f;
        if (VEC && u >= off && u + 1 < end) {
            float2 z0, z1;
            blk_load_pair<FMT>(row, u - off, z0, z1);
            q0 = block_power(z0);
            q1 = block_power(z1);
        } else {
            if (u < off)
                q0 = old_pw[u];
            else if (u < end)
                q0 = block_power(blk_load<FMT>(row, u - off));
            if (u + 1 < off)
                q1 = old_pw[u + 1];
            else if (u + 1 < end)
                q1 = block_power(blk_load<FMT>(row, u + 1 - off));
        }
        if (u >= tail && u < end) new_pw[u - tail] = q0;  // u - tail < S - 1: the block is not complete
        if (u + 1 >= tail && u + 1 < end) new_pw[u + 1 - tail] = q1;
        float v = block_reduce<false>(q0 + q1, 8);  // the sum over the 8 lanes of a sub-block of 16
        v = fminf(v, block_dpp<0x140>(v));          // row_mirror: the other 8 lanes of the row
        v = fminf(v, __shfl_xor(v, 16));
        if (width >= 64) v = fminf(v, __shfl_xor(v, 32));
        const int k = u >> p.log2_block;  // the block of this lane's pair
        if (S <= 2 * BLOCK_WAVE) {
            if ((u & (S - 1)) == 0 && k < p.n_blocks) p.flo[(size_t)k * (size_t)p.n_streams + b] = v * 0.0625f;
        } else {
            if ((tid & (BLOCK_WAVE - 1)) == 0) wmin[tid / BLOCK_WAVE] = v;
            __syncthreads();
            if (tid == 0) {
                const float lo = fminf(wmin[0], wmin[1]), hi = fminf(wmin[2], wmin[3]);
                float *to = p.flo + (size_t)k * (size_t)p.n_streams + b;
                if (S == 4 * BLOCK_WAVE) {  // two blocks of 256 per pass
                    if (k < p.n_blocks) to[0] = lo * 0.0625f;
                    if (k + 1 < p.n_blocks) to[p.n_streams] = hi * 0.0625f;
                } else if (S == BLOCK_PASS) {
                    if (k < p.n_blocks) to[0] = fminf(lo, hi) * 0.0625f;
                } else if (pass == 0) {  // S = 1024: the block's first half
                    half0 = fminf(lo, hi);
                } else if (k < p.n_blocks) {
                    to[0] = fminf(half0, fminf(lo, hi)) * 0.0625f;
                }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(BLOCK_WAVE) void blanker_step_kernel(BlankerParams p) {
    __shared__ glibc::LogfEntry tab[16];
    if (threadIdx.x < 16) tab[threadIdx.x] = glibc::logf_table()[threadIdx.x];
    __syncthreads();
    const int b = (int)blockIdx.x * BLOCK_WAVE + (int)threadIdx.x;
    if (b >= p.n_streams) return;
    const size_t st = blk_state_at(b, p.block), B = (size_t)p.n_streams;
    float L = 0.0f, thr = INFINITY;
    int seeded = 0;
    if (!p.fresh) {
        const float4 s = *reinterpret_cast<const float4 *>(p.state_old + st);
        L = s.x, seeded = __float_as_int(s.y), thr = s.z;
    }
    const float *flo = p.flo + b;
    float *col = p.thr + b;
    auto step = [&](float F, int k) {
        if (!seeded) {
            L = F, seeded = 1;
        } else {
            const float d = F - L;
            L = L + p.beta * d;
        }
        thr = fmaxf(L, p.floor_thr) * p.ratio;
        col[(size_t)k * B] = thr;
    };
    int k = 0;
    for (; k + BLOCK_AHEAD <= p.n_blocks; k += BLOCK_AHEAD) {
        float F[BLOCK_AHEAD];
#pragma unroll
        for (int j = 0; j < BLOCK_AHEAD; j++) F[j] = flo[(size_t)(k + j) * B];
#pragma unroll
        for (int j = 0; j < BLOCK_AHEAD; j++) step(F[j], k + j);
    }
    for (; k < p.n_blocks; k++) step(flo[(size_t)k * B], k);
    if (p.n > 0) *reinterpret_cast<float4 *>(p.state_new + st) = make_float4(L, __int_as_float(seeded), thr, 0.0f);
    if (p.records) {  // the caller's pointer: aligned as its members, no more
        sdrg_blanker_record r;
        r.level = L;
        r.level_db = 10.0f * glibc::log10f_fast(L + 1e-20f, tab);
        r.hits = 0, r.blanked = 0;  // the pass kernel adds its tiles' counts
        p.records[b] = r;
    }
}

// whether any of the bits [lo, hi] of the array is set: 0 <= lo, hi - lo < 64, and the word after hi's exists
__device__ __forceinline__ bool blk_any(const unsigned long long *a, int lo, int hi) {
    const int len = hi - lo + 1;
    if (len <= 0) return false;
    const int w = lo >> 6, s = lo & 63;
    unsigned long long x = a[w] >> s;
    if (s) x |= a[w + 1] << (64 - s);
    return (x & ((1ull << len) - 1ull)) != 0;
}

// VEC: the rows of iq are aligned to two samples; WIDE: in_stride is even and out is 16-byte aligned
template <int FMT, bool VEC, bool WIDE>
__global__ __launch_bounds__(BLOCK_THREADS) void blanker_pass_kernel(const char *iq, BlankerParams p, float2 *out) {
    constexpr int BPS = bytes_per_sample<FMT>();
    constexpr int WORDS = (BLK_HALO + BLANKER_TILE) / 128;  // 64-bit words of each parity: bit m is the input base + 2 m
    __shared__ unsigned long long ev[WORDS + 1], od[WORDS + 1];
    __shared__ __align__(16) float2 zs[BLK_LEAD + BLANKER_TILE];  // the scaled inputs from t0 - BLK_LEAD on
    const int tid = threadIdx.x, b = blockIdx.y, lane = tid & (BLOCK_WAVE - 1), wave = tid / BLOCK_WAVE;
    const int t0 = (int)blockIdx.x * BLANKER_TILE, n = p.n;
    float2 *orow = out + (size_t)b * (size_t)p.in_stride;
    const int j = t0 + 2 * tid;  // this lane's outputs j and j + 1, and after the lead its inputs
    if (t0 >= n) {               // the zero tail only, and every tile of a call without samples
        if (j >= p.in_stride) return;
        if (WIDE) {  // in_stride is even: j + 1 < in_stride
            *reinterpret_cast<float4 *>(orow + j) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        } else {
            orow[j] = make_float2(0.0f, 0.0f);
            if (j + 1 < p.in_stride) orow[j + 1] = make_float2(0.0f, 0.0f);
        }
        return;
    }
    const char *row = iq + (size_t)b * (size_t)p.in_stride * BPS;
    const size_t st = blk_state_at(b, p.block), B = (size_t)p.n_streams;
    const size_t flags_at = st + BLANKER_STATE_HEAD + (size_t)p.block, samp_at = flags_at + BLK_FLAGS;
    const int *flag_old = reinterpret_cast<const int *>(p.state_old + flags_at);
    const float2 *samp_old = reinterpret_cast<const float2 *>(p.state_old + samp_at);
    int *flag_new = reinterpret_cast<int *>(p.state_new + flags_at);
    float2 *samp_new = reinterpret_cast<float2 *>(p.state_new + samp_at);
    const float *col = p.thr + b;
    const float thr_old = p.fresh ? INFINITY : p.state_old[st + 2];  // in force for the block in progress
    const bool fresh = p.fresh != 0;

    auto decide = [&](float2 z, int v) {  // the call's input v in [0, n) against the threshold of the block before its own
        const int k = (p.off + v) >> p.log2_block;
        const float thr = k ? col[(size_t)(k - 1) * B] : thr_old;
        return block_power(z) > thr;
    };
    // the input v, of the call (v >= 0) or of the calls before it: its scaled sample and whether it is a hit
    auto one = [&](int v, float2 &z, bool &h) {
        z = make_float2(0.0f, 0.0f), h = false;
        if (v < 0) {
            if (!fresh && v >= -BLK_FLAGS) h = flag_old[BLK_FLAGS + v] != 0;
            if (!fresh && v >= -BLK_LEAD) z = samp_old[BLK_LEAD + v];
        } else if (v < n) {
            z = blk_load<FMT>(row, v);
            h = decide(z, v);
        }
    };
    auto two = [&](int v, float2 &z0, float2 &z1, bool &h0, bool &h1) {  // v is even
        if (VEC && v >= 0 && v + 1 < n) {
            blk_load_pair<FMT>(row, v, z0, z1);
            h0 = decide(z0, v), h1 = decide(z1, v + 1);
        } else {
            one(v, z0, h0);
            one(v + 1, z1, h1);
        }
    };
    // what the next call reads of the input v: written by the tile that owns it, or carried over by the first tile
    auto keep = [&](int v, float2 z, bool h) {
        if (v >= n) return;
        const int x = v - (n - BLK_FLAGS), y = v - (n - BLK_LEAD);
        if (x >= 0) flag_new[x] = h ? 1 : 0;
        if (y >= 0) samp_new[y] = z;
    };

    float2 z0, z1;
    bool h0, h1;
    two(j, z0, z1, h0, h1);
    keep(j, z0, h0);
    keep(j + 1, z1, h1);
    *reinterpret_cast<float4 *>(&zs[BLK_LEAD + 2 * tid]) = make_float4(z0.x, z0.y, z1.x, z1.y);
    const unsigned long long b0 = __ballot(h0), b1 = __ballot(h1);
    if (lane == 0) ev[1 + wave] = b0, od[1 + wave] = b1;
    const int hits = __popcll(b0) + __popcll(b1);  // of the tile's own inputs: the halo's are the tile's before
    if (tid == 0) ev[WORDS] = 0ull, od[WORDS] = 0ull;
    if (wave == 0) {
        const int v = t0 - BLK_HALO + 2 * lane;
        float2 y0, y1;
        bool g0, g1;
        two(v, y0, y1, g0, g1);
        if (v < 0) keep(v, y0, g0);  // only the call's first tile has inputs below 0
        if (v + 1 < 0) keep(v + 1, y1, g1);
        const int at = v - t0 + BLK_LEAD;
        if (at >= 0) *reinterpret_cast<float4 *>(&zs[at]) = make_float4(y0.x, y0.y, y1.x, y1.y);
        const unsigned long long c0 = __ballot(g0), c1 = __ballot(g1);
        if (lane == 0) ev[0] = c0, od[0] = c1;
    }
    __syncthreads();

    const int W = p.lead + p.tail;
    float2 o[2];
    bool zeroed[2];
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const int jj = j + r;
        const int eb = jj - t0 + BLK_HALO, ea = eb - W;  // the window, counted from t0 - BLK_HALO: ea >= 48
        const bool hit = blk_any(ev, (ea + 1) >> 1, eb >> 1) || blk_any(od, ea >> 1, (eb - 1) >> 1);
        const float2 z = zs[jj - t0 - p.lead + BLK_LEAD];
        const bool live = jj < n && jj >= p.skip;  // an output of the call whose input exists
        zeroed[r] = live && hit;
        o[r] = live && !hit ? z : make_float2(0.0f, 0.0f);
    }
    if (WIDE) {  // in_stride is even: j + 1 < in_stride
        if (j < p.in_stride) *reinterpret_cast<float4 *>(orow + j) = make_float4(o[0].x, o[0].y, o[1].x, o[1].y);
    } else {
        if (j < p.in_stride) orow[j] = o[0];
        if (j + 1 < p.in_stride) orow[j + 1] = o[1];
    }
    if (p.records) {
        const int blanked = __popcll(__ballot(zeroed[0])) + __popcll(__ballot(zeroed[1]));
        if (lane == 0 && hits) atomicAdd(&p.records[b].hits, hits);
        if (lane == 0 && blanked) atomicAdd(&p.records[b].blanked, blanked);
    }
}

template <int FMT>
hipError_t blanker_launch(const char *iq, const BlankerParams &p, float2 *out, hipStream_t stream) {
    constexpr int BPS = bytes_per_sample<FMT>();
    const uintptr_t at = reinterpret_cast<uintptr_t>(iq);
    if ((at & (uintptr_t)(BPS / 2 - 1)) != 0) return hipErrorInvalidValue;  // a component's own alignment
    const bool rows2 = (p.in_stride & 1) == 0 && (at & (uintptr_t)(2 * BPS - 1)) == 0;
    const dim3 lanes(BLOCK_THREADS);
    hipError_t er;
    if (p.n > 0) {
        const dim3 grid((unsigned)((p.off + p.n + p.tile - 1) / p.tile), (unsigned)p.n_streams);
        if (rows2 && (p.off & 1) == 0)
            hipLaunchKernelGGL((blanker_floor_kernel<FMT, true>), grid, lanes, 0, stream, iq, p);
        else
            hipLaunchKernelGGL((blanker_floor_kernel<FMT, false>), grid, lanes, 0, stream, iq, p);
        if ((er = hipGetLastError()) != hipSuccess) return er;
    }
    if (p.n > 0 || p.records) {
        hipLaunchKernelGGL(blanker_step_kernel, dim3((unsigned)((p.n_streams + BLOCK_WAVE - 1) / BLOCK_WAVE)),
                           dim3(BLOCK_WAVE), 0, stream, p);
        if ((er = hipGetLastError()) != hipSuccess) return er;
    }
    if (p.in_stride > 0) {
        const dim3 grid((unsigned)((p.in_stride + BLANKER_TILE - 1) / BLANKER_TILE), (unsigned)p.n_streams);
        const bool wide = (p.in_stride & 1) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
        if (rows2 && wide)
            hipLaunchKernelGGL((blanker_pass_kernel<FMT, true, true>), grid, lanes, 0, stream, iq, p, out);
        else if (rows2)
            hipLaunchKernelGGL((blanker_pass_kernel<FMT, true, false>), grid, lanes, 0, stream, iq, p, out);
        else if (wide)
            hipLaunchKernelGGL((blanker_pass_kernel<FMT, false, true>), grid, lanes, 0, stream, iq, p, out);
        else
            hipLaunchKernelGGL((blanker_pass_kernel<FMT, false, false>), grid, lanes, 0, stream, iq, p, out);
        if ((er = hipGetLastError()) != hipSuccess) return er;
    }
    return hipSuccess;
}

}  // namespace

hipError_t launch_blanker(const void *iq, int fmt, int n_streams, BlankerParams p, float *out, hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    const int S = p.block;
    if (!iq || !out || S < BLANKER_MIN_BLOCK || S > BLOCK_MAX || (S & (S - 1)) != 0 || p.n < 0 || p.n > BLOCK_MAX_IN ||
        p.in_stride < p.n || p.in_stride > BLOCK_MAX_IN || p.off < 0 || p.off >= S || p.n_blocks != (p.off + p.n) / S ||
        n_streams > 65535 || !p.flo || !p.thr || !p.state_old || !p.state_new || (p.fresh && p.off != 0) || p.lead < 0 ||
        p.lead > BLANKER_MAX_LEAD || p.tail < 0 || p.tail > BLANKER_MAX_TAIL || p.skip < 0 || p.skip > p.lead ||
        (reinterpret_cast<uintptr_t>(out) & 7) != 0)
        return hipErrorInvalidValue;
    p.n_streams = n_streams;
    p.log2_block = __builtin_ctz((unsigned)S);
    p.tile = block_tile(S);
    const char *raw = static_cast<const char *>(iq);
    float2 *o = reinterpret_cast<float2 *>(out);
    switch (fmt) {
    case SDRG_IQ_CS8: return blanker_launch<SDRG_IQ_CS8>(raw, p, o, stream);
    case SDRG_IQ_CU8: return blanker_launch<SDRG_IQ_CU8>(raw, p, o, stream);
    case SDRG_IQ_CS16: return blanker_launch<SDRG_IQ_CS16>(raw, p, o, stream);
    case SDRG_IQ_CF32: return blanker_launch<SDRG_IQ_CF32>(raw, p, o, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace sdrg
