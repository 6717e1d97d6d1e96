// tones.hip — the tone detector stage (sdrg_engine_tones_*): the power at K configured frequencies per block of S = 64 Q
// values of a stream, and a latched decision (include/sdrg.h).  A call's values sit at the positions v =
// soff + i, soff = g mod 64: position 0 is the first value of the sub-block of 64 in progress, whose soff leading values
// the previous calls left in the state (TonesParams, sdrg_internal.h).  Two launches:
//   correlate  grid (groups of TONES_GROUP_SUBS sub-blocks, streams), a wave per sub-block, a value per lane: from the
//              call's row, or from the state below soff.  The values of the sub-block the call leaves in progress go to
//              the new state (those below soff among them: a call inside a sub-block carries them over).  For a complete
//              sub-block the lane forms e, and per tone C and S from the table's (c, s) at its in-block index, and the
//              xor butterfly of block_stage.h joins each across the wave: float addition is commutative, so every lane
//              holds the bits of the adjacent-pair tree.  Lane k keeps tone k's two sums, and the wave writes the 2 K + 1
//              sums of its sub-block to sums[stream][sub] in three contiguous stores.
//   step       a wave per stream, lane k holding tone k: serial in the sub-block index, four sub-blocks' sums loaded
//              ahead of the chain.  acc = acc + sub_j; at a block's end P_k, the wave's argmax with the smaller index on
//              ties, the second maximum, the candidate and the latch (every lane computes them alike), and the coalesced
//              row of powers.  Then the zero rows of powers, the new state if n > 0 and the record (lane 0; glibc's
//              log10f, its table in LDS).
// No workgroup reads what another writes in the same launch.  Compiled with -ffp-contract=off: every product and sum is
// rounded on its own.
#include "block_stage.h"

namespace sdrg {
namespace {

constexpr int TONES_AHEAD = 4;  // sub-blocks the step kernel loads ahead of the chain

template <int COMP>
__global__ __launch_bounds__(TONES_GROUP_SUBS *TONES_SUB) void tones_correlate_kernel(const float *in, TonesParams p) {
    const int lane = (int)threadIdx.x & (TONES_SUB - 1), b = (int)blockIdx.y;
    const int j = (int)blockIdx.x * TONES_GROUP_SUBS + ((int)threadIdx.x >> 6);  // sub-blocks from the one in progress
    const int v = j * TONES_SUB + lane, end = p.soff + p.n;
    if (j * TONES_SUB >= end) return;  // the whole wave: no barrier follows
    const int K = p.n_tones, R = 2 * K + 1;
    const size_t st = (size_t)b * (size_t)tones_state_words(K, COMP) + TONES_STATE_HEAD + (size_t)R;
    const float *row = in + (size_t)b * (size_t)p.in_stride * COMP;
    float xr = 0.0f, xi = 0.0f;
    if (v < p.soff) {  // soff is 0 in a fresh stream: state_old is not read
        xr = p.state_old[st + (size_t)(v * COMP)];
        if (COMP == 2) xi = p.state_old[st + (size_t)(v * COMP + 1)];
    } else if (v < end) {
        if (COMP == 2) {
            const float2 z = reinterpret_cast<const float2 *>(row)[v - p.soff];
            xr = z.x, xi = z.y;
        } else {
            xr = row[v - p.soff];
        }
    }
    const int tail = p.n_sub * TONES_SUB;  // the first position of the sub-block left in progress
    if (v >= tail && v < end) {            // v - tail < 63: the sub-block is not complete
        p.state_new[st + (size_t)((v - tail) * COMP)] = xr;
        if (COMP == 2) p.state_new[st + (size_t)((v - tail) * COMP + 1)] = xi;
    }
    if (j >= p.n_sub) return;
    const int S = p.sub_blocks * TONES_SUB;
    const int pos = ((p.sub0 + j) % p.sub_blocks) * TONES_SUB + lane;  // the in-block index
    const float wf = p.wf[pos];
    float e;
    if (COMP == 2) {
        const float a = xr * wf, c = xi * wf;
        const float aa = a * a, cc = c * c;
        e = aa + cc;
    } else {
        const float a = xr * wf;
        e = a * a;
    }
    e = block_reduce<false>(e, BLOCK_WAVE);
    const float2 *tab = reinterpret_cast<const float2 *>(p.table) + pos;
    float keep_c = 0.0f, keep_s = 0.0f;
    for (int k = 0; k < K; k++) {
        const float2 cs = tab[(size_t)k * (size_t)S];
        float C, Sn;
        if (COMP == 2) {
            const float a = xr * cs.x, c = xi * cs.y, d = xi * cs.x, f = xr * cs.y;
            C = a + c;
            Sn = d - f;
        } else {
            C = xr * cs.x;
            Sn = xr * cs.y;
        }
        C = block_reduce<false>(C, BLOCK_WAVE);
        Sn = block_reduce<false>(Sn, BLOCK_WAVE);
        if (lane == k) keep_c = C, keep_s = Sn;
    }
    float *to = p.sums + ((size_t)b * (size_t)p.max_sub + (size_t)j) * (size_t)R;
    if (lane < K) {
        to[lane] = keep_c;
        to[K + lane] = keep_s;
    }
    if (lane == 0) to[2 * K] = e;
}

// a stream's accumulators (lane k: tone k's), latch and what the record repeats, in the registers of its wave
struct TonesStream {
    float C = 0.0f, S = 0.0f, E = 0.0f;
    int tone = -1, last = -1, run = 0, miss = 0;
    float power = 0.0f, share = 0.0f;
    int q = 0, blk = 0, tone_blocks = 0, changes = 0;

    // one sub-block's sums into the accumulators; at a block's end the powers' row, the candidate and the latch
    __device__ __forceinline__ void step(float c, float s, float e, const TonesParams &p, float *prow, int lane) {
        C = C + c;
        S = S + s;
        E = E + e;
        if (++q < p.sub_blocks) return;
        const int K = p.n_tones;
        const bool mine = lane < K;
        const float cc = C * C, ss = S * S;
        const float P = mine ? (cc + ss) * p.pnorm : -1.0f;
        if (mine) prow[(size_t)blk * (size_t)K + lane] = P;
        float bp = P;
        int bi = lane;
#pragma unroll
        for (int d = 1; d < BLOCK_WAVE; d *= 2) {
            const float op = __shfl_xor(bp, d);
            const int oi = __shfl_xor(bi, d);
            if (op > bp || (op == bp && oi < bi)) bp = op, bi = oi;
        }
        float p2 = (mine && lane != bi) ? P : -1.0f;
#pragma unroll
        for (int d = 1; d < BLOCK_WAVE; d *= 2) p2 = fmaxf(p2, __shfl_xor(p2, d));
        if (K == 1) p2 = 0.0f;
        const float Et = E * p.enorm;
        const float by_share = p.share_thr * Et, by_dom = p.dom * p2;
        const int cand = (bp >= p.min_power && bp >= by_share && bp >= by_dom) ? bi : -1;
        power = bp;
        share = bp / fmaxf(Et, 1e-30f);
        const int before = tone;
        run = (cand >= 0 && cand == last) ? min(run + 1, 65535) : (cand >= 0 ? 1 : 0);
        last = cand;
        if (cand >= 0 && run >= p.confirm) {
            tone = cand, miss = 0;
        } else if (tone >= 0) {
            if (cand == tone) {
                miss = 0;
            } else {
                miss = miss + 1;
                if (miss > p.release) tone = -1, miss = 0;
            }
        }
        tone_blocks += tone >= 0 ? 1 : 0;
        changes += tone != before ? 1 : 0;
        C = 0.0f, S = 0.0f, E = 0.0f, q = 0, blk++;
    }
};

__global__ __launch_bounds__(BLOCK_WAVE) void tones_step_kernel(TonesParams p, float *powers) {
    __shared__ glibc::LogfEntry tab[16];
    if (threadIdx.x < 16) tab[threadIdx.x] = glibc::logf_table()[threadIdx.x];
    __syncthreads();
    const int lane = (int)threadIdx.x, b = (int)blockIdx.x, K = p.n_tones, R = 2 * K + 1;
    const bool mine = lane < K;
    const size_t st = (size_t)b * (size_t)tones_state_words(K, p.components);
    TonesStream t;
    t.q = p.sub0;
    if (!p.fresh) {
        const float *so = p.state_old + st;
        t.tone = __float_as_int(so[0]), t.last = __float_as_int(so[1]), t.run = __float_as_int(so[2]);
        t.miss = __float_as_int(so[3]), t.power = so[4], t.share = so[5];
        if (mine) t.C = so[TONES_STATE_HEAD + lane], t.S = so[TONES_STATE_HEAD + K + lane];
        t.E = so[TONES_STATE_HEAD + 2 * K];
    }
    const float *sums = p.sums + (size_t)b * (size_t)p.max_sub * (size_t)R;
    float *prow = powers + (size_t)b * (size_t)p.cap_blocks * (size_t)K;
    const int at_c = mine ? lane : 0, at_s = mine ? K + lane : 0;  // the other lanes' loads are not used
    int j = 0;
    for (; j + TONES_AHEAD <= p.n_sub; j += TONES_AHEAD) {
        float c[TONES_AHEAD], s[TONES_AHEAD], e[TONES_AHEAD];
#pragma unroll
        for (int a = 0; a < TONES_AHEAD; a++) {
            const float *from = sums + (size_t)(j + a) * (size_t)R;
            c[a] = from[at_c], s[a] = from[at_s], e[a] = from[2 * K];
        }
#pragma unroll
        for (int a = 0; a < TONES_AHEAD; a++) t.step(c[a], s[a], e[a], p, prow, lane);
    }
    for (; j < p.n_sub; j++) {
        const float *from = sums + (size_t)j * (size_t)R;
        t.step(from[at_c], from[at_s], from[2 * K], p, prow, lane);
    }
    for (int i = p.n_blocks * K + lane; i < p.cap_blocks * K; i += BLOCK_WAVE) prow[i] = 0.0f;
    if (p.n > 0) {
        float *sn = p.state_new + st;
        if (mine) sn[TONES_STATE_HEAD + lane] = t.C, sn[TONES_STATE_HEAD + K + lane] = t.S;
        if (lane == 0) {
            sn[0] = __int_as_float(t.tone), sn[1] = __int_as_float(t.last), sn[2] = __int_as_float(t.run);
            sn[3] = __int_as_float(t.miss), sn[4] = t.power, sn[5] = t.share, sn[6] = 0.0f, sn[7] = 0.0f;
            sn[TONES_STATE_HEAD + 2 * K] = t.E;
        }
    }
    if (p.records && lane == 0) {  // the caller's pointer: aligned as its int32 members, no more
        sdrg_tones_record r;
        r.tone = t.tone;
        r.candidate = t.last;
        r.power = t.power;
        r.power_db = 10.0f * glibc::log10f_fast(t.power + 1e-20f, tab);
        r.share = t.share;
        r.tone_blocks = t.tone_blocks;
        r.changes = t.changes;
        r.run = t.run;
        p.records[b] = r;
    }
}

}  // namespace

hipError_t launch_tones(const void *in, int n_streams, TonesParams p, float *powers, hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    const int K = p.n_tones, Q = p.sub_blocks;
    if (!in || !powers || (p.components != 1 && p.components != 2) || K < 1 || K > SDRG_TONES_MAX_TONES || Q < 1 ||
        Q > SDRG_TONES_MAX_SUB_BLOCKS || p.n < 0 || p.n > SDRG_TONES_MAX_IN || p.in_stride < p.n ||
        p.in_stride > SDRG_TONES_MAX_IN || p.soff < 0 || p.soff >= TONES_SUB || p.sub0 < 0 || p.sub0 >= Q ||
        p.n_sub != (p.soff + p.n) / TONES_SUB || p.n_blocks != (p.sub0 + p.n_sub) / Q || p.n_blocks > p.cap_blocks ||
        p.n_sub > p.max_sub || n_streams > 65535 || !p.table || !p.wf || !p.sums || !p.state_old || !p.state_new ||
        (p.fresh && (p.soff != 0 || p.sub0 != 0)))
        return hipErrorInvalidValue;
    p.n_streams = n_streams;
    hipError_t er;
    if (p.n > 0) {
        const int subs = (p.soff + p.n + TONES_SUB - 1) / TONES_SUB;  // the one left in progress among them
        const dim3 grid((unsigned)((subs + TONES_GROUP_SUBS - 1) / TONES_GROUP_SUBS), (unsigned)n_streams);
        const float *x = static_cast<const float *>(in);
        if (p.components == 2)
            hipLaunchKernelGGL(tones_correlate_kernel<2>, grid, dim3(TONES_GROUP_SUBS * TONES_SUB), 0, stream, x, p);
        else
            hipLaunchKernelGGL(tones_correlate_kernel<1>, grid, dim3(TONES_GROUP_SUBS * TONES_SUB), 0, stream, x, p);
        if ((er = hipGetLastError()) != hipSuccess) return er;
    }
    hipLaunchKernelGGL(tones_step_kernel, dim3((unsigned)n_streams), dim3(BLOCK_WAVE), 0, stream, p, powers);
    return hipGetLastError();
}

}  // namespace sdrg
