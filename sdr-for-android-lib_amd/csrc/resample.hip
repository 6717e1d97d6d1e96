// resample.hip — the resampler stage (sdrg_engine_resample_*): per stream, real or CF32 rows at exactly L / M times
// their rate through a polyphase FIR of P taps per phase, a gain and the quantisation to int16 or float (DESIGN.md
// §3.15, include/sdrg.h).  One launch per call.
//
// The tile form of fir_tile.h (grid, history, carry_history) with one new idea: each output has its own filter phase.
// Output j of the call has t = phi0 + j M, reads the inputs down from q = q0 + t / L and uses the tap row phi = t mod L
// (q0, phi0: the host's, decim_cursor.h).  j M <= n L < 2^30, so every index here fits 32 bits.
//   tile         RESAMPLE_TILE = 256 consecutive outputs, one per lane; H = P - 1.
//   samples      the tile's outputs read [q_first - H, q_last], at most 255 * 8 + 64 values (M / L <= 8), staged linearly
//                in LDS (indices below 0 from the history).  Lane reads at one tap are monotone in the lane, 32 lanes
//                span about 32 M / L values: broadcast or conflict-free for M <= L, at most ceil(M / L)-way conflicts
//                otherwise, which is why the ratio is capped.  A CF32 value is one 8-byte read.
//   taps         in device memory in polyphase order [L][P].  Phases repeat every L outputs, so a tile needs
//                C = min(nj, L) rows, row c being the phase of its output c; lane j uses column j mod L.  In LDS they
//                are stored [k][c] with the row pitch C | 1: at tap k the lanes read consecutive dwords (equal
//                addresses broadcast), and no gather is left in the FIR loop.  The odd pitch is for the staging
//                alone: consecutive lanes copy consecutive k of one row (coalesced in memory), and with an even pitch
//                their stores would share a bank (256 rows: 108 us with it, 139 us without).
// No workgroup reads what another writes in the same launch.  Compiled with -ffp-contract=off: every product and sum is
// rounded on its own.
#include "fir_tile.h"
#include "sdrg_internal.h"

namespace sdrg {
namespace {

constexpr int RESAMPLE_THREADS = 256;
static_assert(RESAMPLE_TILE == RESAMPLE_THREADS, "one output per lane");
#ifndef RESAMPLE_LAB_PITCH_OR
#define RESAMPLE_LAB_PITCH_OR 1
#endif
constexpr int RESAMPLE_PITCH_OR = RESAMPLE_LAB_PITCH_OR;  // 1: the odd row pitch C | 1 (a lab build may set 0: the pitch C)

typedef float rs_f2 __attribute__((ext_vector_type(2)));

// fir_tile.h's output trait for a value V: a float's, or for a pair its `pair`, made component by component
template <typename V, int FMT>
struct ResampleOut : FirOut<FMT> {};
template <int FMT>
struct ResampleOut<rs_f2, FMT> {
    typedef typename FirOut<FMT>::pair type;
    static __device__ __forceinline__ type make(rs_f2 o) {
        type r;
        r.x = FirOut<FMT>::make(o.x);
        r.y = FirOut<FMT>::make(o.y);
        return r;
    }
};

template <typename V, int FMT>
__global__ __launch_bounds__(RESAMPLE_THREADS) void resample_kernel(const V *__restrict__ in, ResampleParams p,
                                                                    int smp_at,
                                                                    typename ResampleOut<V, FMT>::type *__restrict__ out) {
    typedef typename ResampleOut<V, FMT>::type out_t;
    extern __shared__ __attribute__((aligned(16))) float resample_lds[];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int N = p.n, P = p.taps_per_phase, H = P - 1;
    const unsigned L = (unsigned)p.interp, M = (unsigned)p.decim;
    const V *x = in + (size_t)b * (size_t)p.in_stride;
    const V *hist_old = stream_history<V>(p.hist_old, b, H);
    out_t *orow = out + (size_t)b * (size_t)p.cap;

    if ((int)blockIdx.x == p.n_tiles) {
        close_stream<RESAMPLE_THREADS, 1>(p.hist_new, hist_old, b, N, H, orow, p.n_out, p.cap, tid,
                                          [&](int t) { return x[t]; });
        return;
    }

    const int j0 = (int)blockIdx.x * RESAMPLE_TILE, nj = min(RESAMPLE_TILE, p.n_out - j0);
    const unsigned t_first = (unsigned)p.phi0 + (unsigned)j0 * M;  // t of the tile's first output
    const int qa = p.q0 + (int)(t_first / L);                      // q of the tile's first and last outputs: both in
    const int qb = p.q0 + (int)((t_first + (unsigned)(nj - 1) * M) / L);  // [0, N)
    const int w0 = qa - H;                                         // local index of the window's first value, >= -H
    const int count = qb - w0 + 1;
    const int C = min(nj, (int)L), pitch = C | RESAMPLE_PITCH_OR;
    float *tap_lds = resample_lds;
    V *smp = reinterpret_cast<V *>(resample_lds + smp_at);

    {  // taps: element i = c P + k of the tile's C rows, i = tid, then i += RESAMPLE_THREADS, without a division
        int c = tid / P, k = tid - c * P;
        unsigned ph = (t_first + (unsigned)c * M) % L;  // the phase of output j0 + c
        const int dc = RESAMPLE_THREADS / P, dk = RESAMPLE_THREADS - dc * P;
        const unsigned dph = ((unsigned)dc * M) % L, m1 = M % L;
        while (c < C) {
            tap_lds[k * pitch + c] = p.taps[ph * (unsigned)P + (unsigned)k];
            c += dc, k += dk, ph += dph;
            if (ph >= L) ph -= L;
            if (k >= P) {
                k -= P, c++, ph += m1;
                if (ph >= L) ph -= L;
            }
        }
    }
    for (int u = tid; u < count; u += RESAMPLE_THREADS) {
        const int t = w0 + u;  // <= qb < N
        V v = V(0.0f);
        if (t >= 0)
            v = x[t];
        else if (hist_old)
            v = hist_old[t + H];
        smp[u] = v;
    }
    __syncthreads();

    if (tid < nj) {
        constexpr int AHEAD = 8;  // LDS reads in flight per lane: the sums are one chain, the reads are not
        const unsigned t = t_first + (unsigned)tid * M;
        const V *sp = smp + (p.q0 + (int)(t / L) - w0);       // x[q]; tap k reads sp[-k], down to x[q - H] at smp[>= 0]
        const float *hp = tap_lds + (int)((unsigned)tid % L);  // the column of this lane's phase
        V acc = V(0.0f);
        int k = 0;
        for (; k + AHEAD <= P; k += AHEAD) {
            float h[AHEAD];
            V v[AHEAD];
#pragma unroll
            for (int i = 0; i < AHEAD; i++) {
                h[i] = hp[(k + i) * pitch];
                v[i] = sp[-(k + i)];
            }
#pragma unroll
            for (int i = 0; i < AHEAD; i++) acc = acc + V(h[i]) * v[i];
        }
        for (; k < P; k++) acc = acc + V(hp[k * pitch]) * sp[-k];
        orow[j0 + tid] = ResampleOut<V, FMT>::make(acc * V(p.gain));
    }
}

template <typename V, int FMT>
void resample_enqueue(const void *in, const ResampleParams &p, int smp_at, void *out, dim3 grid, size_t lds,
                      hipStream_t stream) {
    typedef typename ResampleOut<V, FMT>::type out_t;
    hipLaunchKernelGGL((resample_kernel<V, FMT>), grid, dim3(RESAMPLE_THREADS), lds, stream, static_cast<const V *>(in), p,
                       smp_at, static_cast<out_t *>(out));
}

}  // namespace

hipError_t launch_resample(const void *in, int n_streams, const ResampleParams &p0, void *out, hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    ResampleParams p = p0;
    const int L = p.interp, M = p.decim, P = p.taps_per_phase;
    if (!out || !p.taps || p.n < 0 || p.n > SDRG_RESAMPLE_MAX_IN || L < 1 || L > SDRG_RESAMPLE_MAX_FACTOR || M < 1 ||
        M > SDRG_RESAMPLE_MAX_FACTOR || L > 8 * M || M > 8 * L || P < 1 || P > SDRG_RESAMPLE_MAX_TAPS_PER_PHASE ||
        L * P > SDRG_RESAMPLE_MAX_TAPS || (p.components != 1 && p.components != 2) ||
        (p.out_format != SDRG_RESAMPLE_OUT_S16 && p.out_format != SDRG_RESAMPLE_OUT_F32) || p.q0 < 0 || p.phi0 < 0 ||
        p.phi0 >= L || p.n_out < 0 || p.cap < 1 || p.n_out > p.cap || n_streams > 65535)
        return hipErrorInvalidValue;
    // the last output's newest input is inside the frame: nothing is read past n
    if (p.n_out > 0 && (int64_t)p.q0 + ((int64_t)p.phi0 + (int64_t)(p.n_out - 1) * M) / L >= (int64_t)p.n)
        return hipErrorInvalidValue;
    if (p.n > 0 && (!in || p.in_stride < p.n || (P > 1 && !p.hist_new)))
        return hipErrorInvalidValue;
    // a value is loaded and stored whole: 4 or 8 bytes in, 2 to 8 bytes out
    const size_t in_align = sizeof(float) * (size_t)p.components;
    const size_t out_align = (p.out_format == SDRG_RESAMPLE_OUT_F32 ? sizeof(float) : sizeof(int16_t)) * (size_t)p.components;
    if (reinterpret_cast<uintptr_t>(in) % in_align != 0 || reinterpret_cast<uintptr_t>(out) % out_align != 0 ||
        reinterpret_cast<uintptr_t>(p.hist_old) % in_align != 0 || reinterpret_cast<uintptr_t>(p.hist_new) % in_align != 0)
        return hipErrorInvalidValue;
    p.n_tiles = (p.n_out + RESAMPLE_TILE - 1) / RESAMPLE_TILE;
    // LDS: P rows of min(tile, L) | 1 taps, then the widest window a tile has: its first and last outputs are
    // floor((tile - 1) M / L) or one more inputs apart, and the first reads P - 1 further back
    const int smp_at = (P * (std::min(RESAMPLE_TILE, L) | 1) + 3) & ~3;
    const int max_count = (RESAMPLE_TILE - 1) * M / L + 1 + P;
    const size_t lds = sizeof(float) * ((size_t)smp_at + (size_t)max_count * (size_t)p.components);
    const dim3 grid((unsigned)p.n_tiles + 1, (unsigned)n_streams);
    const bool f32 = p.out_format == SDRG_RESAMPLE_OUT_F32;
    if (p.components == 1) {
        if (f32)
            resample_enqueue<float, SDRG_RESAMPLE_OUT_F32>(in, p, smp_at, out, grid, lds, stream);
        else
            resample_enqueue<float, SDRG_RESAMPLE_OUT_S16>(in, p, smp_at, out, grid, lds, stream);
    } else {
        if (f32)
            resample_enqueue<rs_f2, SDRG_RESAMPLE_OUT_F32>(in, p, smp_at, out, grid, lds, stream);
        else
            resample_enqueue<rs_f2, SDRG_RESAMPLE_OUT_S16>(in, p, smp_at, out, grid, lds, stream);
    }
    return hipGetLastError();
}

}  // namespace sdrg
