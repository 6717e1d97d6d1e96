// channelizer.hip — the channelizer stage (sdrg_engine_channelizer_*): per stream a uniform polyphase filter bank of M
// channels, one prototype low-pass of L = M P taps, decimation D = M / O, the written rows as CF32 (DESIGN.md §3.14,
// include/sdrg.h).
//
// The tile form of fir_tile.h (grid, history, staging) on the unpacked samples, 256 threads: H = L - 1, an output is an
// output time (M values), and the history holds unpacked samples.  The stage's own:
//   tile block   `tile` = 2048 / M consecutive output times; the window of (nj - 1) D + L samples is staged linearly.
//   branch sums  thread (p = tid mod M, g = tid / M) owns branch p at the eight output times j = g + i (256 / M):
//                u_p[j] = sum_q h[p + q M] x[j D - p - q M], q ascending, one packed FMA on the (re, im) pair per tap,
//                four taps (read from the device's tap buffer, coalesced over p) and their 32 LDS reads issued per
//                step.  The lanes of a wave sit on consecutive p at one j: consecutive 8-byte words, conflict-free for
//                every M and D (lanes on another j read another contiguous run, or the same words at O = 2).
//   DFT          the tile x M block of branch sums, rows of M + 1 float2 in LDS, through the forward codelets of
//                fft_codelets.h: M <= 32 one thread per output time in registers; M = 64, 128, 256 as A x B = 8 x 8,
//                16 x 8, 16 x 16 in two passes (A-point DFTs over the stride-B subsequences with the twiddles
//                W_M^{b k1} from the device's table, in place; then B-point DFTs).  Y_c = F[(M - c) mod M].
//   stores       the spectra go to LDS transposed, [frequency][output time] (over the window, dead by then), and each
//                written row's run of `tile` outputs leaves as consecutive 8-byte words: 64 bytes (M = 256) to 8 KiB.
//   last block   zeroes the entries from n_out to cap of every written row beside carrying the history.
// An output's value depends only on its window and on (c, m): the order of its sums is fixed, so any cut of a stream
// into calls gives the same bytes.  Contraction stays on (the stage is specified by a bound, not operation by operation).
#include <algorithm>

#include "fir_tile.h"
#include "sdrg_internal.h"

namespace sdrg {
namespace {

namespace chan_fft {
#include "fft_codelets.h"
}
using chan_fft::f2;

constexpr int CHAN_THREADS = 256;
constexpr int CHAN_JPT = 8;             // output times per thread in the branch sums: tile = CHAN_JPT * 256 / M
constexpr int CHAN_LDS_BYTES = 65536;   // window (or transposed spectra) + block, every valid configuration fits

// stage_iq_window's sink: the window is a linear image of the unpacked samples.  (A lane's 8, 4 or 2 stores of a chunk
// land 64 bytes from its neighbour's; one sample per lane and step, with conflict-free stores, measured 14 to 33 %
// slower all the same: the loads' latency, not the stores, is what a tile waits for.  DESIGN.md §3.14.)
template <int FMT>
struct ChanSink {
    f2 *smp;
    __device__ __forceinline__ void hist(int u, f2 v) const { smp[u] = v; }
    __device__ __forceinline__ void sample(int u, int, float xr, float xi) const { smp[u] = f2{xr, xi}; }
    __device__ __forceinline__ void chunk(int u0, int, const uint32_t (&w)[4]) const {
        f2 *dst = smp + u0;
#pragma unroll
        for (int s = 0; s < 16 / bytes_per_sample<FMT>(); s++) {
            float xr, xi;
            iq_chunk_unpack<FMT>(w, s, xr, xi);
            dst[s] = f2{xr, xi};
        }
    }
};

// M = R <= 32: one thread per output time, the whole DFT in registers.  U rows of R + 1, V rows of vs.
template <int R>
__device__ __forceinline__ void chan_dft_small(const f2 *U, f2 *V, int tid, int tile, int vs) {
    for (int j = tid; j < tile; j += CHAN_THREADS) {
        f2 v[R];
#pragma unroll
        for (int k = 0; k < R; k++) v[k] = U[j * (R + 1) + k];
        chan_fft::dft<R>(v);
#pragma unroll
        for (int k = 0; k < R; k++) V[k * vs + j] = v[k];
    }
}

// M = A B: X[k1 + A k2] = sum_b W_B^{b k2} W_M^{b k1} sum_a x[B a + b] W_A^{a k1}.  tw[t] = e^{-j 2 pi t / 256}.
template <int A, int B>
__device__ __forceinline__ void chan_dft_large(f2 *U, f2 *V, const float2 *__restrict__ tw, int tid, int tile,
                                               int log2tile, int vs) {
    constexpr int M = A * B;
    for (int w = tid; w < tile * B; w += CHAN_THREADS) {
        const int j = w & (tile - 1), b = w >> log2tile;
        f2 *row = U + j * (M + 1);
        f2 v[A];
#pragma unroll
        for (int a = 0; a < A; a++) v[a] = row[B * a + b];
        chan_fft::dft<A>(v);
#pragma unroll
        for (int k1 = 1; k1 < A; k1++) {
            const float2 t = tw[b * k1 * (256 / M)];
            v[k1] = chan_fft::cmul_v(v[k1], f2{t.x, t.y});
        }
#pragma unroll
        for (int k1 = 0; k1 < A; k1++) row[B * k1 + b] = v[k1];  // the words this thread read: in place
    }
    __syncthreads();
    for (int w = tid; w < tile * A; w += CHAN_THREADS) {
        const int j = w & (tile - 1), k1 = w >> log2tile;
        const f2 *row = U + j * (M + 1) + B * k1;
        f2 v[B];
#pragma unroll
        for (int b = 0; b < B; b++) v[b] = row[b];
        chan_fft::dft<B>(v);
#pragma unroll
        for (int k2 = 0; k2 < B; k2++) V[(k1 + A * k2) * vs + j] = v[k2];
    }
}

template <int FMT>
__global__ __launch_bounds__(CHAN_THREADS) void chan_kernel(const char *__restrict__ iq, ChanParams p,
                                                            float *__restrict__ out) {
    constexpr int BPS = bytes_per_sample<FMT>();
    extern __shared__ __attribute__((aligned(16))) f2 chan_lds[];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int N = p.n, D = p.decim, M = p.channels, L = M * p.taps_per_channel, H = L - 1;
    const char *frame = iq + (size_t)b * (size_t)N * BPS;
    const f2 *hist_old = stream_history<f2>(p.hist_old, b, H);
    f2 *orows = reinterpret_cast<f2 *>(out) + (size_t)b * (size_t)p.n_channels * (size_t)p.cap;

    if ((int)blockIdx.x == p.n_tiles) {  // the new history and the zero tails of the written rows
        carry_history<CHAN_THREADS>(reinterpret_cast<f2 *>(p.hist_new) + (size_t)b * (size_t)H, hist_old, N, H, tid,
                                    [&](int t) { return f2{load_i1<FMT>(frame, t), load_q1<FMT>(frame, t)}; });
        const int z = p.cap - p.n_out;
        for (int i = tid; i < z * p.n_channels; i += CHAN_THREADS)
            orows[(size_t)(i / z) * (size_t)p.cap + (size_t)(p.n_out + i % z)] = f2{0.0f, 0.0f};
        return;
    }

    const FirWindow w(p, L);
    const int tile = p.tile, j0 = w.j0, nj = w.nj;
    f2 *smp = chan_lds;                      // the window; later the transposed spectra
    f2 *U = chan_lds + p.region;             // [tile][M + 1]: branch sums, then the DFT's intermediate

    stage_iq_window<FMT, CHAN_THREADS>(frame, hist_old, w.w0, w.count, H, p.vec_ok, tid, ChanSink<FMT>{smp});
    __syncthreads();

    // branch sums.  Output times past nj of a last tile read words of the window's region that hold nothing of this
    // tile (inside the allocation: the region is sized for a whole tile); their results are never stored.
    {
        const int pp = tid & (M - 1), g = tid >> p.log2m, G = CHAN_THREADS >> p.log2m;
        const int S = G * D, P = p.taps_per_channel;
        const float *__restrict__ hp = p.taps + pp;
        const f2 *x0 = smp + (g * D + H - pp);  // x[j D - p] of i = 0
        f2 acc[CHAN_JPT];
#pragma unroll
        for (int i = 0; i < CHAN_JPT; i++) acc[i] = f2{0.0f, 0.0f};
        int q = 0;
        for (; q + 4 <= P; q += 4) {
            float h[4];
#pragma unroll
            for (int k = 0; k < 4; k++) h[k] = hp[(q + k) * M];
            f2 v[4][CHAN_JPT];
#pragma unroll
            for (int k = 0; k < 4; k++)
#pragma unroll
                for (int i = 0; i < CHAN_JPT; i++) v[k][i] = x0[i * S - (q + k) * M];
#pragma unroll
            for (int k = 0; k < 4; k++)
#pragma unroll
                for (int i = 0; i < CHAN_JPT; i++) acc[i] = f2{h[k], h[k]} * v[k][i] + acc[i];
        }
        for (; q < P; q++) {
            const float h = hp[q * M];
#pragma unroll
            for (int i = 0; i < CHAN_JPT; i++) acc[i] = f2{h, h} * x0[i * S - q * M] + acc[i];
        }
#pragma unroll
        for (int i = 0; i < CHAN_JPT; i++) U[(g + i * G) * (M + 1) + pp] = acc[i];
    }
    __syncthreads();  // the block is whole, and every read of the window is done: the spectra may take its place

    const int vs = tile + 1;
    f2 *V = smp;  // [M][tile + 1]
    const float2 *tw = reinterpret_cast<const float2 *>(p.taps + L);
    switch (p.log2m) {
    case 1: chan_dft_small<2>(U, V, tid, tile, vs); break;
    case 2: chan_dft_small<4>(U, V, tid, tile, vs); break;
    case 3: chan_dft_small<8>(U, V, tid, tile, vs); break;
    case 4: chan_dft_small<16>(U, V, tid, tile, vs); break;
    case 5: chan_dft_small<32>(U, V, tid, tile, vs); break;
    case 6: chan_dft_large<8, 8>(U, V, tw, tid, tile, p.log2tile, vs); break;
    case 7: chan_dft_large<16, 8>(U, V, tw, tid, tile, p.log2tile, vs); break;
    default: chan_dft_large<16, 16>(U, V, tw, tid, tile, p.log2tile, vs); break;
    }
    __syncthreads();

    // row r is channel k = first_channel + r of the fftshifted order, c = (k + M / 2) mod M, Y_c = F[(M - c) mod M];
    // at O = 2 the output of global time m is (-1)^{c m} Y_c
    for (int idx = tid; idx < p.n_channels * tile; idx += CHAN_THREADS) {
        const int j = idx & (tile - 1), r = idx >> p.log2tile;
        if (j >= nj) continue;
        const int c = (p.first_channel + r + (M >> 1)) & (M - 1);
        f2 y = V[((M - c) & (M - 1)) * vs + j];
        if (p.oversample == 2 && (c & (p.m_parity + j0 + j) & 1)) y = -y;
        orows[(size_t)r * (size_t)p.cap + (size_t)(j0 + j)] = y;
    }
}

}  // namespace

int chan_tile_outputs(int channels) { return CHAN_JPT * CHAN_THREADS / channels; }

hipError_t launch_channelizer(const void *iq, int fmt, int n_streams, const ChanParams &p0, float *out,
                              hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    ChanParams p = p0;
    const int M = p.channels, P = p.taps_per_channel, O = p.oversample;
    if (!iq || !out || !p.taps || !p.hist_new || p.n < 1 || p.n > (1 << 20) || M < 2 ||
        M > SDRG_CHANNELIZER_MAX_CHANNELS || (M & (M - 1)) != 0 || P < 1 || P > SDRG_CHANNELIZER_MAX_TAPS_PER_CHANNEL ||
        M * P > SDRG_CHANNELIZER_MAX_TAPS || (O != 1 && O != 2) || p.decim != M / O || p.first < 0 ||
        p.first >= p.decim || p.n_out < 0 || p.cap != (p.n + p.decim - 1) / p.decim || p.n_out > p.cap ||
        (p.n_out > 0 && (int64_t)p.first + (int64_t)(p.n_out - 1) * p.decim >= p.n) || p.first_channel < 0 ||
        p.n_channels < 1 || p.first_channel + p.n_channels > M || (p.m_parity & ~1) != 0 || n_streams > 65535)
        return hipErrorInvalidValue;
    p.log2m = 0;
    while ((1 << p.log2m) < M) p.log2m++;
    p.tile = chan_tile_outputs(M);
    p.log2tile = 0;
    while ((1 << p.log2tile) < p.tile) p.log2tile++;
    p.n_tiles = (p.n_out + p.tile - 1) / p.tile;
    p.region = std::max((p.tile - 1) * p.decim + M * P, M * (p.tile + 1));
    const size_t lds = sizeof(float) * 2 * ((size_t)p.region + (size_t)p.tile * (size_t)(M + 1));
    if (lds > (size_t)CHAN_LDS_BYTES) return hipErrorInvalidValue;
    void (*k)(const char *, ChanParams, float *) = nullptr;
    const int bps = for_iq_format(fmt, [&](auto f) { k = chan_kernel<decltype(f)::value>; });
    if (bps == 0) return hipErrorInvalidValue;
    // rows of whole samples from a sample-aligned base: no sample straddles a 16-byte chunk
    p.vec_ok = reinterpret_cast<uintptr_t>(iq) % (size_t)bps == 0;
    hipLaunchKernelGGL(k, dim3((unsigned)p.n_tiles + 1, (unsigned)n_streams), dim3(CHAN_THREADS), lds, stream,
                       static_cast<const char *>(iq), p, out);
    return hipGetLastError();
}

}  // namespace sdrg
