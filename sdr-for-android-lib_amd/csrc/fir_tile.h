// fir_tile.h — the tile form the FIR stages share: ddc.hip, demod.hip's FIR kernel and sideband.hip take all of it;
// bank.hip takes all of it with a channel-group dimension in the grid and a close_stream of its own (one history per
// stream, C rows of tail);
// channelizer.hip takes the grid, the history, the window and the staging, and has its own sums; resample.hip takes the
// grid, the history and the output trait, and has a filter phase per output in place of the polyphase layout below.
// DESIGN.md §3.18a says what the frame owns and what a stage supplies.
//
// A stage filters each stream with a window of H + 1 values and decimates by D.  A call's outputs j in [0, n_out) read
// the values at the local indices t = first + j D - k, k in [0, H]; t in [0, N) is this call's frame, t in [-H, 0) the
// history: the H values before the frame, kept per stream in one half of a ping-pong buffer, and zeros after a
// restart, when the call gets hist_old == nullptr (decim_cursor.h has the host's side: first, n_out, the halves).
//   parameters   FirTileParams (sdrg_internal.h): the host's fields, and tile, row, n_tiles, which fir_tile_plan fills
//                in the launcher after the refusals every such stage makes.
//   grid         (tiles of outputs + 1, streams).  A tile workgroup stages the (nj - 1) D + H + 1 values its nj outputs
//                read (FirWindow) into LDS, then computes them.  The last workgroup of a stream (blockIdx.x ==
//                n_tiles) writes the new history, the values at t in [N - H, N), into the other half, and the zero
//                tail of `out` (close_stream): no workgroup reads what another writes in the same launch.
//   staging      of raw IQ (stage_iq_window): indices below 0 from the history, then the frame in 16-byte chunks
//                aligned in memory, one uint4 load each; the chunks the window covers only in part, at its ends, and
//                every chunk of a base that is not sample-aligned, sample by sample.  Both unpack as load_i1 /
//                load_q1 of ssb_common.h.  Where a value lands in LDS, and what is done to it first, is the stage's
//                (its sink).  The taps go to LDS ahead of the window (stage_taps).
//   FIR          (polyphase_fir, a tap per value or per component) one output per lane from the polyphase layout
//                [u mod D][u / D], rows of `row` (odd) values: at tap k lane j reads u = j D + (H - k), one row for the
//                whole wave and consecutive columns for consecutive lanes, so the reads are conflict-free for every D
//                (a linear layout puts the lanes D values apart: gcd(D, 32)-way conflicts), and the row base moves by
//                scalar arithmetic only.
//   output       FirOut: a float as it is, or clamped to [-1, 1], scaled by 32767 and rounded to int16.
// Nothing here sets the contraction mode of a sum of its own: polyphase_fir belongs to stages compiled with
// -ffp-contract=off, and the stages' own sums stay in their files.
#pragma once

#include <algorithm>
#include <type_traits>

#include "sdrg_internal.h"
#include "ssb_common.h"

namespace sdrg {
namespace {

// Outputs per tile workgroup: what `lds_samples` values of window hold in rows of an odd length, at most one output per
// thread, whole waves from 64 up.
inline int fir_tile_outputs(int lds_samples, int threads, int decim, int taps) {
    int max_row = lds_samples / decim;
    if ((max_row & 1) == 0) max_row--;
    const int t = std::min(threads, max_row - (taps + decim - 1) / decim + 1);
    return t > 64 ? t & ~63 : t;  // whole waves in the FIR phase
}

// The launcher's part of FirTileParams.  Refuses what no such stage takes: a decimation or a tap count outside its
// range, an even tap count, a first output outside the first decim samples, more outputs than the row holds, a last
// output whose newest sample lies outside the frame, and a window that does not fit lds_samples.  Otherwise fills
// tile, row and n_tiles and returns true.
inline bool fir_tile_plan(FirTileParams *p, int lds_samples, int threads, int max_decim, int max_taps) {
    if (p->decim < 1 || p->decim > max_decim || p->taps < 1 || p->taps > max_taps || (p->taps & 1) == 0 ||
        p->first < 0 || p->first >= p->decim || p->n_out < 0 || p->cap < 1 || p->n_out > p->cap ||
        (p->n_out > 0 && (int64_t)p->first + (int64_t)(p->n_out - 1) * p->decim >= p->n))
        return false;
    p->tile = fir_tile_outputs(lds_samples, threads, p->decim, p->taps);
    p->row = (p->tile - 1 + (p->taps + p->decim - 1) / p->decim) | 1;
    p->n_tiles = (p->n_out + p->tile - 1) / p->tile;
    return p->tile >= 1 && (int64_t)p->row * p->decim <= lds_samples;
}

// f(std::integral_constant<int, FMT>{}) for a raw-IQ format, where a launcher picks its kernel's instantiation; returns
// the format's bytes per sample, or 0 with f not called: no such format.
template <typename F>
int for_iq_format(int fmt, F f) {
    switch (fmt) {
    case SDRG_IQ_CS8: f(std::integral_constant<int, SDRG_IQ_CS8>{}); return bytes_per_sample<SDRG_IQ_CS8>();
    case SDRG_IQ_CU8: f(std::integral_constant<int, SDRG_IQ_CU8>{}); return bytes_per_sample<SDRG_IQ_CU8>();
    case SDRG_IQ_CS16: f(std::integral_constant<int, SDRG_IQ_CS16>{}); return bytes_per_sample<SDRG_IQ_CS16>();
    case SDRG_IQ_CF32: f(std::integral_constant<int, SDRG_IQ_CF32>{}); return bytes_per_sample<SDRG_IQ_CF32>();
    default: return 0;
    }
}

// What a stage writes per value: FirOut<FMT>::make(o) is o, or o clamped, scaled and rounded to int16; `pair` is two
// of them, stored as one word.  The stages' public out_format values are one pair under three names.
constexpr int FIR_OUT_S16 = 0, FIR_OUT_F32 = 1;
static_assert(SDRG_DEMOD_OUT_S16 == FIR_OUT_S16 && SDRG_SIDEBAND_OUT_S16 == FIR_OUT_S16 &&
                  SDRG_RESAMPLE_OUT_S16 == FIR_OUT_S16 && SDRG_DEMOD_OUT_F32 == FIR_OUT_F32 &&
                  SDRG_SIDEBAND_OUT_F32 == FIR_OUT_F32 && SDRG_RESAMPLE_OUT_F32 == FIR_OUT_F32,
              "one output trait: the three stages' out_format values are the same");
template <int FMT>
struct FirOut {
    typedef float type;
    typedef float pair __attribute__((ext_vector_type(2)));
    static __device__ __forceinline__ float make(float o) { return o; }
};
template <>
struct FirOut<FIR_OUT_S16> {
    typedef int16_t type;
    typedef short pair __attribute__((ext_vector_type(2)));
    static __device__ __forceinline__ int16_t make(float o) {
        return (int16_t)rintf(fminf(fmaxf(o, -1.0f), 1.0f) * 32767.0f);
    }
};

// Stream b's H values of the old history; nullptr (no old history: zeros) stays nullptr.
template <typename V>
__device__ __forceinline__ const V *stream_history(const float *hist_old, int b, int H) {
    return hist_old ? reinterpret_cast<const V *>(hist_old) + (size_t)b * (size_t)H : nullptr;
}

// The new history: element i is the value at t = N - H + i: at(t) for t >= 0, otherwise hist_old[t + H] (nullptr: 0).
template <int THREADS, typename V, typename At>
__device__ __forceinline__ void carry_history(V *hist_new, const V *hist_old, int N, int H, int tid, At at) {
    for (int i = tid; i < H; i += THREADS) {
        const int t = N - H + i;
        V v = V(0.0f);
        if (t >= 0)
            v = at(t);
        else if (hist_old)
            v = hist_old[t + H];
        hist_new[i] = v;
    }
}

// The last workgroup of stream b: the new history (a call without samples keeps the old one) and the zero tail of the
// stream's row of `out`, W values per output.
template <int THREADS, int W, typename V, typename O, typename At>
__device__ __forceinline__ void close_stream(float *hist_new, const V *hist_old, int b, int N, int H, O *orow, int n_out,
                                             int cap, int tid, At at) {
    if (N > 0)
        carry_history<THREADS>(reinterpret_cast<V *>(hist_new) + (size_t)b * (size_t)H, hist_old, N, H, tid, at);
    for (int j = n_out * W + tid; j < cap * W; j += THREADS) orow[j] = O(0);
}

// A tile workgroup's outputs [j0, j0 + nj) and the window of a filter of T = H + 1 values they read: `count` values
// from the local index w0, so that w0 + count - 1 is the last output's newest value.  P has tile, n_out, first, decim.
struct FirWindow {
    int j0, nj, w0, count;
    template <typename P>
    __device__ __forceinline__ FirWindow(const P &p, int T)
        : j0((int)blockIdx.x * p.tile), nj(min(p.tile, p.n_out - j0)), w0(p.first + j0 * p.decim - (T - 1)),
          count((nj - 1) * p.decim + T) {}
};

// The taps to LDS, ahead of the window.
template <int THREADS, typename C>
__device__ __forceinline__ void stage_taps(C *tap_lds, const C *taps, int T, int tid) {
    for (int i = tid; i < T; i += THREADS) tap_lds[i] = taps[i];
}

// Stages the window [w0, w0 + count) of a stream's raw IQ: window index u is local index t = w0 + u.  The sink stores:
//   sink.hist(u, v)             the history's value v (zeros: no history)
//   sink.sample(u, t, xr, xi)   the frame's sample t, unpacked
//   sink.chunk(u0, tc, w)       the whole 16-byte chunk w of the frame, its first sample tc at window index u0
template <int FMT, int THREADS, typename V, typename Sink>
__device__ __forceinline__ void stage_iq_window(const char *__restrict__ frame, const V *hist_old, int w0, int count,
                                                int H, bool vec_ok, int tid, const Sink &sink) {
    constexpr int BPS = bytes_per_sample<FMT>(), SPC = 16 / BPS;
    // the part before the frame: history (zeros after a restart)
    const int n_hist = min(max(-w0, 0), count);
    for (int u = tid; u < n_hist; u += THREADS) {
        V v = V(0.0f);
        if (hist_old) v = hist_old[w0 + u + H];
        sink.hist(u, v);
    }
    // the part inside the frame, in 16-byte chunks aligned in memory
    if (n_hist < count) {
        const int t_lo = w0 + n_hist, t_hi = w0 + count;  // [t_lo, t_hi) of the frame
        const uintptr_t a = reinterpret_cast<uintptr_t>(frame) + (size_t)t_lo * BPS;
        const int mis = vec_ok ? (int)((a & 15) / BPS) : 0;
        const int n_chunks = (t_hi - t_lo + mis + SPC - 1) / SPC;
        for (int c = tid; c < n_chunks; c += THREADS) {
            const int tc = t_lo - mis + c * SPC;  // the chunk's first sample
            if (vec_ok && tc >= t_lo && tc + SPC <= t_hi) {
                const uint4 raw = *reinterpret_cast<const uint4 *>(frame + (size_t)tc * BPS);
                const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
                sink.chunk(tc - w0, tc, w);
            } else {  // a chunk across an end of the window, or an iq base that is not sample-aligned
                for (int t = max(tc, t_lo); t < min(tc + SPC, t_hi); t++)
                    sink.sample(t - w0, t, load_i1<FMT>(frame, t), load_q1<FMT>(frame, t));
            }
        }
    }
}

// Eight taps from LDS, 16 bytes a read: floats four to a read, pairs (a tap per component) two.
__device__ __forceinline__ void read_taps8(const float *tap_lds, float (&h)[8]) {
    const float4 ha = *reinterpret_cast<const float4 *>(tap_lds);
    const float4 hb = *reinterpret_cast<const float4 *>(tap_lds + 4);
    h[0] = ha.x, h[1] = ha.y, h[2] = ha.z, h[3] = ha.w, h[4] = hb.x, h[5] = hb.y, h[6] = hb.z, h[7] = hb.w;
}
template <typename V>
__device__ __forceinline__ void read_taps8(const V *tap_lds, V (&c)[8]) {
#pragma unroll
    for (int i = 0; i < 8; i += 2) {
        const float4 cc = *reinterpret_cast<const float4 *>(tap_lds + i);
        c[i] = V{cc.x, cc.y};
        c[i + 1] = V{cc.z, cc.w};
    }
}

// Output `tid` of a tile: acc = acc + h[k] * v[u], u = tid D + (T - 1 - k), k ascending, v in the polyphase layout.  A
// tap C is a float, for every component of V, or a V (sideband.hip: a two-component vector type whose * and + work per
// component).  The taps come from LDS too (every lane reads the same address): as scalar loads from the kernel
// arguments they return through the counter the LDS reads use, out of order with them, so every group of reads waited
// for a scalar load's whole latency.
template <typename V, typename C>
__device__ __forceinline__ V polyphase_fir(const C *tap_lds, const V *smp, int T, int D, int row, int tid) {
    constexpr int AHEAD = 8;  // LDS reads in flight per lane: the sums are one chain, the reads are not
    const int H = T - 1;
    V acc = V(0.0f);
    int r = H % D;                         // wave-uniform: the row of tap k
    int at = (H % D) * row + H / D + tid;  // [u mod D][u / D] of this lane at k = 0
    const int wrap = (D - 1) * row - 1;
    int k = 0;
    for (; k + AHEAD <= T; k += AHEAD) {
        V v[AHEAD];
        C h[AHEAD];
        read_taps8(tap_lds + k, h);
#pragma unroll
        for (int i = 0; i < AHEAD; i++) {
            v[i] = smp[at];
            at += r == 0 ? wrap : -row;
            r = r == 0 ? D - 1 : r - 1;
        }
#pragma unroll
        for (int i = 0; i < AHEAD; i++) acc = acc + V(h[i]) * v[i];
    }
    for (; k < T; k++) {
        acc = acc + V(tap_lds[k]) * smp[at];
        at += r == 0 ? wrap : -row;
        r = r == 0 ? D - 1 : r - 1;
    }
    return acc;
}

}  // namespace
}  // namespace sdrg
