// fir_tile.h — the tile form the decimating stages share (ddc.hip, demod.hip's FIR kernel, channelizer.hip, sideband.hip;
// resample.hip takes its grid and carry_history, and has a filter phase per output in place of the polyphase layout below).
//
// A stage filters each stream with a window of H + 1 values and decimates by D.  A call's outputs j in [0, n_out) read
// the values at the local indices t = first + j D - k, k in [0, H]; t in [0, N) is this call's frame, t in [-H, 0) the
// history (the H values before the frame, zeros after a restart), kept per stream in one half of a ping-pong buffer
// (decim_cursor.h has the host's side: first, n_out, the halves).
//   grid         (tiles of outputs + 1, streams).  A tile workgroup stages the (nj - 1) D + H + 1 values its nj outputs
//                read into LDS, then computes them.  The last workgroup of a stream (blockIdx.x == n_tiles) writes the new
//                history, the values at t in [N - H, N), into the other half (carry_history), and the zero tail of
//                `out`: no workgroup reads what another writes in the same launch.
//   staging      of raw IQ (stage_iq_window): indices below 0 from the history, then the frame in 16-byte chunks aligned
//                in memory, one uint4 load each; the chunks the window covers only in part, at its ends, and every chunk
//                of a base that is not sample-aligned, sample by sample.  Both unpack as load_i1 / load_q1 of
//                ssb_common.h.  Where a value lands in LDS, and what is done to it first, is the stage's (its sink).
//   FIR          (polyphase_fir; polyphase_fir_pairwise for a tap per component) one output per lane from the polyphase
//                layout [u mod D][u / D], rows of `row` (odd) values: at tap k lane j reads u = j D + (H - k), one row for the whole wave and consecutive columns for
//                consecutive lanes, so the reads are conflict-free for every D (a linear layout puts the lanes D values
//                apart: gcd(D, 32)-way conflicts), and the row base moves by scalar arithmetic only.
// Nothing here sets the contraction mode of a sum of its own: polyphase_fir belongs to stages compiled with
// -ffp-contract=off, and the stages' own sums stay in their files.
#pragma once

#include <algorithm>
#include <type_traits>

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

// The new history: element i is the value at t = N - H + i, at(t) for t >= 0, otherwise hist_old[t + H] (nullptr: zero).
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

// Output `tid` of a tile: acc = acc + h[k] * v[u], u = tid D + (T - 1 - k), k ascending, v in the polyphase layout.  The
// taps come from LDS too (one 16-byte read of the same address by every lane per four taps): as scalar loads from the
// kernel arguments they return through the counter the LDS reads use, out of order with them, so every group of reads
// waited for a scalar load's whole latency.
template <typename V>
__device__ __forceinline__ V polyphase_fir(const float *tap_lds, const V *smp, int T, int D, int row, int tid) {
    constexpr int AHEAD = 8;  // LDS reads in flight per lane: the sums are one chain, the reads are not
    const int H = T - 1;
    V acc = V(0.0f);
    int r = H % D;                         // wave-uniform: the row of tap k
    int at = (H % D) * row + H / D + tid;  // [u mod D][u / D] of this lane at k = 0
    const int wrap = (D - 1) * row - 1;
    int k = 0;
    for (; k + AHEAD <= T; k += AHEAD) {
        V v[AHEAD];
        const float4 ha = *reinterpret_cast<const float4 *>(tap_lds + k);
        const float4 hb = *reinterpret_cast<const float4 *>(tap_lds + k + 4);
        const float h[AHEAD] = {ha.x, ha.y, ha.z, ha.w, hb.x, hb.y, hb.z, hb.w};
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

// polyphase_fir's sibling for a tap per component (sideband.hip): acc = acc + c[k] * v[u] on the pairs, component by
// component, the same u, order and layout.  The taps are pairs in LDS too, two to a 16-byte read.  V is a two-component
// vector type whose * and + work per component.
template <typename V>
__device__ __forceinline__ V polyphase_fir_pairwise(const V *tap_lds, const V *smp, int T, int D, int row, int tid) {
    constexpr int AHEAD = 8;  // LDS reads in flight per lane, as above
    const int H = T - 1;
    V acc = V(0.0f);
    int r = H % D;
    int at = (H % D) * row + H / D + tid;
    const int wrap = (D - 1) * row - 1;
    int k = 0;
    for (; k + AHEAD <= T; k += AHEAD) {
        V v[AHEAD], c[AHEAD];
#pragma unroll
        for (int i = 0; i < AHEAD; i += 2) {
            const float4 cc = *reinterpret_cast<const float4 *>(tap_lds + k + i);
            c[i] = V{cc.x, cc.y};
            c[i + 1] = V{cc.z, cc.w};
        }
#pragma unroll
        for (int i = 0; i < AHEAD; i++) {
            v[i] = smp[at];
            at += r == 0 ? wrap : -row;
            r = r == 0 ? D - 1 : r - 1;
        }
#pragma unroll
        for (int i = 0; i < AHEAD; i++) acc = acc + c[i] * v[i];
    }
    for (; k < T; k++) {
        acc = acc + tap_lds[k] * smp[at];
        at += r == 0 ? wrap : -row;
        r = r == 0 ? D - 1 : r - 1;
    }
    return acc;
}

}  // namespace
}  // namespace sdrg
