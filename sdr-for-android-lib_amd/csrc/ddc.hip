// ddc.hip — the DDC stage (sdrg_engine_ddc_*): per stream, the raw IQ mixed down by a phase-continuous NCO, filtered by
// a T-tap FIR and decimated by D, written as CF32 (include/sdrg.h).
//
// Grid (tiles of outputs + 1, streams).  A call's outputs j in [0, n_out) read the mixed samples at the local indices
// t = first + j D - k, k in [0, T); t in [0, N) is this frame, t in [-(T - 1), 0) the history (the T - 1 mixed samples
// before the frame, zeros after a restart).
//   phasors      every stream sees the same NCO phase at sample t, so a first small kernel writes the frame's N phasors
//                w[t] = hi[ph >> 22] * lo[(ph >> 12) & 1023] (nco_mix's products and order) once, and the tiles read
//                them as consecutive 8-byte words.  Looking both tables up per sample in every tile made the staging
//                alone 253 us at 4096 x 16384 CS8 (the hi entries of neighbouring samples are inc >> 22 entries apart:
//                one cache line per lane and load); DESIGN.md §3.12 has both measurements.
//   tile block   `tile` consecutive outputs.  The workgroup stages the (nj - 1) D + T mixed samples its outputs read
//                into LDS: raw samples in aligned 16-byte loads (the chunks the window covers only in part, at its ends,
//                sample by sample), unpacked as load_i1 / load_q1 of ssb_common.h and multiplied by w[t]; indices below
//                0 come from the history.  Then one output per lane, k ascending: one packed multiply and one packed
//                add per tap on the (re, im) pair, the LDS reads of eight taps (and the taps themselves, kept in LDS
//                too) issued ahead of their sums.
//   LDS layout   polyphase: the window's sample u at [u mod D][u / D], rows of `row` (odd) float2.  At tap k lane j
//                reads u = j D + (T - 1 - k): one row for the whole wave, consecutive columns for consecutive lanes, so
//                the 8-byte reads are conflict-free for every D by construction (a linear layout puts the lanes D * 8
//                bytes apart: gcd(D, 32)-way conflicts).  The row base moves by scalar arithmetic only.
//   last block   (blockIdx.x == n_tiles) writes the stream's new history, the mixed samples at t in [N - (T - 1), N)
//                (re-mixed from the frame, or shifted from the old history where t < 0), into the other half of the
//                ping-pong buffer, and zeroes the entries of `out` from n_out to cap: no workgroup reads what another
//                writes in the same launch.
// Compiled with -ffp-contract=off: every product and sum of the mix and the FIR is rounded on its own.
#include <algorithm>

#include "sdrg_internal.h"
#include "ssb_common.h"

namespace sdrg {
namespace {

constexpr int DDC_THREADS = 256;
#ifndef DDC_LAB_LDS_SAMPLES
#define DDC_LAB_LDS_SAMPLES 3072
#endif
// float2 of window per workgroup: 24 KiB (+ 2 KiB of taps), six workgroups per CU (a lab build may override it)
constexpr int DDC_LDS_SAMPLES = DDC_LAB_LDS_SAMPLES;

constexpr int DDC_TAP_SLOTS = 256;     // float2 slots the taps take at the start of the LDS (512 floats)

typedef float ddc_f2 __attribute__((ext_vector_type(2)));

// w[t] = hi[ph >> 22] * lo[(ph >> 12) & 1023], ph = inc * (g0_lo + t): nco_mix's products and order
__global__ __launch_bounds__(DDC_THREADS) void ddc_phasor_kernel(const float2 *__restrict__ tab, uint32_t inc,
                                                                 uint32_t g0_lo, int n, float2 *__restrict__ w) {
    const int t = (int)blockIdx.x * DDC_THREADS + (int)threadIdx.x;
    if (t >= n) return;
    const uint32_t ph = inc * (g0_lo + (uint32_t)t);
    const float2 h = tab[ph >> 22];
    const float2 l = tab[1024 + ((ph >> 12) & 1023)];
    w[t] = make_float2(h.x * l.x - h.y * l.y, h.x * l.y + h.y * l.x);
}

// (xr + j xi) * w: nco_mix's products and order, and the imaginary part
__device__ __forceinline__ ddc_f2 ddc_mix(float2 w, float xr, float xi) {
    ddc_f2 v;
    v.x = xr * w.x - xi * w.y;
    v.y = xr * w.y + xi * w.x;
    return v;
}

template <int FMT>
__device__ __forceinline__ ddc_f2 ddc_sample(const DdcParams &p, const char *__restrict__ frame, int t) {
    return ddc_mix(reinterpret_cast<const float2 *>(p.phasors)[t], load_i1<FMT>(frame, t), load_q1<FMT>(frame, t));
}

// sample s of a 16-byte chunk (8, 4 or 2 samples by format), the expressions of load_i1 / load_q1
template <int FMT>
__device__ __forceinline__ void ddc_unpack(const uint32_t (&w)[4], int s, float &xr, float &xi) {
    if constexpr (FMT == SDRG_IQ_CS8) {
        const uint32_t h = w[s >> 1] >> (16 * (s & 1));
        xr = (float)(int8_t)(h & 0xff) * (1.0f / 128.0f);
        xi = (float)(int8_t)((h >> 8) & 0xff) * (1.0f / 128.0f);
    } else if constexpr (FMT == SDRG_IQ_CU8) {
        const uint32_t h = w[s >> 1] >> (16 * (s & 1));
        xr = ((float)(h & 0xff) - 127.4f) * (1.0f / 128.0f);
        xi = ((float)((h >> 8) & 0xff) - 127.4f) * (1.0f / 128.0f);
    } else if constexpr (FMT == SDRG_IQ_CS16) {
        xr = (float)(int16_t)(w[s] & 0xffff) * (1.0f / 32768.0f);
        xi = (float)(int16_t)(w[s] >> 16) * (1.0f / 32768.0f);
    } else {
        xr = __uint_as_float(w[2 * s]);
        xi = __uint_as_float(w[2 * s + 1]);
    }
}

template <int FMT>
__global__ __launch_bounds__(DDC_THREADS) void ddc_kernel(const char *__restrict__ iq, DdcParams p, DdcTaps taps,
                                                          float *__restrict__ out) {
    constexpr int BPS = bytes_per_sample<FMT>(), SPC = 16 / BPS;
    extern __shared__ __attribute__((aligned(16))) ddc_f2 ddc_lds[];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int N = p.n, D = p.decim, T = p.taps, H = T - 1;
    const char *frame = iq + (size_t)b * (size_t)N * BPS;
    const ddc_f2 *hist_old = p.hist_old ? reinterpret_cast<const ddc_f2 *>(p.hist_old) + (size_t)b * (size_t)H : nullptr;
    ddc_f2 *orow = reinterpret_cast<ddc_f2 *>(out) + (size_t)b * (size_t)p.cap;

    if ((int)blockIdx.x == p.n_tiles) {  // the new history and the zero tail of out
        ddc_f2 *hist_new = reinterpret_cast<ddc_f2 *>(p.hist_new) + (size_t)b * (size_t)H;
        for (int i = tid; i < H; i += DDC_THREADS) {
            const int t = N - H + i;
            ddc_f2 v = {0.0f, 0.0f};
            if (t >= 0)
                v = ddc_sample<FMT>(p, frame, t);
            else if (hist_old)
                v = hist_old[t + H];
            hist_new[i] = v;
        }
        for (int j = p.n_out + tid; j < p.cap; j += DDC_THREADS) orow[j] = ddc_f2{0.0f, 0.0f};
        return;
    }

    const int j0 = (int)blockIdx.x * p.tile, nj = min(p.tile, p.n_out - j0);
    const int w0 = p.first + j0 * D - H;     // local index of the window's first sample
    const int count = (nj - 1) * D + T;      // samples in the window: w0 + count - 1 = the last output's newest sample
    const int row = p.row;
    float *tap_lds = reinterpret_cast<float *>(ddc_lds);  // the taps, then the window
    ddc_f2 *smp = ddc_lds + DDC_TAP_SLOTS;
    for (int i = tid; i < T; i += DDC_THREADS) tap_lds[i] = taps.h[i];

    // the part before the frame: history (zeros after a restart)
    const int n_hist = min(max(-w0, 0), count);
    for (int u = tid; u < n_hist; u += DDC_THREADS) {
        ddc_f2 v = {0.0f, 0.0f};
        if (hist_old) v = hist_old[w0 + u + H];
        smp[(u % D) * row + u / D] = v;
    }
    // the part inside the frame, in 16-byte chunks aligned in memory
    if (n_hist < count) {
        const int t_lo = w0 + n_hist, t_hi = w0 + count;  // [t_lo, t_hi) of the frame
        const uintptr_t a = reinterpret_cast<uintptr_t>(frame) + (size_t)t_lo * BPS;
        const int mis = p.vec_ok ? (int)((a & 15) / BPS) : 0;
        const int n_chunks = (t_hi - t_lo + mis + SPC - 1) / SPC;
        for (int c = tid; c < n_chunks; c += DDC_THREADS) {
            const int tc = t_lo - mis + c * SPC;  // the chunk's first sample
            if (p.vec_ok && tc >= t_lo && tc + SPC <= t_hi) {
                const uint4 raw = *reinterpret_cast<const uint4 *>(frame + (size_t)tc * BPS);
                const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
                const float2 *pw = reinterpret_cast<const float2 *>(p.phasors) + tc;
                float2 ws[SPC];
#pragma unroll
                for (int s = 0; s < SPC; s++) ws[s] = pw[s];
                const int u0 = tc - w0;
                int r = u0 % D, q = u0 / D;
#pragma unroll
                for (int s = 0; s < SPC; s++) {
                    float xr, xi;
                    ddc_unpack<FMT>(w, s, xr, xi);
                    smp[r * row + q] = ddc_mix(ws[s], xr, xi);
                    if (++r == D) r = 0, q++;
                }
            } else {  // a chunk across an end of the window, or an iq base that is not sample-aligned
                for (int t = max(tc, t_lo); t < min(tc + SPC, t_hi); t++) {
                    const int u = t - w0;
                    smp[(u % D) * row + u / D] = ddc_sample<FMT>(p, frame, t);
                }
            }
        }
    }
    __syncthreads();

    // output j0 + tid: acc = acc + h[k] * v[u], u = tid D + (T - 1 - k), k ascending.  The taps come from LDS too (one
    // 16-byte read of the same address by every lane per four taps): as scalar loads from the kernel arguments they
    // return through the counter the LDS reads use, out of order with them, so every group of reads waited for a scalar
    // load's whole latency.
    if (tid < nj) {
        constexpr int AHEAD = 8;  // LDS reads in flight per lane: the sums are one chain, the reads are not
        ddc_f2 acc = {0.0f, 0.0f};
        int r = H % D;                           // wave-uniform: the row of tap k
        int at = (H % D) * row + H / D + tid;    // [u mod D][u / D] of this lane at k = 0
        const int wrap = (D - 1) * row - 1;
        int k = 0;
        for (; k + AHEAD <= T; k += AHEAD) {
            ddc_f2 v[AHEAD];
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
            for (int i = 0; i < AHEAD; i++) acc = acc + ddc_f2{h[i], h[i]} * v[i];
        }
        for (; k < T; k++) {
            const float h = tap_lds[k];
            acc = acc + ddc_f2{h, h} * smp[at];
            at += r == 0 ? wrap : -row;
            r = r == 0 ? D - 1 : r - 1;
        }
        orow[j0 + tid] = acc;
    }
}

}  // namespace

int ddc_tile_outputs(int decim, int taps) {
    int max_row = DDC_LDS_SAMPLES / decim;
    if ((max_row & 1) == 0) max_row--;
    const int t = std::min(DDC_THREADS, max_row - (taps + decim - 1) / decim + 1);
    return t > 64 ? t & ~63 : t;  // whole waves in the FIR phase
}

hipError_t launch_ddc(const void *iq, int fmt, int n_streams, const DdcParams &p0, const DdcTaps &taps, float *out,
                      hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    DdcParams p = p0;
    if (!iq || !out || !p.nco_tab || !p.phasors || p.n < 1 || p.n > (1 << 20) || p.decim < 1 || p.decim > SDRG_DDC_MAX_DECIMATION ||
        p.taps < 1 || p.taps > SDRG_DDC_MAX_TAPS || (p.taps & 1) == 0 || (p.taps > 1 && !p.hist_new) || p.first < 0 ||
        p.first >= p.decim || p.n_out < 0 || p.cap != (p.n + p.decim - 1) / p.decim || p.n_out > p.cap ||
        (p.n_out > 0 && (int64_t)p.first + (int64_t)(p.n_out - 1) * p.decim >= p.n) || n_streams > 65535)
        return hipErrorInvalidValue;
    p.tile = ddc_tile_outputs(p.decim, p.taps);
    p.row = (p.tile - 1 + (p.taps + p.decim - 1) / p.decim) | 1;
    p.n_tiles = (p.n_out + p.tile - 1) / p.tile;
    if (p.tile < 1 || (int64_t)p.row * p.decim > DDC_LDS_SAMPLES) return hipErrorInvalidValue;
    int bps;
    void (*k)(const char *, DdcParams, DdcTaps, float *);
    switch (fmt) {
    case SDRG_IQ_CS8: k = ddc_kernel<SDRG_IQ_CS8>, bps = 2; break;
    case SDRG_IQ_CU8: k = ddc_kernel<SDRG_IQ_CU8>, bps = 2; break;
    case SDRG_IQ_CS16: k = ddc_kernel<SDRG_IQ_CS16>, bps = 4; break;
    case SDRG_IQ_CF32: k = ddc_kernel<SDRG_IQ_CF32>, bps = 8; break;
    default: return hipErrorInvalidValue;
    }
    // rows of whole samples from a sample-aligned base: no sample straddles a 16-byte chunk
    p.vec_ok = reinterpret_cast<uintptr_t>(iq) % (size_t)bps == 0;
    const size_t lds = sizeof(float) * 2 * ((size_t)p.row * (size_t)p.decim + DDC_TAP_SLOTS);
    hipLaunchKernelGGL(ddc_phasor_kernel, dim3((unsigned)((p.n + DDC_THREADS - 1) / DDC_THREADS)), dim3(DDC_THREADS), 0,
                       stream, reinterpret_cast<const float2 *>(p.nco_tab), p.inc, p.g0_lo, p.n,
                       reinterpret_cast<float2 *>(p.phasors));
    hipError_t er = hipGetLastError();
    if (er != hipSuccess) return er;
    hipLaunchKernelGGL(k, dim3((unsigned)p.n_tiles + 1, (unsigned)n_streams), dim3(DDC_THREADS), lds, stream,
                       static_cast<const char *>(iq), p, taps, out);
    return hipGetLastError();
}

}  // namespace sdrg
