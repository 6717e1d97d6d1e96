// ddc.hip — the DDC stage (sdrg_engine_ddc_*): per stream, the raw IQ mixed down by a phase-continuous NCO, filtered by
// a T-tap FIR and decimated by D, written as CF32 (include/sdrg.h).
//
// The tile form of fir_tile.h (grid, history, staging, polyphase FIR) on the mixed samples: H = T - 1, and the history
// holds mixed samples.  The stage's own:
//   phasors      every stream sees the same NCO phase at sample t, so a first small kernel writes the frame's N phasors
//                w[t] = hi[ph >> 22] * lo[(ph >> 12) & 1023] (nco_mix's products and order) once, and the tiles read
//                them as consecutive 8-byte words.  Looking both tables up per sample in every tile made the staging
//                alone 253 us at 4096 x 16384 CS8 (the hi entries of neighbouring samples are inc >> 22 entries apart:
//                one cache line per lane and load); DESIGN.md §3.12 has both measurements.
//   the mix      a staged sample is multiplied by w[t] on its way into LDS (DdcSink); the last block re-mixes the frame's
//                last T - 1 samples for the new history.
//   the sums     one packed multiply and one packed add per tap on the (re, im) pair.
// Compiled with -ffp-contract=off: every product and sum of the mix and the FIR is rounded on its own.
#include "fir_tile.h"
#include "sdrg_internal.h"

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

// stage_iq_window's sink: a sample is mixed by its phasor and goes to [u mod D][u / D]
template <int FMT>
struct DdcSink {
    ddc_f2 *smp;
    const float2 *phasors;
    int D, row;
    __device__ __forceinline__ void hist(int u, ddc_f2 v) const { smp[(u % D) * row + u / D] = v; }
    __device__ __forceinline__ void sample(int u, int t, float xr, float xi) const { hist(u, ddc_mix(phasors[t], xr, xi)); }
    // the chunk's phasors are loaded ahead of the unpack, and [r][q] walks from sample to sample
    __device__ __forceinline__ void chunk(int u0, int tc, const uint32_t (&w)[4]) const {
        constexpr int SPC = 16 / bytes_per_sample<FMT>();
        const float2 *pw = phasors + tc;
        float2 ws[SPC];
#pragma unroll
        for (int s = 0; s < SPC; s++) ws[s] = pw[s];
        int r = u0 % D, q = u0 / D;
#pragma unroll
        for (int s = 0; s < SPC; s++) {
            float xr, xi;
            iq_chunk_unpack<FMT>(w, s, xr, xi);
            smp[r * row + q] = ddc_mix(ws[s], xr, xi);
            if (++r == D) r = 0, q++;
        }
    }
};

template <int FMT>
__global__ __launch_bounds__(DDC_THREADS) void ddc_kernel(const char *__restrict__ iq, DdcParams p, DdcTaps taps,
                                                          float *__restrict__ out) {
    constexpr int BPS = bytes_per_sample<FMT>();
    extern __shared__ __attribute__((aligned(16))) ddc_f2 ddc_lds[];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int N = p.n, D = p.decim, T = p.taps, H = T - 1;
    const char *frame = iq + (size_t)b * (size_t)N * BPS;
    const ddc_f2 *hist_old = stream_history<ddc_f2>(p.hist_old, b, H);
    const float2 *phasors = reinterpret_cast<const float2 *>(p.phasors);
    ddc_f2 *orow = reinterpret_cast<ddc_f2 *>(out) + (size_t)b * (size_t)p.cap;

    if ((int)blockIdx.x == p.n_tiles) {  // the new history is re-mixed from the frame
        close_stream<DDC_THREADS, 1>(p.hist_new, hist_old, b, N, H, orow, p.n_out, p.cap, tid,
                                     [&](int t) {
                                         return ddc_mix(phasors[t], load_i1<FMT>(frame, t), load_q1<FMT>(frame, t));
                                     });
        return;
    }

    const FirWindow w(p, T);
    float *tap_lds = reinterpret_cast<float *>(ddc_lds);  // the taps, then the window
    ddc_f2 *smp = ddc_lds + DDC_TAP_SLOTS;
    stage_taps<DDC_THREADS>(tap_lds, taps.h, T, tid);
    stage_iq_window<FMT, DDC_THREADS>(frame, hist_old, w.w0, w.count, H, p.vec_ok, tid,
                                      DdcSink<FMT>{smp, phasors, D, p.row});
    __syncthreads();

    if (tid < w.nj) orow[w.j0 + tid] = polyphase_fir(tap_lds, smp, T, D, p.row, tid);
}

}  // namespace

int ddc_tile_outputs(int decim, int taps) { return fir_tile_outputs(DDC_LDS_SAMPLES, DDC_THREADS, decim, taps); }

hipError_t launch_ddc(const void *iq, int fmt, int n_streams, const DdcParams &p0, const DdcTaps &taps, float *out,
                      hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    DdcParams p = p0;
    if (!iq || !out || !p.nco_tab || !p.phasors || p.n < 1 || p.n > (1 << 20) || (p.taps > 1 && !p.hist_new) ||
        n_streams > 65535 ||
        !fir_tile_plan(&p, DDC_LDS_SAMPLES, DDC_THREADS, SDRG_DDC_MAX_DECIMATION, SDRG_DDC_MAX_TAPS) ||
        p.cap != (p.n + p.decim - 1) / p.decim)  // the rows are as long as the frame's outputs can be
        return hipErrorInvalidValue;
    void (*k)(const char *, DdcParams, DdcTaps, float *) = nullptr;
    const int bps = for_iq_format(fmt, [&](auto f) { k = ddc_kernel<decltype(f)::value>; });
    if (bps == 0) return hipErrorInvalidValue;
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
