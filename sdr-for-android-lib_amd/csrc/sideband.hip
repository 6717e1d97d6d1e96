// sideband.hip — the sideband stage (sdrg_engine_sideband_*): per stream, a CF32 channel through a T-tap complex
// band-pass of which only the real part is formed, decimated by R: the upper sideband's audio, the lower's, or both
// (include/sdrg.h).
//
// The tile form of fir_tile.h (grid, history, staging, polyphase FIR) on the channel's samples as they are: H = T - 1,
// and the history holds the last T - 1 samples of the stream.  The stage's own:
//   the sums     Re(c * z) = cr zr - ci zi for the band-pass c = (cr, ci) around +fm, and cr zr + ci zi for its mirror
//                around -fm.  So the two real sums A = sum cr[k] zr and Bm = sum ci[k] zi serve both sidebands: one
//                packed multiply and one packed add per tap on the pair (polyphase_fir with a tap per component),
//                then u = A - Bm and l = A + Bm once per output.
//   the taps     pairs (cr, ci) in device memory (2 x 511 floats do not fit a kernel's arguments beside the
//                parameters), copied to LDS ahead of the window.
//   the output   one value per lane and output, or the pair (u, l) interleaved; the gain and the quantisation follow.
// No workgroup reads what another writes in the same launch.  Compiled with -ffp-contract=off: every product and sum
// is rounded on its own.
#include "fir_tile.h"
#include "sdrg_internal.h"

namespace sdrg {
namespace {

constexpr int SB_THREADS = 256;
constexpr int SB_LDS_SAMPLES = 3072;  // float2 of window per workgroup: 24 KiB (+ 4 KiB of taps)
constexpr int SB_TAP_SLOTS = 512;     // float2 slots the taps take at the start of the LDS

typedef float sb_f2 __attribute__((ext_vector_type(2)));

// stage_iq_window's sink: a sample goes to [u mod R][u / R] as it is
struct SbSink {
    sb_f2 *smp;
    int R, row;
    __device__ __forceinline__ void hist(int u, sb_f2 v) const { smp[(u % R) * row + u / R] = v; }
    __device__ __forceinline__ void sample(int u, int t, float xr, float xi) const { hist(u, sb_f2{xr, xi}); }
    // the chunk's two samples; [r][q] walks from the first to the second
    __device__ __forceinline__ void chunk(int u0, int tc, const uint32_t (&w)[4]) const {
        int r = u0 % R, q = u0 / R;
        smp[r * row + q] = sb_f2{__uint_as_float(w[0]), __uint_as_float(w[1])};
        if (++r == R) r = 0, q++;
        smp[r * row + q] = sb_f2{__uint_as_float(w[2]), __uint_as_float(w[3])};
    }
};

template <int MODE, int FMT>
__global__ __launch_bounds__(SB_THREADS) void sideband_kernel(const float2 *__restrict__ chan, SidebandParams p,
                                                              void *__restrict__ out) {
    typedef typename FirOut<FMT>::type out_t;
    typedef typename FirOut<FMT>::pair pair_t;
    constexpr int W = MODE == SDRG_SIDEBAND_BOTH ? 2 : 1;  // values per output
    extern __shared__ __attribute__((aligned(16))) sb_f2 sb_lds[];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int N = p.n, R = p.decim, T = p.taps, H = T - 1;
    const float2 *row = chan + (size_t)b * (size_t)p.in_stride;
    const sb_f2 *hist_old = stream_history<sb_f2>(p.hist_old, b, H);
    out_t *orow = static_cast<out_t *>(out) + (size_t)b * (size_t)p.cap * W;

    if ((int)blockIdx.x == p.n_tiles) {
        close_stream<SB_THREADS, W>(p.hist_new, hist_old, b, N, H, orow, p.n_out, p.cap, tid,
                                    [&](int t) {
                                        const float2 z = row[t];
                                        return sb_f2{z.x, z.y};
                                    });
        return;
    }

    const FirWindow w(p, T);
    sb_f2 *tap_lds = sb_lds, *smp = sb_lds + SB_TAP_SLOTS;
    stage_taps<SB_THREADS>(tap_lds, reinterpret_cast<const sb_f2 *>(p.taps_dev), T, tid);
    stage_iq_window<SDRG_IQ_CF32, SB_THREADS>(reinterpret_cast<const char *>(row), hist_old, w.w0, w.count, H, p.vec_ok,
                                              tid, SbSink{smp, R, p.row});
    __syncthreads();

    if (tid < w.nj) {
        const sb_f2 acc = polyphase_fir(tap_lds, smp, T, R, p.row, tid);
        const float u = acc.x - acc.y, l = acc.x + acc.y;
        const int j = w.j0 + tid;
        if constexpr (MODE == SDRG_SIDEBAND_BOTH) {
            const out_t ou = FirOut<FMT>::make(u * p.gain), ol = FirOut<FMT>::make(l * p.gain);
            if (p.pair_ok) {  // out aligned to a pair: one store
                pair_t o;
                o.x = ou, o.y = ol;
                reinterpret_cast<pair_t *>(orow)[j] = o;
            } else {
                orow[2 * j] = ou;
                orow[2 * j + 1] = ol;
            }
        } else {
            orow[j] = FirOut<FMT>::make((MODE == SDRG_SIDEBAND_UPPER ? u : l) * p.gain);
        }
    }
}

template <int MODE>
void (*sideband_kernel_for(int fmt))(const float2 *, SidebandParams, void *) {
    return fmt == SDRG_SIDEBAND_OUT_F32 ? sideband_kernel<MODE, SDRG_SIDEBAND_OUT_F32>
                                        : sideband_kernel<MODE, SDRG_SIDEBAND_OUT_S16>;
}

}  // namespace

int sideband_tile_outputs(int decim, int taps) { return fir_tile_outputs(SB_LDS_SAMPLES, SB_THREADS, decim, taps); }

hipError_t launch_sideband(const float *chan, int n_streams, const SidebandParams &p0, void *out, hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    SidebandParams p = p0;
    if (!out || !p.taps_dev || p.n < 0 || p.n > SDRG_SIDEBAND_MAX_IN ||
        (p.mode != SDRG_SIDEBAND_UPPER && p.mode != SDRG_SIDEBAND_LOWER && p.mode != SDRG_SIDEBAND_BOTH) ||
        (p.out_format != SDRG_SIDEBAND_OUT_S16 && p.out_format != SDRG_SIDEBAND_OUT_F32) || n_streams > 65535)
        return hipErrorInvalidValue;
    if (p.n > 0 && (!chan || p.in_stride < p.n || (p.taps > 1 && !p.hist_new))) return hipErrorInvalidValue;
    if (reinterpret_cast<uintptr_t>(chan) % sizeof(float) != 0) return hipErrorInvalidValue;
    if (!fir_tile_plan(&p, SB_LDS_SAMPLES, SB_THREADS, SDRG_SIDEBAND_MAX_DECIMATION, SDRG_SIDEBAND_MAX_TAPS))
        return hipErrorInvalidValue;
    // rows of whole samples from a sample-aligned base: no sample straddles a 16-byte chunk
    p.vec_ok = reinterpret_cast<uintptr_t>(chan) % sizeof(float2) == 0;
    const size_t value = p.out_format == SDRG_SIDEBAND_OUT_F32 ? sizeof(float) : sizeof(int16_t);
    p.pair_ok = reinterpret_cast<uintptr_t>(out) % (2 * value) == 0;
    void (*k)(const float2 *, SidebandParams, void *) = sideband_kernel_for<SDRG_SIDEBAND_BOTH>(p.out_format);
    if (p.mode == SDRG_SIDEBAND_UPPER) k = sideband_kernel_for<SDRG_SIDEBAND_UPPER>(p.out_format);
    if (p.mode == SDRG_SIDEBAND_LOWER) k = sideband_kernel_for<SDRG_SIDEBAND_LOWER>(p.out_format);
    const size_t lds = sizeof(float) * 2 * ((size_t)p.row * (size_t)p.decim + SB_TAP_SLOTS);
    hipLaunchKernelGGL(k, dim3((unsigned)p.n_tiles + 1, (unsigned)n_streams), dim3(SB_THREADS), lds, stream,
                       reinterpret_cast<const float2 *>(chan), p, out);
    return hipGetLastError();
}

}  // namespace sdrg
