// demod.hip — the demodulator stage (sdrg_engine_demod_*): per stream, a CF32 channel through an AM or FM detector, a
// DC block, a de-emphasis, a T2-tap real FIR decimating by R, a gain and the quantisation to int16 or float
// (include/sdrg.h).  Three launches per call:
//   detector     grid (tiles of 256 samples, streams), one sample per lane, one coalesced 8-byte load each.  FM needs the
//                previous sample: the neighbouring lane's (one DPP move per component), and in lane 0 of a wave a second
//                load, or the stream's state at sample 0.  Writes e to the scratch row, and the call's last sample to
//                the new state.
//   recurrences  (only if the DC block or the de-emphasis is on) the two chains are serial in the sample index and their
//                roundings are specified, so a stream is one lane.  A workgroup is one wave and takes DEMOD_GROUP = 16
//                streams: the kernel's time is the chain's latency whatever B is, and what a wave adds per step is its
//                rows' loads and stores, so fewer rows on more CUs are faster (4096 x 16384: 1412, 805, 548, 477 us at
//                64, 32, 16, 8 streams per wave).  The scratch moves through LDS in tiles of
//                [DEMOD_GROUP streams][DEMOD_CHUNK samples], rows of DEMOD_CHUNK + 1 dwords: all 64 lanes load and
//                store whole rows (256 contiguous bytes per instruction, LDS banks lane), and lane l < DEMOD_GROUP
//                walks row l (banks (l + j) mod 32: no conflicts).  The loads of the next tile are issued before the
//                chain of this one.  In place: a workgroup reads and writes the rows of its own streams only.
//   FIR          the tile form of fir_tile.h (grid, history, polyphase FIR) on the real values v of the scratch row,
//                H = T2 - 1: the workgroup stages the (nj - 1) R + T2 values its outputs read one per lane and step, the
//                polyphase position advanced without a division; the gain and the quantisation follow the sum.
// No workgroup reads what another writes in the same launch.  Compiled with -ffp-contract=off: every product, sum,
// quotient and root is rounded on its own; `/` and sqrtf are the compiler's correctly rounded, denormal-keeping
// sequences (tests/cpp/demod_math.hip checks them against IEEE on the device).
#include "fir_tile.h"
#include "sdrg_internal.h"

namespace sdrg {
namespace {

constexpr int DEMOD_THREADS = 256;
constexpr int DEMOD_LDS_SAMPLES = 6144;  // floats of window per FIR workgroup: 24 KiB (+ 1 KiB of taps)
constexpr int DEMOD_TAP_SLOTS = 256;     // floats the taps take at the start of the LDS
#ifndef DEMOD_LAB_GROUP
#define DEMOD_LAB_GROUP 16
#endif
constexpr int DEMOD_GROUP = DEMOD_LAB_GROUP;  // streams per wave of the recurrence kernel (a lab build may override it)
constexpr int DEMOD_WAVE = 64;
constexpr int DEMOD_ROW = DEMOD_CHUNK + 1;

// sdrg_atan2f of sdrg.h, operation by operation
__device__ __forceinline__ float demod_atan2f(float y, float x) {
    const float ax = fabsf(x), ay = fabsf(y);
    const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
    const float q = mx > 0.0f ? mn / mx : 0.0f;
    const float s = q * q;
    float p = -0x1.0bce58p-8f;
    p = p * s + 0x1.68671ep-6f;
    p = p * s + -0x1.cbe51p-5f;
    p = p * s + 0x1.8bc022p-4f;
    p = p * s + -0x1.1d09a6p-3f;
    p = p * s + 0x1.988d5p-3f;
    p = p * s + -0x1.554ce6p-2f;
    p = p * s + 0x1.ffffecp-1f;
    float r = p * q;
    if (ay > ax) r = 0x1.921fb6p+0f - r;
    if (__float_as_uint(x) >> 31) r = 0x1.921fb6p+1f - r;
    return copysignf(r, y);
}

template <int MODE>
__global__ __launch_bounds__(DEMOD_THREADS) void demod_detect_kernel(const float2 *__restrict__ chan, DemodParams p) {
    const int tid = threadIdx.x, b = blockIdx.y;
    const int i = (int)blockIdx.x * DEMOD_THREADS + tid;
    const float2 *row = chan + (size_t)b * (size_t)p.in_stride;
    const bool valid = i < p.n;
    float2 z = make_float2(0.0f, 0.0f);
    if (valid) z = row[i];
    float e;
    if constexpr (MODE == SDRG_DEMOD_FM) {
        float2 w;
        w.x = __shfl_up(z.x, 1);
        w.y = __shfl_up(z.y, 1);
        bool none = false;  // global index 0: no previous sample
        if ((tid & 63) == 0) {
            if (i == 0) {
                none = p.fresh != 0;
                w = none ? make_float2(0.0f, 0.0f) : reinterpret_cast<const float2 *>(p.state_old)[2 * (size_t)b];
            } else if (valid) {
                w = row[i - 1];
            }
        }
        const float pr = z.x * w.x + z.y * w.y;
        const float pi = z.y * w.x - z.x * w.y;
        e = none ? 0.0f : demod_atan2f(pi, pr) * p.kf;
    } else {
        e = sqrtf(z.x * z.x + z.y * z.y);
    }
    if (valid) p.scratch[(size_t)b * (size_t)p.scratch_stride + (size_t)i] = e;
    if (i == p.n - 1) reinterpret_cast<float2 *>(p.state_new)[2 * (size_t)b] = z;
}

// one step of the two chains: e in, v out
template <bool DC, bool DE>
__device__ __forceinline__ float demod_step(float e, float &m, float &s, float alpha, float a) {
    float u = e;
    if constexpr (DC) {
        u = e - m;
        m = m + alpha * u;
    }
    if constexpr (DE) {
        const float t = u - s;
        s = s + a * t;
        return s;
    }
    return u;
}

template <bool DC, bool DE>
__global__ __launch_bounds__(DEMOD_WAVE) void demod_chain_kernel(DemodParams p, int n_streams) {
    __shared__ float tile[DEMOD_GROUP * DEMOD_ROW];
    const int lane = threadIdx.x, s0 = (int)blockIdx.x * DEMOD_GROUP;
    const int rows = min(DEMOD_GROUP, n_streams - s0);  // streams of this wave
    const int n = p.n, n_chunks = (n + DEMOD_CHUNK - 1) / DEMOD_CHUNK;
    const size_t stride = (size_t)p.scratch_stride;
    float *base = p.scratch + (size_t)s0 * stride;
    const bool have = lane < rows;
    float m = 0.0f, s = 0.0f;
    if (have && !p.fresh) {
        const float2 ms = reinterpret_cast<const float2 *>(p.state_old)[2 * (size_t)(s0 + lane) + 1];
        m = ms.x, s = ms.y;
    }
    const float alpha = p.alpha, a = p.a;

    float nx[DEMOD_GROUP];  // the next tile, a row per register
#pragma unroll
    for (int r = 0; r < DEMOD_GROUP; r++) nx[r] = r < rows && lane < n ? base[(size_t)r * stride + lane] : 0.0f;
    for (int c = 0; c < n_chunks; c++) {
        const int at = c * DEMOD_CHUNK, steps = min(DEMOD_CHUNK, n - at);
#pragma unroll
        for (int r = 0; r < DEMOD_GROUP; r++) tile[r * DEMOD_ROW + lane] = nx[r];
        __syncthreads();
        if (c + 1 < n_chunks) {
            const int nt = at + DEMOD_CHUNK + lane;
#pragma unroll
            for (int r = 0; r < DEMOD_GROUP; r++) nx[r] = r < rows && nt < n ? base[(size_t)r * stride + nt] : 0.0f;
        }
        float *mine = tile + (lane % DEMOD_GROUP) * DEMOD_ROW;  // the lanes from DEMOD_GROUP on only load and store
        if (steps == DEMOD_CHUNK) {  // a whole step: every LDS read ahead of the chain, every write behind it
            if (have) {
                float e[DEMOD_CHUNK];
#pragma unroll
                for (int i = 0; i < DEMOD_CHUNK; i++) e[i] = mine[i];
#pragma unroll
                for (int i = 0; i < DEMOD_CHUNK; i++) e[i] = demod_step<DC, DE>(e[i], m, s, alpha, a);
#pragma unroll
                for (int i = 0; i < DEMOD_CHUNK; i++) mine[i] = e[i];
            }
        } else {
            for (int j = 0; j < steps && have; j++) mine[j] = demod_step<DC, DE>(mine[j], m, s, alpha, a);
        }
        __syncthreads();
        if (lane < steps) {
#pragma unroll
            for (int r = 0; r < DEMOD_GROUP; r++)
                if (r < rows) base[(size_t)r * stride + at + lane] = tile[r * DEMOD_ROW + lane];
        }
        __syncthreads();
    }
    if (have) reinterpret_cast<float2 *>(p.state_new)[2 * (size_t)(s0 + lane) + 1] = make_float2(m, s);
}

template <int FMT>
__global__ __launch_bounds__(DEMOD_THREADS) void demod_fir_kernel(DemodParams p, DemodTaps taps, void *__restrict__ out) {
    typedef typename FirOut<FMT>::type out_t;
    extern __shared__ __attribute__((aligned(16))) float demod_lds[];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int N = p.n, R = p.decim, T = p.taps, H = T - 1;
    const float *v = p.scratch + (size_t)b * (size_t)p.scratch_stride;
    const float *hist_old = stream_history<float>(p.hist_old, b, H);
    out_t *orow = static_cast<out_t *>(out) + (size_t)b * (size_t)p.cap;

    if ((int)blockIdx.x == p.n_tiles) {
        close_stream<DEMOD_THREADS, 1>(p.hist_new, hist_old, b, N, H, orow, p.n_out, p.cap, tid,
                                       [&](int t) { return v[t]; });
        return;
    }

    const FirWindow w(p, T);
    const int row = p.row;
    float *tap_lds = demod_lds, *smp = demod_lds + DEMOD_TAP_SLOTS;
    stage_taps<DEMOD_THREADS>(tap_lds, taps.h, T, tid);
    {
        int r = tid % R, q = tid / R;  // [u mod R][u / R] of u = tid, then u += DEMOD_THREADS
        const int dr = DEMOD_THREADS % R, dq = DEMOD_THREADS / R;
        for (int u = tid; u < w.count; u += DEMOD_THREADS) {
            const int t = w.w0 + u;  // < N: the last output's newest value is first + (n_out - 1) R < N
            float x = 0.0f;
            if (t >= 0)
                x = v[t];
            else if (hist_old)
                x = hist_old[t + H];
            smp[r * row + q] = x;
            r += dr, q += dq;
            if (r >= R) r -= R, q++;
        }
    }
    __syncthreads();

    if (tid < w.nj) orow[w.j0 + tid] = FirOut<FMT>::make(polyphase_fir(tap_lds, smp, T, R, row, tid) * p.gain);
}

}  // namespace

int demod_tile_outputs(int decim, int taps) { return fir_tile_outputs(DEMOD_LDS_SAMPLES, DEMOD_THREADS, decim, taps); }

hipError_t launch_demod(const float *chan, int n_streams, const DemodParams &p0, const DemodTaps &taps, void *out,
                        hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    DemodParams p = p0;
    if (!out || p.n < 0 || p.n > SDRG_DEMOD_MAX_IN || (p.mode != SDRG_DEMOD_AM && p.mode != SDRG_DEMOD_FM) ||
        (p.out_format != SDRG_DEMOD_OUT_S16 && p.out_format != SDRG_DEMOD_OUT_F32) || n_streams > 65535)
        return hipErrorInvalidValue;
    if (p.n > 0 && (!chan || !p.scratch || !p.state_new || p.in_stride < p.n || p.scratch_stride < p.n ||
                    (p.taps > 1 && !p.hist_new) || (!p.fresh && (!p.state_old || (p.taps > 1 && !p.hist_old)))))
        return hipErrorInvalidValue;
    if (!fir_tile_plan(&p, DEMOD_LDS_SAMPLES, DEMOD_THREADS, SDRG_DEMOD_MAX_DECIMATION, SDRG_DEMOD_MAX_TAPS))
        return hipErrorInvalidValue;
    hipError_t er;
    if (p.n > 0) {
        const dim3 grid((unsigned)((p.n + DEMOD_THREADS - 1) / DEMOD_THREADS), (unsigned)n_streams);
        const float2 *z = reinterpret_cast<const float2 *>(chan);
        if (p.mode == SDRG_DEMOD_FM)
            hipLaunchKernelGGL(demod_detect_kernel<SDRG_DEMOD_FM>, grid, dim3(DEMOD_THREADS), 0, stream, z, p);
        else
            hipLaunchKernelGGL(demod_detect_kernel<SDRG_DEMOD_AM>, grid, dim3(DEMOD_THREADS), 0, stream, z, p);
        if ((er = hipGetLastError()) != hipSuccess) return er;
        const bool dc = p.alpha != 0.0f, de = p.a != 0.0f;
        if (dc || de) {
            const dim3 groups((unsigned)((n_streams + DEMOD_GROUP - 1) / DEMOD_GROUP));
            void (*k)(DemodParams, int) = dc && de ? demod_chain_kernel<true, true>
                                          : dc     ? demod_chain_kernel<true, false>
                                                   : demod_chain_kernel<false, true>;
            hipLaunchKernelGGL(k, groups, dim3(DEMOD_WAVE), 0, stream, p, n_streams);
            if ((er = hipGetLastError()) != hipSuccess) return er;
        }
    }
    const size_t lds = sizeof(float) * ((size_t)p.row * (size_t)p.decim + DEMOD_TAP_SLOTS);
    const dim3 grid((unsigned)p.n_tiles + 1, (unsigned)n_streams);
    if (p.out_format == SDRG_DEMOD_OUT_F32)
        hipLaunchKernelGGL(demod_fir_kernel<SDRG_DEMOD_OUT_F32>, grid, dim3(DEMOD_THREADS), lds, stream, p, taps, out);
    else
        hipLaunchKernelGGL(demod_fir_kernel<SDRG_DEMOD_OUT_S16>, grid, dim3(DEMOD_THREADS), lds, stream, p, taps, out);
    return hipGetLastError();
}

}  // namespace sdrg
