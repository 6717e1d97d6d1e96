// integrate.hip — the integration stage (sdrg_engine_integrate_*): per stream and bin, the mean or the maximum of the
// last K power spectra, or an exponential moving average (include/sdrg.h).
//
// Every buffer of the stage has the layout [n_streams][N] of the spectra: the input, the output, the EMA state and each
// slot of the ring [slot][stream][N] (slots padded to a multiple of four floats, so each starts on 16 bytes).  The stage
// works bin by bin, so a call is one element-wise pass over count = n_streams * N floats and rows do not matter: a lane
// takes one 16-byte float4 of the flat array whatever N is (N = 1001 or N = 1 pack as densely as N = 16384), the at
// most three floats after the last whole float4 go to a second launch of the scalar instance, and so does the whole
// array when the caller's spectra or out pointer is not 16-byte aligned.
//
//   MEAN / MAX  the lane loads x and the c - 1 older values of its bins (ring slots oldest to newest, INTEGRATE_BATCH
//               loads issued before the first is used), reduces them, stores x into the slot of the frame that leaves
//               and stores the result: 4c + 8 bytes per bin.  The sum is a double, started at -0.0 (x + -0.0 is x for
//               every x) and added oldest first, x last; the slot index and c are host counters passed as arguments.
//   EMA         y = x at the first call, else d = x - y; y = y + alpha * d: 16 bytes per bin.
// A lane reads its bins before it writes them, so out may be the spectra buffer.
// Compiled with -ffp-contract=off: the EMA's multiply and add stay two operations.
#include "sdrg_internal.h"

namespace sdrg {
namespace {

constexpr int INTEGRATE_THREADS = 256;
constexpr int INTEGRATE_BATCH = 8;  // ring loads in flight per lane before the first add (32 VGPRs of float4)

typedef float integrate_v4 __attribute__((ext_vector_type(4)));

// Stores of the ring slot and of out are non-temporal: the slot is read again period - 1 calls later and out by
// another kernel, and at 4096 x 16384 they measured 1 to 6 % faster than plain stores in every mode (DESIGN.md §3.10;
// -DSDRG_INTEGRATE_NT=0 is the lab build of that comparison).
#ifndef SDRG_INTEGRATE_NT
#define SDRG_INTEGRATE_NT 1
#endif
template <typename T>
__device__ __forceinline__ void integrate_store(T *p, const T &v) {
    if (SDRG_INTEGRATE_NT)
        __builtin_nontemporal_store(v, p);
    else
        *p = v;
}

template <typename T>
struct IntegrateLanes;
template <>
struct IntegrateLanes<float> {
    static constexpr int n = 1;
    __device__ static __forceinline__ float get(const float &v, int) { return v; }
    __device__ static __forceinline__ void set(float &v, int, float x) { v = x; }
};
template <>
struct IntegrateLanes<integrate_v4> {
    static constexpr int n = 4;
    __device__ static __forceinline__ float get(const integrate_v4 &v, int e) { return v[e]; }
    __device__ static __forceinline__ void set(integrate_v4 &v, int e, float x) { v[e] = x; }
};

template <int MODE, typename T>
struct IntegrateAcc;
template <typename T>
struct IntegrateAcc<SDRG_INTEGRATE_MEAN, T> {
    double s[IntegrateLanes<T>::n];
    __device__ __forceinline__ IntegrateAcc() {
        for (int e = 0; e < IntegrateLanes<T>::n; e++) s[e] = -0.0;
    }
    __device__ __forceinline__ void add(const T &v) {
        for (int e = 0; e < IntegrateLanes<T>::n; e++) s[e] += (double)IntegrateLanes<T>::get(v, e);
    }
    __device__ __forceinline__ T value(int depth) const {
        T r;
        for (int e = 0; e < IntegrateLanes<T>::n; e++) IntegrateLanes<T>::set(r, e, (float)(s[e] / (double)depth));
        return r;
    }
};
template <typename T>
struct IntegrateAcc<SDRG_INTEGRATE_MAX, T> {
    float m[IntegrateLanes<T>::n];
    __device__ __forceinline__ IntegrateAcc() {
        for (int e = 0; e < IntegrateLanes<T>::n; e++) m[e] = 0.0f;  // the powers are >= +0
    }
    __device__ __forceinline__ void add(const T &v) {
        for (int e = 0; e < IntegrateLanes<T>::n; e++) m[e] = fmaxf(m[e], IntegrateLanes<T>::get(v, e));
    }
    __device__ __forceinline__ T value(int) const {
        T r;
        for (int e = 0; e < IntegrateLanes<T>::n; e++) IntegrateLanes<T>::set(r, e, m[e]);
        return r;
    }
};

// x_in, out: [count] T (out may be x_in).  ring: [period][slot_stride] T, slot_stride >= count.  The frames before
// this one are in the slots slot - (depth - 1) .. slot - 1 (mod period), oldest first; depth <= period, so the slot
// written is none of them.
template <int MODE, typename T>
__global__ __launch_bounds__(INTEGRATE_THREADS) void integrate_ring_kernel(const T *x_in, T *__restrict__ ring,
                                                                           size_t slot_stride, int period, int slot,
                                                                           int depth, size_t count, T *out) {
    const size_t i = (size_t)blockIdx.x * INTEGRATE_THREADS + threadIdx.x;
    if (i >= count) return;
    const T x = x_in[i];
    IntegrateAcc<MODE, T> acc;
    const int older = depth - 1;
    int s = slot - older;
    if (s < 0) s += period;
    for (int j = 0; j < older; j += INTEGRATE_BATCH) {
        T v[INTEGRATE_BATCH];
#pragma unroll
        for (int u = 0; u < INTEGRATE_BATCH; u++)
            if (j + u < older) {
                v[u] = ring[(size_t)s * slot_stride + i];
                s = s + 1 == period ? 0 : s + 1;
            }
#pragma unroll
        for (int u = 0; u < INTEGRATE_BATCH; u++)
            if (j + u < older) acc.add(v[u]);
    }
    acc.add(x);
    integrate_store(ring + (size_t)slot * slot_stride + i, x);
    integrate_store(out + i, acc.value(depth));
}

template <typename T>
__global__ __launch_bounds__(INTEGRATE_THREADS) void integrate_ema_kernel(const T *x_in, T *__restrict__ y, float alpha,
                                                                          int first, size_t count, T *out) {
    const size_t i = (size_t)blockIdx.x * INTEGRATE_THREADS + threadIdx.x;
    if (i >= count) return;
    T r = x_in[i];
    if (!first) {
        const T x = r, yp = y[i];
        for (int e = 0; e < IntegrateLanes<T>::n; e++) {
            const float d = IntegrateLanes<T>::get(x, e) - IntegrateLanes<T>::get(yp, e);
            IntegrateLanes<T>::set(r, e, IntegrateLanes<T>::get(yp, e) + alpha * d);
        }
    }
    y[i] = r;  // read again by the next call
    integrate_store(out + i, r);
}

// `count` elements of T starting `first` floats into every buffer
template <typename T>
hipError_t launch_integrate_t(const float *spectra, size_t first, size_t count, const IntegrateParams &p, float *ring,
                              size_t slot_stride, float *ema, float *out, hipStream_t stream) {
    const size_t blocks = (count + INTEGRATE_THREADS - 1) / INTEGRATE_THREADS;
    if (blocks == 0) return hipSuccess;
    if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
    const T *x = reinterpret_cast<const T *>(spectra + first);
    T *o = reinterpret_cast<T *>(out + first);
    const dim3 grid((unsigned)blocks), block(INTEGRATE_THREADS);
    if (p.mode == SDRG_INTEGRATE_EMA) {
        hipLaunchKernelGGL((integrate_ema_kernel<T>), grid, block, 0, stream, x, reinterpret_cast<T *>(ema + first), p.alpha,
                           p.depth == 1 ? 1 : 0, count, o);
    } else {
        T *r = reinterpret_cast<T *>(ring + first);
        const size_t stride = slot_stride / IntegrateLanes<T>::n;
        if (p.mode == SDRG_INTEGRATE_MEAN)
            hipLaunchKernelGGL((integrate_ring_kernel<SDRG_INTEGRATE_MEAN, T>), grid, block, 0, stream, x, r, stride,
                               p.period, p.slot, p.depth, count, o);
        else
            hipLaunchKernelGGL((integrate_ring_kernel<SDRG_INTEGRATE_MAX, T>), grid, block, 0, stream, x, r, stride,
                               p.period, p.slot, p.depth, count, o);
    }
    return hipGetLastError();
}

}  // namespace

size_t integrate_slot_stride(size_t count) { return (count + 3) & ~(size_t)3; }

hipError_t launch_integrate(const float *spectra, size_t count, const IntegrateParams &p, float *ring, size_t slot_stride,
                            float *ema, float *out, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    if (!spectra || !out) return hipErrorInvalidValue;
    if (p.mode == SDRG_INTEGRATE_EMA) {
        if (!ema || p.depth < 1) return hipErrorInvalidValue;
    } else if (p.mode == SDRG_INTEGRATE_MEAN || p.mode == SDRG_INTEGRATE_MAX) {
        if (!ring || p.period < 1 || p.depth < 1 || p.depth > p.period || p.slot < 0 || p.slot >= p.period ||
            slot_stride < count || (slot_stride & 3) || (reinterpret_cast<uintptr_t>(ring) & 15))
            return hipErrorInvalidValue;
    } else {
        return hipErrorInvalidValue;
    }
    // the engine's own buffers (ring, ema) are 16-byte aligned; the caller's decide between float4s and scalars
    const bool aligned = ((reinterpret_cast<uintptr_t>(spectra) | reinterpret_cast<uintptr_t>(out) |
                           reinterpret_cast<uintptr_t>(ema)) & 15) == 0;
    const size_t n_vec = aligned ? count / 4 : 0;
    hipError_t e = launch_integrate_t<integrate_v4>(spectra, 0, n_vec, p, ring, slot_stride, ema, out, stream);
    if (e != hipSuccess) return e;
    return launch_integrate_t<float>(spectra, 4 * n_vec, count - 4 * n_vec, p, ring, slot_stride, ema, out, stream);
}

}  // namespace sdrg
