// display.hip — the display stage (sdrg_engine_display_*): per stream and frame, a span [lo, lo + nb) of the
// fftshifted power spectrum reduced to W columns (peak or mean per column), converted to dB with the glibc-exact
// log10f the statistics use, and written as float dB or as 8-bit codes (include/sdrg.h).
//
// Column c covers the bins j0 = floor(c nb / W) .. j1 - 1, j1 = floor((c + 1) nb / W), in 64-bit integers, and the one
// bin j0 when that range is empty (W > nb).  The reduction is taken on the powers (log10f is monotone), so a frame
// costs nb loads and W logs.  Two kernels, chosen by the launcher:
//   direct  W >= nb: every column is one bin; a lane per column, consecutive lanes on the same or adjacent bins.
//   tiled   W < nb: a workgroup per (frame group, tile of columns); lanes on consecutive aligned float4s (the span's
//           misaligned head and tail as scalars), each lane's float4 reduced per column first, then one LDS atomic per
//           (lane, column): an unsigned max on the bit pattern (non-negative floats order as unsigned integers) or a
//           double add.  Small spans pack several frames into one workgroup, a wave per frame; long ones are cut into
//           tiles of columns of about 16384 bins each.
// (A third kernel, wave shuffles across the r / 4 lanes of a column for r = nb / W a power of two, measured 3.4 TB/s at
// 4096 x 16384 -> 1024 where the tiled kernel reads 4.8 TB/s, and was dropped: DESIGN.md §3.9.)
// Compiled with -ffp-contract=off: the dB expression and the quantisation are separate float operations.
#include <algorithm>

#include "glibc_logf.h"
#include "sdrg_internal.h"

namespace sdrg {
namespace {

constexpr int DISPLAY_THREADS = 256;
constexpr int DISPLAY_TILE_COLS = 2048;  // columns a tiled workgroup keeps in LDS: 8 KiB of bounds + 16 KiB of doubles
constexpr int DISPLAY_TILE_BINS = 16384;  // bins a tile of a long span covers, about
constexpr int DISPLAY_DIRECT_COLS = 8;    // columns per lane of the direct kernel (2048 per workgroup)

typedef float display_v4 __attribute__((ext_vector_type(4)));

// floor(c * nb / W) for 0 <= c <= W <= 2^20, 1 <= nb <= 2^20: a float estimate corrected against the exact 64-bit
// products (the estimate is off by less than one, the loops make the result exact whatever it is)
__device__ __forceinline__ int column_first(int c, int nb, int W, float nb_over_w) {
    const uint64_t num = (uint64_t)c * (uint64_t)nb;
    int64_t q = (int64_t)((float)c * nb_over_w);
    if (q < 0) q = 0;
    while ((uint64_t)(q + 1) * (uint64_t)W <= num) q++;
    while ((uint64_t)q * (uint64_t)W > num) q--;
    return (int)q;
}

// negative inputs are outside the definition: they (and -0) count as +0, so the unsigned order holds for every input
__device__ __forceinline__ uint32_t power_bits(float p) {
    const uint32_t u = glibc::f2u(p);
    return (u & 0x80000000u) ? 0u : u;
}

// d = 10.0f * log10f(v + 1e-20f) (fft_process.h:74-75, refPower 1)
__device__ __forceinline__ float column_db(float v, const glibc::LogfEntry *tab) {
    return 10.0f * glibc::log10f_fast(v + 1e-20f, tab);
}

__device__ __forceinline__ uint8_t db_code(float d, float db_min, float scale) {
    const float t = (d - db_min) * scale;
    if (t >= 255.0f) return 255;
    if (!(t > 0.0f)) return 0;  // t <= 0 or NaN
    return (uint8_t)(int)(t + 0.5f);
}

template <int FORMAT>
__device__ __forceinline__ void store_column(void *out, size_t idx, float v, const DisplayParams &p,
                                             const glibc::LogfEntry *tab) {
    const float d = column_db(v, tab);
    if (FORMAT == SDRG_DISPLAY_U8)
        static_cast<uint8_t *>(out)[idx] = db_code(d, p.db_min, p.scale);
    else
        static_cast<float *>(out)[idx] = d;
}

__device__ __forceinline__ void load_log_table(glibc::LogfEntry *tab) {
    if (threadIdx.x < 16) tab[threadIdx.x] = glibc::logf_table()[threadIdx.x];
    __syncthreads();
}

// W >= nb: column c is the bin floor(c nb / W), whatever the reduction (a mean of one value is the value).
// DISPLAY_DIRECT_COLS columns per lane, 256 apart: one column per lane made 4096 x 16384 a launch of 262144 workgroups.
template <int FORMAT>
__global__ __launch_bounds__(DISPLAY_THREADS) void display_direct_kernel(const float *__restrict__ spectra, DisplayParams p,
                                                                         int blocks_per_row,
                                                                         void *__restrict__ out) {
    __shared__ glibc::LogfEntry tab[16];
    load_log_table(tab);
    const int s = blockIdx.x / blocks_per_row;  // < n_streams: the grid is n_streams * blocks_per_row
    const int c0 = (blockIdx.x - s * blocks_per_row) * (DISPLAY_THREADS * DISPLAY_DIRECT_COLS) + threadIdx.x;
    const float *row = spectra + (size_t)s * (size_t)p.n + (size_t)p.lo;
    const float ratio = (float)p.nb / (float)p.width;
    float v[DISPLAY_DIRECT_COLS];  // the loads first
#pragma unroll
    for (int u = 0; u < DISPLAY_DIRECT_COLS; u++) {
        const int c = c0 + u * DISPLAY_THREADS;
        if (c < p.width) v[u] = row[p.width == p.nb ? c : column_first(c, p.nb, p.width, ratio)];
    }
#pragma unroll
    for (int u = 0; u < DISPLAY_DIRECT_COLS; u++) {
        const int c = c0 + u * DISPLAY_THREADS;
        if (c < p.width)
            store_column<FORMAT>(out, (size_t)s * (size_t)p.width + (size_t)c, glibc::u2f(power_bits(v[u])), p, tab);
    }
}

template <int REDUCE>
struct DisplayAcc;
template <>
struct DisplayAcc<SDRG_DISPLAY_MAX> {
    typedef uint32_t type;
    __device__ static __forceinline__ void add(type *a, const float *x, int k) {
        uint32_t m = power_bits(x[0]);
        for (int e = 1; e < k; e++) m = max(m, power_bits(x[e]));
        atomicMax(a, m);
    }
    __device__ static __forceinline__ float value(type a, int) { return glibc::u2f(a); }
};
template <>
struct DisplayAcc<SDRG_DISPLAY_MEAN> {
    typedef double type;
    __device__ static __forceinline__ void add(type *a, const float *x, int k) {
        double s = (double)x[0];
        for (int e = 1; e < k; e++) s += (double)x[e];
        atomicAdd(a, s);
    }
    __device__ static __forceinline__ float value(type a, int count) { return (float)(a / (double)count); }
};

// W < nb.  Workgroup b handles the frames [fg * frames_per_wg, ...) and the columns [c0, c0 + tc) of tile t,
// b = fg * n_tiles + t.  LDS: bound[tc + 1] (first bin of each column of the tile, and of the one after it),
// acc[frames_per_wg][tc].  frames_per_wg == 1: the 256 threads share the frame; otherwise a wave per frame.
template <int REDUCE, int FORMAT>
__global__ __launch_bounds__(DISPLAY_THREADS) void display_tiled_kernel(const float *__restrict__ spectra, int n_streams,
                                                                        DisplayParams p, int tile_cols, int n_tiles,
                                                                        int frames_per_wg, void *__restrict__ out) {
    typedef typename DisplayAcc<REDUCE>::type acc_t;
    extern __shared__ __attribute__((aligned(16))) unsigned char display_lds[];
    __shared__ glibc::LogfEntry tab[16];
    const int fg = blockIdx.x / n_tiles, t = blockIdx.x - fg * n_tiles;
    const int c0 = t * tile_cols, tc = min(tile_cols, p.width - c0);
    const int f0 = fg * frames_per_wg, nf = min(frames_per_wg, n_streams - f0);
    acc_t *acc = reinterpret_cast<acc_t *>(display_lds);                         // [frames_per_wg][tc]
    int *bound = reinterpret_cast<int *>(acc + (size_t)frames_per_wg * tile_cols);  // [tc + 1]
    const float ratio = (float)p.nb / (float)p.width, inv_ratio = (float)p.width / (float)p.nb;
    for (int i = threadIdx.x; i <= tc; i += DISPLAY_THREADS) bound[i] = column_first(c0 + i, p.nb, p.width, ratio);
    for (int i = threadIdx.x; i < nf * tc; i += DISPLAY_THREADS) acc[i] = (acc_t)0;
    load_log_table(tab);  // and the barrier for bound / acc

    const int jb = bound[0], je = bound[tc];  // the tile's bins [jb, je) of the span
    const int team = frames_per_wg == 1 ? DISPLAY_THREADS : 64;
    const int tm = threadIdx.x / team, tl = threadIdx.x - tm * team, n_teams = DISPLAY_THREADS / team;
    // the column (tile-relative) of bin j: an estimate from the inverse ratio, corrected against the bounds
    auto column_of = [&](int j) {
        int ci = (int)(((float)j + 0.5f) * inv_ratio) - c0;
        ci = max(0, min(tc - 1, ci));
        while (ci > 0 && j < bound[ci]) ci--;
        while (ci < tc - 1 && j >= bound[ci + 1]) ci++;
        return ci;
    };
    for (int f = tm; f < nf; f += n_teams) {
        const float *row = spectra + (size_t)(f0 + f) * (size_t)p.n + (size_t)p.lo;
        acc_t *a = acc + (size_t)f * tc;
        // scalars up to the first 16-byte aligned bin, aligned float4s, scalars after the last whole float4
        const int mis = (int)((reinterpret_cast<uintptr_t>(row + jb) >> 2) & 3);
        const int head = min((4 - mis) & 3, je - jb);
        const int n_vec = (je - jb - head) / 4;
        const int tail0 = jb + head + 4 * n_vec;
        if (tl < head) {
            const int j = jb + tl;
            const float x = row[j];
            DisplayAcc<REDUCE>::add(a + column_of(j), &x, 1);
        }
        if (tl < je - tail0) {
            const int j = tail0 + tl;
            const float x = row[j];
            DisplayAcc<REDUCE>::add(a + column_of(j), &x, 1);
        }
        // one float4 in flight per lane: with 8 waves per SIMD, 2 or 4 loads issued ahead measured 0 to 7 % slower
        for (int k = tl; k < n_vec; k += team) {
            const int j = jb + head + 4 * k;
            const display_v4 q = *reinterpret_cast<const display_v4 *>(row + j);
            const float x[4] = {q.x, q.y, q.z, q.w};
            int ci = column_of(j);
            if (j + 3 < bound[ci + 1]) {  // the lane's own float4 first: one atomic for the column that holds it
                DisplayAcc<REDUCE>::add(a + ci, x, 4);
            } else {  // a column boundary inside the float4
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    while (j + e >= bound[ci + 1]) ci++;
                    DisplayAcc<REDUCE>::add(a + ci, x + e, 1);
                }
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nf * tc; i += DISPLAY_THREADS) {
        const int f = i / tc, ci = i - f * tc;
        const float v = DisplayAcc<REDUCE>::value(acc[i], bound[ci + 1] - bound[ci]);
        store_column<FORMAT>(out, (size_t)(f0 + f) * (size_t)p.width + (size_t)(c0 + ci), v, p, tab);
    }
}

template <int REDUCE, int FORMAT>
hipError_t launch_display_rf(const float *spectra, int n_streams, const DisplayParams &p, void *out,
                             hipStream_t stream) {
    const size_t B = (size_t)n_streams;
    if (p.width >= p.nb) {
        const int per_block = DISPLAY_THREADS * DISPLAY_DIRECT_COLS;
        const int blocks_per_row = (p.width + per_block - 1) / per_block;
        const size_t blocks = B * (size_t)blocks_per_row;
        if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
        hipLaunchKernelGGL((display_direct_kernel<FORMAT>), dim3((unsigned)blocks), dim3(DISPLAY_THREADS), 0, stream,
                           spectra, p, blocks_per_row, out);
        return hipGetLastError();
    }
    // a tile: at most DISPLAY_TILE_COLS columns and, for long spans, about DISPLAY_TILE_BINS bins (4096 x 16384 gives a
    // workgroup per frame, 1024 x 65536 -> 1920 four per frame: the same number of workgroups for the chip to balance)
    int tile_cols = std::min(p.width, DISPLAY_TILE_COLS);
    const int parts = (p.nb + DISPLAY_TILE_BINS - 1) / DISPLAY_TILE_BINS;
    if (parts > 1) tile_cols = std::min(tile_cols, (p.width + parts - 1) / parts);
    const int n_tiles = (p.width + tile_cols - 1) / tile_cols;
    // small spans: frames of at most 2048 bins share a workgroup, up to 16 of them and DISPLAY_TILE_COLS columns
    int frames_per_wg = 1;
    if (n_tiles == 1 && p.nb <= 2048)
        frames_per_wg = std::max(1, std::min({16, DISPLAY_TILE_COLS / tile_cols, 4096 / p.nb, n_streams}));
    const size_t acc_bytes = REDUCE == SDRG_DISPLAY_MAX ? sizeof(uint32_t) : sizeof(double);
    const size_t lds = acc_bytes * (size_t)frames_per_wg * tile_cols + sizeof(int) * ((size_t)tile_cols + 1);
    const size_t blocks = ((B + frames_per_wg - 1) / frames_per_wg) * (size_t)n_tiles;
    if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL((display_tiled_kernel<REDUCE, FORMAT>), dim3((unsigned)blocks), dim3(DISPLAY_THREADS), lds, stream,
                       spectra, n_streams, p, tile_cols, n_tiles, frames_per_wg, out);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_display(const float *spectra, int n_streams, const DisplayParams &p, void *out, hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    if (!spectra || !out || p.n < 1 || p.lo < 0 || p.nb < 1 || (int64_t)p.lo + p.nb > p.n || p.width < 1 ||
        p.width > (1 << 20))
        return hipErrorInvalidValue;
    const bool u8 = p.format == SDRG_DISPLAY_U8;
    if (p.reduce == SDRG_DISPLAY_MAX)
        return u8 ? launch_display_rf<SDRG_DISPLAY_MAX, SDRG_DISPLAY_U8>(spectra, n_streams, p, out, stream)
                  : launch_display_rf<SDRG_DISPLAY_MAX, SDRG_DISPLAY_DB_F32>(spectra, n_streams, p, out, stream);
    if (p.reduce == SDRG_DISPLAY_MEAN)
        return u8 ? launch_display_rf<SDRG_DISPLAY_MEAN, SDRG_DISPLAY_U8>(spectra, n_streams, p, out, stream)
                  : launch_display_rf<SDRG_DISPLAY_MEAN, SDRG_DISPLAY_DB_F32>(spectra, n_streams, p, out, stream);
    return hipErrorInvalidValue;
}

}  // namespace sdrg
