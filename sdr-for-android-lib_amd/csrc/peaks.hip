// peaks.hip — the peak table stage (sdrg_engine_peaks_*): per stream, the at most max_peaks strongest local maxima of a
// span [lo, lo + nb) of one row of fftshifted power, at least min_separation bins apart and at least threshold_db over
// the span's noise floor (include/sdrg.h).
//
// One workgroup per frame, in three sizes chosen by the launcher:
//   nb <= 2048    64 threads (one wave), the span staged in LDS: an 81-bin focus span costs a wave, not four
//   nb <= 16384   1024 threads, the span staged in LDS (64 KiB; 79 KB with the rest, two workgroups per CU)
//   nb <= 2^20    1024 threads, the span read from memory (L2 / Infinity Cache after the first pass), the candidate scan
//                 in tiles of 16384 bins with the top-K list kept in LDS across them
// Phases, powers handled as their bit patterns (non-negative floats order as unsigned integers):
//   stage      aligned 16-byte loads, the misaligned head and tail as scalars (display_tiled_kernel's scheme); the LDS
//              copy starts at the same offset from 16 bytes as the span does in memory, so its 16-byte stores are aligned
//   maxima     the largest power of every block of 32 (from memory: 64) bins, and the AND / OR of all bits
//   floor      the element of rank nb / 2 by an 8-bit-digit radix select that starts at the highest bit in which the
//              values differ (stats.hip's kth_smallest), the histogram in 8 copies chosen by the lane: exact
//   threshold  the powers whose snr reaches threshold_db are those from p_min up (dB does not decrease with the power):
//              p_min by a 64-way search in wave 0, six logs per lane and frame and none per bin or candidate
//   candidates a bin of at least p_min against its window of +- d bins, early exit: first j +- 1 .. 3 (six loads at once;
//              two survivors are more than 3 bins apart, so at most nb / 4 + 1 of them go to a worklist), then per
//              survivor the rest of its own block, whole blocks through the block maxima, the bins of the partial blocks
//              at the window's ends.  A candidate sets a bit.
//   top-K      repeated workgroup arg-max of the 64-bit keys (power bits << 32 | ~bin: larger power first, then the lower
//              bin) over the bitmap and the list of the tiles before, at most max_peaks rounds, one barrier each; dB and
//              snr of the peaks written, one log each
// Compiled with -ffp-contract=off: the dB expression and the snr subtraction are separate float operations.
#include <algorithm>

#include "glibc_logf.h"
#include "sdrg_internal.h"

namespace sdrg {
namespace {

constexpr int PEAKS_WAVE = 64;
constexpr int PEAKS_WAVE_BINS = 2048;   // spans up to this take the one-wave kernel
constexpr int PEAKS_LDS_BINS = 16384;   // spans up to this are staged in LDS
constexpr int PEAKS_TILE = 16384;       // bins per tile of the candidate scan (one bitmap, 16-bit worklist entries)
constexpr int PEAKS_NEAR = 3;           // the neighbours every bin is tested against before the worklist

typedef unsigned long long peaks_u64;
typedef uint32_t peaks_u4 __attribute__((ext_vector_type(4)));

// word offsets of a workgroup's dynamic LDS (every region a multiple of 4 words, so 16-byte aligned)
struct PeaksLayout {
    int row, bm, bitmap, misc, best, list, work, total;
};
constexpr int PEAKS_HIST_COPIES = 8, PEAKS_HIST_STRIDE = 257;  // the select's histogram: copy c of bin b at c * 257 + b
constexpr int PEAKS_MISC_DIGIT = 8, PEAKS_MISC_ACC = 9, PEAKS_MISC_ABOVE = 10, PEAKS_MISC_WORK = 11,
              PEAKS_MISC_PMIN = 12, PEAKS_MISC_FLOOR_DB = 13;  // [0], [1]: AND, OR

__host__ __device__ inline int peaks_round4(int w) { return (w + 3) & ~3; }
__host__ __device__ inline PeaksLayout peaks_layout(int nb, bool staged) {
    const int shift = staged ? 5 : 6, tile = nb < PEAKS_TILE ? nb : PEAKS_TILE;
    PeaksLayout L;
    int o = 0;
    L.row = o, o += staged ? peaks_round4(nb + 3) : 0;  // + 3: the span's offset from a 16-byte boundary
    L.bm = o, o += peaks_round4((nb + (1 << shift) - 1) >> shift);
    L.bitmap = o, o += peaks_round4((tile + 31) >> 5);
    L.misc = o, o += 16;
    L.best = o, o += 8;      // 3 x 64 bits
    L.list = o, o += 256;    // 2 x SDRG_PEAKS_MAX x 64 bits
    // the worklist's 16-bit entries; before it the select's histograms use the same words
    const int work = (tile / (PEAKS_NEAR + 1) + 1 + 1) >> 1, hist = PEAKS_HIST_COPIES * PEAKS_HIST_STRIDE;
    L.work = o, o += peaks_round4(work > hist ? work : hist);
    L.total = o;
    return L;
}

template <int T, bool STAGED>
__global__ __launch_bounds__(T) void peaks_kernel(const float *__restrict__ spectra, PeaksParams p,
                                                  sdrg_peak *__restrict__ peaks,
                                                  sdrg_peaks_summary *__restrict__ summary) {
    constexpr int BS = STAGED ? 5 : 6, BLK = 1 << BS, N_WAVES = T / PEAKS_WAVE;
    extern __shared__ __attribute__((aligned(16))) uint32_t peaks_lds[];
    __shared__ glibc::LogfEntry tab[16];
    const int tid = threadIdx.x, lane = tid & (PEAKS_WAVE - 1), wave = tid / PEAKS_WAVE;
    const int nb = p.nb, d = p.min_sep, K = p.max_peaks;
    const PeaksLayout L = peaks_layout(nb, STAGED);
    const uint32_t *grow = reinterpret_cast<const uint32_t *>(spectra) + (size_t)blockIdx.x * (size_t)p.n + (size_t)p.lo;
    const int mis = (int)((reinterpret_cast<uintptr_t>(grow) >> 2) & 3);
    uint32_t *sp = peaks_lds + L.row + mis;  // STAGED: sp[j] = p_j
    uint32_t *bm = peaks_lds + L.bm, *bitmap = peaks_lds + L.bitmap, *misc = peaks_lds + L.misc;
    int *hist = reinterpret_cast<int *>(peaks_lds + L.work);  // the select is over before the worklist is used
    peaks_u64 *best = reinterpret_cast<peaks_u64 *>(peaks_lds + L.best);
    peaks_u64 *list = reinterpret_cast<peaks_u64 *>(peaks_lds + L.list);
    uint16_t *work = reinterpret_cast<uint16_t *>(peaks_lds + L.work);
    auto val = [&](int j) -> uint32_t {
        if constexpr (STAGED)
            return sp[j];
        else
            return grow[j];
    };

    if (tid < 16) tab[tid] = glibc::logf_table()[tid];
    if constexpr (STAGED) {
        const int head = min((4 - mis) & 3, nb), n_vec = (nb - head) / 4, tail0 = head + 4 * n_vec;
        if (tid < head) sp[tid] = grow[tid];
        if (tid < nb - tail0) sp[tail0 + tid] = grow[tail0 + tid];
        for (int k = tid; k < n_vec; k += T)
            *reinterpret_cast<peaks_u4 *>(sp + head + 4 * k) = *reinterpret_cast<const peaks_u4 *>(grow + head + 4 * k);
        __syncthreads();
    }

    // block maxima, and the AND / OR of every value
    uint32_t band = 0xffffffffu, bor = 0u;
    for (int j0 = wave * PEAKS_WAVE; j0 < nb; j0 += T) {
        const int j = j0 + lane;
        uint32_t m = 0u;
        if (j < nb) {
            m = val(j);
            band &= m;
            bor |= m;
        }
#pragma unroll
        for (int off = BLK / 2; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off));
        if ((lane & (BLK - 1)) == 0 && j < nb) bm[j >> BS] = m;
    }
#pragma unroll
    for (int off = PEAKS_WAVE / 2; off > 0; off >>= 1) {
        band &= (uint32_t)__shfl_xor((int)band, off);
        bor |= (uint32_t)__shfl_xor((int)bor, off);
    }
    if (N_WAVES > 1) {
        if (tid == 0) misc[0] = 0xffffffffu, misc[1] = 0u;
        __syncthreads();
        if (lane == 0) {
            atomicAnd(&misc[0], band);
            atomicOr(&misc[1], bor);
        }
        __syncthreads();
        band = misc[0];
        bor = misc[1];
    }

    // the floor: rank nb / 2 of the span (radix select, 8-bit digits from the highest bit that differs)
    uint32_t floor_bits = band;
    const uint32_t diff = band ^ bor;
    if (diff != 0) {
        int k = nb / 2;
        int top = 31 - __clz(diff);
        uint32_t mask = top >= 31 ? 0u : ~((2u << top) - 1u);
        uint32_t prefix = band & mask;
        while (top >= 0) {
            const int lo_bit = top >= 7 ? top - 7 : 0;
            const uint32_t dm = (1u << (top - lo_bit + 1)) - 1u;
            for (int i = tid; i < PEAKS_HIST_COPIES * PEAKS_HIST_STRIDE; i += T) hist[i] = 0;
            __syncthreads();
            int *mine = hist + (lane & (PEAKS_HIST_COPIES - 1)) * PEAKS_HIST_STRIDE;  // noise lands in a few bins
            for (int j = tid; j < nb; j += T) {
                const uint32_t b = val(j);
                if ((b & mask) == prefix) atomicAdd(&mine[(b >> lo_bit) & dm], 1);
            }
            __syncthreads();
            if (wave == 0) {  // 4 bins per lane, an inclusive scan over the wave, the bucket that holds rank k
                int hv[4] = {0, 0, 0, 0};
#pragma unroll
                for (int c = 0; c < PEAKS_HIST_COPIES; c++)
#pragma unroll
                    for (int u = 0; u < 4; u++) hv[u] += hist[c * PEAKS_HIST_STRIDE + 4 * lane + u];
                const int own = hv[0] + hv[1] + hv[2] + hv[3];
                int incl = own;
#pragma unroll
                for (int off = 1; off < PEAKS_WAVE; off <<= 1) {
                    const int v = __shfl_up(incl, off);
                    if (lane >= off) incl += v;
                }
                const unsigned long long over = __ballot(incl > k);  // non-empty: k < the values under this prefix
                const int first = __ffsll((long long)over) - 1;
                if (lane == first) {
                    int acc = incl - own, dgt = 0;
                    while (dgt < 3 && acc + hv[dgt] <= k) acc += hv[dgt++];
                    misc[PEAKS_MISC_DIGIT] = (uint32_t)(4 * first + dgt);
                    misc[PEAKS_MISC_ACC] = (uint32_t)acc;
                }
            }
            __syncthreads();
            k -= (int)misc[PEAKS_MISC_ACC];
            prefix |= misc[PEAKS_MISC_DIGIT] << lo_bit;
            mask |= dm << lo_bit;
            top = lo_bit - 1;
            __syncthreads();
        }
        floor_bits = prefix;
    }
    // The powers above the threshold are a range of bit patterns [p_min, p_max]: dB(v) does not decrease with v (every
    // float from +0 to +inf has been compared with its successor), nor does the rounded subtraction of floor_db.  So
    // p_min is found by a search, and a bin below it needs no neighbour and no log at all.  Wave 0 searches, 64 probes
    // per step (six steps for the 2^31 patterns), while the other waves wait: sixteen waves bisecting on their own
    // kept the SIMDs busy for longer than the rest of the kernel took.  A floor of +inf (floor_db = +inf) gives an snr
    // of -inf for finite powers and NaN for +inf.
    const float floor_power = glibc::u2f(floor_bits);
    if (wave == 0) {
        const float fdb = 10.0f * glibc::log10f_fast(floor_power + 1e-20f, tab);
        uint32_t lo = 0u, hi = 0x7f800000u;  // the lowest pattern above is in [lo, hi]; +inf is above (its snr is +inf)
        if (floor_bits < 0x7f800000u) {
            while (lo < hi) {
                const uint32_t step = (hi - lo + 62u) / 63u;
                const uint32_t q = min(hi, lo + (uint32_t)lane * step);
                const float db = 10.0f * glibc::log10f_fast(glibc::u2f(q) + 1e-20f, tab);
                const float snr = db - fdb;
                const unsigned long long yes = __ballot(snr >= p.threshold_db);  // lane 63 probes hi: never empty
                const int first = __ffsll((long long)yes) - 1;
                hi = min(hi, lo + (uint32_t)first * step);
                lo = first == 0 ? hi : lo + (uint32_t)(first - 1) * step + 1u;
            }
        } else if (!(-__builtin_inff() >= p.threshold_db)) {
            lo = 0xffffffffu;
        }
        if (lane == 0) {
            misc[PEAKS_MISC_PMIN] = lo;
            misc[PEAKS_MISC_FLOOR_DB] = glibc::f2u(fdb);
            misc[PEAKS_MISC_ABOVE] = 0u;
        }
    }
    __syncthreads();
    const uint32_t p_min = misc[PEAKS_MISC_PMIN], p_max = floor_bits < 0x7f800000u ? 0x7f800000u : 0x7f7fffffu;
    const float floor_db = glibc::u2f(misc[PEAKS_MISC_FLOOR_DB]);

    int list_cnt = 0, cur = 0;  // the top-K list so far: list[cur * SDRG_PEAKS_MAX + i], descending
    const int near = min(d, PEAKS_NEAR);
    for (int t0 = 0; t0 < nb; t0 += PEAKS_TILE) {
        const int tn = min(PEAKS_TILE, nb - t0);
        for (int w = tid; w < (tn + 31) >> 5; w += T) bitmap[w] = 0u;
        if (tid == 0) {
            misc[PEAKS_MISC_WORK] = 0u;
            best[0] = 0ull;
            best[1] = 0ull;
        }
        __syncthreads();
        // every bin against j +- 1 .. near (clipped to the span): the loads first, then the comparisons
        for (int j = t0 + tid; j < t0 + tn; j += T) {
            const uint32_t v = val(j);
            if (v < p_min || v > p_max) continue;
            uint32_t lv[PEAKS_NEAR], rv[PEAKS_NEAR];
#pragma unroll
            for (int u = 0; u < PEAKS_NEAR; u++) {
                lv[u] = (u < near && j - 1 - u >= 0) ? val(j - 1 - u) : 0u;
                rv[u] = (u < near && j + 1 + u < nb) ? val(j + 1 + u) : 0u;
            }
            bool ok = true;
#pragma unroll
            for (int u = 0; u < PEAKS_NEAR; u++) {
                if (u < near && j - 1 - u >= 0 && lv[u] >= v) ok = false;
                if (rv[u] > v) ok = false;
            }
            if (!ok) continue;
            if (d <= PEAKS_NEAR) {  // the whole window is tested
                atomicOr(&bitmap[(j - t0) >> 5], 1u << ((j - t0) & 31));
                atomicAdd(&misc[PEAKS_MISC_ABOVE], 1u);
            } else {
                work[atomicAdd(&misc[PEAKS_MISC_WORK], 1u)] = (uint16_t)(j - t0);
            }
        }
        __syncthreads();
        // the survivors against the rest of their windows
        const int n_work = (int)misc[PEAKS_MISC_WORK];
        for (int w = tid; w < n_work; w += T) {
            const int j = t0 + (int)work[w];
            const uint32_t v = val(j);
            const int wl = max(0, j - d), wr = min(nb - 1, j + d);  // the window [wl, wr]
            const int bj = j >> BS, b_lo = bj << BS, b_hi = b_lo + BLK - 1;
            bool ok = true;
            for (int i = j - PEAKS_NEAR - 1; ok && i >= max(wl, b_lo); i--) ok = val(i) < v;
            for (int i = j + PEAKS_NEAR + 1; ok && i <= min(wr, b_hi); i++) ok = val(i) <= v;
            if (ok && wl < b_lo) {
                const int first_full = (wl + BLK - 1) >> BS;  // blocks [first_full, bj) lie inside the window
                for (int b = bj - 1; ok && b >= first_full; b--) ok = bm[b] < v;
                for (int i = min((first_full << BS) - 1, j - PEAKS_NEAR - 1); ok && i >= wl; i--) ok = val(i) < v;
            }
            if (ok && wr > b_hi) {
                // blocks (bj, end_full) lie inside the window; the span's last block ends at bin nb - 1
                const int end_full = wr == nb - 1 ? (wr >> BS) + 1 : (wr + 1) >> BS;
                for (int b = bj + 1; ok && b < end_full; b++) ok = bm[b] <= v;
                for (int i = max(end_full << BS, j + PEAKS_NEAR + 1); ok && i <= wr; i++) ok = val(i) <= v;
            }
            if (ok) {
                atomicOr(&bitmap[(j - t0) >> 5], 1u << ((j - t0) & 31));
                atomicAdd(&misc[PEAKS_MISC_ABOVE], 1u);
            }
        }
        __syncthreads();
        // the K largest keys of the list so far and this tile's bits, into the other list
        const int rounds = min(K, (int)min((unsigned)SDRG_PEAKS_MAX, misc[PEAKS_MISC_ABOVE]));
        const peaks_u64 *from = list + cur * SDRG_PEAKS_MAX;
        peaks_u64 *to = list + (cur ^ 1) * SDRG_PEAKS_MAX;
        peaks_u64 last = ~0ull;
        int cnt = 0;
        for (int it = 0; it < rounds; it++) {
            peaks_u64 m = 0ull;
            for (int i = tid; i < list_cnt; i += T) {
                const peaks_u64 key = from[i];
                if (key < last && key > m) m = key;
            }
            for (int w = tid; w < (tn + 31) >> 5; w += T) {
                uint32_t bits = bitmap[w];
                while (bits) {
                    const int bit = __ffs((int)bits) - 1;
                    bits &= bits - 1u;
                    const int j = t0 + 32 * w + bit;
                    const peaks_u64 key = ((peaks_u64)val(j) << 32) | (peaks_u64)(~(uint32_t)j);
                    if (key < last && key > m) m = key;
                }
            }
            if (tid == 0) best[(it + 1) % 3] = 0ull;  // last read two rounds ago
            if (m) atomicMax(&best[it % 3], m);
            __syncthreads();
            last = best[it % 3];
            if (last == 0ull) break;  // none left (every thread reads the same value)
            if (tid == 0) to[it] = last;
            cnt++;
        }
        __syncthreads();
        list_cnt = cnt;
        cur ^= 1;
    }

    // the table: `list_cnt` peaks, then {-1, 0, 0, 0}
    const peaks_u64 *fin = list + cur * SDRG_PEAKS_MAX;
    sdrg_peak *out = peaks + (size_t)blockIdx.x * (size_t)K;
    for (int i = tid; i < K; i += T) {
        sdrg_peak r = {-1, 0.0f, 0.0f, 0.0f};
        if (i < list_cnt) {
            const peaks_u64 key = fin[i];
            const float v = glibc::u2f((uint32_t)(key >> 32));
            const float db = 10.0f * glibc::log10f_fast(v + 1e-20f, tab);
            r.bin = p.lo + (int)(~(uint32_t)key);
            r.power = v;
            r.db = db;
            r.snr_db = db - floor_db;
        }
        out[i] = r;
    }
    if (tid == 0) {
        sdrg_peaks_summary sm;
        sm.count = list_cnt;
        sm.n_above = (int)misc[PEAKS_MISC_ABOVE];
        sm.floor_power = floor_power;
        sm.floor_db = floor_db;
        summary[blockIdx.x] = sm;
    }
}

template <int T, bool STAGED>
hipError_t launch_peaks_as(const float *spectra, int n_streams, const PeaksParams &p, sdrg_peak *peaks,
                           sdrg_peaks_summary *summary, hipStream_t stream) {
    const size_t lds = sizeof(uint32_t) * (size_t)peaks_layout(p.nb, STAGED).total;
    auto k = peaks_kernel<T, STAGED>;
    if (lds > 64 * 1024) {
        const hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void *>(k), (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k, dim3((unsigned)n_streams), dim3(T), lds, stream, spectra, p, peaks, summary);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_peaks(const float *spectra, int n_streams, const PeaksParams &p, sdrg_peak *peaks,
                        sdrg_peaks_summary *summary, hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    if (!spectra || !peaks || !summary || p.n < 1 || p.n > (1 << 20) || p.lo < 0 || p.nb < 1 ||
        (int64_t)p.lo + p.nb > p.n || p.max_peaks < 1 || p.max_peaks > SDRG_PEAKS_MAX || p.min_sep < 1 ||
        p.min_sep > SDRG_PEAKS_MAX_SEPARATION)
        return hipErrorInvalidValue;
    if (p.nb <= PEAKS_WAVE_BINS) return launch_peaks_as<PEAKS_WAVE, true>(spectra, n_streams, p, peaks, summary, stream);
    if (p.nb <= PEAKS_LDS_BINS) return launch_peaks_as<1024, true>(spectra, n_streams, p, peaks, summary, stream);
    return launch_peaks_as<1024, false>(spectra, n_streams, p, peaks, summary, stream);
}

}  // namespace sdrg
