// bank.hip — the DDC bank stage (sdrg_engine_bank_*): per stream, C channels at their own offsets: the raw IQ mixed down
// by each channel's NCO, filtered by one shared T-tap FIR and decimated by D, written as CF32 rows [n_streams * C][cap]
// (include/sdrg.h).  Row s C + c holds the bytes ddc.hip writes for stream s at that offset.
//
// The tile form of fir_tile.h (grid, history, staging, polyphase FIR), with a channel-group dimension: the grid is
// (tiles + 1, groups, streams), and a tile workgroup computes its tile of outputs for the `group` channels of its
// group.  The stage's own:
//   staging      the window of *unmixed* samples is read and unpacked once per workgroup, linearly into LDS (RawSink),
//                beside the taps and the NCO's two tables (16 KiB, as afc_pass_kernel keeps them: the phases differ
//                from row to row, so no phasor row can be shared as ddc.hip's is).
//   per channel  every lane mixes window samples u = tid, tid + 256, ... by ph = inc_c * (g0 + w0 + u) (ddc.hip's
//                products and order) into the polyphase image [u mod D][u / D]; then polyphase_fir and the store.  The
//                (r, q) of a lane's samples advance by (256 mod D, 256 / D) with a carry: no division per sample.
//   history      unmixed: 8 (T - 1) bytes per stream whatever C is.  v_c[g] is a pure function of g and x[g], so the
//                re-mixed history gives ddc.hip's bytes; a zero history mixes to +-0, which moves no sum that starts
//                at +0.  The closing workgroup of group 0 writes it; the closing workgroup of every group zeroes its
//                rows' tails.
//   window       BANK_LDS_SAMPLES = 2048 (ddc.hip: 3072): taps + tables + raw + image is 2 + 16 + 16 + 16 = 50 KiB, under
//                the 64 KiB a launch gets without an attribute, three workgroups per CU.
// Compiled with -ffp-contract=off: every product and sum of the mix and the FIR is rounded on its own.
#include "fir_tile.h"
#include "sdrg_internal.h"

namespace sdrg {
namespace {

constexpr int BANK_THREADS = 256;
#ifndef BANK_LAB_LDS_SAMPLES
#define BANK_LAB_LDS_SAMPLES 2048
#endif
constexpr int BANK_LDS_SAMPLES = BANK_LAB_LDS_SAMPLES;
// lab builds (tools/lab/bank_time.py): the group size scaled or forced to 1, and the mix left out (the raw sample goes
// to the image as it is: staging and FIR alone)
#ifndef BANK_LAB_GROUP_NUM
#define BANK_LAB_GROUP_NUM 1
#endif
#ifndef BANK_LAB_GROUP_DEN
#define BANK_LAB_GROUP_DEN 1
#endif
#ifndef BANK_LAB_SKIP_MIX
#define BANK_LAB_SKIP_MIX 0
#endif

constexpr int BANK_TAP_SLOTS = 256;   // float2 slots the taps take at the start of the LDS (512 floats)
constexpr int BANK_TAB_SLOTS = 2048;  // hi[1024] then lo[1024]

typedef float bank_f2 __attribute__((ext_vector_type(2)));

// x * hi[ph >> 22] * lo[(ph >> 12) & 1023]: ddc_phasor_kernel's and ddc_mix's products and order
__device__ __forceinline__ bank_f2 bank_mix(const float2 *tab, uint32_t ph, bank_f2 x) {
    const float2 h = tab[ph >> 22];
    const float2 l = tab[1024 + ((ph >> 12) & 1023)];
    const float wr = h.x * l.x - h.y * l.y, wi = h.x * l.y + h.y * l.x;
    bank_f2 v;
    v.x = x.x * wr - x.y * wi;
    v.y = x.x * wi + x.y * wr;
    return v;
}

// stage_iq_window's sink: the unmixed sample at window index u goes to raw[u]
template <int FMT>
struct RawSink {
    bank_f2 *raw;
    __device__ __forceinline__ void hist(int u, bank_f2 v) const { raw[u] = v; }
    __device__ __forceinline__ void sample(int u, int, float xr, float xi) const { raw[u] = bank_f2{xr, xi}; }
    __device__ __forceinline__ void chunk(int u0, int, const uint32_t (&w)[4]) const {
        constexpr int SPC = 16 / bytes_per_sample<FMT>();
#pragma unroll
        for (int s = 0; s < SPC; s++) {
            float xr, xi;
            iq_chunk_unpack<FMT>(w, s, xr, xi);
            raw[u0 + s] = bank_f2{xr, xi};
        }
    }
};

template <int FMT>
__global__ __launch_bounds__(BANK_THREADS) void bank_kernel(const char *__restrict__ iq, BankParams p, DdcTaps taps,
                                                            float *__restrict__ out) {
    constexpr int BPS = bytes_per_sample<FMT>();
    extern __shared__ __attribute__((aligned(16))) bank_f2 bank_lds[];
    const int tid = threadIdx.x, grp = blockIdx.y, b = blockIdx.z;
    const int N = p.n, D = p.decim, T = p.taps, H = T - 1, C = p.channels;
    const int c0 = grp * p.group, c1 = min(C, c0 + p.group);
    const char *frame = iq + (size_t)b * (size_t)N * BPS;
    const bank_f2 *hist_old = stream_history<bank_f2>(p.hist_old, b, H);
    bank_f2 *rows = reinterpret_cast<bank_f2 *>(out) + (size_t)b * (size_t)C * (size_t)p.cap;

    if ((int)blockIdx.x == p.n_tiles) {  // the stream's new history (group 0) and this group's zero tails
        if (grp == 0 && N > 0)
            carry_history<BANK_THREADS>(reinterpret_cast<bank_f2 *>(p.hist_new) + (size_t)b * (size_t)H, hist_old, N, H,
                                        tid, [&](int t) {
                                            return bank_f2{load_i1<FMT>(frame, t), load_q1<FMT>(frame, t)};
                                        });
        for (int c = c0; c < c1; c++) {
            bank_f2 *orow = rows + (size_t)c * (size_t)p.cap;
            for (int j = p.n_out + tid; j < p.cap; j += BANK_THREADS) orow[j] = bank_f2(0.0f);
        }
        return;
    }

    const FirWindow w(p, T);
    float *tap_lds = reinterpret_cast<float *>(bank_lds);  // the taps, the tables, the raw window, the image
    float2 *tab = reinterpret_cast<float2 *>(bank_lds + BANK_TAP_SLOTS);
    bank_f2 *raw = bank_lds + BANK_TAP_SLOTS + BANK_TAB_SLOTS;
    bank_f2 *smp = raw + p.row * D;
    stage_taps<BANK_THREADS>(tap_lds, taps.h, T, tid);
    {
        const float4 *from = reinterpret_cast<const float4 *>(p.nco_tab);  // a hipMalloc'ed table: aligned
        float4 *to = reinterpret_cast<float4 *>(tab);
#pragma unroll
        for (int j = 0; j < BANK_TAB_SLOTS / 2 / BANK_THREADS; j++) to[j * BANK_THREADS + tid] = from[j * BANK_THREADS + tid];
    }
    stage_iq_window<FMT, BANK_THREADS>(frame, hist_old, w.w0, w.count, H, p.vec_ok, tid, RawSink<FMT>{raw});

    // this lane's samples u = tid + 256 i sit at [r][q] = [u mod D][u / D]
    const int r0 = tid % D, q0 = tid / D, rs = BANK_THREADS % D, qs = BANK_THREADS / D;
    const uint32_t g_lane = p.g0_lo + (uint32_t)w.w0 + (uint32_t)tid;  // the global index of sample u = tid, mod 2^32
    const uint32_t *incs = p.incs + (size_t)b * (size_t)C;
    for (int c = c0; c < c1; c++) {
        __syncthreads();  // the window is staged; the previous channel's sums have read the image
        const uint32_t inc = incs[c], dph = inc * (uint32_t)BANK_THREADS;
        uint32_t ph = inc * g_lane;
        int r = r0, q = q0;
        for (int u = tid; u < w.count; u += BANK_THREADS) {
            smp[r * p.row + q] = BANK_LAB_SKIP_MIX ? raw[u] : bank_mix(tab, ph, raw[u]);
            ph += dph;
            r += rs, q += qs;
            if (r >= D) r -= D, q++;
        }
        __syncthreads();
        if (tid < w.nj) rows[(size_t)c * (size_t)p.cap + w.j0 + tid] = polyphase_fir(tap_lds, smp, T, D, p.row, tid);
    }
}

}  // namespace

int bank_tile_outputs(int decim, int taps) { return fir_tile_outputs(BANK_LDS_SAMPLES, BANK_THREADS, decim, taps); }

// Channels per workgroup: one while the rows alone (n_streams * channels) leave CUs without a workgroup, then a channel
// more for every 256 rows, up to 8: the staging of the raw window (about one channel's mix) is amortised over the group,
// and past 8 channels it is under an eighth of a workgroup's work.  Of the arguments alone: no call's N enters.
int bank_group(int channels, int n_streams) {
    const int rows = channels * n_streams;
    int g = std::min(std::max(rows / 256, 1), 8);
    g = g * BANK_LAB_GROUP_NUM / BANK_LAB_GROUP_DEN;
    return std::min(std::max(g, 1), channels);
}

hipError_t launch_bank(const void *iq, int fmt, int n_streams, const BankParams &p0, const DdcTaps &taps, float *out,
                       hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    BankParams p = p0;
    if (!iq || !out || !p.nco_tab || !p.incs || p.n < 1 || p.n > (1 << 20) || (p.taps > 1 && !p.hist_new) ||
        p.channels < 1 || p.channels > SDRG_BANK_MAX_CHANNELS || (int64_t)n_streams * p.channels > 65535 ||
        !fir_tile_plan(&p, BANK_LDS_SAMPLES, BANK_THREADS, SDRG_DDC_MAX_DECIMATION, SDRG_DDC_MAX_TAPS) ||
        p.cap != (p.n + p.decim - 1) / p.decim)  // the rows are as long as the frame's outputs can be
        return hipErrorInvalidValue;
    void (*k)(const char *, BankParams, DdcTaps, float *) = nullptr;
    const int bps = for_iq_format(fmt, [&](auto f) { k = bank_kernel<decltype(f)::value>; });
    if (bps == 0) return hipErrorInvalidValue;
    // rows of whole samples from a sample-aligned base: no sample straddles a 16-byte chunk
    p.vec_ok = reinterpret_cast<uintptr_t>(iq) % (size_t)bps == 0;
    p.group = bank_group(p.channels, n_streams);
    const int groups = (p.channels + p.group - 1) / p.group;
    const size_t lds = sizeof(float) * 2 * (2 * (size_t)p.row * (size_t)p.decim + BANK_TAP_SLOTS + BANK_TAB_SLOTS);
    hipLaunchKernelGGL(k, dim3((unsigned)p.n_tiles + 1, (unsigned)groups, (unsigned)n_streams), dim3(BANK_THREADS), lds,
                       stream, static_cast<const char *>(iq), p, taps, out);
    return hipGetLastError();
}

}  // namespace sdrg
