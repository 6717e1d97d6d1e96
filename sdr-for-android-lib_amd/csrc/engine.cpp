// engine.cpp — the C ABI (include/sdrg.h): configuration, per-stream state in HBM, kernel orchestration.
//
// Host-side equivalent of the reference's bridge + FFTProcessor + processSSB_opt control logic:
//   BridgeConfig::initialize / setters     src/bridge-config.h:17-65
//   FFTProcessor::configure                src/dsp/fft_process.cpp:20-39
//   processSSB_opt's static initialisation src/ssb/ssb_demod_opt.cpp:223-282 (mode globals, rfInit, eqInit)
//   soapyCallback's per-frame dispatch     src/sdr-bridge-java-soapy.cpp:424-493
// Everything that runs per sample runs in the HIP kernels (spectrum.hip, stats.hip, ssb.hip).
//
// Work is enqueued on a main HIP stream (spectrum -> stats) and a forked SSB stream that joins back,
// so the two independent halves of the hot path overlap on the GPU and a caller sees one stream.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "decim_cursor.h"
#include "design.h"
#include "gather_ranges.h"
#include "pulse_bank.h"
#include "sdrg_internal.h"

using namespace sdrg;

namespace {
thread_local std::string g_last_error;
}  // namespace

int32_t sdrg::fail(int32_t code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

// The attribute is one limit per (kernel, device) that each set overwrites, and launches asking for more than it
// fail; requests vary with the geometry (statistics) and N (any-N FFT), so the limit only ever rises: the largest
// value set so far is cached per (kernel, device), and a smaller request leaves it as it is.
hipError_t sdrg::ensure_dynamic_lds(const void *kernel, int bytes) {
    static std::mutex mu;
    static std::map<std::pair<const void *, int>, int> limit;  // (kernel, device) -> largest limit set
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lk(mu);
    const auto key = std::make_pair(kernel, dev);
    auto it = limit.find(key);
    if (it != limit.end() && it->second >= bytes) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) limit[key] = bytes;
    return e;
}

namespace {

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return fail(SDRG_E_HIP, "%s: %s", #expr, hipGetErrorString(e_));    \
    } while (0)


// processSSB_opt's statics that every stream of an engine shares (they only depend on the call sequence)
struct SsbControl {
    int64_t samp_count = 0;  // static size_t sampCount, frozen at the first call (:224)
    float agc_target = 0.35f, agc_fast = 0.006f, agc_slow = 0.00035f, gain = 0.5f;  // :17-28
    float lowpass_bd = 3200.0f, lowpass_q = 0.9f, transient_coeff = 0.55f;
    bool rf_init = false;
    float lpf[5] = {0, 0, 0, 0, 0};
    bool eq_init = false;
    float hp[5] = {0, 0, 0, 0, 0}, bp[5] = {0, 0, 0, 0, 0};
    // FIR taps currently uploaded (depend on samp_count, decim and the variant's tap count)
    int64_t taps_samp = -1;
    int taps_decim = -1, taps_req = -1, n_taps = 0;
};

// Page-locked host array (hipHostMalloc) for the host path's engine-owned copies: device-to-host copies into
// pageable memory go through the runtime's staging at a fraction of the PCIe rate.
template <class T>
struct PinnedVec {
    T *p = nullptr;
    size_t n = 0, cap = 0;
    PinnedVec() = default;
    PinnedVec(const PinnedVec &) = delete;
    PinnedVec &operator=(const PinnedVec &) = delete;
    ~PinnedVec() {
        if (p) (void)hipHostFree(p);
    }
    bool resize(size_t k) {  // contents are not preserved on growth (every use refills the array)
        if (k > cap) {
            if (p) (void)hipHostFree(p);
            p = nullptr;
            cap = n = 0;
            if (hipHostMalloc(reinterpret_cast<void **>(&p), sizeof(T) * k, hipHostMallocDefault) != hipSuccess) {
                p = nullptr;
                return false;
            }
            cap = k;
        }
        n = k;
        return true;
    }
    void assign(const T *a, const T *b) {
        if (resize((size_t)(b - a))) memcpy(p, a, sizeof(T) * (size_t)(b - a));
    }
    T *data() { return p; }
    T &operator[](size_t i) { return p[i]; }
};

// An event its owner creates where and with the flags it needs (once: a second create keeps the first) and that is
// destroyed with its owner, in sdrg_engine_destroy with the engine's device current.  Reads as the hipEvent_t.
struct Event {
    hipEvent_t ev = nullptr;
    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    ~Event() {
        if (ev) (void)hipEventDestroy(ev);
    }
    hipError_t create(unsigned flags) { return ev ? hipSuccess : hipEventCreateWithFlags(&ev, flags); }
    operator hipEvent_t() const { return ev; }
};

// stream-to-stream ordering on one device: no timing, no system-scope fence
constexpr unsigned EV_ORDER = hipEventDisableTiming | hipEventDisableSystemFence;

// A device allocation of n values that only grows (ensure_device, ensure_device_keeping, upload_floats) and frees itself
// with its owner (sdrg_engine_destroy: the engine's device current, its streams drained).  View says what p and n are
// read as: an array, or the two halves of a stage's PingPong.
template <typename T>
struct DeviceArray {
    T *p = nullptr;
    size_t n = 0;
};

template <typename T, typename View = DeviceArray<T>>
struct DeviceBuf : View {
    DeviceBuf &operator=(DeviceBuf &&o) noexcept {  // of another buffer (copies are not made): what this held is freed
        release();
        std::swap<View>(*this, o);
        return *this;
    }
    ~DeviceBuf() { release(); }
    void release() {  // freed (hipFree takes a null pointer, and waits for the kernels that use it) and empty again
        (void)hipFree(this->p);
        static_cast<View &>(*this) = View{};
    }
};

template <typename T>
using DevicePingPong = DeviceBuf<T, PingPong<T>>;

// The streaming stages' records: the configuration and whether one is set, the stream position, what the configuration
// designs, and the device buffers.

// DDC stage (sdrg_engine_set_ddc / ddc_device / ddc_host; ddc.hip)
struct DdcStage {
    sdrg_ddc_config cfg{};
    bool set = false;
    DecimCursor cur;
    uint32_t fs = 0;        // the sample rate of the previous ddc call (0: none since set_ddc)
    DevicePingPong<float> hist;  // halves of [n_streams][taps - 1][2]: the mixed samples before the next frame
    DeviceBuf<float> w;     // [N][2]: the phasors of the frame in flight, shared by the streams
    uint32_t taps_fs = 0;   // the sample rate taps was designed for (0: not designed)
    DdcTaps taps{};
    size_t half(int B) const { return (size_t)B * (size_t)(cfg.taps - 1) * 2; }
    void restart() {
        cur.restart();
        fs = 0;
    }
};

// DDC bank stage (sdrg_engine_set_bank / bank_retune / bank_device / bank_host; bank.hip)
struct BankStage {
    sdrg_bank_config cfg{};
    bool set = false;
    DecimCursor cur;
    uint32_t fs = 0;              // the sample rate of the previous bank call (0: none since set_bank)
    std::vector<double> offsets;  // [n_streams][channels], in force
    DevicePingPong<float> hist;   // halves of [n_streams][taps - 1][2]: the unmixed samples before the next frame
    // The increments [n_streams][channels] of `offsets` at inc_fs, in inc[inc_at] (inc_fs == 0: neither table holds
    // them).  A retune or another fs fills the other table, so a launch already issued keeps reading its own; read[i]
    // follows the last launch that read inc[i], and is waited for before inc[i] is filled again.
    DeviceBuf<uint32_t> inc[2];
    Event read[2];
    bool read_marked[2] = {false, false};
    int inc_at = 0;
    uint32_t inc_fs = 0;
    uint32_t taps_fs = 0;         // the sample rate taps was designed for (0: not designed)
    DdcTaps taps{};
    size_t rows(int B) const { return (size_t)B * (size_t)cfg.channels; }
    size_t half(int B) const { return (size_t)B * (size_t)(cfg.taps - 1) * 2; }
    void restart() {
        cur.restart();
        fs = 0;
    }
};

// demodulator stage (sdrg_engine_set_demod / demod_device / demod_host / ddc_demod_host; demod.hip)
struct DemodStage {
    sdrg_demod_config cfg{};
    bool set = false;
    DecimCursor cur;
    float kf = 0.0f, alpha = 0.0f, a = 0.0f;  // demod_design of cfg
    DemodTaps taps{};
    DevicePingPong<float> state;  // halves of {[n_streams][4]: wr, wi, m, s; [n_streams][T2 - 1]: v}
    DeviceBuf<float> scratch;  // [n_streams][max_in]: e, then v, of the call in flight
    int cap() const { return DecimCursor::cap(cfg.max_in, cfg.audio_decimation); }
    size_t half(int B) const { return (size_t)B * 4 + (size_t)B * (size_t)(cfg.audio_taps - 1); }
};

// channelizer stage (sdrg_engine_set_channelizer / channelizer_device / channelizer_host; channelizer.hip)
struct ChanStage {
    sdrg_channelizer_config cfg{};
    bool set = false;
    DecimCursor cur;
    DevicePingPong<float> hist;  // halves of [n_streams][L - 1][2]: the unpacked samples before the next frame
    DeviceBuf<float> d_taps;  // [L] taps, then [CHAN_TWIDDLES][2]: written by set_channelizer
    int decim() const { return cfg.channels / cfg.oversample; }
    size_t half(int B) const { return (size_t)B * ((size_t)cfg.channels * (size_t)cfg.taps_per_channel - 1) * 2; }
};

// resampler stage (sdrg_engine_set_resample / resample_device / resample_host / ddc_demod_resample_host;
// resample.hip)
struct ResampleStage {
    sdrg_resample_config cfg{};
    bool set = false;
    ResampleCursor cur;
    std::vector<float> taps;  // resample_design of cfg: the prototype, [L P]
    DevicePingPong<float> hist;  // halves of [n_streams][P - 1][components]: the values before the next call's
    DeviceBuf<float> d_taps;  // the prototype in polyphase order [L][P]: written by set_resample
    int cap() const { return ResampleCursor::cap(cfg.max_in, cfg.interp, cfg.decim); }
    size_t half(int B) const { return (size_t)B * (size_t)(cfg.taps_per_phase - 1) * (size_t)cfg.components; }
};

// what a block stage (block_stage.h) keeps, whichever its law; Config has block, hang_blocks and max_in
template <typename Config>
struct BlockStage {
    Config cfg{};
    bool set = false;
    BlockCursor cur;
    // halves of [n_streams][S + BLOCK_STATE_HEAD]: the law's four words, the block's powers so far
    DevicePingPong<float> state;
    DeviceBuf<float> blk;   // [the most blocks a call completes][n_streams]: the blocks' statistics, then the law's words
    size_t half(int B) const { return (size_t)B * (size_t)(cfg.block + BLOCK_STATE_HEAD); }
};

// squelch stage (sdrg_engine_set_squelch / squelch_device / squelch_host / ddc_squelch_demod_host; squelch.hip)
struct SquelchStage : BlockStage<sdrg_squelch_config> {
    float open_thr = 0.0f, close_thr = 0.0f, beta = 0.0f;  // squelch_design of cfg
};

// AGC stage (sdrg_engine_set_agc / agc_device / agc_host / listen_host; agc.hip)
struct AgcStage : BlockStage<sdrg_agc_config> {
    float target = 0.0f;  // cfg.target as a float
    AgcDesign des{};      // agc_design of cfg
};

// IQ correction stage (sdrg_engine_set_iqcorr / iqcorr_device / iqcorr_host / iqcorr_process_host; iqcorr.hip)
struct IqcorrStage {
    sdrg_iqcorr_config cfg{};
    bool set = false;
    BlockCursor cur;
    float beta_dc = 0.0f, beta_bal = 0.0f, floor_thr = 0.0f;  // iqcorr_design of cfg
    // halves of [n_streams][2 S + IQCORR_STATE_HEAD]: the twelve words, the block's scaled samples so far
    DevicePingPong<float> state;
    DeviceBuf<float> blk;  // [the most blocks a call completes]: [5][n_streams] moments, then as many [4][n_streams] theta
    // iqcorr_process_host's: the corrected frame, [n_streams][samples_per_reading][2], and the records
    DeviceBuf<float> rows;
    DeviceBuf<sdrg_iqcorr_record> rec;
    size_t half(int B) const { return (size_t)B * (size_t)(2 * cfg.block + IQCORR_STATE_HEAD); }
    size_t blocks() const { return (size_t)BlockCursor::cap(cfg.max_in, cfg.block); }
};

// AFC stage (sdrg_engine_set_afc / afc_device / afc_host / listen_afc_host; afc.hip)
struct AfcStage {
    sdrg_afc_config cfg{};
    bool set = false;
    BlockCursor cur;
    sdrg_afc_design_values des{};  // afc_design of cfg
    // halves of [n_streams][2 S + AFC_STATE_HEAD]: the eight words, the block's samples so far
    DevicePingPong<float> state;
    // [the most blocks a call completes]: [3][n_streams] moments, then one more of [2][n_streams] words (Phi, inc)
    DeviceBuf<float> blk;
    bool track() const { return cfg.mode == SDRG_AFC_TRACK; }
    size_t half(int B) const { return (size_t)B * (size_t)(2 * cfg.block + AFC_STATE_HEAD); }
    size_t blocks() const { return (size_t)BlockCursor::cap(cfg.max_in, cfg.block); }
};

// noise blanker stage (sdrg_engine_set_blanker / blanker_device / blanker_host / clean_process_host; blanker.hip)
struct BlankerStage {
    sdrg_blanker_config cfg{};
    bool set = false;
    BlockCursor cur;
    float beta = 0.0f, ratio = 0.0f, floor_thr = 0.0f;  // blanker_design of cfg
    // halves of [n_streams][blanker_state_words(S)]: the head, the block's powers so far, the flags, the last samples
    DevicePingPong<float> state;
    DeviceBuf<float> blk;  // [the most blocks a call completes][n_streams] floors, then as many thresholds
    // clean_process_host's: the blanked frame, [n_streams][samples_per_reading][2], and the records
    DeviceBuf<float> rows;
    DeviceBuf<sdrg_blanker_record> rec;
    size_t half(int B) const { return (size_t)B * (size_t)blanker_state_words(cfg.block); }
    size_t blocks() const { return (size_t)BlockCursor::cap(cfg.max_in, cfg.block); }
};

// tone detector stage (sdrg_engine_set_tones / tones_device / tones_host / listen_tones_host; tones.hip)
struct TonesStage {
    sdrg_tones_config cfg{};
    bool set = false;
    BlockCursor cur;
    sdrg_tones_scalars sc{};  // tones_design of cfg
    DeviceBuf<float> d_design;  // the table [K][S][2], then wf [S]: written by set_tones
    // halves of [n_streams][tones_state_words(K, components)]: the head, the accumulators, the sub-block's values so far
    DevicePingPong<float> state;
    DeviceBuf<float> sums;  // [n_streams][the call's sub-blocks][2 K + 1]: the sub-blocks' sums of the call in flight
    int S() const { return TONES_SUB * cfg.sub_blocks; }
    int cap_blocks() const { return BlockCursor::cap(cfg.max_in, S()); }
    size_t half(int B) const { return (size_t)B * (size_t)tones_state_words(cfg.n_tones, cfg.components); }
};

// symbol stage (sdrg_engine_set_symbols / symbols_device / symbols_host / listen_symbols_host; symbols.hip)
struct SymbolsStage {
    sdrg_symbols_config cfg{};
    bool set = false;
    BlockCursor cur;
    sdrg_symbols_design_values des{};  // symbols_design of cfg
    DeviceBuf<float> d_tab;            // the table [SDRG_SYM_TABLE][2]: written by set_symbols
    // halves of [n_streams][sym_state_words(S)]: the step's words, the history, the block's values so far
    DevicePingPong<float> state;
    // [the most blocks a call completes]: [5][n_streams] moments, then one more of [4][n_streams] words
    DeviceBuf<float> blk;
    bool soft() const { return cfg.format == SDRG_SYM_SOFT; }
    int cap() const { return (int)(((uint64_t)des.inc * (uint64_t)cfg.max_in) >> 32) + 1; }
    size_t width() const { return soft() ? sizeof(float) : 1; }  // bytes per symbol
    size_t half(int B) const { return (size_t)B * (size_t)sym_state_words(cfg.block); }
    size_t blocks() const { return (size_t)BlockCursor::cap(cfg.max_in, cfg.block); }
};

// sideband stage (sdrg_engine_set_sideband / sideband_device / sideband_host / listen_sideband_host; sideband.hip)
struct SidebandStage {
    sdrg_sideband_config cfg{};
    bool set = false;
    DecimCursor cur;
    std::vector<float> cr, ci;  // sideband_design of cfg
    DevicePingPong<float> hist;  // halves of [n_streams][taps - 1][2]: the samples before the next call's
    DeviceBuf<float> d_taps;    // [taps][2]: (cr, ci), written by set_sideband
    int cap() const { return DecimCursor::cap(cfg.max_in, cfg.audio_decimation); }
    int width() const { return cfg.mode == SDRG_SIDEBAND_BOTH ? 2 : 1; }  // values per output
    size_t half(int B) const { return (size_t)B * (size_t)(cfg.taps - 1) * 2; }
};

// The stages that read spectra: the configuration and whether one is set, what the calls carry, the host calls' rows.

// display stage (sdrg_engine_set_display / display_device / display_host; display.hip)
struct DisplayStage {
    sdrg_display_config cfg{};
    bool set = false;
    DeviceBuf<unsigned char> out;  // the host calls' rows
};

// integration stage (sdrg_engine_set_integration / integrate_device / integrate_host; integrate.hip)
struct IntegrateStage {
    sdrg_integrate_config cfg{};
    bool set = false;
    int64_t t = 0;      // integrate calls since the last reset
    int32_t depth = 0;  // frames the last output integrates
    bool seen = false;  // n, fs and fc hold the configuration at the previous integrate call
    int n = 0;
    int64_t fs = 0, fc = 0;
    DeviceBuf<float> ring;  // MEAN / MAX: [period][integrate_slot_stride(n_streams * N)]
    DeviceBuf<float> ema;   // EMA: y [n_streams][N]
    DeviceBuf<float> out;   // integrate_host's rows (history, as the two above: ensure_device_keeping)
    int out_n = 0;          // N of the rows the last integrate_host call left in out
    void restart() { t = 0, depth = 0; }  // the integration history is forgotten
};

// peak table stage (sdrg_engine_set_peaks / peaks_device / peaks_host; peaks.hip)
struct PeaksStage {
    sdrg_peaks_config cfg{};
    bool set = false;
    DeviceBuf<unsigned char> out;  // the host calls' tables: [n_streams][max_peaks] sdrg_peak, then the summaries
};

// The records of what one call owes another.  Each owns its events: it creates them, and they go with it.

template <size_t N>  // each handle on its own: a failed earlier attempt leaves no null behind in use
int32_t create_events(Event (&evs)[N], unsigned flags) {
    for (Event &ev : evs) HIP_TRY(ev.create(flags));
    return SDRG_OK;
}

// sdrg_engine_gather runs on a stream of its own choosing after the outputs it reads; a later call that writes a buffer
// still being gathered waits for the gather on the GPU first, so a caller rotating its output buffers never delays its
// next call's kernels behind a gather.  Each gather's end sits in a ring; a range a gather read maps to that gather's
// slot (gather_ranges.h), so a call that rewrites it waits for that gather only (waiting on the last gather instead
// made call k + 3's spectrum wait for gather k + 2, and with it for call k + 2's asynchronous statistics).
struct Gathers {
    static constexpr int GRING = 8;
    GatherRanges ranges;
    Event ev_g[GRING];  // created at the slot's first gather
    int64_t g_calls = 0;
    hipEvent_t ev_gather = nullptr;       // the last gather's end, one of ev_g (wait_outputs)
    hipStream_t s_last_gather = nullptr;  // the stream of the last gather

    // a call is about to write [p, p + bytes) on `stream`: after the latest gather that reads any byte of it
    int32_t wait_before_write(hipStream_t stream, const void *p, size_t bytes) const {
        const int slot = ranges.latest(p, bytes);
        if (slot >= 0) HIP_TRY(hipStreamWaitEvent(stream, ev_g[slot], 0));
        return SDRG_OK;
    }
    void written(const void *p, size_t bytes) { ranges.retire(p, bytes); }  // and has enqueued that write

    // A gather is about to run on s.  The focus staging buffer and RCCL's issue order: it follows the previous one
    // even on another stream.
    int32_t begin(hipStream_t s) {
        HIP_TRY(ev_g[g_calls % GRING].create(EV_ORDER));
        if (ev_gather && s != s_last_gather) HIP_TRY(hipStreamWaitEvent(s, ev_gather, 0));
        s_last_gather = s;
        return SDRG_OK;
    }
    // It is enqueued, and read these buffers, mapped to its slot; a slot re-recorded by a later gather still covers
    // this one (gathers follow each other).
    int32_t end(hipStream_t s, std::initializer_list<std::pair<const void *, size_t>> reads) {
        const int slot = (int)(g_calls % GRING);
        HIP_TRY(hipEventRecord(ev_g[slot], s));
        ev_gather = ev_g[slot];
        for (const auto &r : reads) ranges.record(r.first, r.second, slot, g_calls);
        g_calls++;
        return SDRG_OK;
    }
};

// SDRG_PIPELINE_STATS_ASYNC: a pipelined call's statistics (+ spectral pulse detector) run on s_stats after its
// spectrum, beside the next call's spectrum.  The engine keeps the spectra a call's statistics read intact: a call
// that writes the same spectra buffer as the call before waits (on the GPU) for that call's statistics, and the host
// waits for the statistics of the call two before (so a caller rotating two or more spectra buffers never waits on
// the GPU).
struct AsyncStats {
    static constexpr int SA_RING = 3;
    Event ev_spec_done;               // after a call's spectrum on its stream, waited by s_stats
    Event ev_end[SA_RING];            // end of the statistics of call (calls - k) at slot % SA_RING
    const float *spec[SA_RING] = {};  // the spectra buffer each of those calls' statistics read
    bool live[SA_RING] = {};
    int64_t calls = 0;
    hipEvent_t last_end = nullptr;  // the last asynchronous statistics (signal_strength, wait_outputs, gather)

    int32_t create() {  // sdrg_engine_set_pipelining with the bit
        HIP_TRY(ev_spec_done.create(EV_ORDER));
        return create_events(ev_end, EV_ORDER);
    }
    // Before a spectrum into `to` on sm, of a call whose own statistics will run on s_stats (`async`) or on sm: the
    // host's wait, and the GPU's.
    int32_t before_spectrum(hipStream_t sm, const float *to, bool async) const {
        if (calls >= 2 && live[(calls - 2) % SA_RING]) HIP_TRY(hipEventSynchronize(ev_end[(calls - 2) % SA_RING]));
        const int pv = (int)((calls + SA_RING - 1) % SA_RING);
        if (calls >= 1 && live[pv] && (spec[pv] == to || !async)) HIP_TRY(hipStreamWaitEvent(sm, ev_end[pv], 0));
        return SDRG_OK;
    }
    int32_t after_stats(hipStream_t st, const float *from) {  // the statistics of `from` are enqueued on st
        const int k = (int)(calls % SA_RING);
        HIP_TRY(hipEventRecord(ev_end[k], st));
        spec[k] = from;
        live[k] = true;
        calls++;
        last_end = ev_end[k];
        return SDRG_OK;
    }
    // a write of count floats at dst on `stream` (in-place integration of a call's own spectra): after the statistics
    // that may still read any of them
    int32_t wait_before_write(hipStream_t stream, const float *dst, size_t count) const {
        for (int k = 0; k < SA_RING; k++)
            if (live[k] && spec[k] < dst + count && dst < spec[k] + count)
                HIP_TRY(hipStreamWaitEvent(stream, ev_end[k], 0));
        return SDRG_OK;
    }
};

// The audio pulse detector (AudioPulseDetector::process after processSSB_opt, ssb_processor.cpp:109) runs on s_ap after
// the call's SSB pipeline, so the SSB stream (the pipelined step's critical path) carries the SSB kernels alone.  Call
// k's front end (inside its SSB kernel) writes energy-frame set k % NEW_SETS; before it does, the host waits for the
// detector of call k - NEW_SETS, which read that set.
struct AudioDetect {
    Event ev_end[sdrg_pulse_bank::NEW_SETS];  // created with the engine
    bool live[sdrg_pulse_bank::NEW_SETS] = {};
    int64_t calls = 0;
    hipEvent_t last_end = nullptr;  // the last detector (outputs, joins)

    int set() const { return (int)(calls % sdrg_pulse_bank::NEW_SETS); }  // what the next call with the stage writes
    int32_t detected(hipStream_t s_ap) {  // that call's detector is enqueued on s_ap
        const int k = set();
        HIP_TRY(hipEventRecord(ev_end[k], s_ap));
        live[k] = true;
        last_end = ev_end[k];
        calls++;
        return SDRG_OK;
    }
};

struct EvSet {
    Event t0, spec, stats, ssb0, ssb1, end;
    bool has_spec = false, has_stats = false, has_ssb = false, pending = false;
    bool ssb_timed = false;  // ssb0 recorded: this call's SSB duration is measured from its own start marker
    int64_t seq = -1;        // the call's number among ALL calls (pipelined SSB: interval to call seq - 1, if profiled)
    bool stats_marked = false;  // `stats` recorded after the statistics (joined calls, whose `end` follows the join)
};

// profiling: a ring of event sets so consecutive calls are timed without host synchronisation
struct Profiler {
    static constexpr int RING = 64;
    EvSet ring[RING];
    int next = 0, last = -1;
    bool on = false;
    sdrg_timings last_timings{};
    double sum_spec = 0, sum_stats = 0, sum_ssb = 0, sum_total = 0;
    int n_acc = 0, n_ssb = 0;
    int64_t seq_reset = 0;  // seq of the first call after the last reset of the timing statistics

    int32_t create();  // sdrg_engine_set_profiling(1): the first makes the events
    int32_t fold_slot(int slot);
    int32_t fold_all();
    EvSet *begin(int64_t seq, bool do_spec, bool do_stats, bool do_ssb, bool early_fork, bool stats_async);
    void commit() {  // the call of begin()'s slot is enqueued
        ring[next].pending = true;
        last = next;
        next = (next + 1) % RING;
    }
    void reset(int64_t calls_total) {  // after fold_all
        sum_spec = sum_stats = sum_ssb = sum_total = 0;
        n_acc = n_ssb = 0;
        // a pipelined call's SSB interval starts at the previous call's end marker: the window's first call has none
        seq_reset = calls_total;
    }
};

}  // namespace

struct sdrg_engine {
    sdrg_config cfg{};  // BridgeConfig: what the next frame is cut, demodulated and reported with
    // FFTProcessor::config_ (fft_process.h:88, :20-39): the centre frequency, sample rate and focus the statistics
    // use, copied from cfg at each configure() point (create, applyConfig, setFrequency, setFrequencyFocusRange).
    // setSampleRate / setSamplesPerReading / setSoundMode change cfg only (sdr-bridge-java-soapy.cpp:931-1023).
    uint32_t fft_fc = 0, fft_fs = 0;
    int32_t fft_focus = 0;
    int n_streams = 0;
    int device = 0;
    hipStream_t s_main = nullptr, s_ssb = nullptr;
    // CU split (SDRG_CU_SPLIT, lab): the SSB stream and a spectrum/statistics stream restricted to disjoint
    // halves of the CUs (hipExtStreamCreateWithCUMask), so the latency-bound SSB waves share no SIMD with the
    // spectrum's; s_spec is forked from / joined into s_main per call like the SSB stream
    hipStream_t s_spec = nullptr;
    int spec_cus = 0;
    Event ev_fork_spec, ev_join_spec;
    hipStream_t s_own = nullptr;  // the engine's own main stream (s_main is it, or the caller's via set_stream)
    Event ev_fork, ev_join;
    // input release: recorded after the last kernel of a call that reads its iq buffer on each stream (the
    // spectrum on s_main, the SSB pipeline on s_ssb); sdrg_engine_input_released / _wait_input_released
    Event ev_in_main, ev_in_ssb;
    // the markers the last call recorded after its iq readers (ev_in_* or the profiling ring's events)
    hipEvent_t last_in_main = nullptr, last_in_ssb = nullptr;
    Profiler prof;
    int64_t calls_total = 0;  // every enqueue, profiled or not: two calls are consecutive only if their seqs are

    // device state / buffers
    DeviceBuf<StatsState> d_stats;
    DeviceBuf<SsbStreamState> d_ssb;
    DeviceBuf<float> d_twiddles;
    int tw_n = 0;  // the N d_twiddles holds the table of
    DeviceBuf<float> d_taps;
    DeviceBuf<int> d_chunk_table;  // per SSB pipeline chunk: FIR outputs overlapping / completed
    DeviceBuf<float> d_ssb_scratch;
    DeviceBuf<float> d_spec_scratch;
    DeviceBuf<float> d_focus_stage;  // sdrg_engine_gather: the focus-window slices, packed for ncclGather
    bool last_async_stats = false;  // the last call with a statistics stage ran it on s_stats
    bool lab_ssb_first = false;     // lab SDRG_SSB_FIRST: host launch order of a forked SSB stage
    bool lab_stats_cus = false;     // lab SDRG_STATS_CUS: s_stats and s_spec on disjoint CU masks
    hipStream_t s_gather = nullptr;  // lab (SDRG_GATHER_STREAM=1): the gathers on a stream of their own
    Gathers gathers;
    DeviceBuf<float> d_fft_scratch;  // four-step intermediate (N > 16384)
    DeviceBuf<sdrg_frame_record> d_rec_scratch;
    DeviceBuf<float> d_pool;  // statistics' pooled bins beyond the LDS bound (wide focus, N > 65536)
    // host-path staging
    DeviceBuf<char> d_iq_stage;
    DeviceBuf<float> d_spec_stage;
    int host_spec_n = 0;  // N of the spectra the last process_host call with SPECTRUM left in d_spec_stage
    // The caller's spectra, [n_streams][N], of signal_strength_host, display_host, integrate_host and peaks_host.
    // Not d_spec_stage: that one carries each stream's never-written bin N-1 of an odd N from one process_host call
    // to the next (fft_process.cpp:92-97), which a caller's spectra must not replace.  One buffer serves the four:
    // each of them waits on s_main before it returns, so no two uses overlap, and a call that fails after its copy
    // was enqueued leaves that copy ordered on s_main before whatever the next call enqueues there.
    DeviceBuf<float> spec_in;
    DeviceBuf<sdrg_frame_record> d_rec_stage;
    DeviceBuf<int16_t> d_pcm_stage;
    PinnedVec<float> h_spec;
    PinnedVec<sdrg_frame_record> h_rec;
    PinnedVec<int16_t> h_pcm;

    SsbControl ssb;
    // pulse detectors (created at the first call that runs their stage)
    sdrg_pulse_config spec_pulse_cfg{}, audio_pulse_cfg{};
    sdrg_pulse_bank spec_bank, audio_bank;
    bool spec_bank_live = false, audio_bank_live = false;
    PinnedVec<sdrg_pulse_output> h_pspec, h_paudio;
    bool cf_changed_pending = false;
    bool pipelined = false;  // sdrg_engine_set_pipelining: no join of the SSB stream per call
    bool inputs_ready = false;  // SDRG_PIPELINE_INPUTS_READY: no fork wait on the main stream either
    bool stats_async = false;  // SDRG_PIPELINE_STATS_ASYNC (AsyncStats)
    hipStream_t s_stats = nullptr;
    AsyncStats sa;
    hipStream_t s_ap = nullptr;  // the audio pulse detector's (AudioDetect)
    AudioDetect ap;
    // NCO/short-FIR SSB variant (sdrg_engine_set_ssb_variant; a build extension, off by default)
    double nco_hz = 0.0;
    int fir_taps = 0;            // 0: the reference's 255
    uint32_t nco_phase = 0;      // phase of the next call's first sample (advances by inc * samp_count)
    DeviceBuf<float> d_nco_tab;  // nco_tables(), uploaded once
    int upper = 1;
    bool has_cbs = false;
    sdrg_callbacks cbs{};
    // The device calls of the stages below (display, integration, peaks, DDC, demodulator, channelizer, resampler,
    // squelch, AGC, sideband, IQ correction) write their outputs on s_main after the last process call's end marker, which is all a
    // stream other than s_main follows.  Each sets outputs_unmarked; sdrg_engine_wait_outputs then records ev_outputs
    // on s_main for that stream to wait on.
    Event ev_outputs;  // created at the first such wait
    bool outputs_unmarked = false;
    // the stages that read spectra (DisplayStage, IntegrateStage, PeaksStage above)
    DisplayStage disp;
    IntegrateStage integ;
    PeaksStage peaks;
    // the streaming stages (DdcStage ... AgcStage above)
    DdcStage ddc;
    BankStage bank;
    DemodStage demod;
    ChanStage chan;
    ResampleStage rs;
    SquelchStage sq;
    AgcStage agc;
    SidebandStage sb;
    IqcorrStage iqc;
    AfcStage afc;
    BlankerStage blank;
    TonesStage tones;
    SymbolsStage sym;
    // The staging of the streaming stages' host calls (ddc_host, demod_host, channelizer_host, resample_host,
    // squelch_host, agc_host, iqcorr_host and the chains), as bytes: the caller's input, and the rows it gets back (with the squelch's
    // and the AGC's records behind them).  One pair serves them all, as spec_in does its
    // four: each of them waits on s_main before it returns, so no two uses overlap, and a call that fails after its
    // copy was enqueued leaves that copy ordered on s_main before whatever the next call enqueues there.
    DeviceBuf<char> stream_in, stream_out;
    // what a chain call leaves on the device, for the same reason one of each: the channel between the DDC and the
    // demodulator, [n_streams][the DDC's cap][2], and the float audio between the demodulator and the resampler,
    // [n_streams][the demodulator's cap]
    DeviceBuf<float> chain_chan, chain_audio;
};

namespace {

// applyConfig's SpectralPulseDetector configuration (sdr-bridge-java-soapy.cpp:1130-1138): the default
// Config with fsEnergy = sampleRate / samplesPerReading (20 when samplesPerReading <= 0)
sdrg_pulse_config spectral_pulse_cfg_for(const sdrg_config &c) {
    sdrg_pulse_config p;
    sdrg_pulse_config_default(SDRG_PULSE_SPECTRAL, &p);
    p.fs_energy = c.samples_per_reading > 0 ? (float)c.sample_rate / (float)c.samples_per_reading : 20.f;
    return p;
}

// FFTProcessor::configure(FftProcessorConfig{cf, fs, N, focus}) with the bridge's current values
void configure_fft(sdrg_engine *e) {
    e->fft_fc = (uint32_t)e->cfg.center_frequency;
    e->fft_fs = (uint32_t)e->cfg.sample_rate;
    e->fft_focus = e->cfg.freq_focus_range_khz;
}

int32_t validate_config(const sdrg_config *cfg) {
    if (!cfg) return fail(SDRG_E_INVALID, "null config");
    if (cfg->samples_per_reading < 1 || cfg->samples_per_reading > (1 << 20))
        return fail(SDRG_E_UNSUPPORTED, "samples_per_reading %d outside [1, 2^20]", cfg->samples_per_reading);
    if ((uint32_t)cfg->sample_rate == 0) return fail(SDRG_E_INVALID, "sample_rate must be > 0");
    if (cfg->freq_focus_range_khz < 0) return fail(SDRG_E_INVALID, "freq_focus_range_khz must be >= 0");
    return SDRG_OK;
}

// hipMemset is enqueued on the null stream, which the engine's non-blocking streams are not ordered with: without
// the wait, a kernel or copy enqueued next on s_main could run before (or under) the fill -- e.g. a fresh staging
// buffer zeroed after the caller's spectra were copied into it.  Fills happen at allocation and reset only.
hipError_t memset_sync(void *p, int v, size_t bytes) {
    hipError_t e = hipMemset(p, v, bytes);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    return e;
}

// Growth of a buffer that holds nothing across calls (staging, outputs, scratch): the old allocation is freed first,
// so the two never exist together, and a call that cannot have the new one leaves the buffer empty
// `zero`: filled with zeros when allocated or regrown, and only then.
template <typename T, typename View>
int32_t ensure_device(DeviceBuf<T, View> *b, size_t need, bool zero = false) {
    if (b->n >= need && b->p) return SDRG_OK;
    b->release();
    if (need == 0) return SDRG_OK;
    const hipError_t er = hipMalloc(reinterpret_cast<void **>(&b->p), need * sizeof(T));
    if (er == hipErrorOutOfMemory) {  // for every growth policy: each allocates here
        (void)hipGetLastError();
        return fail(SDRG_E_NOMEM, "hipMalloc of %zu bytes failed", need * sizeof(T));
    }
    HIP_TRY(er);
    if (zero) HIP_TRY(memset_sync(b->p, 0, need * sizeof(T)));
    b->n = need;
    return SDRG_OK;
}

// Growth of a buffer that holds history (the integration stage's ring, EMA rows and output rows): the new buffer
// first, so a call that cannot have it leaves the old one (and the history in it) as it was
template <typename T>
int32_t ensure_device_keeping(DeviceBuf<T> *b, size_t need) {
    if (b->n >= need && b->p) return SDRG_OK;
    DeviceBuf<T> grown;
    const int32_t rc = ensure_device(&grown, need);
    if (rc) return rc;
    *b = std::move(grown);  // frees the old one, which synchronises with the kernels that use it
    return SDRG_OK;
}

// Both halves of a decimating stage's ping-pong buffer.  Only another configuration asks for more, and setting one
// restarts the streams: nothing to keep.  Never empty: a launcher wants a pointer even to a history of no values.
template <typename T>
int32_t ensure_halves(DevicePingPong<T> *b, size_t half_elems) {
    return ensure_device(b, std::max<size_t>(2 * half_elems, 2));
}

// The two ends of a streaming stage's or a chain's host call on the main stream: the caller's `in` into stream_in, with
// stream_out made ready for the rows; and those rows to the caller's `out`, and the wait.  Between the two the launches
// read stream_in.p and write stream_out.p.
int32_t host_begin(sdrg_engine *e, const void *in, size_t in_bytes, size_t out_bytes) {
    int32_t rc = ensure_device(&e->stream_in, in_bytes);
    if (rc) return rc;
    rc = ensure_device(&e->stream_out, out_bytes);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(e->stream_in.p, in, in_bytes, hipMemcpyHostToDevice, e->s_main));
    return SDRG_OK;
}

int32_t host_end(sdrg_engine *e, void *out, size_t out_bytes) {  // no rows (the AFC measuring): the wait alone
    if (out_bytes) HIP_TRY(hipMemcpyAsync(out, e->stream_out.p, out_bytes, hipMemcpyDeviceToHost, e->s_main));
    HIP_TRY(hipStreamSynchronize(e->s_main));
    return SDRG_OK;
}

// These host floats become the device buffer *d (`what`: whose they are, for the message).  They go into a buffer of
// their own, so a failed copy leaves the old one in force; the old one is freed afterwards, which waits for the calls
// that still read it.
int32_t upload_floats(DeviceBuf<float> *d, const std::vector<float> &host, const char *what) {
    DeviceBuf<float> fresh;
    const int32_t rc = ensure_device(&fresh, host.size());
    if (rc) return rc;
    const hipError_t er = hipMemcpy(fresh.p, host.data(), sizeof(float) * host.size(), hipMemcpyHostToDevice);
    if (er != hipSuccess) return fail(SDRG_E_HIP, "%s upload: %s", what, hipGetErrorString(er));
    *d = std::move(fresh);
    return SDRG_OK;
}

// nco_tables() on the device, uploaded once: the SSB variant's mixer and the DDC's read the same table
int32_t ensure_nco_table(sdrg_engine *e) {
    if (e->d_nco_tab.p) return SDRG_OK;
    std::vector<float> tab(4096);
    nco_tables(tab.data());
    return upload_floats(&e->d_nco_tab, tab, "NCO table");
}

// ---- the streaming stages: DDC, DDC bank, demodulator, channelizer, resampler, squelch, AGC, sideband, IQ correction, blanker,
// ---- tone detector, AFC --------------------------------------------------------------------------------------------
//
// A call of a stage goes through three steps.  x_resolve makes every refusal and touches nothing; what it finds goes
// into the stage's XCall.  x_reserve does everything that can fail without a launch (the stage's device buffers, the
// NCO table, the DDC's taps) and commits no cursor.  x_launch fills the kernel's parameters, launches, and only then
// advances the cursor.  stage_call runs the three for one stage, chain_host for several.

// what every resolved call has; the DDC's and the channelizer's calls add what their own launches need
struct StageCall {
    int n = 0, n_out = 0, cap = 0;       // samples per stream in, outputs per row, the row length of `out`
    // Values between the rows of the input, for the stages that read rows another stage may have written: the stage's
    // max_in or the caller's, or in a chain the DDC's cap.  The block stages' `out` has the same rows.
    int in_stride = 0;
    size_t in_bytes = 0, out_bytes = 0;  // a host call's input and output
    // A second output, which the squelch and the AGC have (their records): where the launch writes it, nullptr if the
    // caller wants none, and its size.
    void *aux = nullptr;
    size_t aux_bytes = 0;
};

// A host call's second outputs sit in stream_out behind the out_bytes of rows, each 16-byte aligned: HostAux takes the
// callers' host pointers out of the calls (the stages' whose launches write them: one, or in a chain the squelch's and
// the AGC's, either or both; a call without a second output takes no room) and says how much stream_out must hold;
// stage() points the calls at the staging once host_begin has made it; finish() copies back, then host_end.
// listen_tones_host adds the tone stage's powers and records behind those two with add(): `slot` holds the caller's host
// pointer (null: no room taken) and is pointed at the staging by stage().
struct HostAux {
    static constexpr int MAX = 4;
    void **slot[MAX];
    void *host[MAX];
    size_t bytes[MAX], at[MAX], end;
    int count = 0;
    HostAux(size_t out_bytes, StageCall *first, StageCall *second = nullptr) : end(out_bytes) {
        if (first) add(&first->aux, first->aux_bytes);
        if (second) add(&second->aux, second->aux_bytes);
    }
    void add(void **s, size_t n) {
        slot[count] = s;
        host[count] = *s;
        bytes[count] = n;
        at[count] = (end + 15) & ~(size_t)15;
        if (host[count]) end = at[count] + n;
        count++;
    }
    size_t staged_bytes() const { return end; }
    void stage(sdrg_engine *e) const {
        for (int i = 0; i < count; i++)
            if (host[i]) *slot[i] = e->stream_out.p + at[i];
    }
    int32_t finish(sdrg_engine *e, void *out, size_t out_bytes) const {
        for (int i = 0; i < count; i++)
            if (host[i]) HIP_TRY(hipMemcpyAsync(host[i], *slot[i], bytes[i], hipMemcpyDeviceToHost, e->s_main));
        return host_end(e, out, out_bytes);
    }
};

int32_t require_set(bool set, const char *stage) {
    return set ? SDRG_OK : fail(SDRG_E_INVALID, "no %s configuration set (sdrg_engine_set_%s)", stage, stage);
}

// sdrg_engine_<stage>_device (in, out in device memory) and sdrg_engine_<stage>_host (in host memory) of the stage
// with these three steps; `args` are what its resolve takes between the engine and the call
template <typename Call, auto resolve, auto reserve, auto launch, typename... A>
int32_t stage_call(sdrg_engine *e, const char *in_name, const void *in, void *out, int32_t *n_out, bool host, A... args) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    if (!in || !out || !n_out) return fail(SDRG_E_INVALID, "null %s, out or n_out", in_name);
    Call c;
    int32_t rc = resolve(e, args..., &c);
    if (rc) return rc;
    DeviceScope dscope(e->device);
    HIP_TRY(dscope.error());
    rc = reserve(e, c);
    if (!rc && host) {  // c.aux, a second output, is the resolve's: null for the four stages with one output
        const HostAux aux(c.out_bytes, &c);
        rc = host_begin(e, in, c.in_bytes, aux.staged_bytes());
        if (!rc) aux.stage(e);
        if (!rc) rc = launch(e, c, e->stream_in.p, e->stream_out.p);
        if (!rc) rc = aux.finish(e, out, c.out_bytes);
    } else if (!rc) {
        rc = launch(e, c, in, out);
    }
    if (rc) return rc;
    *n_out = c.n_out;
    return SDRG_OK;
}

// The host's part of a tile-form launch (FirTileParams: the DDC, the demodulator, the sideband stage): the call, where
// the cursor puts the first output, and the history's two halves, which start hist_at floats into a half of `pp`.
// After a restart hist_old is nullptr: zeros.
static void fir_tile_fill(FirTileParams *p, const DecimCursor &cur, int decim, int taps, const StageCall &c,
                          const PingPong<float> &pp, size_t half, size_t hist_at = 0) {
    p->n = c.n;
    p->decim = decim;
    p->taps = taps;
    p->first = cur.first(decim);
    p->n_out = c.n_out;
    p->cap = c.cap;
    const float *old = pp.old(cur, half);
    p->hist_old = old ? old + hist_at : nullptr;
    p->hist_new = pp.next(cur, half) + hist_at;
}

// The block stages, squelch and AGC (block_stage.h): their three steps but for the law's constants, and
// sdrg_<stage>_geometry
static int32_t block_geometry(const char *stage, int32_t block, int32_t *tile) {
    if (!tile) return fail(SDRG_E_INVALID, "null tile");
    if (block < BLOCK_MIN || block > BLOCK_MAX || (block & (block - 1)) != 0)
        return fail(SDRG_E_INVALID, "%s: block must be a power of two in [16, 1024]", stage);
    *tile = block_tile(block);
    return SDRG_OK;
}

// n_out is the blocks the call completes (*n_blocks); aux, the records, record_bytes each
template <typename Stage>
static int32_t block_resolve(const sdrg_engine *e, const Stage &s, const char *stage, size_t record_bytes,
                             int32_t in_stride, int32_t n, void *records, StageCall *c) {
    if (int32_t rc = require_set(s.set, stage)) return rc;
    if (n < 0 || n > s.cfg.max_in)
        return fail(SDRG_E_INVALID, "%s: n %d outside [0, max_in = %d]", stage, n, s.cfg.max_in);
    if (in_stride < std::max(n, 1) || in_stride > s.cfg.max_in)
        return fail(SDRG_E_INVALID, "%s: in_stride %d outside [max(n, 1) = %d, max_in = %d]", stage, in_stride,
                    std::max(n, 1), s.cfg.max_in);
    c->n = n;
    c->in_stride = in_stride;
    c->cap = in_stride;
    c->n_out = s.cur.blocks(n, s.cfg.block);
    c->in_bytes = c->out_bytes = (size_t)e->n_streams * (size_t)in_stride * 2 * sizeof(float);
    c->aux = records;
    c->aux_bytes = (size_t)e->n_streams * record_bytes;
    return SDRG_OK;
}

template <typename Stage>
static int32_t block_reserve(sdrg_engine *e, Stage *s) {
    const int32_t rc = ensure_halves(&s->state, s->half(e->n_streams));
    const size_t blocks = (size_t)BlockCursor::cap(s->cfg.max_in, s->cfg.block);
    return rc ? rc : ensure_device(&s->blk, (size_t)e->n_streams * blocks);
}

// One call of a block stage on the main stream: chan and out (rows of in_stride complex samples; out may be chan) and
// c.aux, the records or null, in device memory.  p holds the law's constants; the BlockParams part is filled here.
template <typename Stage, typename Params>
static int32_t block_launch(sdrg_engine *e, Stage *s, const StageCall &c, Params p,
                            hipError_t (*launch)(const float *, int, const Params &, float *, hipStream_t),
                            const void *chan, void *out) {
    const size_t half = s->half(e->n_streams);
    p.n = c.n;
    p.in_stride = c.in_stride;
    p.block = s->cfg.block;
    p.hang = s->cfg.hang_blocks;
    p.off = s->cur.offset(s->cfg.block);
    p.n_blocks = c.n_out;
    p.fresh = s->cur.fresh ? 1 : 0;
    p.state_old = s->state.half(s->cur.old_half(), half);  // not read by a fresh call: p.fresh says so
    p.state_new = s->state.next(s->cur, half);
    p.blk = s->blk.p;
    p.records = static_cast<decltype(p.records)>(c.aux);
    HIP_TRY(launch(static_cast<const float *>(chan), e->n_streams, p, static_cast<float *>(out), e->s_main));
    s->cur.advance(c.n);  // a call without samples wrote out and the records only: the state stays where it is
    e->outputs_unmarked = true;
    return SDRG_OK;
}

// The device rows a display, integrate or peaks host call reads when its caller passes no spectra: those the last
// process_host call left in d_spec_stage, if they are N = n bins wide.  With spectra, *d_rows stays null: a copy-in
// to spec_in is owed, which spectra_round_trip makes.
int32_t resolve_spectra(const sdrg_engine *e, const float *spectra, int n, const float **d_rows) {
    if (spectra) return SDRG_OK;
    if (!e->d_spec_stage.p || e->host_spec_n == 0)
        return fail(SDRG_E_INVALID, "no spectra on the device: no sdrg_engine_process_host call with SDRG_STAGE_SPECTRUM yet");
    if (e->host_spec_n != n)
        return fail(SDRG_E_INVALID, "samples_per_reading changed (%d -> %d) since the spectra on the device were computed",
                    e->host_spec_n, n);
    *d_rows = e->d_spec_stage.p;
    return SDRG_OK;
}

// The rows the last integrate_host call left on the device, if they are N = n bins wide
int32_t resolve_integrated(const sdrg_engine *e, int n, const float **d_rows) {
    if (!e->integ.out.p || e->integ.out_n == 0)
        return fail(SDRG_E_INVALID, "no integrated rows on the device: no sdrg_engine_integrate_host call yet");
    if (e->integ.out_n != n)
        return fail(SDRG_E_INVALID, "samples_per_reading changed (%d -> %d) since the rows on the device were integrated",
                    e->integ.out_n, n);
    *d_rows = e->integ.out.p;
    return SDRG_OK;
}

struct CopyOut { void *to; const void *from; size_t bytes; };  // device -> host; to == nullptr: the caller wants none

// The host call of the stages that read spectra, [n_streams][N] = count floats, on the main stream: the caller's
// `spectra` to spec_in unless the source is d_rows (resolve_spectra, resolve_integrated), enqueue(source), the copies
// out, and the wait.  Every refusal has come before, and the caller has allocated what `outs` reads from.
template <typename Enqueue>
int32_t spectra_round_trip(sdrg_engine *e, const float *spectra, const float *d_rows, size_t count, Enqueue enqueue,
                           std::initializer_list<CopyOut> outs) {
    if (!d_rows) {
        const int32_t rc = ensure_device(&e->spec_in, count);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(e->spec_in.p, spectra, sizeof(float) * count, hipMemcpyHostToDevice, e->s_main));
        d_rows = e->spec_in.p;
    }
    const int32_t rc = enqueue(d_rows);
    if (rc) return rc;
    for (const CopyOut &o : outs)
        if (o.to) HIP_TRY(hipMemcpyAsync(o.to, o.from, o.bytes, hipMemcpyDeviceToHost, e->s_main));
    HIP_TRY(hipStreamSynchronize(e->s_main));
    return SDRG_OK;
}

int32_t upload_twiddles(sdrg_engine *e, int n) {
    if (e->tw_n == n && e->d_twiddles.p) return SDRG_OK;
    std::vector<float> tw(spectrum_twiddle_floats(n));
    spectrum_fill_twiddles(n, tw.data());
    e->d_twiddles.release();  // whatever its size: the free waits for the spectra that read the old table
    e->tw_n = 0;
    const int32_t rc = ensure_device(&e->d_twiddles, tw.size());
    if (rc) return rc;
    HIP_TRY(hipMemcpy(e->d_twiddles.p, tw.data(), tw.size() * sizeof(float), hipMemcpyHostToDevice));
    e->tw_n = n;
    return SDRG_OK;
}

int64_t ssb_frozen_or(const sdrg_engine *e) {
    return e->ssb.samp_count ? e->ssb.samp_count : e->cfg.samples_per_reading;
}

// Resolve one ring slot's events into timings and add them to the running sums.
int32_t Profiler::fold_slot(int slot) {
    EvSet &ev = ring[slot];
    if (!ev.pending) return SDRG_OK;
    HIP_TRY(hipEventSynchronize(ev.end));
    sdrg_timings t{};
    float ms = 0.0f;
    if (ev.has_spec) {
        HIP_TRY(hipEventElapsedTime(&ms, ev.t0, ev.spec));
        t.spectrum_ms = ms;
    }
    if (ev.has_stats) {
        if (ev.stats_marked) HIP_TRY(hipEventSynchronize(ev.stats));  // asynchronous statistics end on s_stats
        HIP_TRY(hipEventElapsedTime(&ms, ev.has_spec ? ev.spec : ev.t0, ev.stats_marked ? ev.stats : ev.end));
        t.stats_ms = ms;
    }
    bool ssb_measured = false;
    if (ev.has_ssb && ev.ssb_timed) {
        // pipelined calls never join the SSB stream into ev.end's stream: wait for its own end event
        HIP_TRY(hipEventSynchronize(ev.ssb1));
        HIP_TRY(hipEventElapsedTime(&ms, ev.ssb0, ev.ssb1));
        t.ssb_ms = ms;
        ssb_measured = true;
    } else if (ev.has_ssb) {
        // pipelined: no start marker (it would sit on the SSB stream, the step's critical path); the call's SSB
        // stream time is the interval from the previous call's SSB end marker to its own.  The previous slot still
        // holds that marker while its seq is this call's - 1 (begin folds a slot's successor before reusing it).
        const EvSet &pv = ring[(slot + RING - 1) % RING];
        if (pv.seq == ev.seq - 1 && pv.has_ssb && ev.seq > seq_reset) {
            HIP_TRY(hipEventSynchronize(ev.ssb1));
            HIP_TRY(hipEventElapsedTime(&ms, pv.ssb1, ev.ssb1));
            t.ssb_ms = ms;
            ssb_measured = true;
        }
    }
    HIP_TRY(hipEventElapsedTime(&ms, ev.t0, ev.end));
    t.total_ms = ms;
    ev.pending = false;
    if (slot == last) last_timings = t;
    sum_spec += t.spectrum_ms;
    sum_stats += t.stats_ms;
    if (ssb_measured) {
        sum_ssb += t.ssb_ms;
        n_ssb++;
    }
    sum_total += t.total_ms;
    n_acc++;
    return SDRG_OK;
}

int32_t Profiler::fold_all() {
    for (int k = 0; k < RING; k++)  // oldest first
        if (int32_t rc = fold_slot((next + k) % RING)) return rc;
    return SDRG_OK;
}

int32_t Profiler::create() {
    // timing only: no system-scope fence (its cache writeback would widen the gaps it measures)
    for (EvSet &r : ring)
        for (Event *p : {&r.t0, &r.spec, &r.stats, &r.ssb0, &r.ssb1, &r.end}) HIP_TRY(p->create(hipEventDisableSystemFence));
    return SDRG_OK;
}

// The slot of call `seq` (every enqueue counts), folded and filled with what the call will record; null if folding fails.
// early_fork: the call is pipelined and not joined.
EvSet *Profiler::begin(int64_t seq, bool do_spec, bool do_stats, bool do_ssb, bool early_fork, bool stats_async) {
    // the next slot's call measures its pipelined SSB interval from this slot's end marker, about to be reused
    if (fold_slot(next) || fold_slot((next + 1) % RING)) return nullptr;
    EvSet *ev = &ring[next];
    ev->has_spec = do_spec;
    ev->has_stats = do_stats;
    ev->has_ssb = do_ssb;
    // the SSB start marker sits on the SSB stream between the fork and the pipeline; pipelined, that stream is
    // the step's critical path, so a call carries one only when its SSB time cannot be measured from the previous
    // call's SSB end marker to its own (fold_slot): the previous call (seq - 1) was not a profiled SSB call of this
    // timing window
    const EvSet &pv = ring[(next + RING - 1) % RING];
    const bool chained = pv.seq == seq - 1 && pv.has_ssb && seq > seq_reset;
    ev->ssb_timed = do_ssb && (!early_fork || !chained);
    ev->seq = seq;
    // a joined call's end marker follows the wait for the SSB stream, and asynchronous statistics end on a
    // stream of their own: the statistics get a marker of their own
    ev->stats_marked = do_stats && (!early_fork || stats_async);
    return ev;
}

// processSSB_opt's per-call control logic (:223-282) -> kernel parameters.  Works on copies of the engine's
// SSB control statics (c) and NCO phase (nco_phase) that the caller commits only once the call's launches have
// succeeded, so a rejected call freezes no frame size and advances no phase.  The taps and chunk table it may
// upload are keyed by the committed statics: a rejected call's upload is simply redone by the next call.
int32_t prepare_ssb(sdrg_engine *e, SsbControl &c, uint32_t &nco_phase, SsbParams *p) {
    const uint32_t fs = (uint32_t)e->cfg.sample_rate;
    if (c.samp_count == 0) c.samp_count = e->cfg.samples_per_reading;  // static size_t sampCount = iq.size()
    const int mode = e->cfg.sound_mode;
    if (mode == 2) {
        c.agc_target = 0.45f; c.agc_fast = 0.008f; c.gain = 4.5f;
        c.lowpass_bd = 2200.0f; c.lowpass_q = 1.2f; c.transient_coeff = 0.7f;
    } else if (mode == 0) {
        c.agc_target = 0.45f; c.agc_fast = 0.008f; c.gain = 10.0f;
        c.lowpass_bd = 2200.0f; c.lowpass_q = 1.2f; c.transient_coeff = 0.7f;
    } else if (mode == 1) {
        c.agc_target = 0.35f; c.agc_fast = 0.006f; c.agc_slow = 0.00035f; c.gain = 0.5f;
        c.lowpass_bd = 3200.0f; c.lowpass_q = 0.9f; c.transient_coeff = 0.55f;
    }
    if (!c.rf_init) {
        design_lowpass((float)fs, c.lowpass_bd, c.lowpass_q, c.lpf);
        c.rf_init = true;
    }
    const int decim = ssb_decim(fs);
    if (c.taps_samp != c.samp_count || c.taps_decim != decim || c.taps_req != e->fir_taps || !e->d_taps.p) {
        // an earlier call's SSB kernels may still read the taps and the chunk table (non-blocking streams)
        HIP_TRY(hipStreamSynchronize(e->s_ssb));
        // the device tables change now, before this call commits its SSB state: the committed key no longer
        // describes them, so a call that fails after this point leaves the next one to upload again
        e->ssb.taps_samp = -1;
        float h[256];
        c.n_taps = design_fir(c.samp_count, decim, 0.45f, h, e->fir_taps);
        c.taps_req = e->fir_taps;
        int32_t rc = ensure_device(&e->d_taps, sizeof(h) / sizeof(h[0]));
        if (rc) return rc;
        HIP_TRY(hipMemcpy(e->d_taps.p, h, sizeof(float) * (size_t)c.n_taps, hipMemcpyHostToDevice));
        c.taps_samp = c.samp_count;
        c.taps_decim = decim;
        // FIR output ranges per pipeline chunk (the kernel then needs no integer division):
        // overlapping: D*o <= t1-1 and D*o + NT - 1 >= t0 ; completed: t0 <= D*o + NT - 1 < t1
        const int CH = ssb_pipe_chunk(), D = decim, NT = c.n_taps;
        const int S = (int)c.samp_count, PL = ssb_pcm_len(c.samp_count, fs, e->fir_taps);
        const int nch = (S + CH - 1) / CH;
        std::vector<int> tab(4 * (size_t)nch);
        int ov_lo = 0, ov_hi = -1, dn_lo = 0, dn_hi = -1;
        for (int ch = 0; ch < nch; ch++) {
            const int t0 = ch * CH, t1 = std::min(t0 + CH, S);
            while (ov_lo < PL && D * ov_lo + NT - 1 < t0) ov_lo++;
            while (ov_hi + 1 < PL && D * (ov_hi + 1) <= t1 - 1) ov_hi++;
            dn_lo = dn_hi + 1;
            while (dn_hi + 1 < PL && D * (dn_hi + 1) + NT - 1 < t1) dn_hi++;
            tab[4 * ch] = ov_lo;
            tab[4 * ch + 1] = ov_hi;
            tab[4 * ch + 2] = dn_lo;
            tab[4 * ch + 3] = dn_hi;
        }
        rc = ensure_device(&e->d_chunk_table, tab.size());
        if (rc) return rc;
        HIP_TRY(hipMemcpy(e->d_chunk_table.p, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice));
    }
    if (!c.eq_init) {
        design_highpass(48000.0f, 1200.0f, 0.7f, c.hp);
        design_bandpass(48000.0f, 2400.0f, 0.6f, c.bp);
        c.eq_init = true;
    }
    memset(p, 0, sizeof(*p));
    p->samp_count = (int32_t)c.samp_count;
    p->n_in = e->cfg.samples_per_reading;
    p->upper = e->upper;  // SSBProcessor always asks for the upper sideband (ssb_processor.cpp:103)
    p->decim = decim;
    p->n_taps = c.n_taps;
    p->pcm_len = ssb_pcm_len(c.samp_count, fs, e->fir_taps);
    p->agc_target = c.agc_target;
    p->agc_fast = c.agc_fast;
    p->agc_slow = c.agc_slow;
    p->gain = c.gain;
    p->transient_coeff = c.transient_coeff;
    memcpy(p->lpf, c.lpf, sizeof(p->lpf));
    memcpy(p->hp, c.hp, sizeof(p->hp));
    memcpy(p->bp, c.bp, sizeof(p->bp));
    if (e->nco_hz != 0.0) {
        const int32_t rc = ensure_nco_table(e);
        if (rc) return rc;
        p->nco_on = 1;
        p->nco_inc = nco_increment(e->nco_hz, fs);
        p->nco_phase = nco_phase;
        p->nco_tab = e->d_nco_tab.p;
        nco_phase += p->nco_inc * (uint32_t)c.samp_count;  // phase-continuous across calls
    }
    return SDRG_OK;
}

int32_t bytes_per_sample(int fmt) {
    switch (fmt) {
    case SDRG_IQ_CF32: return 8;
    case SDRG_IQ_CS16: return 4;
    case SDRG_IQ_CS8:
    case SDRG_IQ_CU8: return 2;
    default: return 0;
    }
}

// The SSB section of a call, on s_ssb, and the audio detector behind it on s_ap: a joined call's fork, the pipeline with
// the detector's front end in it, the stream's end marker mk_end, the detector.  ev: the profiling slot, or null.
int32_t enqueue_ssb(sdrg_engine *e, const void *iq, int32_t fmt, const SsbParams &sp, int16_t *pcm, size_t pcm_bytes,
                    bool do_ap, bool early_fork, const EvSet *ev, hipEvent_t mk_end) {
    if (!early_fork) {  // fork
        HIP_TRY(hipEventRecord(e->ev_fork, e->s_main));
        HIP_TRY(hipStreamWaitEvent(e->s_ssb, e->ev_fork, 0));
    }
    if (int32_t rc = e->gathers.wait_before_write(e->s_ssb, pcm, pcm_bytes)) return rc;  // still being gathered
    if (ev && ev->ssb_timed) HIP_TRY(hipEventRecord(ev->ssb0, e->s_ssb));
    // AudioPulseDetector::process(pcm) after processSSB_opt (ssb_processor.cpp:109): its per-sample front
    // end runs inside the SSB kernel on the PCM it produces, the detector right after
    AudioFront af;
    const int ap_set = e->ap.set();
    if (do_ap) {
        if (e->ap.live[ap_set]) HIP_TRY(hipEventSynchronize(e->ap.ev_end[ap_set]));  // the detector that read the set
        if (int32_t rc = pulse_bank_audio_front(&e->audio_bank, sp.pcm_len, &af, e->s_ssb, ap_set)) return rc;
    }
    // the SSB stream's end marker: input release (the SSB pipeline, an iq reader, is done), join, timing, and
    // the audio detector's start -- completed by the pipeline kernel's own launch where launch_ssb can
    bool end_recorded = false;
    HIP_TRY(launch_ssb(iq, fmt, e->n_streams, sp, e->d_taps.p, e->d_chunk_table.p, e->d_ssb.p, e->d_ssb_scratch.p, pcm,
                       do_ap ? &af : nullptr, e->s_ssb, mk_end, &end_recorded));
    if (!end_recorded) HIP_TRY(hipEventRecord(mk_end, e->s_ssb));
    if (do_ap) {
        HIP_TRY(hipStreamWaitEvent(e->s_ap, mk_end, 0));
        int32_t rc = pulse_bank_audio_detect(&e->audio_bank, e->audio_bank.d_out, e->s_ap, ap_set);
        if (!rc) rc = e->ap.detected(e->s_ap);
        if (rc) return rc;
    }
    return SDRG_OK;
}

int32_t enqueue(sdrg_engine *e, const void *iq, int32_t fmt, int32_t stages, float *spectra,
                sdrg_frame_record *records, int16_t *pcm, int64_t now_ms, bool join) {
    const int n = e->cfg.samples_per_reading;
    const int B = e->n_streams;
    if (!iq) return fail(SDRG_E_INVALID, "null iq");
    if (bytes_per_sample(fmt) == 0) return fail(SDRG_E_INVALID, "unknown iq format %d", fmt);
    if (stages & ~SDRG_STAGE_ALL) return fail(SDRG_E_INVALID, "unknown stage bits 0x%x", stages);
    if ((stages & SDRG_STAGE_STATS) && !(stages & SDRG_STAGE_SPECTRUM))
        return fail(SDRG_E_INVALID, "STATS needs SPECTRUM");
    if ((stages & SDRG_STAGE_SPECTRAL_PULSE) && !(stages & SDRG_STAGE_STATS))
        return fail(SDRG_E_INVALID, "SPECTRAL_PULSE needs STATS");
    if ((stages & SDRG_STAGE_AUDIO_PULSE) && !(stages & SDRG_STAGE_SSB))
        return fail(SDRG_E_INVALID, "AUDIO_PULSE needs SSB");
    const bool do_spec = stages & SDRG_STAGE_SPECTRUM, do_stats = stages & SDRG_STAGE_STATS,
               do_ssb = stages & SDRG_STAGE_SSB, do_sp = stages & SDRG_STAGE_SPECTRAL_PULSE,
               do_ap = stages & SDRG_STAGE_AUDIO_PULSE;
    if (do_sp && !e->spec_bank_live) {
        if (int32_t rc = pulse_bank_init(&e->spec_bank, SDRG_PULSE_SPECTRAL, &e->spec_pulse_cfg, B, e->device)) return rc;
        e->spec_bank_live = true;
    }
    if (do_ap && !e->audio_bank_live) {
        if (int32_t rc = pulse_bank_init(&e->audio_bank, SDRG_PULSE_AUDIO, &e->audio_pulse_cfg, B, e->device)) return rc;
        e->audio_bank_live = true;
    }
    if (do_spec && !spectrum_supported(n))
        return fail(SDRG_E_UNSUPPORTED, "spectrum for N=%d not supported by this build", n);

    // allocations
    float *spec = spectra;
    if (do_spec && !spec) {
        // zeroed: for odd N the reference never writes power_shifted[N-1] (fft_process.cpp:92-97), which keeps the
        // value its vector held -- 0 for a fresh vector, the same stream's last value afterwards
        if (int32_t rc = ensure_device(&e->d_spec_scratch, (size_t)B * n, true)) return rc;
        spec = e->d_spec_scratch.p;
    }
    sdrg_frame_record *recs = records;
    if (do_stats && !recs) {
        if (int32_t rc = ensure_device(&e->d_rec_scratch, (size_t)B)) return rc;
        recs = e->d_rec_scratch.p;
    }
    // the byte ranges this call writes (checked against the ranges pending gathers read)
    const size_t spec_bytes = (size_t)B * (size_t)n * sizeof(float), rec_bytes = (size_t)B * sizeof(sdrg_frame_record);
    size_t pcm_bytes = 0;
    SsbParams sp;
    if (do_ssb) {
        // frame size and PCM length this call will use (sampCount freezes at the first SSB call, :224-227)
        const int64_t samp = ssb_frozen_or(e);
        const int plen = ssb_pcm_len(samp, (uint32_t)e->cfg.sample_rate, e->fir_taps);
        if (!pcm && plen > 0) return fail(SDRG_E_INVALID, "null pcm with SSB stage");
        pcm_bytes = (size_t)B * (size_t)(plen > 0 ? plen : 0) * sizeof(int16_t);
        if (int32_t rc = ensure_device(&e->d_ssb_scratch, (size_t)B * ((size_t)samp + (size_t)plen))) return rc;
    }
    if (do_spec) {
        if (int32_t rc = upload_twiddles(e, n)) return rc;
        if (int32_t rc = ensure_device(&e->d_fft_scratch, spectrum_scratch_floats(n, B))) return rc;
    }
    StatsGeometry geo{};
    if (do_stats) {
        if (e->fft_fs == 0) return fail(SDRG_E_INVALID, "the statistics' sample rate is 0");
        geo = stats_geometry(e->fft_fs, e->fft_fc, n, e->fft_focus);
        geo.cf_changed = e->cf_changed_pending ? 1 : 0;
        if (int32_t rc = ensure_device(&e->d_pool, stats_global_pool_floats(geo, B))) return rc;
    }

    // last of the checks and allocations: the SSB control statics of this call (committed at the end)
    SsbControl ssb_next = e->ssb;
    uint32_t nco_next = e->nco_phase;
    if (do_ssb)
        if (int32_t rc = prepare_ssb(e, ssb_next, nco_next, &sp)) return rc;

    // The spectrum kernel runs alone on the whole chip first (it is HBM-bound and persistent, two
    // workgroups per CU); the SSB pipeline (latency-bound, one workgroup per CU) then runs beside the
    // statistics kernel on a forked stream.  Measured: the same step time as running the spectrum beside
    // the SSB pipeline, with the spectrum kernel's HBM rate not diluted by the SSB workgroups.
    // Pipelined (sdrg_engine_set_pipelining): the SSB stream forks at the start of the call and is not
    // joined at its end, so this call's SSB pipeline and the next call's spectrum share the chip as the
    // other's workgroups retire (steady state measured in tools/overlap_lab.py).
    const bool early_fork = e->pipelined && !join;

    const bool prof = e->prof.on;
    const int64_t seq = e->calls_total++;
    EvSet *ev = nullptr;  // the profiling slot
    if (prof && !(ev = e->prof.begin(seq, do_spec, do_stats, do_ssb, early_fork, e->stats_async))) return SDRG_E_HIP;  // fold_slot's

    // the launches
    // Markers: every event recorded between two kernels of a stream costs that stream a gap (several us
    // measured), so a call records at most one at its start on the main stream (the SSB fork and the timing
    // origin), one after the spectrum (timing only), and one at the end of each stream's work (input release,
    // join, timing).  Profiling uses the ring's timing events for these; otherwise untimed ones.
    hipEvent_t mk_start = prof ? ev->t0 : e->ev_fork;
    hipEvent_t mk_main_end = prof ? ev->end : e->ev_in_main;
    hipEvent_t mk_ssb_end = prof ? ev->ssb1 : e->ev_in_ssb;
    // the fork: the SSB stage waits for what the caller enqueued on the main stream before this call (its
    // producer work on iq) -- unless the caller declared its inputs complete at call time
    // (SDRG_PIPELINE_INPUTS_READY), which saves the SSB stream a cross-stream wait per call (measured ~20 us)
    const bool fork_wait = do_ssb && early_fork && !e->inputs_ready;
    if (prof || fork_wait) HIP_TRY(hipEventRecord(mk_start, e->s_main));
    if (fork_wait) HIP_TRY(hipStreamWaitEvent(e->s_ssb, mk_start, 0));
    // the spectrum / statistics stream: s_main, or the CU-split stream forked from it
    const bool split = e->s_spec && (do_spec || do_stats);
    hipStream_t sm = split ? e->s_spec : e->s_main;
    if (split) {
        HIP_TRY(hipEventRecord(e->ev_fork_spec, e->s_main));
        HIP_TRY(hipStreamWaitEvent(e->s_spec, e->ev_fork_spec, 0));
    }
    const bool async = e->stats_async && early_fork && do_stats && do_spec && (!split || e->lab_stats_cus);
    if (e->stats_async && do_spec)  // earlier calls' statistics may still read their spectra on s_stats
        if (int32_t rc = e->sa.before_spectrum(sm, spec, async)) return rc;
    if (do_spec)
        if (int32_t rc = e->gathers.wait_before_write(sm, spec, spec_bytes)) return rc;  // being gathered
    auto enqueue_spectrum = [&]() -> int32_t {
        if (do_spec) {
            HIP_TRY(launch_spectrum(iq, fmt, n, B, e->d_twiddles.p, spec, e->d_fft_scratch.p, sm,
                                    do_ssb && early_fork && !split, split ? e->spec_cus : 0,
                                    do_stats && stats_uses_wide(geo)));
            if (prof) HIP_TRY(hipEventRecord(ev->spec, sm));
        }
        return SDRG_OK;
    };
    // host launch order (lab SDRG_SSB_FIRST=1: a forked SSB stage is enqueued before the spectrum, so on an idle chip
    // its workgroups are placed first)
    const bool ssb_first = e->lab_ssb_first && do_ssb && early_fork;
    if (!ssb_first)
        if (int32_t rc = enqueue_spectrum()) return rc;
    if (do_ssb)
        if (int32_t rc = enqueue_ssb(e, iq, fmt, sp, pcm, pcm_bytes, do_ap, early_fork, ev, mk_ssb_end)) return rc;
    if (ssb_first)
        if (int32_t rc = enqueue_spectrum()) return rc;
    if (do_stats) {
        hipStream_t st = sm;
        if (async) {  // after this call's spectrum, beside the next call's
            HIP_TRY(hipEventRecord(e->sa.ev_spec_done, sm));
            HIP_TRY(hipStreamWaitEvent(e->s_stats, e->sa.ev_spec_done, 0));
            st = e->s_stats;
        }
        int32_t rc = e->gathers.wait_before_write(st, recs, rec_bytes);  // still being gathered
        if (rc) return rc;
        HIP_TRY(launch_stats(spec, B, geo, now_ms, e->d_stats.p, recs, e->d_pool.p, st));
        // spectralPulseDetector.process(best1kHzSnrSigma, best1kHzCenterFreqHz) (:477-479)
        if (do_sp) rc = pulse_bank_spectral(&e->spec_bank, &recs->best1khz_snr_sigma, &recs->best1khz_center_freq_hz,
                                            (int)sizeof(sdrg_frame_record), e->spec_bank.d_out, st);
        if (rc) return rc;
        if (prof && ev->stats_marked) HIP_TRY(hipEventRecord(ev->stats, st));
        if (async) rc = e->sa.after_stats(st, spec);
        if (rc) return rc;
    }
    // the main stream's end marker: input release (the spectrum reads iq), timing; joined calls place it after
    // the join, so total_ms spans both streams
    if (split) {
        HIP_TRY(hipEventRecord(e->ev_join_spec, e->s_spec));
        HIP_TRY(hipStreamWaitEvent(e->s_main, e->ev_join_spec, 0));
    }
    if (do_ssb && !early_fork) {  // join
        HIP_TRY(hipStreamWaitEvent(e->s_main, mk_ssb_end, 0));
        if (do_ap) HIP_TRY(hipStreamWaitEvent(e->s_main, e->ap.last_end, 0));
    }
    if (do_spec || prof) HIP_TRY(hipEventRecord(mk_main_end, e->s_main));

    // every launch of the call is enqueued: commit its host-side state
    if (prof) e->prof.commit();
    if (do_ssb) {
        e->ssb = ssb_next;
        e->nco_phase = nco_next;
    }
    if (do_stats) e->cf_changed_pending = false;
    if (do_spec) e->gathers.written(spec, spec_bytes);
    if (do_stats) e->gathers.written(recs, rec_bytes);
    if (do_ssb) e->gathers.written(pcm, pcm_bytes);
    if (do_spec) e->last_in_main = mk_main_end;
    if (do_ssb) e->last_in_ssb = mk_ssb_end;
    if (do_spec || do_stats) e->last_async_stats = do_stats && async;
    return SDRG_OK;
}

void dispatch_callbacks(sdrg_engine *e, int32_t stages, int pcm_len) {
    // soapyCallback order (sdr-bridge-java-soapy.cpp:458-475), then the SSB worker's pcm callback
    const sdrg_callbacks &c = e->cbs;
    const int n = e->cfg.samples_per_reading;
    for (int s = 0; s < e->n_streams; s++) {
        if (stages & SDRG_STAGE_STATS) {
            const sdrg_frame_record &r = e->h_rec[s];
            if (c.fft) c.fft(c.user, s, e->h_spec.data() + (size_t)s * n, n);
            if (c.detection_flag) c.detection_flag(c.user, s, r.detection_flag);
            if (c.mean_snr) c.mean_snr(c.user, s, r.mean_snr_db);
            if (c.mean_snr_sigma) c.mean_snr_sigma(c.user, s, r.mean_snr_sigma);
            if (c.peak_frequency) c.peak_frequency(c.user, s, r.tracking_frequency);
            if (c.peak_above_noise_mean) c.peak_above_noise_mean(c.user, s, r.peak_above_noise_mean_db);
            if (c.max_bin) c.max_bin(c.user, s, r.max_bin_snr_db, r.max_bin_snr_sigma);
            if (c.best1khz) c.best1khz(c.user, s, r.best1khz_snr_db, r.best1khz_snr_sigma);
            if (c.noise_level) c.noise_level(c.user, s, r.per_bin_mean);
            if ((stages & SDRG_STAGE_SPECTRAL_PULSE) && c.spectral_pulse) {
                const sdrg_pulse_output &o = e->h_pspec[s];
                c.spectral_pulse(c.user, s, o.input, o.live_etat, o.est_freq_hz_rounded);
            }
        }
        if ((stages & SDRG_STAGE_SSB) && c.pcm && pcm_len > 0)
            c.pcm(c.user, s, e->h_pcm.data() + (size_t)s * pcm_len, pcm_len);
        if ((stages & SDRG_STAGE_AUDIO_PULSE) && c.audio_pulse) {  // every frame (ssb_processor.cpp:109-113)
            const sdrg_pulse_output &o = e->h_paudio[s];
            c.audio_pulse(c.user, s, o.strength, o.live_etat);
        }
    }
}

}  // namespace

extern "C" {

int32_t sdrg_abi_version(void) { return SDRG_ABI_VERSION; }

const char *sdrg_last_error(void) { return g_last_error.c_str(); }

int32_t sdrg_ssb_pcm_len(int32_t n, int64_t sample_rate) {
    if (n <= 0) return 0;
    return ssb_pcm_len(n, (uint32_t)sample_rate);
}

int32_t sdrg_ssb_layout(int64_t sample_rate, int32_t n, int32_t fir_taps, sdrg_ssb_layout_info *out) {
    if (!out) return fail(SDRG_E_INVALID, "null output");
    if (n <= 0 || sample_rate <= 0 || sample_rate > 0xFFFFFFFFll) return fail(SDRG_E_INVALID, "bad n/sample_rate");
    if (fir_taps != 0 && (fir_taps < 3 || fir_taps > 255 || (fir_taps & 1) == 0))
        return fail(SDRG_E_INVALID, "fir_taps must be 0 or odd in [3, 255], got %d", fir_taps);
    SsbParams p{};  // the fields ssb_pipe_supported reads, filled as prepare_ssb fills them
    p.samp_count = n;
    p.decim = ssb_decim((uint32_t)sample_rate);
    p.n_taps = ssb_taps_for(n, fir_taps);
    p.pcm_len = ssb_pcm_len(n, (uint32_t)sample_rate, fir_taps);
    int nsl_mask = 0;
    const bool pipe = ssb_pipe_supported(p, &nsl_mask);
    out->decimation = p.decim;
    out->taps = p.n_taps;
    out->pcm_len = p.pcm_len;
    out->pipeline = pipe ? 1 : 0;
    out->slots = pipe ? nsl_mask + 1 : 0;
    out->chunk = ssb_pipe_chunk();
    out->chunk_outputs = ssb_pipe_chunk_outputs(p.decim);
    out->max_chunk_outputs = ssb_pipe_max_chunk_outputs();
    return SDRG_OK;
}

int32_t sdrg_host_alloc(size_t bytes, void **out) {
    if (!out) return fail(SDRG_E_INVALID, "null out");
    *out = nullptr;
    if (bytes == 0) return fail(SDRG_E_INVALID, "zero-byte host allocation");
    if (hipHostMalloc(out, bytes, hipHostMallocDefault) != hipSuccess) {
        *out = nullptr;
        return fail(SDRG_E_HIP, "hipHostMalloc of %zu bytes failed", bytes);
    }
    return SDRG_OK;
}

int32_t sdrg_host_free(void *p) {
    if (p) HIP_TRY(hipHostFree(p));
    return SDRG_OK;
}

int32_t sdrg_focus_window(int64_t sample_rate, int32_t n, int32_t focus_khz, int32_t *first_bin, int32_t *n_bins) {
    if (!first_bin || !n_bins) return fail(SDRG_E_INVALID, "null output");
    if (n <= 0 || (uint32_t)sample_rate == 0 || focus_khz < 0) return fail(SDRG_E_INVALID, "bad geometry arguments");
    const StatsGeometry g = stats_geometry((uint32_t)sample_rate, 0, n, focus_khz);
    *first_bin = g.focus_lo;
    *n_bins = g.focus_len > 0 ? g.focus_len : 0;
    return SDRG_OK;
}

int32_t sdrg_ssb_design(int32_t samp_count, int64_t sample_rate, int32_t sound_mode, float *lpf, float *hp,
                        float *bp, float *taps, int32_t *n_taps) {
    if (samp_count <= 0 || (uint32_t)sample_rate == 0) return fail(SDRG_E_INVALID, "bad samp_count/sample_rate");
    SsbControl c;
    if (sound_mode == 2 || sound_mode == 0) {
        c.lowpass_bd = 2200.0f;
        c.lowpass_q = 1.2f;
    }
    const uint32_t fs = (uint32_t)sample_rate;
    if (lpf) design_lowpass((float)fs, c.lowpass_bd, c.lowpass_q, lpf);
    if (hp) design_highpass(48000.0f, 1200.0f, 0.7f, hp);
    if (bp) design_bandpass(48000.0f, 2400.0f, 0.6f, bp);
    if (taps) {
        const int nt = design_fir(samp_count, ssb_decim(fs), 0.45f, taps);
        if (n_taps) *n_taps = nt;
    }
    return SDRG_OK;
}

// Lab (SDRG_QUEUES = "dedicated_mask[,eager]"): HIP maps streams onto GPU_MAX_HW_QUEUES hardware queues, shared
// round-robin by creation order, so streams another library creates (RCCL's, at communicator init) change which engine
// streams share a queue.  dedicated_mask bit 1 main, 2 SSB, 4 statistics, 8 audio detector, 16 gathers: that stream is
// created with a full CU mask, which gives it a hardware queue of its own; eager: the statistics and gather streams are
// created with the engine instead of at first use.
struct QueuePlan {
    int dedicated = 0;
    bool eager = false;
};
static QueuePlan queue_plan() {
    static const QueuePlan q = [] {
        QueuePlan r;
        if (const char *v = lab_getenv("SDRG_QUEUES")) {
            int eg = 0;
            if (sscanf(v, "%d,%d", &r.dedicated, &eg) >= 1) r.eager = eg != 0;
        }
        return r;
    }();
    return q;
}
static hipError_t create_engine_stream(hipStream_t *s, int role_bit, int device, int prio = 0) {
    if (queue_plan().dedicated & role_bit) {
        int ncu = 0;
        hipError_t e = hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device);
        if (e != hipSuccess) return e;
        std::vector<uint32_t> m((ncu + 31) / 32, 0u);
        for (int i = 0; i < ncu; i++) m[i / 32] |= 1u << (i % 32);
        return hipExtStreamCreateWithCUMask(s, (uint32_t)m.size(), m.data());
    }
    return prio ? hipStreamCreateWithPriority(s, hipStreamNonBlocking, prio) : hipStreamCreateWithFlags(s, hipStreamNonBlocking);
}

int32_t sdrg_engine_create(const sdrg_config *cfg, int32_t n_streams, int32_t device, sdrg_engine **out) {
    if (!out) return fail(SDRG_E_INVALID, "null out");
    *out = nullptr;
    int32_t rc = validate_config(cfg);
    if (rc) return rc;
    if (n_streams <= 0) return fail(SDRG_E_INVALID, "n_streams must be > 0");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(SDRG_E_NODEVICE, "no HIP device");
    if (device < 0 || device >= count) return fail(SDRG_E_INVALID, "device %d out of range [0, %d)", device, count);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(SDRG_E_NODEVICE, "device %d is %s, this build targets gfx950", device, prop.gcnArchName);
    DeviceScope dscope(device);
    HIP_TRY(dscope.error());
    sdrg_engine *e = new sdrg_engine();
    e->cfg = *cfg;
    e->spec_pulse_cfg = spectral_pulse_cfg_for(*cfg);
    sdrg_pulse_config_default(SDRG_PULSE_AUDIO, &e->audio_pulse_cfg);
    e->n_streams = n_streams;
    e->device = device;
    auto cleanup = [&](int32_t code) {
        sdrg_engine_destroy(e);
        return code;
    };
    // stream priorities (lab: SDRG_STREAM_PRIO = "main,ssb" in hipDeviceGetStreamPriorityRange units; default
    // both normal)
    int prio_main = 0, prio_ssb = 0;
    if (const char *v = lab_getenv("SDRG_STREAM_PRIO")) {
        if (sscanf(v, "%d,%d", &prio_main, &prio_ssb) != 2) prio_main = prio_ssb = 0;
    }
    if (create_engine_stream(&e->s_own, 1, device, prio_main) != hipSuccess ||
        create_engine_stream(&e->s_ssb, 2, device, prio_ssb) != hipSuccess)
        return cleanup(fail(SDRG_E_HIP, "hipStreamCreate failed"));
    e->s_main = e->s_own;
    // lab: SDRG_CU_SPLIT = 1 (SSB on even CU-mask bits, spectrum/statistics on odd) or 2 (low / high half): the
    // SSB stream and the spectrum / statistics stream on disjoint CUs.  (32-stream SSB workgroups on half the CUs
    // with the spectrum on the other half measured slower than co-residency: DESIGN.md 3.3.)
    if (const char *v = lab_getenv("SDRG_CU_SPLIT")) {
        const int mode = atoi(v);
        const int ncu = prop.multiProcessorCount;
        if ((mode == 1 || mode == 2) && ncu >= 2) {
            std::vector<uint32_t> ma((ncu + 31) / 32, 0u), mb((ncu + 31) / 32, 0u);
            for (int i = 0; i < ncu; i++) {
                const bool a = mode == 1 ? (i % 2 == 0) : (i < ncu / 2);
                (a ? ma : mb)[i / 32] |= 1u << (i % 32);
            }
            if (e->s_ssb) (void)hipStreamDestroy(e->s_ssb);
            e->s_ssb = nullptr;
            if (hipExtStreamCreateWithCUMask(&e->s_ssb, (uint32_t)ma.size(), ma.data()) != hipSuccess ||
                hipExtStreamCreateWithCUMask(&e->s_spec, (uint32_t)mb.size(), mb.data()) != hipSuccess ||
                e->ev_fork_spec.create(hipEventDisableTiming) != hipSuccess ||
                e->ev_join_spec.create(hipEventDisableTiming) != hipSuccess)
                return cleanup(fail(SDRG_E_HIP, "CU-masked stream creation failed"));
            e->spec_cus = ncu - ncu / 2;
        }
    }
    configure_fft(e);
    // stream-to-stream ordering events on one device: no system-scope fence needed (lab: SDRG_EVENT_FENCE=1
    // restores the default system-scope release/acquire)
    static const unsigned ev_flags = [] {
        const char *v = lab_getenv("SDRG_EVENT_FENCE");
        return (v && atoi(v) == 1) ? (unsigned)hipEventDisableTiming
                                   : (unsigned)(hipEventDisableTiming | hipEventDisableSystemFence);
    }();
    if (create_engine_stream(&e->s_ap, 8, device) != hipSuccess)
        return cleanup(fail(SDRG_E_HIP, "hipStreamCreate failed"));
    // the statistics stream is created with the engine's other streams: HIP shares GPU_MAX_HW_QUEUES hardware queues
    // among a process's streams by creation order, and created later (after another library's streams, e.g. RCCL's at
    // communicator init) it landed on the main stream's queue, where the asynchronous statistics ran in line with the
    // spectrum (rocprofv3 r5p: --process-group 0.3136 vs 0.3029 ms per step)
    if (create_engine_stream(&e->s_stats, 4, device) != hipSuccess) return cleanup(fail(SDRG_E_HIP, "hipStreamCreate failed"));
    if (const char *v = lab_getenv("SDRG_GATHER_STREAM"))
        if (atoi(v) == 1 && create_engine_stream(&e->s_gather, 16, device) != hipSuccess)
            return cleanup(fail(SDRG_E_HIP, "hipStreamCreate failed"));
    if (const char *v = lab_getenv("SDRG_SSB_FIRST")) e->lab_ssb_first = atoi(v) == 1;
    // lab: SDRG_STATS_CUS = k: the asynchronous statistics on every (ncu / k)-th CU (k CUs), the spectrum on the others
    // (a CU partition for the FFT + statistics schedule with no SSB stage: each kernel on CUs of its own)
    if (const char *v = lab_getenv("SDRG_STATS_CUS")) {
        const int k = atoi(v), ncu = prop.multiProcessorCount;
        if (k > 0 && k < ncu && !e->s_spec) {
            const int stride = ncu / k;
            std::vector<uint32_t> ms((ncu + 31) / 32, 0u), mf((ncu + 31) / 32, 0u);
            int taken = 0;
            for (int i = 0; i < ncu; i++) {
                const bool st = (i % stride == 0) && taken < k;
                taken += st;
                (st ? ms : mf)[i / 32] |= 1u << (i % 32);
            }
            (void)hipStreamDestroy(e->s_stats);
            e->s_stats = nullptr;
            if (hipExtStreamCreateWithCUMask(&e->s_stats, (uint32_t)ms.size(), ms.data()) != hipSuccess ||
                hipExtStreamCreateWithCUMask(&e->s_spec, (uint32_t)mf.size(), mf.data()) != hipSuccess ||
                e->ev_fork_spec.create(hipEventDisableTiming) != hipSuccess ||
                e->ev_join_spec.create(hipEventDisableTiming) != hipSuccess)
                return cleanup(fail(SDRG_E_HIP, "CU-masked stream creation failed"));
            e->spec_cus = ncu - taken;
            e->lab_stats_cus = true;
        }
    }
    for (Event *p : {&e->ev_fork, &e->ev_join, &e->ev_in_main, &e->ev_in_ssb})
        if (p->create(ev_flags) != hipSuccess) return cleanup(fail(SDRG_E_HIP, "hipEventCreate failed"));
    if (create_events(e->ap.ev_end, ev_flags)) return cleanup(fail(SDRG_E_HIP, "hipEventCreate failed"));
    // FFTProcessor::configure (fft_process.cpp:33-35): maxPeakAndFrequency = {-130, cf} on first configure.
    // The device state starts zeroed; max_peak_set = 0 makes the kernel seed it at the first frame with the
    // centre frequency of that frame's configuration, which is what configure() stored.
    rc = ensure_device(&e->d_stats, (size_t)n_streams, true);
    if (!rc) rc = ensure_device(&e->d_ssb, (size_t)n_streams, true);
    if (rc) return cleanup(rc);
    *out = e;
    return SDRG_OK;
}

int32_t sdrg_engine_destroy(sdrg_engine *e) {
    if (!e) return SDRG_OK;
    DeviceScope dscope(e->device);
    // the caller's stream (sdrg_engine_set_stream) must outlive the engine: synchronise it while it is set
    if (e->s_main) (void)hipStreamSynchronize(e->s_main);
    if (e->s_ssb) (void)hipStreamSynchronize(e->s_ssb);
    if (e->s_stats) (void)hipStreamSynchronize(e->s_stats);
    if (e->s_ap) (void)hipStreamSynchronize(e->s_ap);
    e->spec_bank.last_stream = e->audio_bank.last_stream = nullptr;  // drained above
    e->spec_bank.detect_stream = e->audio_bank.detect_stream = nullptr;
    if (e->s_spec) (void)hipStreamSynchronize(e->s_spec);
    if (e->s_gather) (void)hipStreamSynchronize(e->s_gather);
    pulse_bank_release(&e->spec_bank);  // also what a failed lazy init left behind (null-safe)
    pulse_bank_release(&e->audio_bank);
    if (e->s_own) (void)hipStreamDestroy(e->s_own);
    if (e->s_ssb) (void)hipStreamDestroy(e->s_ssb);
    if (e->s_spec) (void)hipStreamDestroy(e->s_spec);
    if (e->s_stats) (void)hipStreamDestroy(e->s_stats);
    if (e->s_ap) (void)hipStreamDestroy(e->s_ap);
    if (e->s_gather) (void)hipStreamDestroy(e->s_gather);
    delete e;  // the buffers and the events, each freed by its owner: the engine's device is current, its streams drained
    return SDRG_OK;
}

int32_t sdrg_engine_apply_config(sdrg_engine *e, const sdrg_config *cfg) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    int32_t rc = validate_config(cfg);
    if (rc) return rc;
    e->cfg = *cfg;  // applied at the next process call (frame boundary)
    configure_fft(e);  // fftProcessor.configure (:1123-1128)
    e->spec_pulse_cfg = spectral_pulse_cfg_for(*cfg);
    if (e->spec_bank_live) return pulse_bank_configure(&e->spec_bank, &e->spec_pulse_cfg);
    return SDRG_OK;
}

int32_t sdrg_engine_set_frequency(sdrg_engine *e, int64_t center_frequency) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    e->cfg.center_frequency = center_frequency;
    configure_fft(e);              // :896-901
    e->cf_changed_pending = true;  // :907 isCenterFrequencyChanged = true
    return SDRG_OK;
}

int32_t sdrg_engine_set_sample_rate(sdrg_engine *e, int64_t sample_rate) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    if ((uint32_t)sample_rate == 0) return fail(SDRG_E_INVALID, "sample_rate must be > 0");
    e->cfg.sample_rate = sample_rate;  // BridgeConfig only (:931-953): the SSB sees it at the next frame
    return SDRG_OK;
}

int32_t sdrg_engine_set_samples_per_reading(sdrg_engine *e, int32_t n) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    if (n < 1 || n > (1 << 20)) return fail(SDRG_E_UNSUPPORTED, "samples_per_reading %d outside [1, 2^20]", n);
    e->cfg.samples_per_reading = n;  // BridgeConfig only (:1015-1021): the frames are cut at n from now on
    return SDRG_OK;
}

int32_t sdrg_engine_input_released(const sdrg_engine *e, int32_t *released) {
    if (!e || !released) return fail(SDRG_E_INVALID, "null argument");
    *released = 1;
    hipEvent_t evs[] = {e->last_in_main, e->last_in_ssb};
    for (hipEvent_t ev : evs) {
        if (!ev) continue;
        const hipError_t q = hipEventQuery(ev);
        if (q == hipErrorNotReady) {
            *released = 0;
        } else if (q != hipSuccess) {
            return fail(SDRG_E_HIP, "hipEventQuery: %s", hipGetErrorString(q));
        }
    }
    return SDRG_OK;
}

int32_t sdrg_engine_wait_input_released(sdrg_engine *e, void *hip_stream) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    DeviceScope dscope(e->device);
    HIP_TRY(dscope.error());
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : e->s_main;
    if (e->last_in_main && s != e->s_main) HIP_TRY(hipStreamWaitEvent(s, e->last_in_main, 0));
    if (e->last_in_ssb) HIP_TRY(hipStreamWaitEvent(s, e->last_in_ssb, 0));
    return SDRG_OK;
}

int32_t sdrg_engine_wait_outputs(sdrg_engine *e, void *hip_stream) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    DeviceScope dscope(e->device);
    HIP_TRY(dscope.error());
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : e->s_main;
    if (e->last_in_main && s != e->s_main) HIP_TRY(hipStreamWaitEvent(s, e->last_in_main, 0));  // spectra
    if (e->last_in_ssb) HIP_TRY(hipStreamWaitEvent(s, e->last_in_ssb, 0));                    // PCM
    if (e->ap.last_end) HIP_TRY(hipStreamWaitEvent(s, e->ap.last_end, 0));                    // audio pulse
    if (e->stats_async && e->sa.last_end) HIP_TRY(hipStreamWaitEvent(s, e->sa.last_end, 0));  // records
    if (e->gathers.ev_gather) HIP_TRY(hipStreamWaitEvent(s, e->gathers.ev_gather, 0));  // the gathered outputs on the root
    if (s != e->s_main) {  // the later stages' outputs: enqueued on the main stream after the call's own end marker
        if (e->outputs_unmarked) {
            HIP_TRY(e->ev_outputs.create(EV_ORDER));
            HIP_TRY(hipEventRecord(e->ev_outputs, e->s_main));
            e->outputs_unmarked = false;
        }
        if (e->ev_outputs) HIP_TRY(hipStreamWaitEvent(s, e->ev_outputs, 0));
    }
    return SDRG_OK;
}

int32_t sdrg_engine_set_frequency_focus_range(sdrg_engine *e, int32_t khz) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    if (khz < 0) return fail(SDRG_E_INVALID, "focus range must be >= 0");
    e->cfg.freq_focus_range_khz = khz;
    configure_fft(e);  // :1031-1036
    return SDRG_OK;
}

int32_t sdrg_engine_set_sound_mode(sdrg_engine *e, int32_t mode) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    e->cfg.sound_mode = mode;
    return SDRG_OK;
}

int32_t sdrg_engine_set_upper_sideband(sdrg_engine *e, int32_t upper) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    e->upper = upper ? 1 : 0;
    return SDRG_OK;
}

int32_t sdrg_engine_set_ssb_variant(sdrg_engine *e, double nco_hz, int32_t fir_taps) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    if (fir_taps != 0 && (fir_taps < 3 || fir_taps > 255 || (fir_taps & 1) == 0))
        return fail(SDRG_E_INVALID, "fir_taps must be 0 or odd in [3, 255], got %d", fir_taps);
    if (!std::isfinite(nco_hz)) return fail(SDRG_E_INVALID, "nco_hz must be finite");
    DeviceScope dscope(e->device);
    HIP_TRY(dscope.error());
    HIP_TRY(hipStreamSynchronize(e->s_ssb));  // in-flight SSB kernels read the taps being replaced
    e->nco_hz = nco_hz;
    e->fir_taps = fir_taps;
    e->nco_phase = 0;
    return SDRG_OK;
}

int32_t sdrg_engine_get_ssb_variant(const sdrg_engine *e, double *nco_hz, int32_t *fir_taps,
                                    uint32_t *nco_increment_out, uint32_t *nco_phase) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    if (nco_hz) *nco_hz = e->nco_hz;
    if (fir_taps) *fir_taps = ssb_taps_for(ssb_frozen_or(e), e->fir_taps);
    if (nco_increment_out) *nco_increment_out = e->nco_hz != 0.0 ? nco_increment(e->nco_hz, (uint32_t)e->cfg.sample_rate) : 0;
    if (nco_phase) *nco_phase = e->nco_phase;
    return SDRG_OK;
}

int32_t sdrg_engine_get_config(const sdrg_engine *e, sdrg_config *out) {
    if (!e || !out) return fail(SDRG_E_INVALID, "null argument");
    *out = e->cfg;
    return SDRG_OK;
}

int32_t sdrg_engine_n_streams(const sdrg_engine *e) { return e ? e->n_streams : 0; }

int32_t sdrg_engine_pcm_len(const sdrg_engine *e) {
    if (!e) return 0;
    return ssb_pcm_len(ssb_frozen_or(e), (uint32_t)e->cfg.sample_rate, e->fir_taps);
}

int32_t sdrg_engine_reset_state(sdrg_engine *e) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    DeviceScope dscope(e->device);
    HIP_TRY(dscope.error());
    HIP_TRY(hipStreamSynchronize(e->s_main));
    HIP_TRY(hipStreamSynchronize(e->s_ssb));
    if (e->s_stats) HIP_TRY(hipStreamSynchronize(e->s_stats));
    HIP_TRY(hipStreamSynchronize(e->s_ap));
    HIP_TRY(memset_sync(e->d_stats.p, 0, sizeof(StatsState) * (size_t)e->n_streams));
    HIP_TRY(memset_sync(e->d_ssb.p, 0, sizeof(SsbStreamState) * (size_t)e->n_streams));
    e->ssb = SsbControl{};
    e->nco_phase = 0;
    e->cf_changed_pending = false;
    e->spec_bank.reset_pending = true;
    e->audio_bank.reset_pending = true;
    e->integ.restart();
    return SDRG_OK;
}

int32_t sdrg_engine_set_pipelining(sdrg_engine *e, int32_t on) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    DeviceScope dscope(e->device);
    HIP_TRY(dscope.error());
    const int mode = on & ~SDRG_PIPELINE_STATS_ASYNC;
    const bool async = (on & SDRG_PIPELINE_STATS_ASYNC) != 0;
    if ((mode != SDRG_PIPELINE_OFF && mode != SDRG_PIPELINE_ON && mode != SDRG_PIPELINE_INPUTS_READY) ||
        (async && mode == SDRG_PIPELINE_OFF))
        return fail(SDRG_E_INVALID, "pipelining mode must be 0, 1 or 2 (1 or 2 may add SDRG_PIPELINE_STATS_ASYNC), got %d",
                    on);
    if (e->pipelined && !mode) {  // re-join what is in flight so later work on s_main follows it
        HIP_TRY(hipEventRecord(e->ev_join, e->s_ssb));
        HIP_TRY(hipStreamWaitEvent(e->s_main, e->ev_join, 0));
        if (e->ap.last_end) HIP_TRY(hipStreamWaitEvent(e->s_main, e->ap.last_end, 0));
    }
    if (e->stats_async && !async && e->sa.last_end)  // the asynchronous statistics in flight, likewise
        HIP_TRY(hipStreamWaitEvent(e->s_main, e->sa.last_end, 0));
    if (async) {  // created lazily, each handle on its own: a failed earlier attempt leaves no null behind in use
        if (!e->s_stats) HIP_TRY(create_engine_stream(&e->s_stats, 4, e->device));
        if (int32_t rc = e->sa.create()) return rc;
    }
    e->pipelined = mode != SDRG_PIPELINE_OFF;
    e->inputs_ready = mode == SDRG_PIPELINE_INPUTS_READY;
    e->stats_async = async;
    return SDRG_OK;
}

int32_t sdrg_engine_set_stream(sdrg_engine *e, void *hip_stream) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    DeviceScope dscope(e->device);
    HIP_TRY(dscope.error());
    HIP_TRY(hipStreamSynchronize(e->s_main));  // work already enqueued stays ordered before the switch
    e->s_main = hip_stream ? static_cast<hipStream_t>(hip_stream) : e->s_own;
    return SDRG_OK;
}

int32_t sdrg_engine_set_spectral_pulse_config(sdrg_engine *e, const sdrg_pulse_config *cfg) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    int32_t rc = pulse_config_check(SDRG_PULSE_SPECTRAL, cfg);
    if (rc) return rc;
    e->spec_pulse_cfg = *cfg;
    if (e->spec_bank_live) return pulse_bank_configure(&e->spec_bank, cfg);
    return SDRG_OK;
}

int32_t sdrg_engine_set_audio_pulse_config(sdrg_engine *e, const sdrg_pulse_config *cfg) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    int32_t rc = pulse_config_check(SDRG_PULSE_AUDIO, cfg);
    if (rc) return rc;
    e->audio_pulse_cfg = *cfg;
    if (e->audio_bank_live) return pulse_bank_configure(&e->audio_bank, cfg);
    return SDRG_OK;
}

int32_t sdrg_engine_pulse_outputs(const sdrg_engine *e, const sdrg_pulse_output **spectral,
                                  const sdrg_pulse_output **audio) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    if (spectral) *spectral = e->spec_bank_live ? e->spec_bank.d_out : nullptr;
    if (audio) *audio = e->audio_bank_live ? e->audio_bank.d_out : nullptr;
    return SDRG_OK;
}

int32_t sdrg_engine_get_pulse_outputs(sdrg_engine *e, sdrg_pulse_output *spectral, sdrg_pulse_output *audio) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    DeviceScope dscope(e->device);
    HIP_TRY(dscope.error());
    HIP_TRY(hipStreamSynchronize(e->s_main));
    HIP_TRY(hipStreamSynchronize(e->s_ssb));
    if (e->s_stats) HIP_TRY(hipStreamSynchronize(e->s_stats));
    HIP_TRY(hipStreamSynchronize(e->s_ap));
    const size_t bytes = sizeof(sdrg_pulse_output) * (size_t)e->n_streams;
    if (spectral) {
        if (!e->spec_bank_live) return fail(SDRG_E_INVALID, "the spectral pulse stage has not run");
        HIP_TRY(hipMemcpy(spectral, e->spec_bank.d_out, bytes, hipMemcpyDeviceToHost));
    }
    if (audio) {
        if (!e->audio_bank_live) return fail(SDRG_E_INVALID, "the audio pulse stage has not run");
        HIP_TRY(hipMemcpy(audio, e->audio_bank.d_out, bytes, hipMemcpyDeviceToHost));
    }
    return SDRG_OK;
}

int32_t sdrg_engine_process_device(sdrg_engine *e, const void *iq, int32_t format, int32_t stages, float *spectra,
                                   sdrg_frame_record *records, int16_t *pcm, int64_t now_ms) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    DeviceScope dscope(e->device);
    HIP_TRY(dscope.error());
    return enqueue(e, iq, format, stages, spectra, records, pcm, now_ms, false);
}

// evaluateSignalStrength (fft_process.cpp:122-379) on spectra the caller supplies: the FFTProcessor's
// power_shifted member in, the getters' values out, the stream state (tracking latch, detection ring, stale
// outputs) carried exactly as a process() call carries it.  Ordered on the main stream.
static int32_t signal_strength(sdrg_engine *e, const float *spectra, sdrg_frame_record *records, int64_t now_ms) {
    const int n = e->cfg.samples_per_reading, B = e->n_streams;
    if (e->fft_fs == 0) return fail(SDRG_E_INVALID, "the statistics' sample rate is 0");
    StatsGeometry geo = stats_geometry(e->fft_fs, e->fft_fc, n, e->fft_focus);
    geo.cf_changed = e->cf_changed_pending ? 1 : 0;
    int32_t rc = ensure_device(&e->d_pool, stats_global_pool_floats(geo, B));
    if (rc) return rc;
    // asynchronous statistics of an earlier pipelined call (SDRG_PIPELINE_STATS_ASYNC) may still run on s_stats and
    // read / write the same stream state (d_stats) and pool scratch: this launch follows them
    if (e->stats_async && e->sa.last_end) HIP_TRY(hipStreamWaitEvent(e->s_main, e->sa.last_end, 0));
    HIP_TRY(launch_stats(spectra, B, geo, now_ms, e->d_stats.p, records, e->d_pool.p, e->s_main));
    e->cf_changed_pending = false;
    return SDRG_OK;
}

int32_t sdrg_engine_signal_strength_device(sdrg_engine *e, const float *spectra, sdrg_frame_record *records,
                                           int64_t now_ms) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    if (!spectra || !records) return fail(SDRG_E_INVALID, "null spectra or records");
    DeviceScope dscope(e->device);
    HIP_TRY(dscope.error());
    return signal_strength(e, spectra, records, now_ms);
}

int32_t sdrg_engine_signal_strength_host(sdrg_engine *e, const float *spectra, sdrg_frame_record *records,
                                         int64_t now_ms) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    if (!spectra || !records) return fail(SDRG_E_INVALID, "null spectra or records");
    if (e->fft_fs == 0) return fail(SDRG_E_INVALID, "the statistics' sample rate is 0");  // signal_strength's, up front
    DeviceScope dscope(e->device);
    HIP_TRY(dscope.error());
    const size_t B = (size_t)e->n_streams;
    const int32_t rc = ensure_device(&e->d_rec_stage, B);
    if (rc) return rc;
    return spectra_round_trip(
        e, spectra, nullptr, B * (size_t)e->cfg.samples_per_reading,
        [&](const float *src) { return signal_strength(e, src, e->d_rec_stage.p, now_ms); },
        {{records, e->d_rec_stage.p, sizeof(sdrg_frame_record) * B}});
}

int32_t sdrg_engine_synchronize(sdrg_engine *e) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    HIP_TRY(hipStreamSynchronize(e->s_main));
    HIP_TRY(hipStreamSynchronize(e->s_ssb));  // not joined into s_main when pipelined
    if (e->s_stats) HIP_TRY(hipStreamSynchronize(e->s_stats));  // SDRG_PIPELINE_STATS_ASYNC
    HIP_TRY(hipStreamSynchronize(e->s_ap));                      // the audio pulse detector
    if (e->s_gather) HIP_TRY(hipStreamSynchronize(e->s_gather));
    static const bool stamps = [] {
        const char *v = lab_getenv("SDRG_PIPE_STAMPS");
        return v && v[0] == '1';
    }();
    if (stamps) ssb_report_stamps();
    return SDRG_OK;
}

// ---- IQ correction stage (iqcorr.hip) ------------------------------------------------------------------------------

int32_t sdrg_iqcorr_design(const sdrg_iqcorr_config *cfg, float *beta_dc, float *beta_bal, float *floor_thr) {
    if (!cfg) return fail(SDRG_E_INVALID, "null iqcorr config");
    if (const char *bad = iqcorr_check(*cfg)) return fail(SDRG_E_INVALID, "iqcorr: %s", bad);
    iqcorr_design(*cfg, beta_dc, beta_bal, floor_thr);
    return SDRG_OK;
}

int32_t sdrg_iqcorr_geometry(int32_t block, int32_t *tile) {
    if (!tile) return fail(SDRG_E_INVALID, "null tile");
    if (block < IQCORR_MIN_BLOCK || block > BLOCK_MAX || (block & (block - 1)) != 0)
        return fail(SDRG_E_INVALID, "iqcorr: block must be a power of two in [64, 1024]");
    *tile = block_tile(block);
    return SDRG_OK;
}

int32_t sdrg_engine_set_iqcorr(sdrg_engine *e, const sdrg_iqcorr_config *cfg) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    IqcorrStage &s = e->iqc;
    if (cfg) {
        if (const char *bad = iqcorr_check(*cfg)) return fail(SDRG_E_INVALID, "iqcorr: %s", bad);
        s.cfg = *cfg;
        iqcorr_design(*cfg, &s.beta_dc, &s.beta_bal, &s.floor_thr);
    }
    s.set = cfg != nullptr;
    s.cur.restart();
    return SDRG_OK;
}

int32_t sdrg_engine_get_iqcorr(const sdrg_engine *e, sdrg_iqcorr_config *cfg, float *beta_dc, float *beta_bal,
                               float *floor_thr, uint64_t *samples_consumed) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    const IqcorrStage &s = e->iqc;
    if (!s.set) return fail(SDRG_E_INVALID, "no iqcorr configuration set");
    if (cfg) *cfg = s.cfg;
    if (beta_dc) *beta_dc = s.beta_dc;
    if (beta_bal) *beta_bal = s.beta_bal;
    if (floor_thr) *floor_thr = s.floor_thr;
    if (samples_consumed) *samples_consumed = s.cur.g;
    return SDRG_OK;
}

int32_t sdrg_engine_iqcorr_reset(sdrg_engine *e) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    e->iqc.cur.restart();
    return SDRG_OK;
}

struct IqcorrCall : StageCall {
    int fmt = 0;
};

static int32_t iqc_resolve(const sdrg_engine *e, int32_t fmt, int32_t in_stride, int32_t n, sdrg_iqcorr_record *records,
                           IqcorrCall *c) {
    const IqcorrStage &s = e->iqc;
    if (int32_t rc = require_set(s.set, "iqcorr")) return rc;
    const int bps = bytes_per_sample(fmt);
    if (!bps) return fail(SDRG_E_INVALID, "unknown iq format %d", fmt);
    if (n < 0 || n > s.cfg.max_in)
        return fail(SDRG_E_INVALID, "iqcorr: n %d outside [0, max_in = %d]", n, s.cfg.max_in);
    if (in_stride < std::max(n, 1) || in_stride > s.cfg.max_in)
        return fail(SDRG_E_INVALID, "iqcorr: in_stride %d outside [max(n, 1) = %d, max_in = %d]", in_stride,
                    std::max(n, 1), s.cfg.max_in);
    c->fmt = fmt;
    c->n = n;
    c->in_stride = in_stride;
    c->cap = in_stride;
    c->n_out = s.cur.blocks(n, s.cfg.block);
    c->in_bytes = (size_t)e->n_streams * (size_t)in_stride * (size_t)bps;
    c->out_bytes = (size_t)e->n_streams * (size_t)in_stride * 2 * sizeof(float);
    c->aux = records;
    c->aux_bytes = (size_t)e->n_streams * sizeof(*records);
    return SDRG_OK;
}

static int32_t iqc_reserve(sdrg_engine *e, const IqcorrCall &) {
    IqcorrStage &s = e->iqc;
    const int32_t rc = ensure_halves(&s.state, s.half(e->n_streams));
    return rc ? rc : ensure_device(&s.blk, (size_t)e->n_streams * s.blocks() * 9);
}

// The three launches on the main stream, the cursor left where it is: iq (rows of in_stride raw samples), out (rows of
// in_stride complex samples) and c.aux, the records or null, in device memory.
static int32_t iqc_enqueue(sdrg_engine *e, const IqcorrCall &c, const void *iq, void *out) {
    IqcorrStage &s = e->iqc;
    const size_t half = s.half(e->n_streams);
    IqcorrParams p{};
    p.n = c.n;
    p.in_stride = c.in_stride;
    p.block = s.cfg.block;
    p.mode = s.cfg.mode;
    p.off = s.cur.offset(s.cfg.block);
    p.n_blocks = c.n_out;
    p.fresh = s.cur.fresh ? 1 : 0;
    p.beta_dc = s.beta_dc;
    p.beta_bal = s.beta_bal;
    p.floor_thr = s.floor_thr;
    p.state_old = s.state.half(s.cur.old_half(), half);  // not read by a fresh call: p.fresh says so
    p.state_new = s.state.next(s.cur, half);
    p.mom = s.blk.p;
    p.theta = s.blk.p + (size_t)e->n_streams * s.blocks() * 5;
    p.records = static_cast<sdrg_iqcorr_record *>(c.aux);
    HIP_TRY(launch_iqcorr(iq, c.fmt, e->n_streams, p, static_cast<float *>(out), e->s_main));
    return SDRG_OK;
}

static void iqc_commit(sdrg_engine *e, const IqcorrCall &c) {
    e->iqc.cur.advance(c.n);  // a call without samples wrote out and the records only: the state stays where it is
    e->outputs_unmarked = true;
}

static int32_t iqc_launch(sdrg_engine *e, const IqcorrCall &c, const void *iq, void *out) {
    const int32_t rc = iqc_enqueue(e, c, iq, out);
    if (!rc) iqc_commit(e, c);
    return rc;
}

static constexpr auto iqc_stage =
    &stage_call<IqcorrCall, iqc_resolve, iqc_reserve, iqc_launch, int32_t, int32_t, int32_t, sdrg_iqcorr_record *>;

int32_t sdrg_engine_iqcorr_device(sdrg_engine *e, const void *iq, int32_t fmt, int32_t in_stride, int32_t n, void *out,
                                  sdrg_iqcorr_record *records, int32_t *n_blocks) {
    return iqc_stage(e, "iq", iq, out, n_blocks, false, fmt, in_stride, n, records);
}

int32_t sdrg_engine_iqcorr_host(sdrg_engine *e, const void *iq, int32_t fmt, int32_t in_stride, int32_t n, void *out,
                                sdrg_iqcorr_record *records, int32_t *n_blocks) {
    return iqc_stage(e, "iq", iq, out, n_blocks, true, fmt, in_stride, n, records);
}

// ---- AFC stage (afc.hip) -------------------------------------------------------------------------------------------

int32_t sdrg_afc_design(const sdrg_afc_config *cfg, sdrg_afc_design_values *design) {
    if (!cfg || !design) return fail(SDRG_E_INVALID, "null afc config or design");
    if (const char *bad = afc_check(*cfg)) return fail(SDRG_E_INVALID, "afc: %s", bad);
    *design = afc_design(*cfg);
    return SDRG_OK;
}

int32_t sdrg_afc_geometry(int32_t block, int32_t *tile) { return block_geometry("afc", block, tile); }

double sdrg_afc_offset_hz(int32_t inc, double channel_rate) {
    if (!std::isfinite(channel_rate) || !(channel_rate > 0.0)) return NAN;
    return (double)inc * channel_rate / 4294967296.0;
}

int32_t sdrg_engine_set_afc(sdrg_engine *e, const sdrg_afc_config *cfg) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    AfcStage &s = e->afc;
    if (cfg) {
        if (const char *bad = afc_check(*cfg)) return fail(SDRG_E_INVALID, "afc: %s", bad);
        s.cfg = *cfg;
        s.des = afc_design(*cfg);
    }
    s.set = cfg != nullptr;
    s.cur.restart();
    return SDRG_OK;
}

int32_t sdrg_engine_get_afc(const sdrg_engine *e, sdrg_afc_config *cfg, sdrg_afc_design_values *design,
                            uint64_t *samples_consumed) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    const AfcStage &s = e->afc;
    if (!s.set) return fail(SDRG_E_INVALID, "no afc configuration set");
    if (cfg) *cfg = s.cfg;
    if (design) *design = s.des;
    if (samples_consumed) *samples_consumed = s.cur.g;
    return SDRG_OK;
}

int32_t sdrg_engine_afc_reset(sdrg_engine *e) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    e->afc.cur.restart();
    return SDRG_OK;
}

// out_bytes is the rows' when the stage tracks, and 0 when it measures: it writes no rows then
static int32_t afc_resolve(const sdrg_engine *e, int32_t in_stride, int32_t n, sdrg_afc_record *records, StageCall *c) {
    const int32_t rc = block_resolve(e, e->afc, "afc", sizeof(*records), in_stride, n, records, c);
    if (!rc && !e->afc.track()) c->out_bytes = 0;
    return rc;
}

static int32_t afc_reserve(sdrg_engine *e, const StageCall &) {
    AfcStage &s = e->afc;
    int32_t rc = ensure_halves(&s.state, s.half(e->n_streams));
    if (!rc) rc = ensure_device(&s.blk, (size_t)e->n_streams * (s.blocks() * 3 + (s.blocks() + 1) * 2));
    if (!rc && s.track()) rc = ensure_nco_table(e);
    return rc;
}

// One call on the main stream: chan and out (rows of in_stride complex samples; out may be chan, and is null when the
// stage measures) and c.aux, the records or null, in device memory.
static int32_t afc_launch(sdrg_engine *e, const StageCall &c, const void *chan, void *out) {
    AfcStage &s = e->afc;
    const size_t half = s.half(e->n_streams);
    AfcParams p{};
    p.n = c.n;
    p.in_stride = c.in_stride;
    p.block = s.cfg.block;
    p.track = s.track() ? 1 : 0;
    p.off = s.cur.offset(s.cfg.block);
    p.n_blocks = c.n_out;
    p.fresh = s.cur.fresh ? 1 : 0;
    p.beta = s.des.beta, p.floor_thr = s.des.floor_thr, p.lock_thr = s.des.lock_thr, p.max_s = s.des.max_s;
    p.K = s.des.K, p.hz_per_inc = s.des.hz_per_inc, p.rad_per_inc = s.des.rad_per_inc;
    p.nco_tab = e->d_nco_tab.p;
    p.state_old = s.state.half(s.cur.old_half(), half);  // not read by a fresh call: p.fresh says so
    p.state_new = s.state.next(s.cur, half);
    p.mom = s.blk.p;
    p.blk = reinterpret_cast<uint32_t *>(s.blk.p + (size_t)e->n_streams * s.blocks() * 3);
    p.records = static_cast<sdrg_afc_record *>(c.aux);
    HIP_TRY(launch_afc(static_cast<const float *>(chan), e->n_streams, p, static_cast<float *>(out), e->s_main));
    s.cur.advance(c.n);  // a call without samples wrote out and the records only: the state stays where it is
    e->outputs_unmarked = true;
    return SDRG_OK;
}

// stage_call for a stage whose `out` is null in one of its modes
static int32_t afc_call(sdrg_engine *e, const void *chan, int32_t in_stride, int32_t n, void *out,
                        sdrg_afc_record *records, int32_t *n_blocks, bool host) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    if (!chan || !n_blocks) return fail(SDRG_E_INVALID, "null chan or n_blocks");
    StageCall c;
    int32_t rc = afc_resolve(e, in_stride, n, records, &c);
    if (rc) return rc;
    const bool track = e->afc.track();
    if (track && !out) return fail(SDRG_E_INVALID, "afc: null out in SDRG_AFC_TRACK mode");
    if (!track && out) return fail(SDRG_E_INVALID, "afc: out must be NULL in SDRG_AFC_MEASURE mode");
    DeviceScope dscope(e->device);
    HIP_TRY(dscope.error());
    rc = afc_reserve(e, c);
    if (!rc && host) {
        const HostAux aux(c.out_bytes, &c);
        rc = host_begin(e, chan, c.in_bytes, aux.staged_bytes());
        if (!rc) aux.stage(e);
        if (!rc) rc = afc_launch(e, c, e->stream_in.p, track ? e->stream_out.p : nullptr);
        if (!rc) rc = aux.finish(e, out, c.out_bytes);
    } else if (!rc) {
        rc = afc_launch(e, c, chan, out);
    }
    if (rc) return rc;
    *n_blocks = c.n_out;
    return SDRG_OK;
}

int32_t sdrg_engine_afc_device(sdrg_engine *e, const void *chan, int32_t in_stride, int32_t n, void *out,
                               sdrg_afc_record *records, int32_t *n_blocks) {
    return afc_call(e, chan, in_stride, n, out, records, n_blocks, false);
}

int32_t sdrg_engine_afc_host(sdrg_engine *e, const void *chan, int32_t in_stride, int32_t n, void *out,
                             sdrg_afc_record *records, int32_t *n_blocks) {
    return afc_call(e, chan, in_stride, n, out, records, n_blocks, true);
}

// ---- noise blanker stage (blanker.hip) -----------------------------------------------------------------------------

int32_t sdrg_blanker_design(const sdrg_blanker_config *cfg, float *beta, float *ratio, float *floor_thr) {
    if (!cfg) return fail(SDRG_E_INVALID, "null blanker config");
    if (const char *bad = blanker_check(*cfg)) return fail(SDRG_E_INVALID, "blanker: %s", bad);
    blanker_design(*cfg, beta, ratio, floor_thr);
    return SDRG_OK;
}

int32_t sdrg_blanker_geometry(int32_t block, int32_t *floor_tile, int32_t *pass_tile) {
    if (!floor_tile && !pass_tile) return fail(SDRG_E_INVALID, "null floor_tile and pass_tile");
    if (block < BLANKER_MIN_BLOCK || block > BLOCK_MAX || (block & (block - 1)) != 0)
        return fail(SDRG_E_INVALID, "blanker: block must be a power of two in [64, 1024]");
    if (floor_tile) *floor_tile = block_tile(block);
    if (pass_tile) *pass_tile = BLANKER_TILE;
    return SDRG_OK;
}

int32_t sdrg_engine_set_blanker(sdrg_engine *e, const sdrg_blanker_config *cfg) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    BlankerStage &s = e->blank;
    if (cfg) {
        if (const char *bad = blanker_check(*cfg)) return fail(SDRG_E_INVALID, "blanker: %s", bad);
        s.cfg = *cfg;
        blanker_design(*cfg, &s.beta, &s.ratio, &s.floor_thr);
    }
    s.set = cfg != nullptr;
    s.cur.restart();
    return SDRG_OK;
}

int32_t sdrg_engine_get_blanker(const sdrg_engine *e, sdrg_blanker_config *cfg, float *beta, float *ratio,
                                float *floor_thr, uint64_t *samples_consumed) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    const BlankerStage &s = e->blank;
    if (!s.set) return fail(SDRG_E_INVALID, "no blanker configuration set");
    if (cfg) *cfg = s.cfg;
    if (beta) *beta = s.beta;
    if (ratio) *ratio = s.ratio;
    if (floor_thr) *floor_thr = s.floor_thr;
    if (samples_consumed) *samples_consumed = s.cur.g;
    return SDRG_OK;
}

int32_t sdrg_engine_blanker_reset(sdrg_engine *e) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    e->blank.cur.restart();
    return SDRG_OK;
}

using BlankerCall = IqcorrCall;  // a block stage's call and the format of its raw rows

static int32_t blank_resolve(const sdrg_engine *e, int32_t fmt, int32_t in_stride, int32_t n,
                             sdrg_blanker_record *records, BlankerCall *c) {
    const BlankerStage &s = e->blank;
    if (int32_t rc = require_set(s.set, "blanker")) return rc;
    const int bps = bytes_per_sample(fmt);
    if (!bps) return fail(SDRG_E_INVALID, "unknown iq format %d", fmt);
    if (n < 0 || n > s.cfg.max_in)
        return fail(SDRG_E_INVALID, "blanker: n %d outside [0, max_in = %d]", n, s.cfg.max_in);
    if (in_stride < std::max(n, 1) || in_stride > s.cfg.max_in)
        return fail(SDRG_E_INVALID, "blanker: in_stride %d outside [max(n, 1) = %d, max_in = %d]", in_stride,
                    std::max(n, 1), s.cfg.max_in);
    c->fmt = fmt;
    c->n = n;
    c->in_stride = in_stride;
    c->cap = in_stride;
    c->n_out = s.cur.blocks(n, s.cfg.block);
    c->in_bytes = (size_t)e->n_streams * (size_t)in_stride * (size_t)bps;
    c->out_bytes = (size_t)e->n_streams * (size_t)in_stride * 2 * sizeof(float);
    c->aux = records;
    c->aux_bytes = (size_t)e->n_streams * sizeof(*records);
    return SDRG_OK;
}

static int32_t blank_reserve(sdrg_engine *e, const BlankerCall &) {
    BlankerStage &s = e->blank;
    const int32_t rc = ensure_halves(&s.state, s.half(e->n_streams));
    return rc ? rc : ensure_device(&s.blk, (size_t)e->n_streams * s.blocks() * 2);
}

// The three launches on the main stream, the cursor left where it is: iq (rows of in_stride raw samples), out (rows of
// in_stride complex samples, not overlapping iq) and c.aux, the records or null, in device memory.
static int32_t blank_enqueue(sdrg_engine *e, const BlankerCall &c, const void *iq, void *out) {
    BlankerStage &s = e->blank;
    const size_t half = s.half(e->n_streams);
    BlankerParams p{};
    p.n = c.n;
    p.in_stride = c.in_stride;
    p.block = s.cfg.block;
    p.lead = s.cfg.lead;
    p.tail = s.cfg.tail;
    p.off = s.cur.offset(s.cfg.block);
    p.n_blocks = c.n_out;
    p.fresh = s.cur.fresh ? 1 : 0;
    p.skip = s.cur.g < (uint64_t)s.cfg.lead ? s.cfg.lead - (int)s.cur.g : 0;
    p.beta = s.beta;
    p.ratio = s.ratio;
    p.floor_thr = s.floor_thr;
    p.state_old = s.state.half(s.cur.old_half(), half);  // not read by a fresh call: p.fresh says so
    p.state_new = s.state.next(s.cur, half);
    p.flo = s.blk.p;
    p.thr = s.blk.p + (size_t)e->n_streams * s.blocks();
    p.records = static_cast<sdrg_blanker_record *>(c.aux);
    HIP_TRY(launch_blanker(iq, c.fmt, e->n_streams, p, static_cast<float *>(out), e->s_main));
    return SDRG_OK;
}

static void blank_commit(sdrg_engine *e, const BlankerCall &c) {
    e->blank.cur.advance(c.n);  // a call without samples wrote out and the records only: the state stays where it is
    e->outputs_unmarked = true;
}

static int32_t blank_launch(sdrg_engine *e, const BlankerCall &c, const void *iq, void *out) {
    const int32_t rc = blank_enqueue(e, c, iq, out);
    if (!rc) blank_commit(e, c);
    return rc;
}

static constexpr auto blank_stage =
    &stage_call<BlankerCall, blank_resolve, blank_reserve, blank_launch, int32_t, int32_t, int32_t, sdrg_blanker_record *>;

int32_t sdrg_engine_blanker_device(sdrg_engine *e, const void *iq, int32_t fmt, int32_t in_stride, int32_t n, void *out,
                                   sdrg_blanker_record *records, int32_t *n_blocks) {
    return blank_stage(e, "iq", iq, out, n_blocks, false, fmt, in_stride, n, records);
}

int32_t sdrg_engine_blanker_host(sdrg_engine *e, const void *iq, int32_t fmt, int32_t in_stride, int32_t n, void *out,
                                 sdrg_blanker_record *records, int32_t *n_blocks) {
    return blank_stage(e, "iq", iq, out, n_blocks, true, fmt, in_stride, n, records);
}

// sdrg_engine_process_host; sdrg_engine_iqcorr_process_host with `corr`, the resolved correction of the frame; and
// sdrg_engine_clean_process_host with `blank`, the resolved blanking of the frame (fmt: what it reads, CF32 behind a
// correction), and with or without `corr`.  The stages then read the last cleaning stage's rows (e->iqc.rows,
// e->blank.rows) as CF32, and the cleaning stages' cursors move once everything is enqueued.
static int32_t process_host_frames(sdrg_engine *e, const void *iq, int32_t format, int32_t stages, float *spectra,
                                   sdrg_frame_record *records, int16_t *pcm, int64_t now_ms, IqcorrCall *corr,
                                   sdrg_iqcorr_record *iq_records, BlankerCall *blank = nullptr,
                                   sdrg_blanker_record *blank_records = nullptr) {
    const int bps = bytes_per_sample(format);
    DeviceScope dscope(e->device);
    HIP_TRY(dscope.error());
    const int n = e->cfg.samples_per_reading;
    const int B = e->n_streams;
    const size_t iq_bytes = (size_t)B * n * bps;
    int32_t rc = ensure_device(&e->d_iq_stage, iq_bytes);
    if (!rc && corr) rc = iqc_reserve(e, *corr);
    if (!rc && corr) rc = ensure_device(&e->iqc.rows, (size_t)B * n * 2);
    if (!rc && corr) rc = ensure_device(&e->iqc.rec, (size_t)B);
    if (!rc && blank) rc = blank_reserve(e, *blank);
    if (!rc && blank) rc = ensure_device(&e->blank.rows, (size_t)B * n * 2);
    if (!rc && blank) rc = ensure_device(&e->blank.rec, (size_t)B);
    if (rc) return rc;
    const bool want_cb = e->has_cbs;
    const bool do_spec = stages & SDRG_STAGE_SPECTRUM, do_stats = stages & SDRG_STAGE_STATS,
               do_ssb = stages & SDRG_STAGE_SSB;
    if (do_spec) {
        e->host_spec_n = 0;  // until this call's spectra are enqueued
        rc = ensure_device(&e->d_spec_stage, (size_t)B * n, true);  // see enqueue
    }
    if (!rc && do_stats) rc = ensure_device(&e->d_rec_stage, (size_t)B);
    if (rc) return rc;
    int pcm_len = 0;
    if (do_ssb) {
        // pcm length is known before the call: frozen (or about-to-be frozen) size and current fs
        pcm_len = ssb_pcm_len(ssb_frozen_or(e), (uint32_t)e->cfg.sample_rate, e->fir_taps);
        rc = ensure_device(&e->d_pcm_stage, (size_t)B * (pcm_len > 0 ? pcm_len : 1));
        if (rc) return rc;
    }
    HIP_TRY(hipMemcpyAsync(e->d_iq_stage.p, iq, iq_bytes, hipMemcpyHostToDevice, e->s_main));
    const void *frames = e->d_iq_stage.p;
    if (corr) {
        corr->aux = e->iqc.rec.p;
        rc = iqc_enqueue(e, *corr, e->d_iq_stage.p, e->iqc.rows.p);
        if (rc) return rc;
        frames = e->iqc.rows.p;
        format = SDRG_IQ_CF32;
    }
    if (blank) {
        blank->aux = e->blank.rec.p;
        rc = blank_enqueue(e, *blank, frames, e->blank.rows.p);
        if (rc) return rc;
        frames = e->blank.rows.p;
        format = SDRG_IQ_CF32;
    }
    rc = enqueue(e, frames, format, stages, do_spec ? e->d_spec_stage.p : nullptr,
                 do_stats ? e->d_rec_stage.p : nullptr, do_ssb ? e->d_pcm_stage.p : nullptr, now_ms, true);
    if (rc) return rc;
    if (corr) {
        iqc_commit(e, *corr);
        if (iq_records)
            HIP_TRY(hipMemcpyAsync(iq_records, e->iqc.rec.p, sizeof(sdrg_iqcorr_record) * (size_t)B, hipMemcpyDeviceToHost,
                                   e->s_main));
    }
    if (blank) {
        blank_commit(e, *blank);
        if (blank_records)
            HIP_TRY(hipMemcpyAsync(blank_records, e->blank.rec.p, sizeof(sdrg_blanker_record) * (size_t)B,
                                   hipMemcpyDeviceToHost, e->s_main));
    }
    if (do_spec) e->host_spec_n = n;  // sdrg_engine_display_host(spectra = NULL) reads these spectra
    float *h_spec = spectra;
    sdrg_frame_record *h_rec = records;
    int16_t *h_pcm = pcm;
    if (want_cb) {
        if ((do_spec && !e->h_spec.resize((size_t)B * n)) || (do_stats && !e->h_rec.resize(B)) ||
            (do_ssb && !e->h_pcm.resize((size_t)B * std::max(pcm_len, 1))) ||
            ((stages & SDRG_STAGE_SPECTRAL_PULSE) && !e->h_pspec.resize(B)) ||
            ((stages & SDRG_STAGE_AUDIO_PULSE) && !e->h_paudio.resize(B)))
            return fail(SDRG_E_HIP, "hipHostMalloc failed for the callback copies");
        if (do_spec && !h_spec) h_spec = e->h_spec.data();
        if (do_stats && !h_rec) h_rec = e->h_rec.data();
        if (do_ssb && !h_pcm) h_pcm = e->h_pcm.data();
    }
    if (do_spec && h_spec)
        HIP_TRY(hipMemcpyAsync(h_spec, e->d_spec_stage.p, sizeof(float) * (size_t)B * n, hipMemcpyDeviceToHost, e->s_main));
    if (do_stats && h_rec)
        HIP_TRY(hipMemcpyAsync(h_rec, e->d_rec_stage.p, sizeof(sdrg_frame_record) * (size_t)B, hipMemcpyDeviceToHost,
                               e->s_main));
    if (do_ssb && h_pcm && pcm_len > 0)
        HIP_TRY(hipMemcpyAsync(h_pcm, e->d_pcm_stage.p, sizeof(int16_t) * (size_t)B * pcm_len, hipMemcpyDeviceToHost,
                               e->s_main));
    if (want_cb && (stages & SDRG_STAGE_SPECTRAL_PULSE)) {
        HIP_TRY(hipMemcpyAsync(e->h_pspec.data(), e->spec_bank.d_out, sizeof(sdrg_pulse_output) * (size_t)B,
                               hipMemcpyDeviceToHost, e->s_main));
    }
    if (want_cb && (stages & SDRG_STAGE_AUDIO_PULSE)) {
        HIP_TRY(hipMemcpyAsync(e->h_paudio.data(), e->audio_bank.d_out, sizeof(sdrg_pulse_output) * (size_t)B,
                               hipMemcpyDeviceToHost, e->s_main));
    }
    HIP_TRY(hipStreamSynchronize(e->s_main));
    if (want_cb) {
        // callbacks read the engine-owned host copies; make sure they hold this call's data
        if (do_spec && h_spec != e->h_spec.data()) e->h_spec.assign(h_spec, h_spec + (size_t)B * n);
        if (do_stats && h_rec != e->h_rec.data()) e->h_rec.assign(h_rec, h_rec + B);
        if (do_ssb && h_pcm != e->h_pcm.data() && pcm_len > 0) e->h_pcm.assign(h_pcm, h_pcm + (size_t)B * pcm_len);
        dispatch_callbacks(e, stages, pcm_len);
    }
    return SDRG_OK;
}

int32_t sdrg_engine_process_host(sdrg_engine *e, const void *iq, int32_t format, int32_t stages, float *spectra,
                                 sdrg_frame_record *records, int16_t *pcm, int64_t now_ms) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    if (!iq) return fail(SDRG_E_INVALID, "null iq");
    if (!bytes_per_sample(format)) return fail(SDRG_E_INVALID, "unknown iq format %d", format);
    return process_host_frames(e, iq, format, stages, spectra, records, pcm, now_ms, nullptr, nullptr);
}

int32_t sdrg_engine_iqcorr_process_host(sdrg_engine *e, const void *iq, int32_t fmt, int32_t stages, float *spectra,
                                        sdrg_frame_record *records, int16_t *pcm, int64_t now_ms,
                                        sdrg_iqcorr_record *iq_records) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    if (!iq) return fail(SDRG_E_INVALID, "null iq");
    if (int32_t rc = require_set(e->iqc.set, "iqcorr")) return rc;
    const int n = e->cfg.samples_per_reading;
    if (e->iqc.cfg.max_in < n)
        return fail(SDRG_E_INVALID, "iqcorr max_in %d smaller than the frame's %d samples", e->iqc.cfg.max_in, n);
    IqcorrCall c;
    if (int32_t rc = iqc_resolve(e, fmt, n, n, nullptr, &c)) return rc;
    return process_host_frames(e, iq, fmt, stages, spectra, records, pcm, now_ms, &c, iq_records);
}

int32_t sdrg_engine_clean_process_host(sdrg_engine *e, const void *iq, int32_t fmt, int32_t mask, int32_t stages,
                                       float *spectra, sdrg_frame_record *records, int16_t *pcm, int64_t now_ms,
                                       sdrg_iqcorr_record *iq_records, sdrg_blanker_record *blank_records) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    if (!iq) return fail(SDRG_E_INVALID, "null iq");
    if (mask & ~SDRG_CLEAN_IQCORR) return fail(SDRG_E_INVALID, "clean mask %d has bits other than SDRG_CLEAN_IQCORR", mask);
    const bool correct = mask & SDRG_CLEAN_IQCORR;
    if (int32_t rc = require_set(e->blank.set, "blanker")) return rc;
    if (correct)
        if (int32_t rc = require_set(e->iqc.set, "iqcorr")) return rc;
    const int n = e->cfg.samples_per_reading;
    if (e->blank.cfg.max_in < n)
        return fail(SDRG_E_INVALID, "blanker max_in %d smaller than the frame's %d samples", e->blank.cfg.max_in, n);
    if (correct && e->iqc.cfg.max_in < n)
        return fail(SDRG_E_INVALID, "iqcorr max_in %d smaller than the frame's %d samples", e->iqc.cfg.max_in, n);
    IqcorrCall c;
    BlankerCall k;
    if (correct)
        if (int32_t rc = iqc_resolve(e, fmt, n, n, nullptr, &c)) return rc;
    if (int32_t rc = blank_resolve(e, correct ? SDRG_IQ_CF32 : fmt, n, n, nullptr, &k)) return rc;
    return process_host_frames(e, iq, fmt, stages, spectra, records, pcm, now_ms, correct ? &c : nullptr, iq_records, &k,
                               blank_records);
}

// ---- display stage (display.hip) ----------------------------------------------------------------------------------

int32_t sdrg_display_column_range(int32_t n_bins, int32_t width, int32_t column, int32_t *first, int32_t *count) {
    if (!first || !count) return fail(SDRG_E_INVALID, "null output");
    if (n_bins < 1 || n_bins > (1 << 20) || width < 1 || width > (1 << 20) || column < 0 || column >= width)
        return fail(SDRG_E_INVALID, "n_bins %d / width %d outside [1, 2^20] or column %d outside [0, width)", n_bins,
                    width, column);
    const int64_t j0 = (int64_t)column * n_bins / width, j1 = ((int64_t)column + 1) * n_bins / width;
    *first = (int32_t)j0;
    *count = j1 > j0 ? (int32_t)(j1 - j0) : 1;  // width > n_bins: the nearest bin, repeated
    return SDRG_OK;
}

static bool display_db_range_ok(float db_min, float db_max) {
    return std::isfinite(db_min) && std::isfinite(db_max) && db_max > db_min;
}

int32_t sdrg_display_code(float db, float db_min, float db_max, uint8_t *code) {
    if (!code) return fail(SDRG_E_INVALID, "null output");
    if (!display_db_range_ok(db_min, db_max)) return fail(SDRG_E_INVALID, "db_min / db_max must be finite, db_max > db_min");
    const float scale = 255.0f / (db_max - db_min);
    const float t = (db - db_min) * scale;  // two float operations (this file is built without contraction)
    *code = t >= 255.0f ? 255 : !(t > 0.0f) ? 0 : (uint8_t)(int)(t + 0.5f);
    return SDRG_OK;
}

int32_t sdrg_engine_set_display(sdrg_engine *e, const sdrg_display_config *cfg) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    if (!cfg) return fail(SDRG_E_INVALID, "null display config");
    if (cfg->span != SDRG_DISPLAY_SPAN_FULL && cfg->span != SDRG_DISPLAY_SPAN_FOCUS && cfg->span != SDRG_DISPLAY_SPAN_BINS)
        return fail(SDRG_E_INVALID, "unknown display span %d", cfg->span);
    if (cfg->reduce != SDRG_DISPLAY_MAX && cfg->reduce != SDRG_DISPLAY_MEAN)
        return fail(SDRG_E_INVALID, "unknown display reduction %d", cfg->reduce);
    if (cfg->format != SDRG_DISPLAY_DB_F32 && cfg->format != SDRG_DISPLAY_U8)
        return fail(SDRG_E_INVALID, "unknown display format %d", cfg->format);
    if (cfg->width < 1 || cfg->width > (1 << 20)) return fail(SDRG_E_INVALID, "display width %d outside [1, 2^20]", cfg->width);
    if (cfg->span == SDRG_DISPLAY_SPAN_BINS && (cfg->first_bin < 0 || cfg->n_bins < 1))
        return fail(SDRG_E_INVALID, "display span: first_bin %d must be >= 0 and n_bins %d >= 1", cfg->first_bin, cfg->n_bins);
    if (cfg->format == SDRG_DISPLAY_U8 && !display_db_range_ok(cfg->db_min, cfg->db_max))
        return fail(SDRG_E_INVALID, "display db_min / db_max must be finite, db_max > db_min");
    e->disp.cfg = *cfg;
    e->disp.set = true;
    return SDRG_OK;
}

int32_t sdrg_engine_get_display(const sdrg_engine *e, sdrg_display_config *out) {
    if (!e || !out) return fail(SDRG_E_INVALID, "null argument");
    if (!e->disp.set) return fail(SDRG_E_INVALID, "no display configuration set");
    *out = e->disp.cfg;
    return SDRG_OK;
}

// a span (SDRG_DISPLAY_SPAN_*, first_bin, n_bins) of the display or the peak table stage (`what`) resolved against the
// current N and focus window: the bins [*lo, *lo + *nb) of a row of *n
static int32_t resolve_span(const sdrg_engine *e, const char *what, int32_t span, int32_t first_bin, int32_t n_bins,
                            int *n_out, int *lo_out, int *nb_out) {
    const int n = e->cfg.samples_per_reading;
    int64_t lo = 0, nb = n;
    if (span == SDRG_DISPLAY_SPAN_FOCUS) {
        if (e->fft_fs == 0) return fail(SDRG_E_INVALID, "the statistics' sample rate is 0");
        const StatsGeometry geo = stats_geometry(e->fft_fs, e->fft_fc, n, e->fft_focus);
        if (geo.focus_len <= 0) return fail(SDRG_E_INVALID, "the focus window is empty (focus range %d kHz)", e->fft_focus);
        lo = geo.focus_lo;
        nb = geo.focus_len;
    } else if (span == SDRG_DISPLAY_SPAN_BINS) {
        lo = first_bin;
        nb = n_bins;
    }
    if (lo < 0 || nb < 1 || lo + nb > n)
        return fail(SDRG_E_INVALID, "%s span [%lld, %lld) outside the %d bins of a frame", what, (long long)lo,
                    (long long)(lo + nb), n);
    *n_out = n;
    *lo_out = (int)lo;
    *nb_out = (int)nb;
    return SDRG_OK;
}

// the configuration in force resolved against the current N and focus window
static int32_t display_params(const sdrg_engine *e, DisplayParams *p) {
    if (!e->disp.set) return fail(SDRG_E_INVALID, "no display configuration set (sdrg_engine_set_display)");
    const sdrg_display_config &c = e->disp.cfg;
    int n, lo, nb;
    const int32_t rc = resolve_span(e, "display", c.span, c.first_bin, c.n_bins, &n, &lo, &nb);
    if (rc) return rc;
    *p = DisplayParams{n, lo, nb, c.width, c.reduce, c.format, 0.0f, 0.0f};
    if (c.format == SDRG_DISPLAY_U8) {
        p->db_min = c.db_min;
        p->scale = 255.0f / (c.db_max - c.db_min);
    }
    return SDRG_OK;
}

static size_t display_row_bytes(const DisplayParams &p) {
    return (size_t)p.width * (p.format == SDRG_DISPLAY_U8 ? 1 : sizeof(float));
}

int32_t sdrg_engine_display_geometry(const sdrg_engine *e, int32_t *first_bin, int32_t *n_bins, int32_t *row_bytes) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    DisplayParams p;
    int32_t rc = display_params(e, &p);
    if (rc) return rc;
    if (first_bin) *first_bin = p.lo;
    if (n_bins) *n_bins = p.nb;
    if (row_bytes) *row_bytes = (int32_t)display_row_bytes(p);
    return SDRG_OK;
}

int32_t sdrg_engine_display_device(sdrg_engine *e, const float *spectra, void *out) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    if (!spectra || !out) return fail(SDRG_E_INVALID, "null spectra or out");
    DisplayParams p;
    int32_t rc = display_params(e, &p);
    if (rc) return rc;
    DeviceScope dscope(e->device);
    HIP_TRY(dscope.error());
    HIP_TRY(launch_display(spectra, e->n_streams, p, out, e->s_main));
    e->outputs_unmarked = true;
    return SDRG_OK;
}

// the caller's spectra, or the device rows d_rows, -> the caller's host rows, synchronous
static int32_t display_to_host(sdrg_engine *e, const DisplayParams &p, const float *spectra, const float *d_rows, void *out) {
    DeviceScope dscope(e->device);
    HIP_TRY(dscope.error());
    const size_t B = (size_t)e->n_streams, out_bytes = B * display_row_bytes(p);
    const int32_t rc = ensure_device(&e->disp.out, out_bytes);
    if (rc) return rc;
    return spectra_round_trip(
        e, spectra, d_rows, B * (size_t)p.n,
        [&](const float *src) -> int32_t {
            HIP_TRY(launch_display(src, e->n_streams, p, e->disp.out.p, e->s_main));
            return SDRG_OK;
        },
        {{out, e->disp.out.p, out_bytes}});
}

int32_t sdrg_engine_display_host(sdrg_engine *e, const float *spectra, void *out) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    if (!out) return fail(SDRG_E_INVALID, "null out");
    DisplayParams p;
    const float *d_rows = nullptr;
    int32_t rc = display_params(e, &p);
    if (!rc) rc = resolve_spectra(e, spectra, p.n, &d_rows);
    return rc ? rc : display_to_host(e, p, spectra, d_rows, out);
}

// ---- integration stage (integrate.hip) ----------------------------------------------------------------------------

int32_t sdrg_engine_set_integration(sdrg_engine *e, const sdrg_integrate_config *cfg) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    if (!cfg) return fail(SDRG_E_INVALID, "null integration config");
    if (cfg->mode == SDRG_INTEGRATE_MEAN || cfg->mode == SDRG_INTEGRATE_MAX) {
        if (cfg->period < 1 || cfg->period > SDRG_INTEGRATE_MAX_PERIOD)
            return fail(SDRG_E_INVALID, "integration period %d outside [1, %d]", cfg->period, SDRG_INTEGRATE_MAX_PERIOD);
    } else if (cfg->mode == SDRG_INTEGRATE_EMA) {
        if (!(cfg->alpha > 0.0f && cfg->alpha <= 1.0f))  // also NaN
            return fail(SDRG_E_INVALID, "integration alpha %g outside (0, 1]", (double)cfg->alpha);
    } else {
        return fail(SDRG_E_INVALID, "unknown integration mode %d", cfg->mode);
    }
    e->integ.cfg = *cfg;
    e->integ.set = true;
    e->integ.restart();
    return SDRG_OK;
}

int32_t sdrg_engine_get_integration(const sdrg_engine *e, sdrg_integrate_config *cfg_out, int32_t *depth_out) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    if (cfg_out && !e->integ.set) return fail(SDRG_E_INVALID, "no integration configuration set");
    if (cfg_out) *cfg_out = e->integ.cfg;
    if (depth_out) *depth_out = e->integ.depth;
    return SDRG_OK;
}

int32_t sdrg_engine_integrate_reset(sdrg_engine *e) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    e->integ.restart();
    return SDRG_OK;
}

// one integrate call on the main stream: src, dst device [n_streams][N], dst may be src
static int32_t integrate_enqueue(sdrg_engine *e, const float *src, float *dst) {
    IntegrateStage &s = e->integ;
    const sdrg_integrate_config &c = s.cfg;
    const int n = e->cfg.samples_per_reading;
    const size_t count = (size_t)e->n_streams * (size_t)n, stride = integrate_slot_stride(count);
    // a resize or a retune since the previous call: the bins mean other frequencies, the history is forgotten
    const bool moved = s.seen && (n != s.n || e->cfg.sample_rate != s.fs || e->cfg.center_frequency != s.fc);
    const int64_t t = moved ? 0 : s.t;
    IntegrateParams p{c.mode, 1, 0, (int)std::min<int64_t>(t + 1, INT32_MAX), c.alpha};
    int32_t rc;
    if (c.mode == SDRG_INTEGRATE_EMA) {
        rc = ensure_device_keeping(&s.ema, count);
    } else {
        p.period = c.period;
        p.slot = (int)(t % c.period);
        p.depth = (int)std::min<int64_t>(t + 1, c.period);
        rc = ensure_device_keeping(&s.ring, (size_t)c.period * stride);
    }
    if (rc) return rc;
    // SDRG_PIPELINE_STATS_ASYNC: statistics of earlier calls may still read their spectra on s_stats; a dst that
    // overlaps such a buffer (in-place integration of the call's own spectra) is written after them
    if (e->stats_async) rc = e->sa.wait_before_write(e->s_main, dst, count);
    if (rc) return rc;
    HIP_TRY(launch_integrate(src, count, p, s.ring.p, stride, s.ema.p, dst, e->s_main));
    s.t = t + 1;
    s.depth = p.depth;
    s.seen = true;
    s.n = n;
    s.fs = e->cfg.sample_rate;
    s.fc = e->cfg.center_frequency;
    if (dst == s.out.p) s.out_n = n;  // integrate_host's rows: the _integrated_host calls read them
    e->outputs_unmarked = true;
    return SDRG_OK;
}

int32_t sdrg_engine_integrate_device(sdrg_engine *e, const float *spectra, float *out) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    if (!spectra || !out) return fail(SDRG_E_INVALID, "null spectra or out");
    if (!e->integ.set) return fail(SDRG_E_INVALID, "no integration configuration set (sdrg_engine_set_integration)");
    DeviceScope dscope(e->device);
    HIP_TRY(dscope.error());
    return integrate_enqueue(e, spectra, out);
}

int32_t sdrg_engine_integrate_host(sdrg_engine *e, const float *spectra, float *out) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    if (!e->integ.set) return fail(SDRG_E_INVALID, "no integration configuration set (sdrg_engine_set_integration)");
    const int n = e->cfg.samples_per_reading;
    const float *d_rows = nullptr;
    int32_t rc = resolve_spectra(e, spectra, n, &d_rows);
    if (rc) return rc;
    DeviceScope dscope(e->device);
    HIP_TRY(dscope.error());
    const size_t count = (size_t)e->n_streams * (size_t)n;
    rc = ensure_device_keeping(&e->integ.out, count);
    if (rc) return rc;
    return spectra_round_trip(
        e, spectra, d_rows, count,
        [&](const float *src) { return integrate_enqueue(e, src, e->integ.out.p); },
        {{out, e->integ.out.p, sizeof(float) * count}});
}

int32_t sdrg_engine_display_integrated_host(sdrg_engine *e, void *rows_out) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    if (!rows_out) return fail(SDRG_E_INVALID, "null rows_out");
    DisplayParams p;
    const float *d_rows = nullptr;
    int32_t rc = display_params(e, &p);
    if (!rc) rc = resolve_integrated(e, p.n, &d_rows);
    return rc ? rc : display_to_host(e, p, nullptr, d_rows, rows_out);
}

// ---- peak table stage (peaks.hip) ---------------------------------------------------------------------------------

int32_t sdrg_bin_offset_hz(int32_t n, int64_t sample_rate, int32_t bin, double *out) {
    if (!out) return fail(SDRG_E_INVALID, "null output");
    if (n < 1 || bin < 0 || bin >= n) return fail(SDRG_E_INVALID, "n %d must be >= 1 and bin %d in [0, n)", n, bin);
    *out = ((double)(bin - n / 2) * (double)sample_rate) / (double)n;
    return SDRG_OK;
}

int32_t sdrg_engine_set_peaks(sdrg_engine *e, const sdrg_peaks_config *cfg) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    if (!cfg) return fail(SDRG_E_INVALID, "null peaks config");
    if (cfg->span != SDRG_DISPLAY_SPAN_FULL && cfg->span != SDRG_DISPLAY_SPAN_FOCUS && cfg->span != SDRG_DISPLAY_SPAN_BINS)
        return fail(SDRG_E_INVALID, "unknown peaks span %d", cfg->span);
    if (cfg->span == SDRG_DISPLAY_SPAN_BINS && (cfg->first_bin < 0 || cfg->n_bins < 1))
        return fail(SDRG_E_INVALID, "peaks span: first_bin %d must be >= 0 and n_bins %d >= 1", cfg->first_bin, cfg->n_bins);
    if (cfg->max_peaks < 1 || cfg->max_peaks > SDRG_PEAKS_MAX)
        return fail(SDRG_E_INVALID, "max_peaks %d outside [1, %d]", cfg->max_peaks, SDRG_PEAKS_MAX);
    if (cfg->min_separation < 1 || cfg->min_separation > SDRG_PEAKS_MAX_SEPARATION)
        return fail(SDRG_E_INVALID, "min_separation %d outside [1, %d]", cfg->min_separation, SDRG_PEAKS_MAX_SEPARATION);
    if (std::isnan(cfg->threshold_db) || cfg->threshold_db == INFINITY)
        return fail(SDRG_E_INVALID, "threshold_db must be finite or -inf");
    e->peaks.cfg = *cfg;
    e->peaks.set = true;
    return SDRG_OK;
}

int32_t sdrg_engine_get_peaks(const sdrg_engine *e, sdrg_peaks_config *out) {
    if (!e || !out) return fail(SDRG_E_INVALID, "null argument");
    if (!e->peaks.set) return fail(SDRG_E_INVALID, "no peaks configuration set");
    *out = e->peaks.cfg;
    return SDRG_OK;
}

// the configuration in force resolved against the current N and focus window
static int32_t peaks_params(const sdrg_engine *e, PeaksParams *p) {
    if (!e->peaks.set) return fail(SDRG_E_INVALID, "no peaks configuration set (sdrg_engine_set_peaks)");
    const sdrg_peaks_config &c = e->peaks.cfg;
    int n, lo, nb;
    const int32_t rc = resolve_span(e, "peaks", c.span, c.first_bin, c.n_bins, &n, &lo, &nb);
    if (rc) return rc;
    *p = PeaksParams{n, lo, nb, c.max_peaks, c.min_separation, c.threshold_db};
    return SDRG_OK;
}

int32_t sdrg_engine_peaks_device(sdrg_engine *e, const float *spectra, sdrg_peak *peaks, sdrg_peaks_summary *summary) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    if (!spectra || !peaks || !summary) return fail(SDRG_E_INVALID, "null spectra, peaks or summary");
    PeaksParams p;
    int32_t rc = peaks_params(e, &p);
    if (rc) return rc;
    DeviceScope dscope(e->device);
    HIP_TRY(dscope.error());
    HIP_TRY(launch_peaks(spectra, e->n_streams, p, peaks, summary, e->s_main));
    e->outputs_unmarked = true;
    return SDRG_OK;
}

// the caller's spectra, or the device rows d_rows, -> the caller's host tables, synchronous
static int32_t peaks_to_host(sdrg_engine *e, const PeaksParams &p, const float *spectra, const float *d_rows,
                             sdrg_peak *peaks, sdrg_peaks_summary *summary) {
    DeviceScope dscope(e->device);
    HIP_TRY(dscope.error());
    const size_t B = (size_t)e->n_streams, pk_bytes = B * (size_t)p.max_peaks * sizeof(sdrg_peak),
                 sm_bytes = B * sizeof(sdrg_peaks_summary);
    const int32_t rc = ensure_device(&e->peaks.out, pk_bytes + sm_bytes);
    if (rc) return rc;
    sdrg_peak *d_pk = reinterpret_cast<sdrg_peak *>(e->peaks.out.p);
    sdrg_peaks_summary *d_sm = reinterpret_cast<sdrg_peaks_summary *>(e->peaks.out.p + pk_bytes);
    return spectra_round_trip(
        e, spectra, d_rows, B * (size_t)p.n,
        [&](const float *src) -> int32_t {
            HIP_TRY(launch_peaks(src, e->n_streams, p, d_pk, d_sm, e->s_main));
            return SDRG_OK;
        },
        {{peaks, d_pk, pk_bytes}, {summary, d_sm, sm_bytes}});
}

int32_t sdrg_engine_peaks_host(sdrg_engine *e, const float *spectra, sdrg_peak *peaks, sdrg_peaks_summary *summary) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    if (!peaks || !summary) return fail(SDRG_E_INVALID, "null peaks or summary");
    PeaksParams p;
    const float *d_rows = nullptr;
    int32_t rc = peaks_params(e, &p);
    if (!rc) rc = resolve_spectra(e, spectra, p.n, &d_rows);
    return rc ? rc : peaks_to_host(e, p, spectra, d_rows, peaks, summary);
}

int32_t sdrg_engine_peaks_integrated_host(sdrg_engine *e, sdrg_peak *peaks, sdrg_peaks_summary *summary) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    if (!peaks || !summary) return fail(SDRG_E_INVALID, "null peaks or summary");
    PeaksParams p;
    const float *d_rows = nullptr;
    int32_t rc = peaks_params(e, &p);
    if (!rc) rc = resolve_integrated(e, p.n, &d_rows);
    return rc ? rc : peaks_to_host(e, p, nullptr, d_rows, peaks, summary);
}

// ---- DDC stage (ddc.hip) ------------------------------------------------------------------------------------------

int32_t sdrg_ddc_design(int64_t sample_rate, const sdrg_ddc_config *cfg, float *taps) {
    if (!cfg || !taps) return fail(SDRG_E_INVALID, "null ddc config or taps");
    if (sample_rate < 1 || sample_rate > (int64_t)UINT32_MAX)
        return fail(SDRG_E_INVALID, "sample_rate %lld outside [1, 2^32)", (long long)sample_rate);
    if (const char *bad = ddc_check((uint32_t)sample_rate, cfg->offset_hz, cfg->cutoff_hz, cfg->decimation, cfg->taps))
        return fail(SDRG_E_INVALID, "ddc: %s", bad);
    ddc_design((uint32_t)sample_rate, cfg->cutoff_hz, cfg->taps, taps);
    return SDRG_OK;
}

int32_t sdrg_nco_tables(float *tab) {
    if (!tab) return fail(SDRG_E_INVALID, "null table");
    nco_tables(tab);
    return SDRG_OK;
}

int32_t sdrg_ddc_tile_outputs(int32_t decimation, int32_t taps, int32_t *tile) {
    if (!tile) return fail(SDRG_E_INVALID, "null tile");
    if (const char *bad = ddc_check(2, 0.0, 1.0, decimation, taps)) return fail(SDRG_E_INVALID, "ddc: %s", bad);
    *tile = ddc_tile_outputs(decimation, taps);
    return SDRG_OK;
}

int32_t sdrg_engine_set_ddc(sdrg_engine *e, const sdrg_ddc_config *cfg) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    if (cfg) {
        if (const char *bad = ddc_check((uint32_t)e->cfg.sample_rate, cfg->offset_hz, cfg->cutoff_hz, cfg->decimation,
                                        cfg->taps))
            return fail(SDRG_E_INVALID, "ddc: %s", bad);
        e->ddc.cfg = *cfg;
    }
    e->ddc.set = cfg != nullptr;
    e->ddc.taps_fs = 0;
    e->ddc.restart();
    return SDRG_OK;
}

int32_t sdrg_engine_get_ddc(const sdrg_engine *e, sdrg_ddc_config *cfg, uint32_t *nco_increment_out,
                            uint64_t *samples_consumed) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    if (!e->ddc.set) return fail(SDRG_E_INVALID, "no ddc configuration set");
    if (cfg) *cfg = e->ddc.cfg;
    if (nco_increment_out) *nco_increment_out = nco_increment(e->ddc.cfg.offset_hz, (uint32_t)e->cfg.sample_rate);
    if (samples_consumed) *samples_consumed = e->ddc.cur.g;
    return SDRG_OK;
}

int32_t sdrg_engine_ddc_reset(sdrg_engine *e) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    e->ddc.restart();
    return SDRG_OK;
}

int32_t sdrg_engine_ddc_max_out(const sdrg_engine *e, int32_t *cap) {
    if (!e || !cap) return fail(SDRG_E_INVALID, "null argument");
    if (int32_t rc = require_set(e->ddc.set, "ddc")) return rc;
    *cap = DecimCursor::cap(e->cfg.samples_per_reading, e->ddc.cfg.decimation);
    return SDRG_OK;
}

struct DdcCall : StageCall {
    int32_t fmt;
    uint32_t fs;
    DecimCursor cur;  // where the call starts: the engine's, restarted if the sample rate changed since the previous call
};

static int32_t ddc_resolve(const sdrg_engine *e, int32_t fmt, DdcCall *c) {
    const DdcStage &s = e->ddc;
    if (int32_t rc = require_set(s.set, "ddc")) return rc;
    if (bytes_per_sample(fmt) == 0) return fail(SDRG_E_INVALID, "unknown iq format %d", fmt);
    c->fmt = fmt;
    c->fs = (uint32_t)e->cfg.sample_rate;
    if (s.cfg.cutoff_hz > (double)c->fs / 2.0)
        return fail(SDRG_E_INVALID, "ddc cutoff %g Hz above half the sample rate %u", s.cfg.cutoff_hz, c->fs);
    c->cur = s.cur;
    if (s.fs != 0 && s.fs != c->fs) c->cur.restart();
    c->n = e->cfg.samples_per_reading;
    c->cap = DecimCursor::cap(c->n, s.cfg.decimation);
    c->n_out = c->cur.n_out(c->n, s.cfg.decimation);
    c->in_bytes = (size_t)e->n_streams * (size_t)c->n * (size_t)bytes_per_sample(fmt);
    c->out_bytes = (size_t)e->n_streams * (size_t)c->cap * 2 * sizeof(float);
    return SDRG_OK;
}

static int32_t ddc_reserve(sdrg_engine *e, const DdcCall &c) {
    DdcStage &s = e->ddc;
    int32_t rc = ensure_halves(&s.hist, s.half(e->n_streams));
    if (rc) return rc;
    // a longer frame than any before: hipFree waits for the calls that read the old row
    rc = ensure_device(&s.w, 2 * (size_t)c.n);
    if (rc) return rc;
    rc = ensure_nco_table(e);
    if (rc) return rc;
    if (s.taps_fs != c.fs) {  // the taps travel in the kernel arguments: nothing on the device to replace
        ddc_design(c.fs, s.cfg.cutoff_hz, s.cfg.taps, s.taps.h);
        s.taps_fs = c.fs;
    }
    return SDRG_OK;
}

// one ddc call on the main stream: iq, out in device memory
static int32_t ddc_launch(sdrg_engine *e, const DdcCall &c, const void *iq, void *out) {
    DdcStage &s = e->ddc;
    DdcParams p{};
    fir_tile_fill(&p, c.cur, s.cfg.decimation, s.cfg.taps, c, s.hist, s.half(e->n_streams));
    p.inc = nco_increment(s.cfg.offset_hz, c.fs);
    p.g0_lo = (uint32_t)c.cur.g;
    p.nco_tab = e->d_nco_tab.p;
    p.phasors = s.w.p;
    HIP_TRY(launch_ddc(iq, c.fmt, e->n_streams, p, s.taps, static_cast<float *>(out), e->s_main));
    s.cur = c.cur;
    s.cur.advance(c.n);
    s.fs = c.fs;
    e->outputs_unmarked = true;
    return SDRG_OK;
}

static constexpr auto ddc_stage = &stage_call<DdcCall, ddc_resolve, ddc_reserve, ddc_launch, int32_t>;

int32_t sdrg_engine_ddc_device(sdrg_engine *e, const void *iq, int32_t fmt, void *out, int32_t *n_out) {
    return ddc_stage(e, "iq", iq, out, n_out, false, fmt);
}

int32_t sdrg_engine_ddc_host(sdrg_engine *e, const void *iq, int32_t fmt, void *out, int32_t *n_out) {
    return ddc_stage(e, "iq", iq, out, n_out, true, fmt);
}

// ---- DDC bank stage (bank.hip) ------------------------------------------------------------------------------------

int32_t sdrg_bank_geometry(int32_t decimation, int32_t taps, int32_t channels, int32_t n_streams, int32_t *tile_outputs,
                           int32_t *channels_per_group) {
    if (const char *bad = bank_check(2, 1.0, decimation, taps, channels, n_streams))
        return fail(SDRG_E_INVALID, "bank: %s", bad);
    if (tile_outputs) *tile_outputs = bank_tile_outputs(decimation, taps);
    if (channels_per_group) *channels_per_group = bank_group(channels, n_streams);
    return SDRG_OK;
}

int32_t sdrg_engine_set_bank(sdrg_engine *e, const sdrg_bank_config *cfg, const double *offsets_hz) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    BankStage &s = e->bank;
    if (cfg) {
        const char *bad = bank_check((uint32_t)e->cfg.sample_rate, cfg->cutoff_hz, cfg->decimation, cfg->taps,
                                     cfg->channels, e->n_streams);
        if (!bad) bad = bank_offsets_check(offsets_hz, (size_t)e->n_streams * (size_t)cfg->channels);
        if (bad) return fail(SDRG_E_INVALID, "bank: %s", bad);
        s.cfg = *cfg;
        s.offsets.assign(offsets_hz, offsets_hz + s.rows(e->n_streams));
    }
    s.set = cfg != nullptr;
    s.taps_fs = 0;
    s.inc_fs = 0;
    s.restart();
    return SDRG_OK;
}

int32_t sdrg_engine_bank_retune(sdrg_engine *e, const double *offsets_hz) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    BankStage &s = e->bank;
    if (int32_t rc = require_set(s.set, "bank")) return rc;
    if (const char *bad = bank_offsets_check(offsets_hz, s.rows(e->n_streams)))
        return fail(SDRG_E_INVALID, "bank: %s", bad);
    s.offsets.assign(offsets_hz, offsets_hz + s.rows(e->n_streams));
    s.inc_fs = 0;  // the next call fills the table no launch in flight reads
    return SDRG_OK;
}

int32_t sdrg_engine_get_bank(const sdrg_engine *e, sdrg_bank_config *cfg, uint64_t *samples_consumed) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    if (!e->bank.set) return fail(SDRG_E_INVALID, "no bank configuration set");
    if (cfg) *cfg = e->bank.cfg;
    if (samples_consumed) *samples_consumed = e->bank.cur.g;
    return SDRG_OK;
}

int32_t sdrg_engine_bank_offsets(const sdrg_engine *e, double *offsets_hz, uint32_t *increments) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    const BankStage &s = e->bank;
    if (!s.set) return fail(SDRG_E_INVALID, "no bank configuration set");
    for (size_t i = 0; i < s.offsets.size(); i++) {
        if (offsets_hz) offsets_hz[i] = s.offsets[i];
        if (increments) increments[i] = nco_increment(s.offsets[i], (uint32_t)e->cfg.sample_rate);
    }
    return SDRG_OK;
}

int32_t sdrg_engine_bank_reset(sdrg_engine *e) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    e->bank.restart();
    return SDRG_OK;
}

int32_t sdrg_engine_bank_max_out(const sdrg_engine *e, int32_t *cap) {
    if (!e || !cap) return fail(SDRG_E_INVALID, "null argument");
    if (int32_t rc = require_set(e->bank.set, "bank")) return rc;
    *cap = DecimCursor::cap(e->cfg.samples_per_reading, e->bank.cfg.decimation);
    return SDRG_OK;
}

using BankCall = DdcCall;  // the format, the sample rate and the cursor the call starts from

static int32_t bank_resolve(const sdrg_engine *e, int32_t fmt, BankCall *c) {
    const BankStage &s = e->bank;
    if (int32_t rc = require_set(s.set, "bank")) return rc;
    if (bytes_per_sample(fmt) == 0) return fail(SDRG_E_INVALID, "unknown iq format %d", fmt);
    c->fmt = fmt;
    c->fs = (uint32_t)e->cfg.sample_rate;
    if (s.cfg.cutoff_hz > (double)c->fs / 2.0)
        return fail(SDRG_E_INVALID, "bank cutoff %g Hz above half the sample rate %u", s.cfg.cutoff_hz, c->fs);
    c->cur = s.cur;
    if (s.fs != 0 && s.fs != c->fs) c->cur.restart();
    c->n = e->cfg.samples_per_reading;
    c->cap = DecimCursor::cap(c->n, s.cfg.decimation);
    c->n_out = c->cur.n_out(c->n, s.cfg.decimation);
    c->in_bytes = (size_t)e->n_streams * (size_t)c->n * (size_t)bytes_per_sample(fmt);
    c->out_bytes = s.rows(e->n_streams) * (size_t)c->cap * 2 * sizeof(float);
    return SDRG_OK;
}

static int32_t bank_reserve(sdrg_engine *e, const BankCall &c) {
    BankStage &s = e->bank;
    int32_t rc = ensure_halves(&s.hist, s.half(e->n_streams));
    if (rc) return rc;
    rc = ensure_nco_table(e);
    if (rc) return rc;
    if (s.inc_fs != c.fs) {  // new offsets or another rate: into the table the last launch does not read
        const int at = s.inc_at ^ 1;
        const size_t rows = s.rows(e->n_streams);
        HIP_TRY(s.read[at].create(hipEventDisableTiming));
        if (s.read_marked[at]) HIP_TRY(hipEventSynchronize(s.read[at]));  // the launch before the last
        rc = ensure_device(&s.inc[at], rows);
        if (rc) return rc;
        std::vector<uint32_t> inc(rows);
        for (size_t i = 0; i < rows; i++) inc[i] = nco_increment(s.offsets[i], c.fs);
        HIP_TRY(hipMemcpy(s.inc[at].p, inc.data(), sizeof(uint32_t) * rows, hipMemcpyHostToDevice));
        s.inc_at = at;  // what is committed here is the offsets in force at this rate: no call's state
        s.inc_fs = c.fs;
    }
    HIP_TRY(s.read[s.inc_at].create(hipEventDisableTiming));
    if (s.taps_fs != c.fs) {  // the taps travel in the kernel arguments: nothing on the device to replace
        ddc_design(c.fs, s.cfg.cutoff_hz, s.cfg.taps, s.taps.h);
        s.taps_fs = c.fs;
    }
    return SDRG_OK;
}

// one bank call on the main stream: iq, out in device memory
static int32_t bank_launch(sdrg_engine *e, const BankCall &c, const void *iq, void *out) {
    BankStage &s = e->bank;
    BankParams p{};
    fir_tile_fill(&p, c.cur, s.cfg.decimation, s.cfg.taps, c, s.hist, s.half(e->n_streams));
    p.g0_lo = (uint32_t)c.cur.g;
    p.nco_tab = e->d_nco_tab.p;
    p.incs = s.inc[s.inc_at].p;
    p.channels = s.cfg.channels;
    HIP_TRY(launch_bank(iq, c.fmt, e->n_streams, p, s.taps, static_cast<float *>(out), e->s_main));
    HIP_TRY(hipEventRecord(s.read[s.inc_at], e->s_main));
    s.read_marked[s.inc_at] = true;
    s.cur = c.cur;
    s.cur.advance(c.n);
    s.fs = c.fs;
    e->outputs_unmarked = true;
    return SDRG_OK;
}

static constexpr auto bank_stage = &stage_call<BankCall, bank_resolve, bank_reserve, bank_launch, int32_t>;

int32_t sdrg_engine_bank_device(sdrg_engine *e, const void *iq, int32_t fmt, void *out, int32_t *n_out) {
    return bank_stage(e, "iq", iq, out, n_out, false, fmt);
}

int32_t sdrg_engine_bank_host(sdrg_engine *e, const void *iq, int32_t fmt, void *out, int32_t *n_out) {
    return bank_stage(e, "iq", iq, out, n_out, true, fmt);
}

// ---- demodulator stage (demod.hip) --------------------------------------------------------------------------------

int32_t sdrg_demod_design(const sdrg_demod_config *cfg, float *kf, float *alpha, float *a, float *taps) {
    if (!cfg) return fail(SDRG_E_INVALID, "null demod config");
    if (const char *bad = demod_check(*cfg)) return fail(SDRG_E_INVALID, "demod: %s", bad);
    demod_design(*cfg, kf, alpha, a, taps);
    return SDRG_OK;
}

int32_t sdrg_demod_geometry(int32_t audio_decimation, int32_t audio_taps, int32_t *tile, int32_t *chunk) {
    if (!tile || !chunk) return fail(SDRG_E_INVALID, "null tile or chunk");
    if (audio_decimation < 1 || audio_decimation > SDRG_DEMOD_MAX_DECIMATION || audio_taps < 1 ||
        audio_taps > SDRG_DEMOD_MAX_TAPS || (audio_taps & 1) == 0)
        return fail(SDRG_E_INVALID, "demod: audio_decimation outside [1, 64] or audio_taps not odd in [1, 255]");
    *tile = demod_tile_outputs(audio_decimation, audio_taps);
    *chunk = DEMOD_CHUNK;
    return SDRG_OK;
}

int32_t sdrg_engine_set_demod(sdrg_engine *e, const sdrg_demod_config *cfg) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    DemodStage &s = e->demod;
    if (cfg) {
        if (const char *bad = demod_check(*cfg)) return fail(SDRG_E_INVALID, "demod: %s", bad);
        s.cfg = *cfg;
        demod_design(*cfg, &s.kf, &s.alpha, &s.a, s.taps.h);
    }
    s.set = cfg != nullptr;
    s.cur.restart();
    return SDRG_OK;
}

int32_t sdrg_engine_get_demod(const sdrg_engine *e, sdrg_demod_config *cfg, float *kf, float *alpha, float *a,
                              float *taps, uint64_t *samples_consumed) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    const DemodStage &s = e->demod;
    if (!s.set) return fail(SDRG_E_INVALID, "no demod configuration set");
    if (cfg) *cfg = s.cfg;
    if (kf) *kf = s.kf;
    if (alpha) *alpha = s.alpha;
    if (a) *a = s.a;
    if (taps) std::copy(s.taps.h, s.taps.h + s.cfg.audio_taps, taps);
    if (samples_consumed) *samples_consumed = s.cur.g;
    return SDRG_OK;
}

int32_t sdrg_engine_demod_reset(sdrg_engine *e) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    e->demod.cur.restart();
    return SDRG_OK;
}

int32_t sdrg_engine_demod_max_out(const sdrg_engine *e, int32_t *cap) {
    if (!e || !cap) return fail(SDRG_E_INVALID, "null argument");
    if (int32_t rc = require_set(e->demod.set, "demod")) return rc;
    *cap = e->demod.cap();
    return SDRG_OK;
}

static int32_t demod_resolve(const sdrg_engine *e, int32_t n, StageCall *c) {
    const DemodStage &s = e->demod;
    if (int32_t rc = require_set(s.set, "demod")) return rc;
    if (n < 0 || n > s.cfg.max_in) return fail(SDRG_E_INVALID, "demod: n %d outside [0, max_in = %d]", n, s.cfg.max_in);
    c->n = n;
    c->in_stride = s.cfg.max_in;
    c->cap = s.cap();
    c->n_out = s.cur.n_out(n, s.cfg.audio_decimation);
    c->in_bytes = (size_t)e->n_streams * (size_t)c->in_stride * 2 * sizeof(float);
    c->out_bytes = (size_t)e->n_streams * (size_t)c->cap *
                   (s.cfg.out_format == SDRG_DEMOD_OUT_F32 ? sizeof(float) : sizeof(int16_t));
    return SDRG_OK;
}

static int32_t demod_reserve(sdrg_engine *e, const StageCall &) {
    const int32_t rc = ensure_halves(&e->demod.state, e->demod.half(e->n_streams));
    return rc ? rc : ensure_device(&e->demod.scratch, (size_t)e->n_streams * (size_t)e->demod.cfg.max_in);
}

// one demod call on the main stream: chan (rows of in_stride complex samples), out in device memory
static int32_t demod_launch(sdrg_engine *e, const StageCall &c, const void *chan, void *out) {
    DemodStage &s = e->demod;
    const size_t B = (size_t)e->n_streams, half = s.half(e->n_streams);
    DemodParams p{};
    // a half holds the streams' four state words, then the history
    fir_tile_fill(&p, s.cur, s.cfg.audio_decimation, s.cfg.audio_taps, c, s.state, half, B * 4);
    p.in_stride = c.in_stride;
    p.scratch_stride = s.cfg.max_in;
    p.mode = s.cfg.mode;
    p.out_format = s.cfg.out_format;
    p.fresh = s.cur.fresh ? 1 : 0;
    p.kf = s.kf;
    p.alpha = s.alpha;
    p.a = s.a;
    p.gain = s.cfg.gain;
    p.state_old = s.state.half(s.cur.old_half(), half);  // not read by a fresh call: p.fresh says so
    p.state_new = s.state.next(s.cur, half);
    p.scratch = s.scratch.p;
    HIP_TRY(launch_demod(static_cast<const float *>(chan), e->n_streams, p, s.taps, out, e->s_main));
    s.cur.advance(c.n);  // a call without samples wrote out only: the state stays where it is
    e->outputs_unmarked = true;
    return SDRG_OK;
}

static constexpr auto demod_stage = &stage_call<StageCall, demod_resolve, demod_reserve, demod_launch, int32_t>;

int32_t sdrg_engine_demod_device(sdrg_engine *e, const void *chan, int32_t n, void *out, int32_t *n_out) {
    return demod_stage(e, "chan", chan, out, n_out, false, n);
}

int32_t sdrg_engine_demod_host(sdrg_engine *e, const void *chan, int32_t n, void *out, int32_t *n_out) {
    return demod_stage(e, "chan", chan, out, n_out, true, n);
}

// ---- channelizer stage (channelizer.hip) ---------------------------------------------------------------------------

int32_t sdrg_channelizer_design(const sdrg_channelizer_config *cfg, float *taps) {
    if (!cfg || !taps) return fail(SDRG_E_INVALID, "null channelizer config or taps");
    if (const char *bad = chan_check(*cfg)) return fail(SDRG_E_INVALID, "channelizer: %s", bad);
    chan_design(*cfg, taps);
    return SDRG_OK;
}

int32_t sdrg_channelizer_tile_outputs(const sdrg_channelizer_config *cfg, int32_t *tile) {
    if (!cfg || !tile) return fail(SDRG_E_INVALID, "null channelizer config or tile");
    if (const char *bad = chan_check(*cfg)) return fail(SDRG_E_INVALID, "channelizer: %s", bad);
    *tile = chan_tile_outputs(cfg->channels);
    return SDRG_OK;
}

int32_t sdrg_engine_set_channelizer(sdrg_engine *e, const sdrg_channelizer_config *cfg) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    if (cfg) {
        if (const char *bad = chan_check(*cfg)) return fail(SDRG_E_INVALID, "channelizer: %s", bad);
        // the taps, then the DFT's twiddles
        const size_t L = (size_t)cfg->channels * (size_t)cfg->taps_per_channel;
        std::vector<float> host(L + 2 * (size_t)CHAN_TWIDDLES);
        chan_design(*cfg, host.data());
        for (int t = 0; t < CHAN_TWIDDLES; t++) {
            const double a = 2.0 * M_PI * (double)t / (double)CHAN_TWIDDLES;
            host[L + 2 * (size_t)t] = (float)std::cos(a);
            host[L + 2 * (size_t)t + 1] = (float)-std::sin(a);
        }
        DeviceScope dscope(e->device);
        HIP_TRY(dscope.error());
        const int32_t rc = upload_floats(&e->chan.d_taps, host, "channelizer taps");
        if (rc) return rc;
        e->chan.cfg = *cfg;
    }
    e->chan.set = cfg != nullptr;
    e->chan.cur.restart();
    return SDRG_OK;
}

int32_t sdrg_engine_get_channelizer(const sdrg_engine *e, sdrg_channelizer_config *cfg, uint64_t *samples_consumed) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    if (!e->chan.set) return fail(SDRG_E_INVALID, "no channelizer configuration set");
    if (cfg) *cfg = e->chan.cfg;
    if (samples_consumed) *samples_consumed = e->chan.cur.g;
    return SDRG_OK;
}

int32_t sdrg_engine_channelizer_reset(sdrg_engine *e) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    e->chan.cur.restart();
    return SDRG_OK;
}

int32_t sdrg_engine_channelizer_max_out(const sdrg_engine *e, int32_t *cap) {
    if (!e || !cap) return fail(SDRG_E_INVALID, "null argument");
    if (int32_t rc = require_set(e->chan.set, "channelizer")) return rc;
    *cap = DecimCursor::cap(e->cfg.samples_per_reading, e->chan.decim());
    return SDRG_OK;
}

struct ChanCall : StageCall {
    int32_t fmt;
};

static int32_t chan_resolve(const sdrg_engine *e, int32_t fmt, ChanCall *c) {
    const ChanStage &s = e->chan;
    if (int32_t rc = require_set(s.set, "channelizer")) return rc;
    if (bytes_per_sample(fmt) == 0) return fail(SDRG_E_INVALID, "unknown iq format %d", fmt);
    c->fmt = fmt;
    c->n = e->cfg.samples_per_reading;
    c->cap = DecimCursor::cap(c->n, s.decim());
    c->n_out = s.cur.n_out(c->n, s.decim());
    c->in_bytes = (size_t)e->n_streams * (size_t)c->n * (size_t)bytes_per_sample(fmt);
    c->out_bytes = (size_t)e->n_streams * (size_t)s.cfg.n_channels * (size_t)c->cap * 2 * sizeof(float);
    return SDRG_OK;
}

static int32_t chan_reserve(sdrg_engine *e, const ChanCall &) { return ensure_halves(&e->chan.hist, e->chan.half(e->n_streams)); }

// one channelizer call on the main stream: iq, out in device memory
static int32_t chan_launch(sdrg_engine *e, const ChanCall &c, const void *iq, void *out) {
    ChanStage &s = e->chan;
    const size_t half = s.half(e->n_streams);
    ChanParams p{};
    p.n = c.n;
    p.channels = s.cfg.channels;
    p.taps_per_channel = s.cfg.taps_per_channel;
    p.oversample = s.cfg.oversample;
    p.decim = s.decim();
    p.first = s.cur.first(p.decim);
    p.n_out = c.n_out;
    p.cap = c.cap;
    p.first_channel = s.cfg.first_channel;
    p.n_channels = s.cfg.n_channels;
    p.m_parity = (int)(s.cur.first_output(p.decim) & 1);
    p.taps = s.d_taps.p;
    p.hist_old = s.hist.old(s.cur, half);
    p.hist_new = s.hist.next(s.cur, half);
    HIP_TRY(launch_channelizer(iq, c.fmt, e->n_streams, p, static_cast<float *>(out), e->s_main));
    s.cur.advance(c.n);
    e->outputs_unmarked = true;
    return SDRG_OK;
}

static constexpr auto chan_stage = &stage_call<ChanCall, chan_resolve, chan_reserve, chan_launch, int32_t>;

int32_t sdrg_engine_channelizer_device(sdrg_engine *e, const void *iq, int32_t fmt, void *out, int32_t *n_out) {
    return chan_stage(e, "iq", iq, out, n_out, false, fmt);
}

int32_t sdrg_engine_channelizer_host(sdrg_engine *e, const void *iq, int32_t fmt, void *out, int32_t *n_out) {
    return chan_stage(e, "iq", iq, out, n_out, true, fmt);
}

// ---- resampler stage (resample.hip) --------------------------------------------------------------------------------

int32_t sdrg_resample_design(const sdrg_resample_config *cfg, float *taps) {
    if (!cfg || !taps) return fail(SDRG_E_INVALID, "null resample config or taps");
    if (const char *bad = resample_check(*cfg)) return fail(SDRG_E_INVALID, "resample: %s", bad);
    resample_design(*cfg, taps);
    return SDRG_OK;
}

int32_t sdrg_resample_tile_outputs(const sdrg_resample_config *cfg, int32_t *tile) {
    if (!cfg || !tile) return fail(SDRG_E_INVALID, "null resample config or tile");
    if (const char *bad = resample_check(*cfg)) return fail(SDRG_E_INVALID, "resample: %s", bad);
    *tile = RESAMPLE_TILE;
    return SDRG_OK;
}

int32_t sdrg_resample_ratio(uint64_t in_num, uint64_t in_den, uint64_t out_hz, int32_t *interp, int32_t *decim) {
    if (!interp || !decim) return fail(SDRG_E_INVALID, "null interp or decim");
    int L, M;
    if (!resample_ratio(in_num, in_den, out_hz, &L, &M))
        return fail(SDRG_E_INVALID,
                    "resample: %llu Hz from %llu / %llu Hz is no ratio of integers in [1, 512] inside [1/8, 8]",
                    (unsigned long long)out_hz, (unsigned long long)in_num, (unsigned long long)in_den);
    *interp = L;
    *decim = M;
    return SDRG_OK;
}

int32_t sdrg_engine_set_resample(sdrg_engine *e, const sdrg_resample_config *cfg) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    if (cfg) {
        if (const char *bad = resample_check(*cfg)) return fail(SDRG_E_INVALID, "resample: %s", bad);
        // the device's copy is transposed to the polyphase order [phi][k] = h[phi + k L]
        const int L = cfg->interp, P = cfg->taps_per_phase;
        std::vector<float> h((size_t)L * (size_t)P), poly(h.size());
        resample_design(*cfg, h.data());
        for (int phi = 0; phi < L; phi++)
            for (int k = 0; k < P; k++) poly[(size_t)phi * (size_t)P + (size_t)k] = h[(size_t)phi + (size_t)k * (size_t)L];
        DeviceScope dscope(e->device);
        HIP_TRY(dscope.error());
        const int32_t rc = upload_floats(&e->rs.d_taps, poly, "resample taps");
        if (rc) return rc;
        e->rs.taps.swap(h);
        e->rs.cfg = *cfg;
    }
    e->rs.set = cfg != nullptr;
    e->rs.cur.restart();
    return SDRG_OK;
}

int32_t sdrg_engine_get_resample(const sdrg_engine *e, sdrg_resample_config *cfg, float *taps, uint64_t *samples_consumed) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    if (!e->rs.set) return fail(SDRG_E_INVALID, "no resample configuration set");
    if (cfg) *cfg = e->rs.cfg;
    if (taps) std::copy(e->rs.taps.begin(), e->rs.taps.end(), taps);
    if (samples_consumed) *samples_consumed = e->rs.cur.g;
    return SDRG_OK;
}

int32_t sdrg_engine_resample_reset(sdrg_engine *e) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    e->rs.cur.restart();
    return SDRG_OK;
}

int32_t sdrg_engine_resample_max_out(const sdrg_engine *e, int32_t *cap) {
    if (!e || !cap) return fail(SDRG_E_INVALID, "null argument");
    if (int32_t rc = require_set(e->rs.set, "resample")) return rc;
    *cap = e->rs.cap();
    return SDRG_OK;
}

static int32_t rs_resolve(const sdrg_engine *e, int32_t in_stride, int32_t n, StageCall *c) {
    const ResampleStage &s = e->rs;
    if (int32_t rc = require_set(s.set, "resample")) return rc;
    if (n < 0 || n > s.cfg.max_in) return fail(SDRG_E_INVALID, "resample: n %d outside [0, max_in = %d]", n, s.cfg.max_in);
    if (in_stride < n) return fail(SDRG_E_INVALID, "resample: in_stride %d smaller than n %d", in_stride, n);
    c->n = n;
    c->in_stride = in_stride;
    c->cap = s.cap();
    c->n_out = s.cur.n_out(n, s.cfg.interp, s.cfg.decim);
    c->in_bytes = (size_t)e->n_streams * (size_t)in_stride * (size_t)s.cfg.components * sizeof(float);
    c->out_bytes = (size_t)e->n_streams * (size_t)c->cap * (size_t)s.cfg.components *
                   (s.cfg.out_format == SDRG_RESAMPLE_OUT_F32 ? sizeof(float) : sizeof(int16_t));
    return SDRG_OK;
}

static int32_t rs_reserve(sdrg_engine *e, const StageCall &) { return ensure_halves(&e->rs.hist, e->rs.half(e->n_streams)); }

// one resample call on the main stream: in (rows of in_stride values), out in device memory
static int32_t rs_launch(sdrg_engine *e, const StageCall &c, const void *in, void *out) {
    ResampleStage &s = e->rs;
    const size_t half = s.half(e->n_streams);
    ResampleParams p{};
    p.n = c.n;
    p.in_stride = c.in_stride;
    p.interp = s.cfg.interp;
    p.decim = s.cfg.decim;
    p.taps_per_phase = s.cfg.taps_per_phase;
    p.q0 = s.cur.q0(s.cfg.interp, s.cfg.decim);
    p.phi0 = s.cur.phi0(s.cfg.interp, s.cfg.decim);
    p.n_out = c.n_out;
    p.cap = c.cap;
    p.components = s.cfg.components;
    p.out_format = s.cfg.out_format;
    p.gain = s.cfg.gain;
    p.taps = s.d_taps.p;
    p.hist_old = s.hist.old(s.cur, half);  // nullptr after a restart: zeros
    p.hist_new = s.hist.next(s.cur, half);
    HIP_TRY(launch_resample(in, e->n_streams, p, out, e->s_main));
    s.cur.advance(c.n);  // a call without samples wrote out only: the state stays where it is
    e->outputs_unmarked = true;
    return SDRG_OK;
}

static constexpr auto rs_stage = &stage_call<StageCall, rs_resolve, rs_reserve, rs_launch, int32_t, int32_t>;

int32_t sdrg_engine_resample_device(sdrg_engine *e, const void *in, int32_t in_stride, int32_t n, void *out,
                                    int32_t *n_out) {
    return rs_stage(e, "in", in, out, n_out, false, in_stride, n);
}

int32_t sdrg_engine_resample_host(sdrg_engine *e, const void *in, int32_t in_stride, int32_t n, void *out,
                                  int32_t *n_out) {
    return rs_stage(e, "in", in, out, n_out, true, in_stride, n);
}

// ---- squelch stage (squelch.hip) -----------------------------------------------------------------------------------

int32_t sdrg_squelch_design(const sdrg_squelch_config *cfg, float *open_thr, float *close_thr, float *beta) {
    if (!cfg) return fail(SDRG_E_INVALID, "null squelch config");
    if (const char *bad = squelch_check(*cfg)) return fail(SDRG_E_INVALID, "squelch: %s", bad);
    squelch_design(*cfg, open_thr, close_thr, beta);
    return SDRG_OK;
}

int32_t sdrg_squelch_geometry(int32_t block, int32_t *tile) { return block_geometry("squelch", block, tile); }

int32_t sdrg_engine_set_squelch(sdrg_engine *e, const sdrg_squelch_config *cfg) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    SquelchStage &s = e->sq;
    if (cfg) {
        if (const char *bad = squelch_check(*cfg)) return fail(SDRG_E_INVALID, "squelch: %s", bad);
        s.cfg = *cfg;
        squelch_design(*cfg, &s.open_thr, &s.close_thr, &s.beta);
    }
    s.set = cfg != nullptr;
    s.cur.restart();
    return SDRG_OK;
}

int32_t sdrg_engine_get_squelch(const sdrg_engine *e, sdrg_squelch_config *cfg, float *open_thr, float *close_thr,
                                float *beta, uint64_t *samples_consumed) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    const SquelchStage &s = e->sq;
    if (!s.set) return fail(SDRG_E_INVALID, "no squelch configuration set");
    if (cfg) *cfg = s.cfg;
    if (open_thr) *open_thr = s.open_thr;
    if (close_thr) *close_thr = s.close_thr;
    if (beta) *beta = s.beta;
    if (samples_consumed) *samples_consumed = s.cur.g;
    return SDRG_OK;
}

int32_t sdrg_engine_squelch_reset(sdrg_engine *e) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    e->sq.cur.restart();
    return SDRG_OK;
}

static int32_t sq_resolve(const sdrg_engine *e, int32_t in_stride, int32_t n, sdrg_squelch_record *records, StageCall *c) {
    return block_resolve(e, e->sq, "squelch", sizeof(*records), in_stride, n, records, c);
}

static int32_t sq_reserve(sdrg_engine *e, const StageCall &) { return block_reserve(e, &e->sq); }

static int32_t sq_launch(sdrg_engine *e, const StageCall &c, const void *chan, void *out) {
    SquelchParams p{};
    p.beta = e->sq.beta;
    p.open_thr = e->sq.open_thr;
    p.close_thr = e->sq.close_thr;
    return block_launch(e, &e->sq, c, p, launch_squelch, chan, out);
}

static constexpr auto sq_stage =
    &stage_call<StageCall, sq_resolve, sq_reserve, sq_launch, int32_t, int32_t, sdrg_squelch_record *>;

int32_t sdrg_engine_squelch_device(sdrg_engine *e, const void *chan, int32_t in_stride, int32_t n, void *out,
                                   sdrg_squelch_record *records, int32_t *n_blocks) {
    return sq_stage(e, "chan", chan, out, n_blocks, false, in_stride, n, records);
}

int32_t sdrg_engine_squelch_host(sdrg_engine *e, const void *chan, int32_t in_stride, int32_t n, void *out,
                                 sdrg_squelch_record *records, int32_t *n_blocks) {
    return sq_stage(e, "chan", chan, out, n_blocks, true, in_stride, n, records);
}

// ---- AGC stage (agc.hip) ---------------------------------------------------------------------------------------------

static void agc_design_out(const AgcDesign &d, float *max_gain, float *init_gain, float *floor_thr, float *alpha_a,
                           float *alpha_d) {
    if (max_gain) *max_gain = d.max_gain;
    if (init_gain) *init_gain = d.init_gain;
    if (floor_thr) *floor_thr = d.floor_thr;
    if (alpha_a) *alpha_a = d.alpha_a;
    if (alpha_d) *alpha_d = d.alpha_d;
}

int32_t sdrg_agc_design(const sdrg_agc_config *cfg, float *max_gain, float *init_gain, float *floor_thr, float *alpha_a,
                        float *alpha_d) {
    if (!cfg) return fail(SDRG_E_INVALID, "null agc config");
    if (const char *bad = agc_check(*cfg)) return fail(SDRG_E_INVALID, "agc: %s", bad);
    agc_design_out(agc_design(*cfg), max_gain, init_gain, floor_thr, alpha_a, alpha_d);
    return SDRG_OK;
}

int32_t sdrg_agc_geometry(int32_t block, int32_t *tile) { return block_geometry("agc", block, tile); }

int32_t sdrg_engine_set_agc(sdrg_engine *e, const sdrg_agc_config *cfg) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    AgcStage &s = e->agc;
    if (cfg) {
        if (const char *bad = agc_check(*cfg)) return fail(SDRG_E_INVALID, "agc: %s", bad);
        s.cfg = *cfg;
        s.target = (float)cfg->target;
        s.des = agc_design(*cfg);
    }
    s.set = cfg != nullptr;
    s.cur.restart();
    return SDRG_OK;
}

int32_t sdrg_engine_get_agc(const sdrg_engine *e, sdrg_agc_config *cfg, float *max_gain, float *init_gain,
                            float *floor_thr, float *alpha_a, float *alpha_d, uint64_t *samples_consumed) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    const AgcStage &s = e->agc;
    if (!s.set) return fail(SDRG_E_INVALID, "no agc configuration set");
    if (cfg) *cfg = s.cfg;
    agc_design_out(s.des, max_gain, init_gain, floor_thr, alpha_a, alpha_d);
    if (samples_consumed) *samples_consumed = s.cur.g;
    return SDRG_OK;
}

int32_t sdrg_engine_agc_reset(sdrg_engine *e) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    e->agc.cur.restart();
    return SDRG_OK;
}

static int32_t agc_resolve(const sdrg_engine *e, int32_t in_stride, int32_t n, sdrg_agc_record *records, StageCall *c) {
    return block_resolve(e, e->agc, "agc", sizeof(*records), in_stride, n, records, c);
}

static int32_t agc_reserve(sdrg_engine *e, const StageCall &) { return block_reserve(e, &e->agc); }

static int32_t agc_launch(sdrg_engine *e, const StageCall &c, const void *chan, void *out) {
    const AgcStage &s = e->agc;
    AgcParams p{};
    p.detector = s.cfg.detector;
    p.target = s.target;
    p.max_gain = s.des.max_gain;
    p.init_gain = s.des.init_gain;
    p.floor_thr = s.des.floor_thr;
    p.alpha_a = s.des.alpha_a;
    p.alpha_d = s.des.alpha_d;
    return block_launch(e, &e->agc, c, p, launch_agc, chan, out);
}

static constexpr auto agc_stage =
    &stage_call<StageCall, agc_resolve, agc_reserve, agc_launch, int32_t, int32_t, sdrg_agc_record *>;

int32_t sdrg_engine_agc_device(sdrg_engine *e, const void *chan, int32_t in_stride, int32_t n, void *out,
                               sdrg_agc_record *records, int32_t *n_blocks) {
    return agc_stage(e, "chan", chan, out, n_blocks, false, in_stride, n, records);
}

int32_t sdrg_engine_agc_host(sdrg_engine *e, const void *chan, int32_t in_stride, int32_t n, void *out,
                             sdrg_agc_record *records, int32_t *n_blocks) {
    return agc_stage(e, "chan", chan, out, n_blocks, true, in_stride, n, records);
}

// ---- sideband stage (sideband.hip) ---------------------------------------------------------------------------------

int32_t sdrg_sideband_design(const sdrg_sideband_config *cfg, float *cr, float *ci) {
    if (!cfg) return fail(SDRG_E_INVALID, "null sideband config");
    if (const char *bad = sideband_check(*cfg)) return fail(SDRG_E_INVALID, "sideband: %s", bad);
    sideband_design(*cfg, cr, ci);
    return SDRG_OK;
}

int32_t sdrg_sideband_geometry(int32_t audio_decimation, int32_t taps, int32_t *tile) {
    if (!tile) return fail(SDRG_E_INVALID, "null tile");
    if (audio_decimation < 1 || audio_decimation > SDRG_SIDEBAND_MAX_DECIMATION || taps < 1 ||
        taps > SDRG_SIDEBAND_MAX_TAPS || (taps & 1) == 0)
        return fail(SDRG_E_INVALID, "sideband: audio_decimation outside [1, 64] or taps not odd in [1, 511]");
    *tile = sideband_tile_outputs(audio_decimation, taps);
    return SDRG_OK;
}

int32_t sdrg_engine_set_sideband(sdrg_engine *e, const sdrg_sideband_config *cfg) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    SidebandStage &s = e->sb;
    if (cfg) {
        if (const char *bad = sideband_check(*cfg)) return fail(SDRG_E_INVALID, "sideband: %s", bad);
        const size_t T = (size_t)cfg->taps;
        std::vector<float> cr(T), ci(T), pairs(2 * T);  // the device's copy is the pairs (cr, ci)
        sideband_design(*cfg, cr.data(), ci.data());
        for (size_t k = 0; k < T; k++) pairs[2 * k] = cr[k], pairs[2 * k + 1] = ci[k];
        DeviceScope dscope(e->device);
        HIP_TRY(dscope.error());
        const int32_t rc = upload_floats(&s.d_taps, pairs, "sideband taps");
        if (rc) return rc;
        s.cr.swap(cr);
        s.ci.swap(ci);
        s.cfg = *cfg;
    }
    s.set = cfg != nullptr;
    s.cur.restart();
    return SDRG_OK;
}

int32_t sdrg_engine_get_sideband(const sdrg_engine *e, sdrg_sideband_config *cfg, float *cr, float *ci,
                                 uint64_t *samples_consumed) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    const SidebandStage &s = e->sb;
    if (!s.set) return fail(SDRG_E_INVALID, "no sideband configuration set");
    if (cfg) *cfg = s.cfg;
    if (cr) std::copy(s.cr.begin(), s.cr.end(), cr);
    if (ci) std::copy(s.ci.begin(), s.ci.end(), ci);
    if (samples_consumed) *samples_consumed = s.cur.g;
    return SDRG_OK;
}

int32_t sdrg_engine_sideband_reset(sdrg_engine *e) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    e->sb.cur.restart();
    return SDRG_OK;
}

int32_t sdrg_engine_sideband_max_out(const sdrg_engine *e, int32_t *cap) {
    if (!e || !cap) return fail(SDRG_E_INVALID, "null argument");
    if (int32_t rc = require_set(e->sb.set, "sideband")) return rc;
    *cap = e->sb.cap();
    return SDRG_OK;
}

static int32_t sb_resolve(const sdrg_engine *e, int32_t n, StageCall *c) {
    const SidebandStage &s = e->sb;
    if (int32_t rc = require_set(s.set, "sideband")) return rc;
    if (n < 0 || n > s.cfg.max_in) return fail(SDRG_E_INVALID, "sideband: n %d outside [0, max_in = %d]", n, s.cfg.max_in);
    c->n = n;
    c->in_stride = s.cfg.max_in;
    c->cap = s.cap();
    c->n_out = s.cur.n_out(n, s.cfg.audio_decimation);
    c->in_bytes = (size_t)e->n_streams * (size_t)c->in_stride * 2 * sizeof(float);
    c->out_bytes = (size_t)e->n_streams * (size_t)c->cap * (size_t)s.width() *
                   (s.cfg.out_format == SDRG_SIDEBAND_OUT_F32 ? sizeof(float) : sizeof(int16_t));
    return SDRG_OK;
}

static int32_t sb_reserve(sdrg_engine *e, const StageCall &) { return ensure_halves(&e->sb.hist, e->sb.half(e->n_streams)); }

// one sideband call on the main stream: chan (rows of in_stride complex samples), out in device memory
static int32_t sb_launch(sdrg_engine *e, const StageCall &c, const void *chan, void *out) {
    SidebandStage &s = e->sb;
    SidebandParams p{};
    fir_tile_fill(&p, s.cur, s.cfg.audio_decimation, s.cfg.taps, c, s.hist, s.half(e->n_streams));
    p.in_stride = c.in_stride;
    p.mode = s.cfg.mode;
    p.out_format = s.cfg.out_format;
    p.gain = s.cfg.gain;
    p.taps_dev = s.d_taps.p;
    HIP_TRY(launch_sideband(static_cast<const float *>(chan), e->n_streams, p, out, e->s_main));
    s.cur.advance(c.n);  // a call without samples wrote out only: the state stays where it is
    e->outputs_unmarked = true;
    return SDRG_OK;
}

static constexpr auto sb_stage = &stage_call<StageCall, sb_resolve, sb_reserve, sb_launch, int32_t>;

int32_t sdrg_engine_sideband_device(sdrg_engine *e, const void *chan, int32_t n, void *out, int32_t *n_out) {
    return sb_stage(e, "chan", chan, out, n_out, false, n);
}

int32_t sdrg_engine_sideband_host(sdrg_engine *e, const void *chan, int32_t n, void *out, int32_t *n_out) {
    return sb_stage(e, "chan", chan, out, n_out, true, n);
}

// ---- tone detector stage (tones.hip) -------------------------------------------------------------------------------

int32_t sdrg_tones_design(const sdrg_tones_config *cfg, float *table, float *wf, sdrg_tones_scalars *scalars) {
    if (!cfg) return fail(SDRG_E_INVALID, "null tones config");
    if (const char *bad = tones_check(*cfg)) return fail(SDRG_E_INVALID, "tones: %s", bad);
    tones_design(*cfg, table, wf, scalars);
    return SDRG_OK;
}

int32_t sdrg_tones_geometry(int32_t *sub_blocks_per_group) {
    if (!sub_blocks_per_group) return fail(SDRG_E_INVALID, "null sub_blocks_per_group");
    *sub_blocks_per_group = TONES_GROUP_SUBS;
    return SDRG_OK;
}

int32_t sdrg_engine_set_tones(sdrg_engine *e, const sdrg_tones_config *cfg) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    TonesStage &s = e->tones;
    if (cfg) {
        if (const char *bad = tones_check(*cfg)) return fail(SDRG_E_INVALID, "tones: %s", bad);
        const size_t S = (size_t)TONES_SUB * (size_t)cfg->sub_blocks, K = (size_t)cfg->n_tones;
        std::vector<float> des(K * S * 2 + S);
        sdrg_tones_scalars sc;
        tones_design(*cfg, des.data(), des.data() + K * S * 2, &sc);
        DeviceScope dscope(e->device);
        HIP_TRY(dscope.error());
        const int32_t rc = upload_floats(&s.d_design, des, "tones design");
        if (rc) return rc;
        s.cfg = *cfg;
        s.sc = sc;
    }
    s.set = cfg != nullptr;
    s.cur.restart();
    return SDRG_OK;
}

int32_t sdrg_engine_get_tones(const sdrg_engine *e, sdrg_tones_config *cfg, sdrg_tones_scalars *scalars,
                              uint64_t *samples_consumed) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    const TonesStage &s = e->tones;
    if (!s.set) return fail(SDRG_E_INVALID, "no tones configuration set");
    if (cfg) *cfg = s.cfg;
    if (scalars) *scalars = s.sc;
    if (samples_consumed) *samples_consumed = s.cur.g;
    return SDRG_OK;
}

int32_t sdrg_engine_tones_reset(sdrg_engine *e) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    e->tones.cur.restart();
    return SDRG_OK;
}

int32_t sdrg_engine_tones_max_blocks(const sdrg_engine *e, int32_t *cap_blocks) {
    if (!e || !cap_blocks) return fail(SDRG_E_INVALID, "null engine or cap_blocks");
    if (int32_t rc = require_set(e->tones.set, "tones")) return rc;
    *cap_blocks = e->tones.cap_blocks();
    return SDRG_OK;
}

// n_out is the blocks the call completes (*n_blocks); out is powers; aux, the records
static int32_t tones_resolve(const sdrg_engine *e, int32_t in_stride, int32_t n, sdrg_tones_record *records, StageCall *c) {
    const TonesStage &s = e->tones;
    if (int32_t rc = require_set(s.set, "tones")) return rc;
    if (n < 0 || n > s.cfg.max_in) return fail(SDRG_E_INVALID, "tones: n %d outside [0, max_in = %d]", n, s.cfg.max_in);
    if (in_stride < std::max(n, 1) || in_stride > s.cfg.max_in)
        return fail(SDRG_E_INVALID, "tones: in_stride %d outside [max(n, 1) = %d, max_in = %d]", in_stride, std::max(n, 1),
                    s.cfg.max_in);
    c->n = n;
    c->in_stride = in_stride;
    c->cap = s.cap_blocks();
    c->n_out = s.cur.blocks(n, s.S());
    c->in_bytes = (size_t)e->n_streams * (size_t)in_stride * (size_t)s.cfg.components * sizeof(float);
    c->out_bytes = (size_t)e->n_streams * (size_t)c->cap * (size_t)s.cfg.n_tones * sizeof(float);
    c->aux = records;
    c->aux_bytes = (size_t)e->n_streams * sizeof(*records);
    return SDRG_OK;
}

// the sub-blocks a call of n values completes at most: the rows per stream of the sums
static size_t tones_max_sub(int n) { return (size_t)(n + TONES_SUB - 1) / TONES_SUB; }

static int32_t tones_reserve(sdrg_engine *e, const StageCall &c) {
    TonesStage &s = e->tones;
    const int32_t rc = ensure_halves(&s.state, s.half(e->n_streams));
    const size_t sums = (size_t)e->n_streams * tones_max_sub(c.n) * (size_t)(2 * s.cfg.n_tones + 1);
    return rc ? rc : ensure_device(&s.sums, std::max<size_t>(sums, 1));
}

// One call on the main stream: in (rows of in_stride values) and powers, and c.aux, the records or null, in device memory
static int32_t tones_launch(sdrg_engine *e, const StageCall &c, const void *in, void *powers) {
    TonesStage &s = e->tones;
    const size_t half = s.half(e->n_streams), K = (size_t)s.cfg.n_tones, S = (size_t)s.S();
    TonesParams p{};
    p.n = c.n;
    p.in_stride = c.in_stride;
    p.components = s.cfg.components;
    p.n_tones = s.cfg.n_tones;
    p.sub_blocks = s.cfg.sub_blocks;
    p.soff = s.cur.offset(TONES_SUB);
    p.sub0 = s.cur.offset(s.S()) / TONES_SUB;
    p.n_sub = (p.soff + c.n) / TONES_SUB;
    p.n_blocks = c.n_out;
    p.cap_blocks = c.cap;
    p.max_sub = (int)tones_max_sub(c.n);
    p.fresh = s.cur.fresh ? 1 : 0;
    p.confirm = s.cfg.confirm_blocks;
    p.release = s.cfg.release_blocks;
    p.pnorm = s.sc.pnorm, p.enorm = s.sc.enorm, p.min_power = s.sc.min_power, p.dom = s.sc.dom, p.share_thr = s.sc.share_thr;
    p.table = s.d_design.p;
    p.wf = s.d_design.p + K * S * 2;
    p.state_old = s.state.half(s.cur.old_half(), half);  // not read by a fresh call: p.fresh says so
    p.state_new = s.state.next(s.cur, half);
    p.sums = s.sums.p;
    p.records = static_cast<sdrg_tones_record *>(c.aux);
    HIP_TRY(launch_tones(in, e->n_streams, p, static_cast<float *>(powers), e->s_main));
    s.cur.advance(c.n);  // a call without values wrote powers and the records only: the state stays where it is
    e->outputs_unmarked = true;
    return SDRG_OK;
}

static constexpr auto tones_stage =
    &stage_call<StageCall, tones_resolve, tones_reserve, tones_launch, int32_t, int32_t, sdrg_tones_record *>;

int32_t sdrg_engine_tones_device(sdrg_engine *e, const void *in, int32_t in_stride, int32_t n, void *powers,
                                 sdrg_tones_record *records, int32_t *n_blocks) {
    return tones_stage(e, "in", in, powers, n_blocks, false, in_stride, n, records);
}

int32_t sdrg_engine_tones_host(sdrg_engine *e, const void *in, int32_t in_stride, int32_t n, void *powers,
                               sdrg_tones_record *records, int32_t *n_blocks) {
    return tones_stage(e, "in", in, powers, n_blocks, true, in_stride, n, records);
}

// ---- symbol stage (symbols.hip) ------------------------------------------------------------------------------------

int32_t sdrg_symbols_design(const sdrg_symbols_config *cfg, sdrg_symbols_design_values *design, float *table) {
    if (!cfg || !design) return fail(SDRG_E_INVALID, "null symbols config or design");
    if (const char *bad = symbols_check(*cfg)) return fail(SDRG_E_INVALID, "symbols: %s", bad);
    *design = symbols_design(*cfg, table);
    return SDRG_OK;
}

int32_t sdrg_symbols_geometry(int32_t block, int32_t *tile, int32_t *pass_tile) {
    if (block < SDRG_SYM_MIN_BLOCK || block > BLOCK_MAX || (block & (block - 1)) != 0)
        return fail(SDRG_E_INVALID, "symbols: block must be a power of two in [64, 1024]");
    if (tile) *tile = block_tile(block);
    if (pass_tile) *pass_tile = SYM_PASS_TILE;
    return SDRG_OK;
}

int64_t sdrg_symbols_count(uint32_t inc, uint64_t g, uint64_t n) {
    if (inc < (1u << 26) || inc > (1u << 31)) return -1;
    return (int64_t)symbols_count(inc, g, n);
}

int32_t sdrg_engine_set_symbols(sdrg_engine *e, const sdrg_symbols_config *cfg) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    SymbolsStage &s = e->sym;
    if (cfg) {
        if (const char *bad = symbols_check(*cfg)) return fail(SDRG_E_INVALID, "symbols: %s", bad);
        std::vector<float> tab((size_t)SDRG_SYM_TABLE * 2);
        const sdrg_symbols_design_values des = symbols_design(*cfg, tab.data());
        DeviceScope dscope(e->device);
        HIP_TRY(dscope.error());
        const int32_t rc = upload_floats(&s.d_tab, tab, "symbols table");
        if (rc) return rc;
        s.cfg = *cfg;
        s.des = des;
    }
    s.set = cfg != nullptr;
    s.cur.restart();
    return SDRG_OK;
}

int32_t sdrg_engine_get_symbols(const sdrg_engine *e, sdrg_symbols_config *cfg, sdrg_symbols_design_values *design,
                                uint64_t *samples_consumed) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    const SymbolsStage &s = e->sym;
    if (!s.set) return fail(SDRG_E_INVALID, "no symbols configuration set");
    if (cfg) *cfg = s.cfg;
    if (design) *design = s.des;
    if (samples_consumed) *samples_consumed = s.cur.g;
    return SDRG_OK;
}

int32_t sdrg_engine_symbols_reset(sdrg_engine *e) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    e->sym.cur.restart();
    return SDRG_OK;
}

int32_t sdrg_engine_symbols_max_out(const sdrg_engine *e, int32_t *cap) {
    if (!e || !cap) return fail(SDRG_E_INVALID, "null engine or cap");
    if (int32_t rc = require_set(e->sym.set, "symbols")) return rc;
    *cap = e->sym.cap();
    return SDRG_OK;
}

// n_out is the symbols the call writes (*n_sym); out is symbols; aux, the records.  n_blocks: the blocks it completes.
struct SymbolsCall : StageCall {
    int n_blocks = 0;
};

static int32_t sym_resolve(const sdrg_engine *e, int32_t in_stride, int32_t n, sdrg_symbols_record *records,
                           SymbolsCall *c) {
    const SymbolsStage &s = e->sym;
    if (int32_t rc = require_set(s.set, "symbols")) return rc;
    if (n < 0 || n > s.cfg.max_in) return fail(SDRG_E_INVALID, "symbols: n %d outside [0, max_in = %d]", n, s.cfg.max_in);
    if (in_stride < std::max(n, 1) || in_stride > s.cfg.max_in)
        return fail(SDRG_E_INVALID, "symbols: in_stride %d outside [max(n, 1) = %d, max_in = %d]", in_stride,
                    std::max(n, 1), s.cfg.max_in);
    c->n = n;
    c->in_stride = in_stride;
    c->cap = s.cap();
    c->n_out = (int)symbols_count(s.des.inc, s.cur.g, (uint64_t)n);
    c->n_blocks = s.cur.blocks(n, s.cfg.block);
    c->in_bytes = (size_t)e->n_streams * (size_t)in_stride * sizeof(float);
    c->out_bytes = (size_t)e->n_streams * (size_t)c->cap * s.width();
    c->aux = records;
    c->aux_bytes = (size_t)e->n_streams * sizeof(*records);
    return SDRG_OK;
}

static int32_t sym_reserve(sdrg_engine *e, const SymbolsCall &) {
    SymbolsStage &s = e->sym;
    const int32_t rc = ensure_halves(&s.state, s.half(e->n_streams));
    return rc ? rc : ensure_device(&s.blk, (size_t)e->n_streams * (s.blocks() * 5 + (s.blocks() + 1) * 4));
}

// One call on the main stream: in (rows of in_stride floats) and symbols, and c.aux, the records or null, in device memory
static int32_t sym_launch(sdrg_engine *e, const SymbolsCall &c, const void *in, void *symbols) {
    SymbolsStage &s = e->sym;
    const size_t half = s.half(e->n_streams);
    const sdrg_symbols_design_values &d = s.des;
    const uint64_t g = s.cur.g;
    SymParams p{};
    p.n = c.n;
    p.in_stride = c.in_stride;
    p.block = s.cfg.block;
    p.off = s.cur.offset(s.cfg.block);
    p.n_blocks = c.n_blocks;
    p.fresh = s.cur.fresh ? 1 : 0;
    p.levels = s.cfg.levels;
    p.track = s.cfg.level_mode == SDRG_SYM_LEVEL_TRACK ? 1 : 0;
    p.soft = s.soft() ? 1 : 0;
    p.n_sym = c.n_out;
    p.cap = c.cap;
    p.inc = d.inc;
    p.c0 = (uint32_t)((uint64_t)d.inc * (g & 0xffffffffull));  // inc g mod 2^32
    p.cpos0 = p.c0 - d.inc * (uint32_t)p.off;
    p.tau0 = (uint32_t)(uint64_t)(2147483648ll + d.trim);
    p.emit0 = (uint64_t)p.c0 + ((g >= 1 && p.c0 < d.inc) ? 0x100000000ull : 0ull);
    p.trim = d.trim;
    p.rinc = d.rinc, p.beta = d.beta, p.beta_level = d.beta_level, p.floor_thr = d.floor_thr, p.lock_thr = d.lock_thr;
    p.K = d.K, p.rs = d.rs, p.level_scale = d.scale, p.fixed_centre = d.centre, p.fixed_thr = d.threshold;
    p.tab = s.d_tab.p;
    p.state_old = s.state.half(s.cur.old_half(), half);  // not read by a fresh call: p.fresh says so
    p.state_new = s.state.next(s.cur, half);
    p.mom = s.blk.p;
    p.blk = reinterpret_cast<uint32_t *>(s.blk.p + (size_t)e->n_streams * s.blocks() * 5);
    p.records = static_cast<sdrg_symbols_record *>(c.aux);
    HIP_TRY(launch_symbols(static_cast<const float *>(in), e->n_streams, p, symbols, e->s_main));
    s.cur.advance(c.n);  // a call without values wrote symbols and the records only: the state stays where it is
    e->outputs_unmarked = true;
    return SDRG_OK;
}

static constexpr auto sym_stage =
    &stage_call<SymbolsCall, sym_resolve, sym_reserve, sym_launch, int32_t, int32_t, sdrg_symbols_record *>;

int32_t sdrg_engine_symbols_device(sdrg_engine *e, const void *in, int32_t in_stride, int32_t n, void *symbols,
                                   sdrg_symbols_record *records, int32_t *n_sym) {
    return sym_stage(e, "in", in, symbols, n_sym, false, in_stride, n, records);
}

int32_t sdrg_engine_symbols_host(sdrg_engine *e, const void *in, int32_t in_stride, int32_t n, void *symbols,
                                 sdrg_symbols_record *records, int32_t *n_sym) {
    return sym_stage(e, "in", in, symbols, n_sym, true, in_stride, n, records);
}

// ---- the chains: DDC (-> AFC) (-> squelch) (-> AGC) -> demodulator or sideband (-> resampler), host memory in and out

// The stage that turns the channel into audio.  What a chain asks of it, whichever it is: whether it is set, its
// max_in and cap, whether it writes floats, how many components an output has, and its three steps.
enum class Detector { Demod, Sideband };

struct DetectorView {
    const char *name;      // for require_set and the messages
    const char *f32_name;  // the out_format the resampler needs, as the header spells it
    bool set, f32;
    int max_in, cap, components;
    int32_t (*resolve)(const sdrg_engine *, int32_t n, StageCall *);
    int32_t (*reserve)(sdrg_engine *, const StageCall &);
    int32_t (*launch)(sdrg_engine *, const StageCall &, const void *chan, void *out);
};

static DetectorView detector_view(const sdrg_engine *e, Detector det) {
    if (det == Detector::Sideband)
        return {"sideband", "SDRG_SIDEBAND_OUT_F32", e->sb.set, e->sb.cfg.out_format == SDRG_SIDEBAND_OUT_F32,
                e->sb.cfg.max_in, e->sb.set ? e->sb.cap() : 0, e->sb.width(), sb_resolve, sb_reserve, sb_launch};
    return {"demod", "SDRG_DEMOD_OUT_F32", e->demod.set, e->demod.cfg.out_format == SDRG_DEMOD_OUT_F32,
            e->demod.cfg.max_in, e->demod.set ? e->demod.cap() : 0, 1, demod_resolve, demod_reserve, demod_launch};
}

// sdrg_engine_listen_host, and the four chain calls that are its masks without the AGC; with the sideband stage as the
// detector, sdrg_engine_listen_sideband_host.
// Every refusal comes first, in the order the header lists them; then every stage's reserve and the buffers between
// the stages; then the copy in, the launches, the copy out and the wait.  No x_launch is reachable before every
// x_reserve of the call has returned SDRG_OK, so a call that fails for want of memory has advanced no stage's cursor:
// "commits nothing in any stage" (include/sdrg.h) holds for SDRG_E_NOMEM as for the refusals.
// The squelch, then the AGC, work in place on the channel between the DDC and the demodulator, and their records
// (unless null) come back with the audio, staged behind it in stream_out.  With `tap` (listen_tones_host) the tone stage
// reads the detector's float rows where they lie on the device, ahead of the resampler, and its powers and records are
// staged behind the other records.
struct ToneTap {
    float *powers;
    sdrg_tones_record *records;
    int32_t *n_blocks;
};

// With `afc` (listen_afc_host) the AFC runs first on that channel, in place, and its records are staged behind the
// squelch's and the AGC's.
struct AfcStep {
    sdrg_afc_record *records;
};

// With `sym` (listen_symbols_host) the symbol stage reads the demodulator's float rows where the tone stage would, and
// its symbols and records are staged behind the squelch's and the AGC's records; `out` may then be null: the audio is
// not copied back.
struct SymbolTap {
    void *symbols;
    sdrg_symbols_record *records;
    int32_t *n_sym;
};

static int32_t chain_host(sdrg_engine *e, Detector det, int32_t steps, const void *iq, int32_t fmt, void *out,
                          int32_t *n_out, sdrg_squelch_record *sq_records = nullptr,
                          sdrg_agc_record *agc_records = nullptr, const ToneTap *tap = nullptr,
                          const AfcStep *afc = nullptr, const SymbolTap *sym = nullptr) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    if (!iq || (!out && !sym) || !n_out) return fail(SDRG_E_INVALID, "null iq, out or n_out");
    if (sym && (!sym->symbols || !sym->n_sym)) return fail(SDRG_E_INVALID, "null symbols or n_sym");
    if (tap && (!tap->powers || !tap->n_blocks)) return fail(SDRG_E_INVALID, "null powers or n_blocks");
    if (steps & ~(SDRG_LISTEN_SQUELCH | SDRG_LISTEN_AGC | SDRG_LISTEN_RESAMPLE))
        return fail(SDRG_E_INVALID, "listen: unknown bits in steps 0x%x", (unsigned)steps);
    const bool squelch = steps & SDRG_LISTEN_SQUELCH, agc = steps & SDRG_LISTEN_AGC, resample = steps & SDRG_LISTEN_RESAMPLE;
    const DetectorView v = detector_view(e, det);
    int32_t rc = require_set(v.set, v.name);
    if (!rc && resample) rc = require_set(e->rs.set, "resample");
    if (!rc && squelch) rc = require_set(e->sq.set, "squelch");
    if (!rc && agc) rc = require_set(e->agc.set, "agc");
    if (!rc && tap) rc = require_set(e->tones.set, "tones");
    if (!rc && afc) rc = require_set(e->afc.set, "afc");
    if (!rc && afc && !e->afc.track())
        rc = fail(SDRG_E_INVALID, "the chain corrects the channel: afc mode must be SDRG_AFC_TRACK");
    if (!rc && sym) rc = require_set(e->sym.set, "symbols");
    DdcCall d;
    // the squelch's, the AGC's, the detector's, the resampler's, the tone stage's and the AFC's
    StageCall q, g, a, r, t, f;
    SymbolsCall y;  // the symbol stage's
    if (!rc) rc = ddc_resolve(e, fmt, &d);
    if (rc) return rc;
    // the checks between the stages come before the later stages' own: after them those cannot refuse their n
    if (v.max_in < d.cap)
        return fail(SDRG_E_INVALID, "%s max_in %d smaller than the ddc's row length %d", v.name, v.max_in, d.cap);
    if (squelch && e->sq.cfg.max_in < d.cap)
        return fail(SDRG_E_INVALID, "squelch max_in %d smaller than the ddc's row length %d", e->sq.cfg.max_in, d.cap);
    if (agc && e->agc.cfg.max_in < d.cap)
        return fail(SDRG_E_INVALID, "agc max_in %d smaller than the ddc's row length %d", e->agc.cfg.max_in, d.cap);
    if (afc && e->afc.cfg.max_in < d.cap)
        return fail(SDRG_E_INVALID, "afc max_in %d smaller than the ddc's row length %d", e->afc.cfg.max_in, d.cap);
    if (resample) {
        if (!v.f32)
            return fail(SDRG_E_INVALID, "the resampler reads float audio: %s out_format must be %s", v.name, v.f32_name);
        if (e->rs.cfg.components != v.components)
            return fail(SDRG_E_INVALID, "the resampler reads %s: resample components must be %d",
                        v.components == 1 ? "real audio" : "both sidebands", v.components);
        if (e->rs.cfg.max_in < v.cap)
            return fail(SDRG_E_INVALID, "resample max_in %d smaller than the %s's row length %d", e->rs.cfg.max_in, v.name,
                        v.cap);
    }
    if (tap) {
        if (e->tones.cfg.components != 1)
            return fail(SDRG_E_INVALID, "the tone stage reads real audio here: tones components must be 1");
        if (!v.f32)
            return fail(SDRG_E_INVALID, "the tone stage reads float audio: %s out_format must be %s", v.name, v.f32_name);
        if (v.components != 1) return fail(SDRG_E_INVALID, "the tone stage reads one value per output of the %s", v.name);
        if (e->tones.cfg.max_in < v.cap)
            return fail(SDRG_E_INVALID, "tones max_in %d smaller than the %s's row length %d", e->tones.cfg.max_in, v.name,
                        v.cap);
    }
    if (sym) {
        if (!v.f32 || v.components != 1)
            return fail(SDRG_E_INVALID, "the symbol stage reads real float audio: %s out_format must be %s", v.name,
                        v.f32_name);
        if (e->sym.cfg.max_in < v.cap)
            return fail(SDRG_E_INVALID, "symbols max_in %d smaller than the %s's row length %d", e->sym.cfg.max_in, v.name,
                        v.cap);
    }
    rc = v.resolve(e, d.n_out, &a);
    a.in_stride = d.cap;  // the channel's rows are the DDC's
    if (!rc && sym) rc = sym_resolve(e, a.cap, a.n_out, sym->records, &y);
    if (!rc && tap) rc = tones_resolve(e, a.cap, a.n_out, tap->records, &t);
    if (!rc && resample) rc = rs_resolve(e, a.cap, a.n_out, &r);
    if (!rc && squelch) rc = sq_resolve(e, d.cap, d.n_out, sq_records, &q);
    if (!rc && agc) rc = agc_resolve(e, d.cap, d.n_out, agc_records, &g);
    if (!rc && afc) rc = afc_resolve(e, d.cap, d.n_out, afc->records, &f);
    if (rc) return rc;
    const StageCall &last = resample ? r : a;
    // a stage that is not in the mask was not resolved: its aux is null, and nothing is staged or copied for it
    HostAux aux(last.out_bytes, &q, &g);
    void *powers = tap ? tap->powers : nullptr;  // the caller's, then where the launch writes them
    if (tap) aux.add(&powers, t.out_bytes);
    if (tap) aux.add(&t.aux, t.aux_bytes);
    if (afc) aux.add(&f.aux, f.aux_bytes);
    void *symbols = sym ? sym->symbols : nullptr;  // the caller's, then where the launch writes them
    if (sym) aux.add(&symbols, y.out_bytes);
    if (sym) aux.add(&y.aux, y.aux_bytes);
    DeviceScope dscope(e->device);
    HIP_TRY(dscope.error());
    rc = ddc_reserve(e, d);
    if (!rc && sym) rc = sym_reserve(e, y);
    if (!rc && tap) rc = tones_reserve(e, t);
    if (!rc && afc) rc = afc_reserve(e, f);
    if (!rc && squelch) rc = sq_reserve(e, q);
    if (!rc && agc) rc = agc_reserve(e, g);
    if (!rc) rc = v.reserve(e, a);
    if (!rc && resample) rc = rs_reserve(e, r);
    if (!rc) rc = ensure_device(&e->chain_chan, d.out_bytes / sizeof(float));
    if (!rc && resample) rc = ensure_device(&e->chain_audio, a.out_bytes / sizeof(float));
    if (!rc) rc = host_begin(e, iq, d.in_bytes, aux.staged_bytes());
    if (!rc) aux.stage(e);
    if (!rc) rc = ddc_launch(e, d, e->stream_in.p, e->chain_chan.p);
    if (!rc && afc) rc = afc_launch(e, f, e->chain_chan.p, e->chain_chan.p);
    if (!rc && squelch) rc = sq_launch(e, q, e->chain_chan.p, e->chain_chan.p);
    if (!rc && agc) rc = agc_launch(e, g, e->chain_chan.p, e->chain_chan.p);
    void *audio = resample ? (void *)e->chain_audio.p : (void *)e->stream_out.p;
    if (!rc) rc = v.launch(e, a, e->chain_chan.p, audio);
    if (!rc && tap) rc = tones_launch(e, t, audio, powers);
    if (!rc && sym) rc = sym_launch(e, y, audio, symbols);
    if (!rc && resample) rc = rs_launch(e, r, e->chain_audio.p, e->stream_out.p);
    if (!rc) rc = aux.finish(e, out, out ? last.out_bytes : 0);  // a null out (listen_symbols_host): no rows back
    if (rc) return rc;
    *n_out = last.n_out;
    if (tap) *tap->n_blocks = t.n_out;
    if (sym) *sym->n_sym = y.n_out;
    return SDRG_OK;
}

int32_t sdrg_engine_listen_host(sdrg_engine *e, int32_t steps, const void *iq, int32_t fmt, void *out, int32_t *n_out,
                                sdrg_squelch_record *squelch_records, sdrg_agc_record *agc_records) {
    return chain_host(e, Detector::Demod, steps, iq, fmt, out, n_out, squelch_records, agc_records);
}

int32_t sdrg_engine_listen_afc_host(sdrg_engine *e, int32_t steps, const void *iq, int32_t fmt, void *out, int32_t *n_out,
                                    sdrg_squelch_record *squelch_records, sdrg_agc_record *agc_records,
                                    sdrg_afc_record *afc_records) {
    const AfcStep afc{afc_records};
    return chain_host(e, Detector::Demod, steps, iq, fmt, out, n_out, squelch_records, agc_records, nullptr, &afc);
}

int32_t sdrg_engine_listen_tones_host(sdrg_engine *e, int32_t steps, const void *iq, int32_t fmt, void *out, int32_t *n_out,
                                      sdrg_squelch_record *squelch_records, sdrg_agc_record *agc_records, float *powers,
                                      sdrg_tones_record *tone_records, int32_t *n_blocks) {
    const ToneTap tap{powers, tone_records, n_blocks};
    return chain_host(e, Detector::Demod, steps, iq, fmt, out, n_out, squelch_records, agc_records, &tap);
}

int32_t sdrg_engine_listen_symbols_host(sdrg_engine *e, int32_t steps, const void *iq, int32_t fmt, void *out,
                                        int32_t *n_out, sdrg_squelch_record *squelch_records,
                                        sdrg_agc_record *agc_records, void *symbols, sdrg_symbols_record *symbol_records,
                                        int32_t *n_sym) {
    const SymbolTap sym{symbols, symbol_records, n_sym};
    return chain_host(e, Detector::Demod, steps, iq, fmt, out, n_out, squelch_records, agc_records, nullptr, nullptr, &sym);
}

int32_t sdrg_engine_ddc_demod_host(sdrg_engine *e, const void *iq, int32_t fmt, void *out, int32_t *n_out) {
    return chain_host(e, Detector::Demod, 0, iq, fmt, out, n_out);
}

int32_t sdrg_engine_ddc_demod_resample_host(sdrg_engine *e, const void *iq, int32_t fmt, void *out, int32_t *n_out) {
    return chain_host(e, Detector::Demod, SDRG_LISTEN_RESAMPLE, iq, fmt, out, n_out);
}

int32_t sdrg_engine_ddc_squelch_demod_host(sdrg_engine *e, const void *iq, int32_t fmt, void *out, int32_t *n_out,
                                           sdrg_squelch_record *records) {
    return chain_host(e, Detector::Demod, SDRG_LISTEN_SQUELCH, iq, fmt, out, n_out, records);
}

int32_t sdrg_engine_ddc_squelch_demod_resample_host(sdrg_engine *e, const void *iq, int32_t fmt, void *out,
                                                    int32_t *n_out, sdrg_squelch_record *records) {
    return chain_host(e, Detector::Demod, SDRG_LISTEN_SQUELCH | SDRG_LISTEN_RESAMPLE, iq, fmt, out, n_out, records);
}

int32_t sdrg_engine_listen_sideband_host(sdrg_engine *e, int32_t steps, const void *iq, int32_t fmt, void *out,
                                         int32_t *n_out, sdrg_squelch_record *squelch_records,
                                         sdrg_agc_record *agc_records) {
    return chain_host(e, Detector::Sideband, steps, iq, fmt, out, n_out, squelch_records, agc_records);
}

int32_t sdrg_engine_set_callbacks(sdrg_engine *e, const sdrg_callbacks *cbs) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    if (cbs) {
        e->cbs = *cbs;
        e->has_cbs = true;
    } else {
        e->cbs = sdrg_callbacks{};
        e->has_cbs = false;
    }
    return SDRG_OK;
}

int32_t sdrg_engine_set_profiling(sdrg_engine *e, int32_t enabled) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    DeviceScope dscope(e->device);
    HIP_TRY(dscope.error());
    if (enabled)
        if (int32_t rc = e->prof.create()) return rc;
    // calls made while profiling was off break the chain of SSB end markers (their seqs are not profiled), so the first
    // profiled call after re-enabling takes a start marker of its own (Profiler::begin's `chained`)
    e->prof.on = enabled != 0;
    return SDRG_OK;
}

int32_t sdrg_engine_get_timings(const sdrg_engine *ce, sdrg_timings *out) {
    if (!ce || !out) return fail(SDRG_E_INVALID, "null argument");
    Profiler &p = const_cast<sdrg_engine *>(ce)->prof;
    if (p.last < 0) return fail(SDRG_E_INVALID, "no profiled call yet");
    if (int32_t rc = p.fold_slot(p.last)) return rc;
    *out = p.last_timings;
    return SDRG_OK;
}

int32_t sdrg_engine_get_timing_stats(const sdrg_engine *ce, sdrg_timings *mean, int32_t *count) {
    if (!ce || !mean) return fail(SDRG_E_INVALID, "null argument");
    Profiler &p = const_cast<sdrg_engine *>(ce)->prof;
    if (int32_t rc = p.fold_all()) return rc;
    const double k = p.n_acc > 0 ? 1.0 / p.n_acc : 0.0;
    mean->spectrum_ms = (float)(p.sum_spec * k);
    mean->stats_ms = (float)(p.sum_stats * k);
    mean->ssb_ms = (float)(p.n_ssb > 0 ? p.sum_ssb / p.n_ssb : 0.0);
    mean->total_ms = (float)(p.sum_total * k);
    if (count) *count = p.n_acc;
    return SDRG_OK;
}

// Multi-GPU gather (include/sdrg.h; dist.cpp holds RCCL).  A gather runs on the stream that produced what it reads, in
// order behind it and with no cross-stream wait: the statistics stream when the last call ran its statistics there
// (records, and the spectra its statistics already waited for), else the main stream; with PCM, the audio detector's
// stream, which follows the SSB stream's end marker, waiting for the main or statistics stream's last marker.  (On a
// stream of its own the gather's waits shared a hardware queue with the engine's streams: HIP maps a process's streams
// onto GPU_MAX_HW_QUEUES queues, and a wait blocks the whole queue.)  A later call that writes a buffer a gather reads
// waits for that gather's event first (enqueue).
int32_t sdrg_engine_gather(sdrg_engine *e, sdrg_dist *d, int32_t root, const sdrg_gather_buffers *b) {
    if (!e || !d || !b) return fail(SDRG_E_INVALID, "null argument");
    if (dist_device(d) != e->device)
        return fail(SDRG_E_INVALID, "communicator on device %d, engine on device %d", dist_device(d), e->device);
    if (root < 0 || root >= dist_world(d)) return fail(SDRG_E_INVALID, "root %d outside [0, %d)", root, dist_world(d));
    DeviceScope dscope(e->device);
    HIP_TRY(dscope.error());
    const bool at_root = dist_rank(d) == root;
    const size_t B = (size_t)e->n_streams;
    const int n = e->cfg.samples_per_reading;
    const int plen = ssb_pcm_len(ssb_frozen_or(e), (uint32_t)e->cfg.sample_rate, e->fir_taps);
    const bool g_rec = b->records, g_foc = b->focus_spectra, g_spec = b->spectra, g_pcm = b->pcm && plen > 0;
    if ((g_rec && at_root && !b->records_out) || (g_foc && at_root && !b->focus_out) ||
        (g_spec && at_root && !b->spectra_out) || (g_pcm && at_root && !b->pcm_out))
        return fail(SDRG_E_INVALID, "null output buffer on the root");
    StatsGeometry geo{};
    if (g_foc) {
        geo = stats_geometry(e->fft_fs, e->fft_fc, n, e->fft_focus);
        if (geo.focus_len <= 0) return fail(SDRG_E_INVALID, "the focus window is empty (focus wider than the band)");
        int32_t rc = ensure_device(&e->d_focus_stage, B * (size_t)geo.focus_len);
        if (rc) return rc;
    }
    if (!(g_rec || g_foc || g_spec || g_pcm)) return SDRG_OK;
    const bool on_stats = !g_pcm && e->last_async_stats && !e->s_gather;
    hipStream_t s = e->s_gather ? e->s_gather : g_pcm ? e->s_ap : on_stats ? e->s_stats : e->s_main;
    if (e->s_gather || g_pcm) {  // on the lab's stream or the detector's: waits for every producer
        if ((g_rec || g_foc || g_spec) && e->last_in_main) HIP_TRY(hipStreamWaitEvent(s, e->last_in_main, 0));
        if (g_rec && e->sa.last_end) HIP_TRY(hipStreamWaitEvent(s, e->sa.last_end, 0));  // any async records
        if (g_pcm && e->last_in_ssb) HIP_TRY(hipStreamWaitEvent(s, e->last_in_ssb, 0));
    }
    // records an earlier call's asynchronous statistics wrote (the last call ran no statistics there)
    if (!e->s_gather && !g_pcm && !on_stats && g_rec && e->sa.last_end)
        HIP_TRY(hipStreamWaitEvent(s, e->sa.last_end, 0));
    if (int32_t rc = e->gathers.begin(s)) return rc;
    GatherItem items[4];
    int k = 0;
    if (g_rec) items[k++] = {b->records, b->records_out, B * sizeof(sdrg_frame_record)};
    if (g_foc) {
        HIP_TRY(launch_focus_pack(b->focus_spectra, (int)B, n, geo.focus_lo, geo.focus_len, e->d_focus_stage.p, s));
        items[k++] = {e->d_focus_stage.p, b->focus_out, B * (size_t)geo.focus_len * sizeof(float)};
    }
    if (g_spec) items[k++] = {b->spectra, b->spectra_out, B * (size_t)n * sizeof(float)};
    if (g_pcm) items[k++] = {b->pcm, b->pcm_out, B * (size_t)plen * sizeof(int16_t)};
    int32_t rc = dist_gather(d, items, k, root, s);
    if (rc) return rc;
    return e->gathers.end(s, {{g_rec ? (const void *)b->records : nullptr, B * sizeof(sdrg_frame_record)},
                               {g_foc ? (const void *)b->focus_spectra : nullptr, B * (size_t)n * sizeof(float)},
                               {g_spec ? (const void *)b->spectra : nullptr, B * (size_t)n * sizeof(float)},
                               {g_pcm ? (const void *)b->pcm : nullptr, B * (size_t)plen * sizeof(int16_t)}});
}

int32_t sdrg_engine_gather_records(sdrg_engine *e, sdrg_dist *d, int32_t root, const sdrg_frame_record *records,
                                   sdrg_frame_record *records_out) {
    if (!records) return fail(SDRG_E_INVALID, "null records");
    sdrg_gather_buffers b{};
    b.records = records;
    b.records_out = records_out;
    return sdrg_engine_gather(e, d, root, &b);
}

int32_t sdrg_engine_gather_focus(sdrg_engine *e, sdrg_dist *d, int32_t root, const float *spectra, float *focus_out) {
    if (!spectra) return fail(SDRG_E_INVALID, "null spectra");
    sdrg_gather_buffers b{};
    b.focus_spectra = spectra;
    b.focus_out = focus_out;
    return sdrg_engine_gather(e, d, root, &b);
}

int32_t sdrg_engine_gather_spectra(sdrg_engine *e, sdrg_dist *d, int32_t root, const float *spectra,
                                   float *spectra_out) {
    if (!spectra) return fail(SDRG_E_INVALID, "null spectra");
    sdrg_gather_buffers b{};
    b.spectra = spectra;
    b.spectra_out = spectra_out;
    return sdrg_engine_gather(e, d, root, &b);
}

int32_t sdrg_engine_gather_pcm(sdrg_engine *e, sdrg_dist *d, int32_t root, const int16_t *pcm, int16_t *pcm_out) {
    if (!pcm) return fail(SDRG_E_INVALID, "null pcm");
    sdrg_gather_buffers b{};
    b.pcm = pcm;
    b.pcm_out = pcm_out;
    return sdrg_engine_gather(e, d, root, &b);
}

int32_t sdrg_engine_reset_timing_stats(sdrg_engine *e) {
    if (!e) return fail(SDRG_E_INVALID, "null engine");
    if (int32_t rc = e->prof.fold_all()) return rc;
    e->prof.reset(e->calls_total);
    return SDRG_OK;
}

}  // extern "C"
