// sdrg_internal.h — kernel launchers shared by the engine (host C++) and the HIP translation units.
// Not part of the public ABI (include/sdrg.h is).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sdrg_types.h"

#include <stdlib.h>

// Lab knobs (tools/: role maps, priorities, CU splits, stamps ...) are read from the environment only in lab
// builds (-DSDRG_LAB=1, tools/build_variant.sh); the product library (make) ignores them, so a stray variable in
// a deployed process cannot change its results or its schedule.
#ifndef SDRG_LAB
#define SDRG_LAB 0
#endif
static inline const char *lab_getenv(const char *name) { return SDRG_LAB ? getenv(name) : nullptr; }

namespace sdrg {

// Raise a kernel's dynamic-LDS limit to `bytes` on the CURRENT device, once per (kernel, device): the
// attribute is per device, and engines on several devices or threads may launch the same kernel
// concurrently (engine.cpp; mutex-protected).
hipError_t ensure_dynamic_lds(const void *kernel, int bytes);

// Makes `device` current for the scope of an entry point and restores the caller's current device on
// exit, so the C ABI never leaves the calling thread on another device (engine.cpp, pulse_bank.cpp).
class DeviceScope {
public:
    explicit DeviceScope(int device) {
        if (hipGetDevice(&prev_) != hipSuccess) prev_ = -1;
        err_ = (prev_ == device) ? hipSuccess : hipSetDevice(device);
        changed_ = err_ == hipSuccess && prev_ != device;
    }
    ~DeviceScope() {
        if (changed_ && prev_ >= 0) (void)hipSetDevice(prev_);
    }
    DeviceScope(const DeviceScope &) = delete;
    DeviceScope &operator=(const DeviceScope &) = delete;
    hipError_t error() const { return err_; }

private:
    int prev_ = -1;
    bool changed_ = false;
    hipError_t err_ = hipSuccess;
};

// ------------------------------------------------------------------------------------------------
// Launchers (defined in the .hip translation units).  All are asynchronous on `stream`.
// ------------------------------------------------------------------------------------------------
// Spectrum kernels, every N in [1, 2^20]: powers of two 64 .. 16384 one LDS-resident workgroup per frame,
// 32768/65536 two-kernel four-step in waves of spectrum_wave_frames(n) frames, 128 MiB of complex intermediate
// (`scratch`, spectrum_scratch_floats() floats) that stays in the 256 MiB Infinity Cache (measured at 65536:
// 64 / 128 / 256 / 512 frames per wave 0.418 / 0.356 / 0.318 / 0.393 ms per 1024 frames); every other N through
// fftany.hip (mixed radix, four-step, Bluestein).
#ifndef SDRG_SPECTRUM_WAVE_FRAMES  // lab override of the 65536-point wave (tools/build_variant.sh); 0: 128 MiB
#define SDRG_SPECTRUM_WAVE_FRAMES 0
#endif
constexpr size_t SPECTRUM_WAVE_BYTES = (size_t)128 << 20;
inline int spectrum_wave_frames(int n) {
    if (SDRG_SPECTRUM_WAVE_FRAMES > 0) return SDRG_SPECTRUM_WAVE_FRAMES * (65536 / n);
    return (int)(SPECTRUM_WAVE_BYTES / ((size_t)n * 8));
}
bool spectrum_supported(int n);
size_t spectrum_scratch_floats(int n, int n_frames);
// Twiddle buffer the spectrum kernels read (floats) and its contents for frame size n.
size_t spectrum_twiddle_floats(int n);
void spectrum_fill_twiddles(int n, float *out);
// twiddles: exp(-2 pi i m / N), m in [0, N), float2, computed in double on the host.
// beside_ssb: the previous call's SSB pipeline is expected to hold the CUs (pipelined calls); the persistent
// N = 16384 kernel then launches one workgroup per CU, the one that co-resides with it (measured +2-3 % per
// step over two), instead of two per CU for the chip alone.
// n_cus: CUs the stream may use (0 = the device's; a CU-masked stream passes its share) for persistent grids.
// beside_wide_stats: the call's statistics take the wide kernel (its workgroups share the CUs with the next call's
// FFT): N = 32768 / 65536 then launch one tile per workgroup instead of the persistent four-step kernels.
hipError_t launch_spectrum(const void *iq, int fmt, int n, int n_frames, const float *twiddles,
                           float *spectra, float *scratch, hipStream_t stream, bool beside_ssb = false, int n_cus = 0,
                           bool beside_wide_stats = false);
// true when launch_stats runs this geometry with the wide kernel (stats.hip)
bool stats_uses_wide(const StatsGeometry &geo);

// gpool: [n_frames][stats_global_pool_floats / n_frames] device scratch for the pooled-bin median when the
// pool exceeds what the kernel keeps in LDS (stats_global_pool_floats > 0; wide focus windows at N > 65536)
size_t stats_global_pool_floats(const StatsGeometry &geo, int n_frames);
hipError_t launch_stats(const float *spectra, int n_frames, const StatsGeometry &geo, int64_t now_ms,
                        StatsState *state, sdrg_frame_record *records, float *gpool, hipStream_t stream);

// SSB chain.  The pipelined kernel needs no scratch; the lane-per-stream reference kernels (used for
// sample rates below ~0.9 MHz, or when SDRG_SSB_REFERENCE_KERNELS=1) need
// scratch: [n_frames][samp_count + pcm_len] floats.  taps: [n_taps] device floats.
bool ssb_force_reference_kernels();
void ssb_report_stamps();  // diagnostic (SDRG_PIPE_STAMPS=1)
// chunk_table: per chunk of ssb_pipe_chunk() samples {first, last output overlapping it, first, last output
// completed in it} (host-computed, see engine.cpp); may be null (reference kernels).
int ssb_pipe_chunk(void);
// The launcher's choice for p (samp_count, decim, n_taps, pcm_len): true = the pipeline kernel with
// *nsl_mask + 1 FIR slots per stream, false = the lane-per-stream kernels.  Host-only (sdrg_ssb_layout asks it too).
bool ssb_pipe_supported(const SsbParams &p, int *nsl_mask);
int ssb_pipe_chunk_outputs(int decim);  // FIR outputs one chunk can complete
int ssb_pipe_max_chunk_outputs(void);   // the most the pipeline kernel holds
// audio (nullable): run the audio pulse detector's front end on the PCM as it is produced
// stop: an event the pipeline kernel may complete itself (*stop_recorded = true); otherwise the caller records it
hipError_t launch_ssb(const void *iq, int fmt, int n_frames, const SsbParams &p, const float *taps,
                      const int *chunk_table, SsbStreamState *state, float *scratch, int16_t *pcm,
                      const AudioFront *audio, hipStream_t stream, hipEvent_t stop = nullptr,
                      bool *stop_recorded = nullptr);

// Pulse detectors (pulse.hip): one wavefront per stream.  Rings are [n_streams][cap] (cap = cap_mask + 1),
// fh [n_streams][2][PULSE_FH_SLOTS].
hipError_t launch_pulse_reset(PulseStreamState *states, int n_streams, float t_target_init, hipStream_t stream);
hipError_t launch_spectral_pulse(const PulseParams &p, int n_streams, PulseStreamState *states, float *ebuf,
                                 float *fbuf, float *roi_t, int *roi_etat, float *fh, const float *snr_sigma,
                                 const float *freq_hz, int stride_bytes, sdrg_pulse_output *out, hipStream_t stream);
// audio: the front end (lane per stream; also fused into the SSB kernels, see launch_ssb) writes each call's
// energy values to a.new_e [n_streams][a.max_new] (a.max_new >= n_samples / frame_samples + 1) and counts;
// the detector (wave per stream) consumes them.
hipError_t launch_audio_front(const AudioFront &a, const void *audio, int fmt, int n_samples, int stride, int n_streams,
                              hipStream_t stream);
hipError_t launch_audio_detect(const PulseParams &p, int n_streams, PulseStreamState *states, float *ebuf, float *roi_t,
                               int *roi_etat, const float *new_e, int max_new, const int *new_count,
                               sdrg_pulse_output *out, hipStream_t stream);

// Sets the thread's sdrg_last_error message and returns code (engine.cpp).
int32_t fail(int32_t code, const char *fmt, ...);

// Multi-GPU (dist.cpp, gather.hip).  One gather per item, all in one RCCL group on `stream`: every rank sends
// items[i].bytes from items[i].send; the root receives world x bytes at items[i].recv in rank order.
struct GatherItem {
    const void *send;
    void *recv;
    size_t bytes;
};
int32_t dist_gather(sdrg_dist *d, const GatherItem *items, int n_items, int root, hipStream_t stream);
int dist_device(const sdrg_dist *d);
int dist_world(const sdrg_dist *d);
int dist_rank(const sdrg_dist *d);
// out[s][j] = spectra[s][lo + j], j < nb: each stream's focus-window slice, contiguous for the gather
// gather.hip: the read + write GB/s of a float4 streaming copy of `bytes` (reps timed launches) on the current device
hipError_t measure_stream_copy(size_t bytes, int reps, double *gbs);
hipError_t launch_focus_pack(const float *spectra, int n_streams, int n, int lo, int nb, float *out, hipStream_t stream);

// Display stage (display.hip): rows of n floats, the span [lo, lo + nb) of each reduced to `width` columns
// (reduce: SDRG_DISPLAY_MAX / _MEAN), 10 log10f(v + 1e-20f), written as float dB or 8-bit codes (format:
// SDRG_DISPLAY_DB_F32 / _U8, code = (d - db_min) * scale clamped and rounded).  out: [n_streams][width], rows dense.
struct DisplayParams {
    int n, lo, nb, width, reduce, format;
    float db_min, scale;  // U8 only; scale = 255.0f / (db_max - db_min)
};
hipError_t launch_display(const float *spectra, int n_streams, const DisplayParams &p, void *out, hipStream_t stream);

// Integration stage (integrate.hip): element-wise over count = n_streams * N floats.  MEAN / MAX: ring is
// [period][slot_stride] floats (slot_stride = integrate_slot_stride(count), 16-byte aligned), the depth - 1 frames before
// this one in the slots slot - (depth - 1) .. slot - 1 (mod period); the call writes its input to `slot`.  EMA: ema is
// [count] floats, not read when depth == 1.  out may be spectra.
struct IntegrateParams {
    int mode, period, slot, depth;
    float alpha;
};
size_t integrate_slot_stride(size_t count);
hipError_t launch_integrate(const float *spectra, size_t count, const IntegrateParams &p, float *ring, size_t slot_stride,
                            float *ema, float *out, hipStream_t stream);

// Peak table stage (peaks.hip): per row of n floats, the span [lo, lo + nb): noise floor (rank nb / 2), the candidates
// (first maximum of a window of +- min_sep bins), those at least threshold_db over the floor, the max_peaks strongest.
// peaks: [n_streams][max_peaks], summary: [n_streams]; every byte of both is written.
struct PeaksParams {
    int n, lo, nb, max_peaks, min_sep;
    float threshold_db;
};
hipError_t launch_peaks(const float *spectra, int n_streams, const PeaksParams &p, sdrg_peak *peaks,
                        sdrg_peaks_summary *summary, hipStream_t stream);

// What the stages in fir_tile.h's tile form share (DDC, demodulator's FIR, sideband): per stream, out[j] is a sum over
// the values at t = first + j decim - k, k in [0, taps), j in [0, n_out); t in [0, n) is the call's frame and t in
// [-(taps - 1), 0) the history hist_old [n_streams][taps - 1] values (nullptr: zeros, the call follows a restart).  The
// call writes rows of cap outputs whole (zeros from n_out on) and the values at t in [n - (taps - 1), n) to hist_new.
// The host fills all but the last line (engine.cpp: fir_tile_fill); fir_tile_plan (fir_tile.h) checks that and fills
// the last line in the launcher.
struct FirTileParams {
    int n, decim, taps, first, n_out, cap;
    const float *hist_old;
    float *hist_new;
    int tile, row, n_tiles;
};

// DDC stage (ddc.hip): per stream, out[j] = sum_k h[k] v[first + j decim - k], v the frame's n raw samples mixed by the
// NCO (phase inc * (g0_lo + t) at local index t); the history holds mixed samples, [taps - 1][2] per stream.  Writes
// out [n_streams][cap][2] and the frame's phasors to `phasors` (scratch of n float2, all streams share it).  vec_ok is
// the launcher's.
struct DdcParams : FirTileParams {
    uint32_t inc, g0_lo;
    const float *nco_tab;    // nco_tables() on the device
    float *phasors;
    int vec_ok;
};
struct DdcTaps {
    float h[SDRG_DDC_MAX_TAPS];
};
int ddc_tile_outputs(int decim, int taps);  // outputs per workgroup
hipError_t launch_ddc(const void *iq, int fmt, int n_streams, const DdcParams &p, const DdcTaps &taps, float *out,
                      hipStream_t stream);

// DDC bank stage (bank.hip): per stream s and channel c < channels, row s channels + c of out is launch_ddc's row for the
// stream's n raw samples at inc = incs[s channels + c] (phase inc * (g0_lo + t) at local index t), through the same
// taps.  The history holds *unmixed* samples, [taps - 1][2] per stream.  Writes out [n_streams * channels][cap][2].
// group (channels per workgroup: bank_group) and vec_ok are the launcher's.
struct BankParams : FirTileParams {
    uint32_t g0_lo;
    const float *nco_tab;  // nco_tables() on the device
    const uint32_t *incs;  // [n_streams][channels]
    int channels, group, vec_ok;
};
int bank_tile_outputs(int decim, int taps);       // outputs per workgroup
int bank_group(int channels, int n_streams);      // channels per workgroup
hipError_t launch_bank(const void *iq, int fmt, int n_streams, const BankParams &p, const DdcTaps &taps, float *out,
                       hipStream_t stream);

// Demodulator stage (demod.hip): per stream the n complex samples at chan + stream * in_stride (float2) through the
// detector (mode, kf; the previous sample from state_old), the DC block and the de-emphasis (alpha, a; m and s from
// state_old) in `scratch` [n_streams][scratch_stride] floats, then out[j] = gain * sum_k h[k] v[first + j decim - k];
// the history holds values of v.  Writes out [n_streams][cap] (int16 or float by out_format), and, if n > 0, {wr, wi,
// m, s} per stream to state_new and the history.  fresh: no previous sample, and state_old is not read (the FIR reads
// hist_old, which is then nullptr).  n = 0 writes out only.
struct DemodParams : FirTileParams {
    int in_stride, scratch_stride;
    int mode, out_format, fresh;
    float kf, alpha, a, gain;
    const float *state_old;
    float *state_new;
    float *scratch;
};
struct DemodTaps {
    float h[SDRG_DEMOD_MAX_TAPS];
};
constexpr int DEMOD_CHUNK = 64;                // samples of a stream per step of the recurrence kernel
int demod_tile_outputs(int decim, int taps);  // FIR outputs per workgroup
hipError_t launch_demod(const float *chan, int n_streams, const DemodParams &p, const DemodTaps &taps, void *out,
                        hipStream_t stream);

// Channelizer stage (channelizer.hip): per stream and output time j in [0, n_out), the branch sums u_p = sum_q
// h[p + q channels] x[first + j decim - p - q channels] (x the frame's n unpacked samples and, at indices in
// [-(L - 1), 0), hist_old [n_streams][L - 1][2], nullptr: zeros; L = channels taps_per_channel), their DFT
// Y_c = sum_p u_p e^{+j 2 pi c p / channels}, and at oversample 2 the sign (-1)^{c (m_parity + j)}.  Writes the rows
// [first_channel, first_channel + n_channels) of the fftshifted order to out [n_streams][n_channels][cap][2] whole
// (zeros from n_out on) and the unpacked samples at [n - (L - 1), n) to hist_new.  taps: [L] floats, then
// e^{-j 2 pi t / 256}, t in [0, 256), as float pairs, in device memory.  log2m, tile, log2tile, n_tiles, region and
// vec_ok are the launcher's.
struct ChanParams {
    int n, channels, taps_per_channel, oversample, decim, first, n_out, cap;
    int first_channel, n_channels, m_parity;
    const float *taps;
    const float *hist_old;
    float *hist_new;
    int log2m, tile, log2tile, n_tiles, region, vec_ok;
};
constexpr int CHAN_TWIDDLES = 256;
int chan_tile_outputs(int channels);  // output times per workgroup
hipError_t launch_channelizer(const void *iq, int fmt, int n_streams, const ChanParams &p, float *out,
                              hipStream_t stream);

// Resampler stage (resample.hip): per stream and output j in [0, n_out), t = phi0 + j decim, q = q0 + t / interp,
// phi = t mod interp, out[j] = gain * sum_k taps[phi][k] x[q - k], k in [0, taps_per_phase): x the n values at
// in + stream * in_stride (floats, or float pairs at components 2) and, at indices in [-(taps_per_phase - 1), 0),
// hist_old [n_streams][taps_per_phase - 1] values (nullptr: zeros).  Writes out [n_streams][cap] whole (zeros
// from n_out on; float or int16 by out_format, pairs at components 2) and, if n > 0, the values at
// [n - (taps_per_phase - 1), n) to hist_new.  taps: [interp][taps_per_phase] floats in device memory.  n_tiles is the
// launcher's.
struct ResampleParams {
    int n, in_stride, interp, decim, taps_per_phase, q0, phi0, n_out, cap;
    int components, out_format;
    float gain;
    const float *taps;
    const float *hist_old;
    float *hist_new;
    int n_tiles;
};
constexpr int RESAMPLE_TILE = 256;  // outputs per workgroup, one per lane
hipError_t launch_resample(const void *in, int n_streams, const ResampleParams &p, void *out, hipStream_t stream);

// The block stages (block_stage.h: the squelch and the AGC): per stream the n complex samples at chan + stream *
// in_stride (float2) are the positions [off, off + n) of a run of blocks of `block` samples, off = g mod block: n_blocks
// = (off + n) / block of them complete.  state_old / state_new [n_streams][block + BLOCK_STATE_HEAD] floats: the law's
// four words, then the powers so far of the block in progress; fresh: state_old is not read (and off is 0).  blk
// [blocks][n_streams] floats is scratch: the completed blocks' statistics, then, in their place, what the law leaves
// for the pass kernel.  Writes out [n_streams][in_stride][2] whole (zeros from n on; out may be chan), and, if n > 0,
// state_new; the stage's records [n_streams] unless nullptr.  n_streams, log2_block, tile and inv_block are the
// launcher's.
struct BlockParams {
    int n, in_stride, block, hang, off, n_blocks, fresh;
    const float *state_old;
    float *state_new;
    float *blk;
    int n_streams, log2_block, tile;
    float inv_block;
};
constexpr int BLOCK_STATE_HEAD = 4;
constexpr int BLOCK_PASS = 512;  // positions a workgroup takes at a time
constexpr int BLOCK_MIN = SDRG_SQUELCH_MIN_BLOCK, BLOCK_MAX = SDRG_SQUELCH_MAX_BLOCK, BLOCK_MAX_IN = SDRG_SQUELCH_MAX_IN;
static_assert(BLOCK_MIN == SDRG_AGC_MIN_BLOCK && BLOCK_MAX == SDRG_AGC_MAX_BLOCK && BLOCK_MAX_IN == SDRG_AGC_MAX_IN,
              "one skeleton: the two stages' limits are the same");
// consecutive samples per workgroup of the power and of the pass kernel
inline int block_tile(int block) { return block > BLOCK_PASS ? block : BLOCK_PASS; }

// Squelch stage (squelch.hip).  The state's words: {L, open, hang, the code of the block in progress} (the last three as
// int bits); a fresh stream's read as zeros.  blk ends as the code of the block after each; out is the gated samples.
struct SquelchParams : BlockParams {
    float beta, open_thr, close_thr;
    sdrg_squelch_record *records;
};
hipError_t launch_squelch(const float *chan, int n_streams, const SquelchParams &p, float *out, hipStream_t stream);

// AGC stage (agc.hip).  The state's words: {G, G_prev, hang (int bits), P_last}; a fresh stream's read as {init_gain,
// init_gain, 0, +0}.  blk's statistics are the mean or the peak power (detector), and it ends as the gain after each
// block; out is block b of the stream under the ramp from gain[b - 2] to gain[b - 1].
struct AgcParams : BlockParams {
    int detector;
    float target, max_gain, init_gain, floor_thr, alpha_a, alpha_d;
    sdrg_agc_record *records;
};
hipError_t launch_agc(const float *chan, int n_streams, const AgcParams &p, float *out, hipStream_t stream);

// IQ correction stage (iqcorr.hip): per stream the n raw samples at iq + stream * in_stride (in fmt) are the positions
// [off, off + n) of a run of blocks of `block` samples, as the block stages' are.  state_old / state_new [n_streams]
// [2 block + IQCORR_STATE_HEAD] floats: {dr, di, wr, wi} after the last completed block, the same after the one before,
// {A, B, P, seeded (int bits)}, then the scaled samples so far of the block in progress; fresh: state_old is not read
// (zeros, and off is 0).  mom [blocks][5][n_streams] and theta [blocks][4][n_streams] floats are scratch: the completed
// blocks' moments, and the four parameters after each.  Writes out [n_streams][in_stride][2] whole (zeros from n on; out
// may be iq at CF32), and, if n > 0, state_new; records [n_streams] unless nullptr.  n_streams, log2_block, tile and
// inv_block are the launcher's.
struct IqcorrParams {
    int n, in_stride, block, mode, off, n_blocks, fresh;
    float beta_dc, beta_bal, floor_thr;
    const float *state_old;
    float *state_new;
    float *mom, *theta;
    sdrg_iqcorr_record *records;
    int n_streams, log2_block, tile;
    float inv_block;
};
constexpr int IQCORR_STATE_HEAD = 12;
constexpr int IQCORR_MIN_BLOCK = SDRG_IQCORR_MIN_BLOCK;
static_assert(SDRG_IQCORR_MAX_BLOCK == BLOCK_MAX && SDRG_IQCORR_MAX_IN == BLOCK_MAX_IN && IQCORR_MIN_BLOCK >= 64,
              "the block stages' positions and butterfly: a block is at least a wave's 32 pairs");
hipError_t launch_iqcorr(const void *iq, int fmt, int n_streams, IqcorrParams p, float *out, hipStream_t stream);

// AFC stage (afc.hip): per stream the n complex samples at chan + stream * in_stride (float2) are the positions
// [off, off + n) of a run of blocks of `block` samples, as the block stages' are.  state_old / state_new [n_streams]
// [2 block + AFC_STATE_HEAD] floats: {A, B, P, coh, inc (int bits), Phi of the block in progress (uint bits), flags
// (locked | seeded << 1, int bits), 0}, then the samples so far of the block in progress; fresh: state_old is not read
// (zeros, and off is 0).  mom [blocks][3][n_streams] floats and blk [blocks + 1][2][n_streams] words are scratch: the
// completed blocks' Rr, Ri and W, and (Phi, inc) as uint bits for the call's block j (the block in progress when the
// call began is block 0): the phase at its first sample and the increment it is mixed by.  With track, writes out
// [n_streams][in_stride][2] whole (zeros from n on; out may be chan); without, out is not touched.  If n > 0, state_new;
// records [n_streams] unless nullptr.  n_streams, log2_block, tile and inv_block are the launcher's.
struct AfcParams {
    int n, in_stride, block, track, off, n_blocks, fresh;
    float beta, floor_thr, lock_thr, max_s, K, hz_per_inc, rad_per_inc;
    const float *nco_tab;  // nco_tables() on the device
    const float *state_old;
    float *state_new;
    float *mom;
    uint32_t *blk;
    sdrg_afc_record *records;
    int n_streams, log2_block, tile;
    float inv_block;
};
constexpr int AFC_STATE_HEAD = 8;
static_assert(SDRG_AFC_MIN_BLOCK == BLOCK_MIN && SDRG_AFC_MAX_BLOCK == BLOCK_MAX && SDRG_AFC_MAX_IN == BLOCK_MAX_IN,
              "the block stages' positions and butterfly");
hipError_t launch_afc(const float *chan, int n_streams, AfcParams p, float *out, hipStream_t stream);

// Symbol stage (symbols.hip): per stream the n floats at in + stream * in_stride are the positions [off, off + n) of a
// run of blocks of `block` values, as the block stages' are.  state_old / state_new [n_streams][block + SYM_STATE_HEAD +
// SYM_HISTORY] floats: {A, B, U, M, Q, coh, tau (uint bits), flags (locked | seeded << 1, int bits), slips (int bits),
// centre, thr, 0 ...}, the SYM_HISTORY values before the block in progress (+0 for what lies before the stream), then
// that block's values so far; fresh: state_old is not read (a restarted stream, and off is 0).  mom [blocks][5]
// [n_streams] floats and blk [blocks + 1][4][n_streams] words are scratch: the completed blocks' Ab, Bb, Ub, Mb and Qb,
// and (tau, centre, thr, locked) for the call's block j (the block in progress when the call began is block 0).  c0 is
// c at the call's first value, (uint32)(inc g); cpos0 that at position 0; emit0 = c0, plus 2^32 if the call's first
// value emits: the call's value t is the last of floor((emit0 + inc t) / 2^32) symbols.  Writes symbols [n_streams][cap]
// whole (bytes, or floats at soft; zeros from n_sym on), and, if n > 0, state_new; records [n_streams] unless nullptr.
// n_streams, log2_block and tile are the launcher's.
struct SymParams {
    int n, in_stride, block, off, n_blocks, fresh;
    int levels, track, soft, n_sym, cap;
    uint32_t inc, c0, cpos0, tau0;
    uint64_t emit0;
    int64_t trim;
    float rinc, beta, beta_level, floor_thr, lock_thr, K, rs, level_scale, fixed_centre, fixed_thr;
    const float *tab;  // [SDRG_SYM_TABLE][2] on the device
    const float *state_old;
    float *state_new;
    float *mom;
    uint32_t *blk;
    sdrg_symbols_record *records;
    int n_streams, log2_block, tile;
};
constexpr int SYM_STATE_HEAD = 14, SYM_HISTORY = SDRG_SYM_HISTORY;
constexpr int SYM_PASS_TILE = 256;  // symbols per workgroup of the pass kernel, one per lane
static_assert(SDRG_SYM_MIN_BLOCK >= 64 && SDRG_SYM_MAX_BLOCK == BLOCK_MAX && SDRG_SYM_MAX_IN == BLOCK_MAX_IN &&
                  (SYM_STATE_HEAD + SYM_HISTORY) % 4 == 0,
              "the block stages' positions and butterfly: a block is at least a wave's 32 pairs; 16-byte state rows");
constexpr int sym_state_words(int block) { return SYM_STATE_HEAD + SYM_HISTORY + block; }
hipError_t launch_symbols(const float *in, int n_streams, SymParams p, void *symbols, hipStream_t stream);

// Noise blanker stage (blanker.hip): per stream the n raw samples at iq + stream * in_stride (in fmt) are the positions
// [off, off + n) of a run of blocks of `block` samples, as the block stages' are.  state_old / state_new [n_streams]
// [blanker_state_words(block)] floats: {L, seeded (int bits), the threshold in force for the block in progress, 0}, the
// powers so far of the block in progress, the hit flags of the last BLANKER_FLAGS inputs (ints, the oldest first; 0 for
// what lies before the stream) and the last BLANKER_MAX_LEAD scaled samples (pairs, zeros before the stream); fresh:
// state_old is not read (L = 0, unseeded, +inf, no flags, zeros, and off is 0).  flo and thr [blocks][n_streams] floats
// are scratch: the completed blocks' F, and the threshold after each.  skip = max(lead - g, 0): the call's outputs whose
// input lies before the stream.  Writes out [n_streams][in_stride][2] whole (zeros from n on; out must not overlap iq),
// and, if n > 0, state_new; records [n_streams] unless nullptr.  n_streams, log2_block and tile are the launcher's.
struct BlankerParams {
    int n, in_stride, block, lead, tail, off, n_blocks, fresh, skip;
    float beta, floor_thr, ratio;
    const float *state_old;
    float *state_new;
    float *flo, *thr;
    sdrg_blanker_record *records;
    int n_streams, log2_block, tile;
};
constexpr int BLANKER_STATE_HEAD = 4;
constexpr int BLANKER_MIN_BLOCK = SDRG_BLANKER_MIN_BLOCK;
constexpr int BLANKER_MAX_LEAD = SDRG_BLANKER_MAX_LEAD, BLANKER_MAX_TAIL = SDRG_BLANKER_MAX_TAIL;
constexpr int BLANKER_FLAGS = BLANKER_MAX_LEAD + BLANKER_MAX_TAIL;
constexpr int BLANKER_TILE = BLOCK_PASS;  // outputs per workgroup of the pass kernel
static_assert(SDRG_BLANKER_MAX_BLOCK == BLOCK_MAX && SDRG_BLANKER_MAX_IN == BLOCK_MAX_IN && BLANKER_MIN_BLOCK >= 64,
              "the block stages' positions and butterfly: a block is at least a wave's 32 pairs");
constexpr int blanker_state_words(int block) { return BLANKER_STATE_HEAD + block + BLANKER_FLAGS + 2 * BLANKER_MAX_LEAD; }
hipError_t launch_blanker(const void *iq, int fmt, int n_streams, BlankerParams p, float *out, hipStream_t stream);

// Tone detector stage (tones.hip): per stream the n values at in + stream * in_stride (floats, or float pairs at
// components 2) are the positions [soff, soff + n) counted from the start of the sub-block of 64 in progress, soff = g
// mod 64; that sub-block is the sub0-th of its block of sub_blocks, sub0 = (g mod S) / 64.  n_sub = (soff + n) / 64
// sub-blocks and n_blocks = (sub0 + n_sub) / sub_blocks blocks complete.  table [K][S][2] (c, s) and wf [S] are the
// design.  state_old / state_new [n_streams][tones_state_words(K, components)] floats: the TONES_STATE_HEAD words {tone,
// last, run, miss (int bits), power, share, 0, 0}, the 2 K + 1 accumulators (C_0 .. C_(K-1), S_0 .. S_(K-1), E) of the
// block in progress, and the values so far of the sub-block in progress; fresh: state_old is not read (and soff, sub0
// are 0).  sums [n_streams][max_sub][2 K + 1] floats is scratch, the completed sub-blocks' sums in the accumulators'
// order, max_sub the rows per stream.  Writes powers [n_streams][cap_blocks][K] whole (+0 from n_blocks on), and, if n >
// 0, state_new; records [n_streams] unless nullptr.  n_streams is the launcher's.
struct TonesParams {
    int n, in_stride, components, n_tones, sub_blocks, soff, sub0, n_sub, n_blocks, cap_blocks, max_sub, fresh;
    int confirm, release;
    float pnorm, enorm, min_power, dom, share_thr;
    const float *table, *wf;
    const float *state_old;
    float *state_new;
    float *sums;
    sdrg_tones_record *records;
    int n_streams;
};
constexpr int TONES_STATE_HEAD = 8;
constexpr int TONES_SUB = 64;        // values per sub-block: one per lane of a wave
constexpr int TONES_GROUP_SUBS = 4;  // sub-blocks per workgroup of the correlate kernel, one per wave
constexpr int tones_state_words(int K, int components) { return TONES_STATE_HEAD + 2 * K + 1 + (TONES_SUB - 1) * components; }
hipError_t launch_tones(const void *in, int n_streams, TonesParams p, float *powers, hipStream_t stream);

// Sideband stage (sideband.hip): per stream and output j, A = sum_k cr[k] zr[first + j decim - k] and Bm = sum_k ci[k]
// zi[first + j decim - k], z the n complex samples at chan + stream * in_stride (float2); u = A - Bm, l = A + Bm.  The
// history holds samples, [taps - 1][2] per stream.  Writes out [n_streams][cap] (u gain, l gain, or at mode BOTH the
// pairs of them; float or int16 by out_format) and, if n > 0, the history.  taps_dev: [taps][2] floats (cr, ci) in
// device memory.  vec_ok and pair_ok are the launcher's.
struct SidebandParams : FirTileParams {
    int in_stride;
    int mode, out_format;
    float gain;
    const float *taps_dev;
    int vec_ok, pair_ok;
};
int sideband_tile_outputs(int decim, int taps);  // outputs per workgroup
hipError_t launch_sideband(const float *chan, int n_streams, const SidebandParams &p, void *out, hipStream_t stream);

}  // namespace sdrg
