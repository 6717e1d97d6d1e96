// design.cpp — host-side filter design and window geometry, with the reference's own float expressions.
//
// Everything here is per configuration, not per sample, so it runs on the host once and the kernels
// receive the resulting coefficients.  The expressions are kept exactly as the reference writes them
// (mixed double/float promotions included) and this file is compiled without FP contraction, so the
// coefficients are bit-identical to the reference's x86-64 build (checked by tests/test_engine_host.py
// against tests/golden/golden_ssb_design.npz, which comes from the reference build).
#include <math.h>

#include <cmath>
#include <stdint.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "design.h"
#include "glibc_logf.h"

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif


namespace sdrg {

// iir2InitLowpass (src/ssb/ssb_demod_opt.cpp:60-73)
void design_lowpass(float fs, float fc, float Q, float c[5]) {
    float w0 = 2.0f * M_PI * fc / fs;
    float cosw0 = cosf(w0);
    float sinw0 = sinf(w0);
    float alpha = sinw0 / (2.0f * Q);
    float norm = 1.0f / (1.0f + alpha);
    c[0] = (1.0f - cosw0) / 2.0f * norm;
    c[1] = (1.0f - cosw0) * norm;
    c[2] = c[0];
    c[3] = -2.0f * cosw0 * norm;
    c[4] = (1.0f - alpha) * norm;
}

// biquadInitHighpass (:148-164)
void design_highpass(float fs, float f0, float Q, float c[5]) {
    float w0 = 2.0f * M_PI * f0 / fs;
    float cosw0 = cosf(w0);
    float sinw0 = sinf(w0);
    float alpha = sinw0 / (2.0f * Q);
    float b0 = (1 + cosw0) / 2.0f;
    float b1 = -(1 + cosw0);
    float b2 = (1 + cosw0) / 2.0f;
    float a0 = 1 + alpha;
    float a1 = -2 * cosw0;
    float a2 = 1 - alpha;
    c[0] = b0 / a0;
    c[1] = b1 / a0;
    c[2] = b2 / a0;
    c[3] = a1 / a0;
    c[4] = a2 / a0;
}

// biquadInitBandpass (:166-175)
void design_bandpass(float fs, float f0, float Q, float c[5]) {
    float w0 = 2.0f * M_PI * f0 / fs;
    float alpha = sinf(w0) / (2.0f * Q);
    float cosw0 = cosf(w0);
    float b0 = alpha, b1 = 0.0f, b2 = -alpha;
    float a0 = 1.0f + alpha, a1 = -2.0f * cosw0, a2 = 1.0f - alpha;
    c[0] = b0 / a0;
    c[1] = b1 / a0;
    c[2] = b2 / a0;
    c[3] = a1 / a0;
    c[4] = a2 / a0;
}

// simpleFIRDecimate's Hann-windowed sinc (:121-134); returns the tap count.  taps0: the length asked
// for (0 = the reference's 255; other values only through the NCO/short-FIR variant, sdrg.h)
int design_fir(int64_t in_size, int decim, float cutoff_rel, float *h, int taps0) {
    int N = ssb_taps_for(in_size, taps0);
    int M = N - 1;
    float fc = cutoff_rel / decim;
    for (int n = 0; n < N; n++) {
        int k = n - M / 2;
        float sinc = (k == 0) ? 2.0f * M_PI * fc : sinf(2.0f * M_PI * fc * k) / (float)k;
        float w = 0.5f - 0.5f * cosf(2.0f * M_PI * n / M);
        h[n] = (sinc / M_PI) * w;
    }
    float sum = 0.0f;
    for (int n = 0; n < N; n++) sum += h[n];
    if (sum != 0.0f)
        for (int n = 0; n < N; n++) h[n] /= sum;
    return N;
}

int ssb_decim(uint32_t sample_rate) {  // processSSB_opt :273
    const int d = (int)(sample_rate / 48000.0f);
    return d > 1 ? d : 1;
}

int ssb_taps_for(int64_t samp_count, int taps0) {
    int N = taps0 > 0 ? taps0 : 255;
    if (N > (int)samp_count) N = (int)samp_count | 1;
    return N;
}

int ssb_pcm_len(int64_t samp_count, uint32_t sample_rate, int taps0) {
    const int N = ssb_taps_for(samp_count, taps0);
    if (samp_count < N) return 0;
    return (int)((samp_count - N) / ssb_decim(sample_rate) + 1);
}

static int off_to_bin(float offset_hz, float nyquist, float freq_per_bin) {  // fft_process.cpp:131-133
    return (int)((offset_hz + nyquist) / freq_per_bin);
}

// Window geometry of evaluateSignalStrength (fft_process.cpp:124-216)
StatsGeometry stats_geometry(uint32_t sample_rate, uint32_t center_frequency, int n, int focus_khz) {
    StatsGeometry g{};
    g.n = n;
    const float freq_per_bin = static_cast<float>(sample_rate) / static_cast<float>(n);
    const float X_hz = focus_khz * 1000.0f;
    const float nyquist = sample_rate / 2.0f;
    int lo = off_to_bin(-X_hz, nyquist, freq_per_bin);
    int hi = off_to_bin(+X_hz, nyquist, freq_per_bin) - 1;
    g.focus_lo = lo > 0 ? lo : 0;
    g.focus_hi = hi < n - 1 ? hi : n - 1;
    g.focus_len = g.focus_hi - g.focus_lo + 1;
    // the Gumbel term's logN (:282): geometry only, so computed here with the reference's libm (glibc's logf,
    // restated in glibc_logf.h so the value does not depend on the host's C library)
    g.log_focus_len = g.focus_len > 0 ? glibc::logf(static_cast<float>(g.focus_len)) : 0.0f;
    const int w = (int)ceilf(1000.0f / freq_per_bin);
    g.win_bins_1k = w > 1 ? w : 1;
    int nr = 0;
    for (int k = 1; k <= 5; k++) {
        const float nearX = (4 * k - 2) * X_hz;
        const float farX = 4 * k * X_hz;
        if (farX >= nyquist) break;
        for (int side = 0; side < 2; side++) {
            int l, h;
            if (side == 0) {
                l = off_to_bin(+nearX, nyquist, freq_per_bin);
                h = off_to_bin(+farX, nyquist, freq_per_bin) - 1;
            } else {
                l = off_to_bin(-farX, nyquist, freq_per_bin);
                h = off_to_bin(-nearX, nyquist, freq_per_bin) - 1;
            }
            l = l > 0 ? l : 0;
            h = h < n - 1 ? h : n - 1;
            if (h <= l) continue;
            g.win_lo[nr] = l;
            g.win_hi[nr] = h;
            nr++;
        }
    }
    g.n_ref = nr;
    // pooled bins: the nBottom longest windows bound the pool whatever the sort order
    int lens[10];
    for (int i = 0; i < nr; i++) lens[i] = g.win_hi[i] - g.win_lo[i] + 1;
    for (int i = 1; i < nr; i++)
        for (int j = i; j > 0 && lens[j] > lens[j - 1]; j--) {
            const int t = lens[j];
            lens[j] = lens[j - 1];
            lens[j - 1] = t;
        }
    const int nb0 = (int)(nr * 0.4f);
    const int n_bottom = nb0 > 1 ? nb0 : 1;
    int pool = 0;
    for (int i = 0; i < n_bottom && i < nr; i++) pool += lens[i];
    g.max_pool = pool;
    int slo = g.focus_lo, shi = g.focus_hi;
    for (int i = 0; i < nr; i++) {
        slo = g.win_lo[i] < slo ? g.win_lo[i] : slo;
        shi = g.win_hi[i] > shi ? g.win_hi[i] : shi;
    }
    g.span_lo = slo;
    g.span_len = g.focus_len > 0 ? shi - slo + 1 : 0;
    g.freq_per_bin = freq_per_bin;
    g.nyquist = nyquist;
    g.cf_float = static_cast<float>(center_frequency);
    g.cf_minus_nyq = static_cast<float>(center_frequency) - nyquist;  // :327
    g.cf_u32_minus_nyq = (center_frequency - nyquist);                // :350, uint32 promoted to float
    g.cf_changed = 0;
    return g;
}

// Bilinear-transform Butterworth sections of the audio pulse detector, in float with the reference's
// expression order (audio_pulse_detector.cpp:4, :29-55).
void design_pulse_sos(float fs, float fc, bool highpass, float c[5]) {
    const float pi = 3.14159265358979f;
    const float Q = 0.7071f;
    const float K = tanf(pi * fc / fs);
    const float K2 = K * K;
    const float norm = K2 + K / Q + 1.f;
    if (highpass) {
        c[0] = 1.f / norm;
        c[1] = -2.f / norm;
        c[2] = 1.f / norm;
    } else {
        c[0] = K2 / norm;
        c[1] = 2.f * K2 / norm;
        c[2] = K2 / norm;
    }
    c[3] = 2.f * (K2 - 1.f) / norm;
    c[4] = (K2 - K / Q + 1.f) / norm;
}

// NCO of the SSB variant (sdrg.h, sdrg_engine_set_ssb_variant): phase increment per sample of a 32-bit
// phase accumulator, round(hz / fs * 2^32) modulo 2^32 (negative frequencies wrap)
uint32_t nco_increment(double hz, uint32_t sample_rate) {
    const double turns = hz / (double)sample_rate;
    const double frac = turns - std::floor(turns);  // [0, 1)
    return (uint32_t)(uint64_t)std::llround(frac * 4294967296.0);  // 2^32 wraps to 0 through the cast
}

// e^{-j 2 pi ph / 2^32} = hi[ph >> 22] * lo[(ph >> 12) & 1023]: hi[a] = e^{-j 2 pi a / 2^10}, lo[b] =
// e^{-j 2 pi b / 2^20}, each computed in double and rounded to float; interleaved {re, im}, hi then lo
void nco_tables(float *tab) {
    for (int a = 0; a < 1024; a++) {
        const double t = 2.0 * M_PI * (double)a / 1024.0;
        tab[2 * a] = (float)std::cos(t);
        tab[2 * a + 1] = (float)-std::sin(t);
    }
    for (int b = 0; b < 1024; b++) {
        const double t = 2.0 * M_PI * (double)b / 1048576.0;
        tab[2048 + 2 * b] = (float)std::cos(t);
        tab[2048 + 2 * b + 1] = (float)-std::sin(t);
    }
}

// The DDC stage's configuration rules (sdrg.h): nullptr, or what is wrong
const char *ddc_check(uint32_t sample_rate, double offset_hz, double cutoff_hz, int decimation, int taps) {
    if (sample_rate == 0) return "sample_rate must be > 0";
    if (!std::isfinite(offset_hz)) return "offset_hz must be finite";
    if (decimation < 1 || decimation > 512) return "decimation outside [1, 512]";
    if (taps < 1 || taps > 511 || (taps & 1) == 0) return "taps must be odd and in [1, 511]";
    if (!(cutoff_hz > 0.0 && cutoff_hz <= (double)sample_rate / 2.0)) return "cutoff_hz outside (0, sample_rate / 2]";
    return nullptr;
}

// The DDC bank's configuration rules (sdrg.h): the DDC's for the shared filter, the channel count and the row limit of
// the launch; nullptr, or what is wrong
const char *bank_check(uint32_t sample_rate, double cutoff_hz, int decimation, int taps, int channels, int n_streams) {
    if (const char *bad = ddc_check(sample_rate, 0.0, cutoff_hz, decimation, taps)) return bad;
    if (channels < 1 || channels > SDRG_BANK_MAX_CHANNELS) return "channels outside [1, 4096]";
    if (n_streams < 1 || (int64_t)n_streams * channels > 65535) return "n_streams * channels above 65535";
    return nullptr;
}

// and its offsets', count = n_streams * channels of them: every one finite
const char *bank_offsets_check(const double *offsets_hz, size_t count) {
    if (!offsets_hz) return "null offsets_hz";
    for (size_t i = 0; i < count; i++)
        if (!std::isfinite(offsets_hz[i])) return "every offset must be finite";
    return nullptr;
}

// The DDC stage's low-pass (sdrg.h): a Hann-windowed sinc of `taps` (odd) coefficients with unit DC gain, in double
void ddc_design(uint32_t sample_rate, double cutoff_hz, int taps, float *h) {
    lowpass_design(cutoff_hz / (double)sample_rate, taps, h);
}

void lowpass_design(double f, int taps, float *h) { lowpass_design_scaled(f, taps, 1.0, h); }

// scale = 1 multiplies exactly: lowpass_design's floats are what they were as v[k] / sum
// the windowed sinc before its normalisation, in double: v[k], and their sum returned
static double lowpass_window(double f, int taps, std::vector<double> &v) {
    v.resize((size_t)taps);  // the resampler's prototype has up to 8192 coefficients
    double sum = 0.0;
    for (int k = 0; k < taps; k++) {
        const int c = k - (taps - 1) / 2;
        const double ideal = c == 0 ? 2.0 * f : std::sin(2.0 * M_PI * f * (double)c) / (M_PI * (double)c);
        const double w = 0.5 - 0.5 * std::cos(2.0 * M_PI * (double)(k + 1) / (double)(taps + 1));
        v[k] = ideal * w;
        sum += v[k];
    }
    return sum;
}

void lowpass_design_scaled(double f, int taps, double scale, float *h) {
    std::vector<double> v;
    const double sum = lowpass_window(f, taps, v);
    for (int k = 0; k < taps; k++) h[k] = (float)(scale * v[k] / sum);
}

// The channelizer stage's configuration rules (sdrg.h): nullptr, or what is wrong
const char *chan_check(const sdrg_channelizer_config &c) {
    const int M = c.channels, P = c.taps_per_channel;
    if (M < 2 || M > SDRG_CHANNELIZER_MAX_CHANNELS || (M & (M - 1)) != 0) return "channels must be a power of two in [2, 256]";
    if (P < 1 || P > SDRG_CHANNELIZER_MAX_TAPS_PER_CHANNEL) return "taps_per_channel outside [1, 32]";
    if (M * P > SDRG_CHANNELIZER_MAX_TAPS) return "channels * taps_per_channel above 4096";
    if (c.oversample != 1 && c.oversample != 2) return "oversample must be 1 or 2";
    if (!(c.cutoff_rel > 0.0 && c.cutoff_rel <= (double)M / 2.0)) return "cutoff_rel outside (0, channels / 2]";
    if (c.n_channels < 1 || c.first_channel < 0 || c.first_channel > M - c.n_channels)
        return "[first_channel, first_channel + n_channels) outside [0, channels]";
    return nullptr;
}

// The channelizer's prototype (sdrg.h): the DDC's low-pass of L - 1 coefficients at f = cutoff_rel / M, then +0
void chan_design(const sdrg_channelizer_config &c, float *h) {
    const int L = c.channels * c.taps_per_channel;
    lowpass_design(c.cutoff_rel / (double)c.channels, L - 1, h);
    h[L - 1] = 0.0f;
}

// The demodulator stage's configuration rules (sdrg.h): nullptr, or what is wrong
const char *demod_check(const sdrg_demod_config &c) {
    if (c.mode != SDRG_DEMOD_AM && c.mode != SDRG_DEMOD_FM) return "mode must be SDRG_DEMOD_AM or SDRG_DEMOD_FM";
    if (!(c.channel_rate_hz > 0.0) || !std::isfinite(c.channel_rate_hz)) return "channel_rate_hz must be > 0 and finite";
    if (c.mode == SDRG_DEMOD_FM) {
        if (!(c.deviation_hz > 0.0) || !std::isfinite(c.deviation_hz)) return "deviation_hz must be > 0 and finite";
        if (!std::isfinite((float)(c.channel_rate_hz / (2.0 * M_PI * c.deviation_hz))))
            return "channel_rate_hz / (2 pi deviation_hz) is not a finite float";
    }
    if (!(c.dc_cutoff_hz >= 0.0) || !std::isfinite(c.dc_cutoff_hz)) return "dc_cutoff_hz must be >= 0 and finite";
    if (!(c.deemphasis_us >= 0.0) || !std::isfinite(c.deemphasis_us)) return "deemphasis_us must be >= 0 and finite";
    if (c.audio_decimation < 1 || c.audio_decimation > SDRG_DEMOD_MAX_DECIMATION) return "audio_decimation outside [1, 64]";
    if (c.audio_taps < 1 || c.audio_taps > SDRG_DEMOD_MAX_TAPS || (c.audio_taps & 1) == 0)
        return "audio_taps must be odd and in [1, 255]";
    if (!(c.audio_cutoff_hz > 0.0 && c.audio_cutoff_hz <= c.channel_rate_hz / 2.0))
        return "audio_cutoff_hz outside (0, channel_rate_hz / 2]";
    if (!std::isfinite(c.gain)) return "gain must be finite";
    if (c.out_format != SDRG_DEMOD_OUT_S16 && c.out_format != SDRG_DEMOD_OUT_F32)
        return "out_format must be SDRG_DEMOD_OUT_S16 or SDRG_DEMOD_OUT_F32";
    if (c.max_in < 1 || c.max_in > SDRG_DEMOD_MAX_IN) return "max_in outside [1, 2^20]";
    return nullptr;
}

// The demodulator stage's constants (sdrg.h), in double, each rounded to float once
void demod_design(const sdrg_demod_config &c, float *kf, float *alpha, float *a, float *h) {
    const double fc = c.channel_rate_hz;
    if (kf) *kf = c.mode == SDRG_DEMOD_FM ? (float)(fc / (2.0 * M_PI * c.deviation_hz)) : 0.0f;
    if (alpha) *alpha = (float)(1.0 - std::exp(-2.0 * M_PI * c.dc_cutoff_hz / fc));
    if (a) *a = c.deemphasis_us > 0.0 ? (float)(1.0 - std::exp(-1.0 / (fc * c.deemphasis_us * 1e-6))) : 0.0f;
    if (h) lowpass_design(c.audio_cutoff_hz / fc, c.audio_taps, h);
}

// The sideband stage's configuration rules (sdrg.h): nullptr, or what is wrong
const char *sideband_check(const sdrg_sideband_config &c) {
    if (!(c.channel_rate_hz > 0.0) || !std::isfinite(c.channel_rate_hz)) return "channel_rate_hz must be > 0 and finite";
    if (!std::isfinite(c.low_hz) || !std::isfinite(c.high_hz)) return "low_hz and high_hz must be finite";
    if (!(c.low_hz >= 0.0 && c.low_hz < c.high_hz && c.high_hz <= c.channel_rate_hz / 2.0))
        return "0 <= low_hz < high_hz <= channel_rate_hz / 2 does not hold";
    if (c.mode != SDRG_SIDEBAND_UPPER && c.mode != SDRG_SIDEBAND_LOWER && c.mode != SDRG_SIDEBAND_BOTH)
        return "mode must be SDRG_SIDEBAND_UPPER, SDRG_SIDEBAND_LOWER or SDRG_SIDEBAND_BOTH";
    if (c.audio_decimation < 1 || c.audio_decimation > SDRG_SIDEBAND_MAX_DECIMATION)
        return "audio_decimation outside [1, 64]";
    if (c.taps < 1 || c.taps > SDRG_SIDEBAND_MAX_TAPS || (c.taps & 1) == 0) return "taps must be odd and in [1, 511]";
    if (c.out_format != SDRG_SIDEBAND_OUT_S16 && c.out_format != SDRG_SIDEBAND_OUT_F32)
        return "out_format must be SDRG_SIDEBAND_OUT_S16 or SDRG_SIDEBAND_OUT_F32";
    if (c.max_in < 1 || c.max_in > SDRG_SIDEBAND_MAX_IN) return "max_in outside [1, 2^20]";
    if (!std::isfinite(c.gain)) return "gain must be finite";
    return nullptr;
}

// The sideband stage's band-pass (sdrg.h): the DDC's low-pass of half the band's width, not rounded, turned to the
// band's middle fm; in double, each component rounded to float once
void sideband_design(const sdrg_sideband_config &c, float *cr, float *ci) {
    const double fc = c.channel_rate_hz, fm = (c.low_hz + c.high_hz) / 2.0;
    const int T = c.taps;
    std::vector<double> v;
    const double sum = lowpass_window((c.high_hz - c.low_hz) / (2.0 * fc), T, v);
    for (int k = 0; k < T; k++) {
        const double p = v[k] / sum;
        const double theta = 2.0 * M_PI * fm * (double)(k - (T - 1) / 2) / fc;
        if (cr) cr[k] = (float)(p * std::cos(theta));
        if (ci) ci[k] = (float)(p * std::sin(theta));
    }
}

// The squelch stage's configuration rules (sdrg.h): nullptr, or what is wrong
const char *squelch_check(const sdrg_squelch_config &c) {
    if (!std::isfinite(c.open_db) || !std::isfinite(c.close_db)) return "open_db and close_db must be finite";
    if (c.close_db > c.open_db) return "close_db above open_db";
    if (!(c.tau_blocks >= 0.0) || !std::isfinite(c.tau_blocks)) return "tau_blocks must be >= 0 and finite";
    if (c.block < SDRG_SQUELCH_MIN_BLOCK || c.block > SDRG_SQUELCH_MAX_BLOCK || (c.block & (c.block - 1)) != 0)
        return "block must be a power of two in [16, 1024]";
    if (c.hang_blocks < 0 || c.hang_blocks > SDRG_SQUELCH_MAX_HANG) return "hang_blocks outside [0, 65535]";
    if (c.max_in < 1 || c.max_in > SDRG_SQUELCH_MAX_IN) return "max_in outside [1, 2^20]";
    float open_thr, close_thr;
    squelch_design(c, &open_thr, &close_thr, nullptr);
    if (!std::isfinite(open_thr) || !(open_thr > 0.0f)) return "10^(open_db / 10) is not a finite, positive float";
    if (!std::isfinite(close_thr) || !(close_thr > 0.0f)) return "10^(close_db / 10) is not a finite, positive float";
    return nullptr;
}

// The squelch stage's constants (sdrg.h), in double, each rounded to float once
void squelch_design(const sdrg_squelch_config &c, float *open_thr, float *close_thr, float *beta) {
    if (open_thr) *open_thr = (float)std::pow(10.0, c.open_db / 10.0);
    if (close_thr) *close_thr = (float)std::pow(10.0, c.close_db / 10.0);
    if (beta) *beta = c.tau_blocks > 0.0 ? (float)(1.0 - std::exp(-1.0 / c.tau_blocks)) : 1.0f;
}

// The IQ correction stage's configuration rules (sdrg.h): nullptr, or what is wrong
const char *iqcorr_check(const sdrg_iqcorr_config &c) {
    if (!(c.dc_tau_blocks >= 0.0) || !std::isfinite(c.dc_tau_blocks)) return "dc_tau_blocks must be >= 0 and finite";
    if (!(c.balance_tau_blocks >= 0.0) || !std::isfinite(c.balance_tau_blocks))
        return "balance_tau_blocks must be >= 0 and finite";
    if (!std::isfinite(c.floor_db)) return "floor_db must be finite";
    if (c.mode == 0 || (c.mode & ~(SDRG_IQCORR_DC | SDRG_IQCORR_BALANCE)) != 0)
        return "mode must be SDRG_IQCORR_DC, SDRG_IQCORR_BALANCE or both";
    if (c.block < SDRG_IQCORR_MIN_BLOCK || c.block > SDRG_IQCORR_MAX_BLOCK || (c.block & (c.block - 1)) != 0)
        return "block must be a power of two in [64, 1024]";
    if (c.max_in < 1 || c.max_in > SDRG_IQCORR_MAX_IN) return "max_in outside [1, 2^20]";
    float floor_thr;
    iqcorr_design(c, nullptr, nullptr, &floor_thr);
    if (!std::isfinite(floor_thr) || !(floor_thr > 0.0f)) return "10^(floor_db / 10) is not a finite, positive float";
    return nullptr;
}

// The IQ correction stage's constants (sdrg.h), in double, each rounded to float once
void iqcorr_design(const sdrg_iqcorr_config &c, float *beta_dc, float *beta_bal, float *floor_thr) {
    if (beta_dc) *beta_dc = c.dc_tau_blocks > 0.0 ? (float)(1.0 - std::exp(-1.0 / c.dc_tau_blocks)) : 1.0f;
    if (beta_bal) *beta_bal = c.balance_tau_blocks > 0.0 ? (float)(1.0 - std::exp(-1.0 / c.balance_tau_blocks)) : 1.0f;
    if (floor_thr) *floor_thr = (float)std::pow(10.0, c.floor_db / 10.0);
}

// The AFC stage's configuration rules (sdrg.h): nullptr, or what is wrong
const char *afc_check(const sdrg_afc_config &c) {
    if (!std::isfinite(c.channel_rate) || !(c.channel_rate > 0.0)) return "channel_rate must be > 0 and finite";
    if (!(c.max_offset_hz > 0.0) || !(c.max_offset_hz <= c.channel_rate / 4.0))
        return "max_offset_hz must be in (0, channel_rate / 4]";
    if (!(c.tau_blocks >= 0.0) || !std::isfinite(c.tau_blocks)) return "tau_blocks must be >= 0 and finite";
    if (!std::isfinite(c.floor_db)) return "floor_db must be finite";
    if (!(c.lock_threshold >= 0.0) || !(c.lock_threshold <= 1.0)) return "lock_threshold must be in [0, 1]";
    if (c.mode != SDRG_AFC_TRACK && c.mode != SDRG_AFC_MEASURE) return "mode must be SDRG_AFC_TRACK or SDRG_AFC_MEASURE";
    if (c.block < SDRG_AFC_MIN_BLOCK || c.block > SDRG_AFC_MAX_BLOCK || (c.block & (c.block - 1)) != 0)
        return "block must be a power of two in [16, 1024]";
    if (c.max_in < 1 || c.max_in > SDRG_AFC_MAX_IN) return "max_in outside [1, 2^20]";
    const float floor_thr = afc_design(c).floor_thr;
    if (!std::isfinite(floor_thr) || !(floor_thr > 0.0f)) return "10^(floor_db / 10) is not a finite, positive float";
    return nullptr;
}

// The AFC stage's constants (sdrg.h), in double, each rounded to float once
sdrg_afc_design_values afc_design(const sdrg_afc_config &c) {
    sdrg_afc_design_values d;
    d.beta = c.tau_blocks > 0.0 ? (float)(1.0 - std::exp(-1.0 / c.tau_blocks)) : 1.0f;
    d.floor_thr = (float)std::pow(10.0, c.floor_db / 10.0);
    d.lock_thr = (float)c.lock_threshold;
    d.max_s = (float)(4294967296.0 * c.max_offset_hz / c.channel_rate);  // at most 2^30: max_offset_hz <= rate / 4
    d.K = (float)(2147483648.0 / M_PI);
    d.hz_per_inc = (float)(c.channel_rate / 4294967296.0);
    d.rad_per_inc = (float)(M_PI / 2147483648.0);
    return d;
}

// The symbol stage's configuration rules (sdrg.h): nullptr, or what is wrong
const char *symbols_check(const sdrg_symbols_config &c) {
    if (!std::isfinite(c.sample_rate) || !(c.sample_rate > 0.0)) return "sample_rate must be > 0 and finite";
    if (!std::isfinite(c.symbol_rate) || !(c.symbol_rate > 0.0)) return "symbol_rate must be > 0 and finite";
    const double sps = c.sample_rate / c.symbol_rate;
    if (!(sps >= 2.0) || !(sps <= 64.0)) return "sample_rate / symbol_rate must be in [2, 64]";
    if (c.levels != 2 && c.levels != 4) return "levels must be 2 or 4";
    if (c.block < SDRG_SYM_MIN_BLOCK || c.block > SDRG_SYM_MAX_BLOCK || (c.block & (c.block - 1)) != 0)
        return "block must be a power of two in [64, 1024]";
    if (!(c.tau_blocks >= 0.0) || !std::isfinite(c.tau_blocks)) return "tau_blocks must be >= 0 and finite";
    if (!(c.tau_level_blocks >= 0.0) || !std::isfinite(c.tau_level_blocks))
        return "tau_level_blocks must be >= 0 and finite";
    if (!std::isfinite(c.floor_db)) return "floor_db must be finite";
    if (!(c.lock_threshold >= 0.0) || !(c.lock_threshold <= 1.0)) return "lock_threshold must be in [0, 1]";
    if (!(c.phase_trim >= -0.5) || !(c.phase_trim <= 0.5)) return "phase_trim must be in [-0.5, 0.5]";
    if (c.level_mode != SDRG_SYM_LEVEL_TRACK && c.level_mode != SDRG_SYM_LEVEL_FIXED)
        return "level_mode must be SDRG_SYM_LEVEL_TRACK or SDRG_SYM_LEVEL_FIXED";
    if (!(c.level_scale > 0.0) || !std::isfinite(c.level_scale)) return "level_scale must be > 0 and finite";
    if (!std::isfinite(c.fixed_centre)) return "fixed_centre must be finite";
    if (!(c.fixed_threshold > 0.0) || !std::isfinite(c.fixed_threshold)) return "fixed_threshold must be > 0 and finite";
    if (c.format != SDRG_SYM_HARD && c.format != SDRG_SYM_SOFT) return "format must be SDRG_SYM_HARD or SDRG_SYM_SOFT";
    if (c.max_in < 1 || c.max_in > SDRG_SYM_MAX_IN) return "max_in outside [1, 2^20]";
    const double inc = std::rint(4294967296.0 * c.symbol_rate / c.sample_rate);
    if (!(inc >= 67108864.0) || !(inc <= 2147483648.0)) return "2^32 symbol_rate / sample_rate outside [2^26, 2^31]";
    const float floor_thr = (float)std::pow(10.0, c.floor_db / 10.0);
    if (!std::isfinite(floor_thr) || !(floor_thr > 0.0f)) return "10^(floor_db / 10) is not a finite, positive float";
    return nullptr;
}

// The symbol stage's constants and table (sdrg.h), in double, each rounded once; cfg has passed symbols_check
sdrg_symbols_design_values symbols_design(const sdrg_symbols_config &c, float *table) {
    sdrg_symbols_design_values d;
    d.trim = (int64_t)std::rint(c.phase_trim * 4294967296.0);
    d.inc = (uint32_t)std::rint(4294967296.0 * c.symbol_rate / c.sample_rate);
    d.rinc = (float)(1.0 / (double)d.inc);
    d.beta = c.tau_blocks > 0.0 ? (float)(1.0 - std::exp(-1.0 / c.tau_blocks)) : 1.0f;
    d.beta_level = c.tau_level_blocks > 0.0 ? (float)(1.0 - std::exp(-1.0 / c.tau_level_blocks)) : 1.0f;
    d.floor_thr = (float)std::pow(10.0, c.floor_db / 10.0);
    d.lock_thr = (float)c.lock_threshold;
    d.K = (float)(2147483648.0 / M_PI);
    d.rs = (float)(1.0 / (double)c.block);
    d.scale = (float)c.level_scale;
    d.centre = (float)c.fixed_centre;
    d.threshold = (float)c.fixed_threshold;
    if (table)
        for (int k = 0; k < SDRG_SYM_TABLE; k++) {
            const double w = 2.0 * M_PI * ((double)k + 0.5) / (double)SDRG_SYM_TABLE;
            table[2 * k] = (float)std::cos(w);
            table[2 * k + 1] = (float)std::sin(w);
        }
    return d;
}

// K(g + n) - K(g), K(g) = floor(inc (g - 1) / 2^32) for g >= 1 and K(0) = 0: inc (g - 1) passes 2^64
uint64_t symbols_count(uint32_t inc, uint64_t g, uint64_t n) {
    const auto K = [inc](unsigned __int128 x) -> unsigned __int128 { return x ? ((x - 1) * inc) >> 32 : 0; };
    return (uint64_t)(K((unsigned __int128)g + n) - K(g));
}

// The noise blanker stage's configuration rules (sdrg.h): nullptr, or what is wrong
const char *blanker_check(const sdrg_blanker_config &c) {
    if (!(c.tau_blocks >= 0.0) || !std::isfinite(c.tau_blocks)) return "tau_blocks must be >= 0 and finite";
    if (!std::isfinite(c.threshold_db)) return "threshold_db must be finite";
    if (!std::isfinite(c.floor_db)) return "floor_db must be finite";
    if (c.block < SDRG_BLANKER_MIN_BLOCK || c.block > SDRG_BLANKER_MAX_BLOCK || (c.block & (c.block - 1)) != 0)
        return "block must be a power of two in [64, 1024]";
    if (c.lead < 0 || c.lead > SDRG_BLANKER_MAX_LEAD) return "lead outside [0, 16]";
    if (c.tail < 0 || c.tail > SDRG_BLANKER_MAX_TAIL) return "tail outside [0, 64]";
    if (c.max_in < 1 || c.max_in > SDRG_BLANKER_MAX_IN) return "max_in outside [1, 2^20]";
    float ratio, floor_thr;
    blanker_design(c, nullptr, &ratio, &floor_thr);
    if (!std::isfinite(ratio) || !(ratio > 0.0f)) return "10^(threshold_db / 10) is not a finite, positive float";
    if (!std::isfinite(floor_thr) || !(floor_thr > 0.0f)) return "10^(floor_db / 10) is not a finite, positive float";
    return nullptr;
}

// The noise blanker stage's constants (sdrg.h), in double, each rounded to float once
void blanker_design(const sdrg_blanker_config &c, float *beta, float *ratio, float *floor_thr) {
    if (beta) *beta = c.tau_blocks > 0.0 ? (float)(1.0 - std::exp(-1.0 / c.tau_blocks)) : 1.0f;
    if (ratio) *ratio = (float)std::pow(10.0, c.threshold_db / 10.0);
    if (floor_thr) *floor_thr = (float)std::pow(10.0, c.floor_db / 10.0);
}

// The tone detector stage's configuration rules (sdrg.h): nullptr, or what is wrong
const char *tones_check(const sdrg_tones_config &c) {
    if (!std::isfinite(c.rate_hz) || !(c.rate_hz > 0.0)) return "rate_hz must be > 0 and finite";
    if (c.components != 1 && c.components != 2) return "components must be 1 or 2";
    if (c.n_tones < 1 || c.n_tones > SDRG_TONES_MAX_TONES) return "n_tones outside [1, 64]";
    for (int k = 0; k < c.n_tones; k++) {
        const double f = c.freq_hz[k];
        if (!std::isfinite(f)) return "freq_hz must be finite";
        if (c.components == 1 && !(f > 0.0 && f < c.rate_hz / 2.0)) return "freq_hz outside (0, rate_hz / 2) at components 1";
        if (c.components == 2 && !(std::fabs(f) <= c.rate_hz / 2.0)) return "|freq_hz| over rate_hz / 2 at components 2";
    }
    if (c.sub_blocks < 1 || c.sub_blocks > SDRG_TONES_MAX_SUB_BLOCKS) return "sub_blocks outside [1, 256]";
    if (c.window != SDRG_TONES_RECT && c.window != SDRG_TONES_HANN) return "unknown window";
    if (!std::isfinite(c.min_db)) return "min_db must be finite";
    if (!std::isfinite(c.dominance_db) || !(c.dominance_db >= 0.0)) return "dominance_db must be >= 0 and finite";
    if (!(c.share >= 0.0 && c.share <= 1.0)) return "share outside [0, 1]";
    if (c.confirm_blocks < 1 || c.confirm_blocks > 255) return "confirm_blocks outside [1, 255]";
    if (c.release_blocks < 0 || c.release_blocks > 255) return "release_blocks outside [0, 255]";
    if (c.max_in < 1 || c.max_in > SDRG_TONES_MAX_IN) return "max_in outside [1, 65536]";
    return nullptr;
}

// The tone detector stage's design (sdrg.h), in double, each result rounded to float once: table [K][S][2], wf [S] and
// the scalars; any pointer may be null
void tones_design(const sdrg_tones_config &c, float *table, float *wf, sdrg_tones_scalars *sc) {
    const int S = 64 * c.sub_blocks, K = c.n_tones;
    std::vector<double> w((size_t)S);
    double W1 = 0.0, W2 = 0.0;
    for (int i = 0; i < S; i++) {
        w[(size_t)i] = c.window == SDRG_TONES_HANN ? 0.5 - 0.5 * std::cos(2.0 * M_PI * (double)(i + 1) / (double)(S + 1)) : 1.0;
        W1 += w[(size_t)i];
        W2 += w[(size_t)i] * w[(size_t)i];
    }
    if (wf)
        for (int i = 0; i < S; i++) wf[i] = (float)w[(size_t)i];
    if (table)
        for (int k = 0; k < K; k++)
            for (int i = 0; i < S; i++) {
                const double t = c.freq_hz[k] * (double)i / c.rate_hz;
                const double theta = 2.0 * M_PI * (t - std::floor(t));
                float *to = table + ((size_t)k * (size_t)S + (size_t)i) * 2;
                to[0] = (float)(w[(size_t)i] * std::cos(theta));
                to[1] = (float)(w[(size_t)i] * std::sin(theta));
            }
    if (sc) {
        const double two = c.components == 1 ? 2.0 : 1.0;
        sc->pnorm = (float)(two * two / (W1 * W1));
        sc->enorm = (float)(two / W2);
        sc->min_power = (float)std::pow(10.0, c.min_db / 10.0);
        sc->dom = (float)std::pow(10.0, c.dominance_db / 10.0);
        sc->share_thr = (float)c.share;
    }
}

// The AGC stage's configuration rules (sdrg.h): nullptr, or what is wrong
const char *agc_check(const sdrg_agc_config &c) {
    if (!std::isfinite(c.target) || !std::isfinite((float)c.target) || !((float)c.target > 0.0f))
        return "target is not a finite, positive float";
    if (!std::isfinite(c.max_gain_db) || !std::isfinite(c.initial_gain_db))
        return "max_gain_db and initial_gain_db must be finite";
    if (std::isnan(c.floor_db) || c.floor_db == INFINITY) return "floor_db must be finite or -INFINITY";
    if (!(c.attack_blocks >= 0.0) || !std::isfinite(c.attack_blocks)) return "attack_blocks must be >= 0 and finite";
    if (!(c.decay_blocks >= 0.0) || !std::isfinite(c.decay_blocks)) return "decay_blocks must be >= 0 and finite";
    if (c.detector != SDRG_AGC_DET_MEAN && c.detector != SDRG_AGC_DET_PEAK)
        return "detector must be SDRG_AGC_DET_MEAN or SDRG_AGC_DET_PEAK";
    if (c.block < SDRG_AGC_MIN_BLOCK || c.block > SDRG_AGC_MAX_BLOCK || (c.block & (c.block - 1)) != 0)
        return "block must be a power of two in [16, 1024]";
    if (c.hang_blocks < 0 || c.hang_blocks > SDRG_AGC_MAX_HANG) return "hang_blocks outside [0, 65535]";
    if (c.max_in < 1 || c.max_in > SDRG_AGC_MAX_IN) return "max_in outside [1, 2^20]";
    const AgcDesign d = agc_design(c);
    if (!std::isfinite(d.max_gain) || !(d.max_gain > 0.0f)) return "10^(max_gain_db / 20) is not a finite, positive float";
    if (!std::isfinite(d.init_gain) || !(d.init_gain > 0.0f))
        return "10^(initial_gain_db / 20) is not a finite, positive float";
    if (d.init_gain > d.max_gain) return "initial_gain_db above max_gain_db";
    if (!std::isfinite(d.floor_thr)) return "10^(floor_db / 10) is not a finite float";
    return nullptr;
}

// The AGC stage's constants (sdrg.h), in double, each rounded to float once
AgcDesign agc_design(const sdrg_agc_config &c) {
    AgcDesign d;
    d.max_gain = (float)std::pow(10.0, c.max_gain_db / 20.0);
    d.init_gain = (float)std::pow(10.0, c.initial_gain_db / 20.0);
    d.floor_thr = (float)std::pow(10.0, c.floor_db / 10.0);  // pow(10, -inf) = +0
    d.alpha_a = c.attack_blocks > 0.0 ? (float)(1.0 - std::exp(-1.0 / c.attack_blocks)) : 1.0f;
    d.alpha_d = c.decay_blocks > 0.0 ? (float)(1.0 - std::exp(-1.0 / c.decay_blocks)) : 1.0f;
    return d;
}

// The resampler stage's configuration rules (sdrg.h): nullptr, or what is wrong
const char *resample_check(const sdrg_resample_config &c) {
    const int L = c.interp, M = c.decim, P = c.taps_per_phase;
    if (L < 1 || L > SDRG_RESAMPLE_MAX_FACTOR) return "interp outside [1, 512]";
    if (M < 1 || M > SDRG_RESAMPLE_MAX_FACTOR) return "decim outside [1, 512]";
    if (std::gcd(L, M) != 1) return "interp and decim have a common factor (sdrg_resample_ratio reduces a ratio)";
    if (L > 8 * M || M > 8 * L) return "interp / decim outside [1/8, 8]";
    if (P < 1 || P > SDRG_RESAMPLE_MAX_TAPS_PER_PHASE) return "taps_per_phase outside [1, 64]";
    if (L * P > SDRG_RESAMPLE_MAX_TAPS) return "interp * taps_per_phase above 8192";
    if (!(c.cutoff_rel > 0.0 && c.cutoff_rel <= 1.0)) return "cutoff_rel outside (0, 1]";
    if (c.components != 1 && c.components != 2) return "components must be 1 (real) or 2 (CF32)";
    if (c.out_format != SDRG_RESAMPLE_OUT_S16 && c.out_format != SDRG_RESAMPLE_OUT_F32)
        return "out_format must be SDRG_RESAMPLE_OUT_S16 or SDRG_RESAMPLE_OUT_F32";
    if (!std::isfinite(c.gain)) return "gain must be finite";
    if (c.max_in < 1 || c.max_in > SDRG_RESAMPLE_MAX_IN) return "max_in outside [1, 2^20]";
    return nullptr;
}

// The resampler's prototype (sdrg.h): the DDC's low-pass of T coefficients (T = L P, less one if that is even) at
// f = cutoff_rel / (2 max(L, M)) cycles per upsampled sample with the DC gain L, then +0
void resample_design(const sdrg_resample_config &c, float *h) {
    const int n = c.interp * c.taps_per_phase, T = (n & 1) ? n : n - 1;
    lowpass_design_scaled(c.cutoff_rel / (2.0 * (double)std::max(c.interp, c.decim)), T, (double)c.interp, h);
    for (int k = T; k < n; k++) h[k] = 0.0f;
}

// L / M = out_hz in_den / in_num in lowest terms, inside the resampler's limits
bool resample_ratio(uint64_t in_num, uint64_t in_den, uint64_t out_hz, int *interp, int *decim) {
    if (in_num == 0 || in_den == 0 || out_hz == 0) return false;
    unsigned __int128 num = (unsigned __int128)out_hz * in_den, den = in_num;
    unsigned __int128 a = num, b = den;
    while (b != 0) {
        const unsigned __int128 t = a % b;
        a = b;
        b = t;
    }
    num /= a;
    den /= a;
    if (num > SDRG_RESAMPLE_MAX_FACTOR || den > SDRG_RESAMPLE_MAX_FACTOR) return false;
    const int L = (int)num, M = (int)den;
    if (L > 8 * M || M > 8 * L) return false;
    *interp = L;
    *decim = M;
    return true;
}

}  // namespace sdrg
