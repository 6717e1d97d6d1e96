// design.h — host-side filter design and window geometry (see design.cpp).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "sdrg_types.h"

namespace sdrg {

void design_lowpass(float fs, float fc, float Q, float c[5]);
void design_highpass(float fs, float f0, float Q, float c[5]);
void design_bandpass(float fs, float f0, float Q, float c[5]);
int design_fir(int64_t in_size, int decim, float cutoff_rel, float *h, int taps0 = 0);
int ssb_decim(uint32_t sample_rate);
int ssb_taps_for(int64_t samp_count, int taps0 = 0);
int ssb_pcm_len(int64_t samp_count, uint32_t sample_rate, int taps0 = 0);
uint32_t nco_increment(double hz, uint32_t sample_rate);
void nco_tables(float *tab);  // [2][1024][2] floats
// DDC stage: the configuration rules (nullptr = valid) and the Hann-sinc low-pass of unit DC gain
const char *ddc_check(uint32_t sample_rate, double offset_hz, double cutoff_hz, int decimation, int taps);
void ddc_design(uint32_t sample_rate, double cutoff_hz, int taps, float *h);
// DDC bank: the configuration rules (nullptr = valid), and the offsets' (count = n_streams * channels values), which a
// retune checks alone
const char *bank_check(uint32_t sample_rate, double cutoff_hz, int decimation, int taps, int channels, int n_streams);
const char *bank_offsets_check(const double *offsets_hz, size_t count);
// the same low-pass at the relative cutoff f = cutoff / rate (cycles per sample)
void lowpass_design(double f, int taps, float *h);
// the same with the DC gain `scale`: h[k] = (float)(scale v[k] / sum), one rounding
void lowpass_design_scaled(double f, int taps, double scale, float *h);
// Channelizer stage: the configuration rules (nullptr = valid) and the prototype, channels * taps_per_channel floats
const char *chan_check(const sdrg_channelizer_config &cfg);
void chan_design(const sdrg_channelizer_config &cfg, float *h);
// Demodulator stage: the configuration rules (nullptr = valid) and kf, alpha, a and the taps (any pointer may be null)
const char *demod_check(const sdrg_demod_config &cfg);
void demod_design(const sdrg_demod_config &cfg, float *kf, float *alpha, float *a, float *h);
// Resampler stage: the configuration rules (nullptr = valid), the prototype, interp * taps_per_phase floats, and the
// reduced ratio out_hz in_den / in_num (false: zero arguments, or outside the stage's limits)
const char *resample_check(const sdrg_resample_config &cfg);
void resample_design(const sdrg_resample_config &cfg, float *h);
bool resample_ratio(uint64_t in_num, uint64_t in_den, uint64_t out_hz, int *interp, int *decim);
// Squelch stage: the configuration rules (nullptr = valid) and open_thr, close_thr and beta (any pointer may be null)
const char *squelch_check(const sdrg_squelch_config &cfg);
void squelch_design(const sdrg_squelch_config &cfg, float *open_thr, float *close_thr, float *beta);
// IQ correction stage: the configuration rules (nullptr = valid) and beta_dc, beta_bal and floor_thr (any pointer may
// be null)
const char *iqcorr_check(const sdrg_iqcorr_config &cfg);
void iqcorr_design(const sdrg_iqcorr_config &cfg, float *beta_dc, float *beta_bal, float *floor_thr);
// AFC stage: the configuration rules (nullptr = valid) and the seven design values
const char *afc_check(const sdrg_afc_config &cfg);
sdrg_afc_design_values afc_design(const sdrg_afc_config &cfg);
// symbol stage: the configuration rules (nullptr = valid), the design values, the table [SDRG_SYM_TABLE][2] (null: not
// wanted), and K(g + n) - K(g), the symbols a call of n values writes at stream position g
const char *symbols_check(const sdrg_symbols_config &cfg);
sdrg_symbols_design_values symbols_design(const sdrg_symbols_config &cfg, float *table);
uint64_t symbols_count(uint32_t inc, uint64_t g, uint64_t n);
const char *blanker_check(const sdrg_blanker_config &cfg);
void blanker_design(const sdrg_blanker_config &cfg, float *beta, float *ratio, float *floor_thr);
// tone detector stage: the configuration rules (nullptr = valid) and the design, table [K][S][2], wf [S] and the five
// scalars (any pointer may be null)
const char *tones_check(const sdrg_tones_config &cfg);
void tones_design(const sdrg_tones_config &cfg, float *table, float *wf, sdrg_tones_scalars *scalars);
// AGC stage: the configuration rules (nullptr = valid) and the five design values (any pointer may be null)
struct AgcDesign {
    float max_gain, init_gain, floor_thr, alpha_a, alpha_d;
};
const char *agc_check(const sdrg_agc_config &cfg);
AgcDesign agc_design(const sdrg_agc_config &cfg);
// Sideband stage: the configuration rules (nullptr = valid) and the band-pass as cr and ci, taps floats each (either
// pointer may be null)
const char *sideband_check(const sdrg_sideband_config &cfg);
void sideband_design(const sdrg_sideband_config &cfg, float *cr, float *ci);
// AudioPulseDetector::makeLP2 / makeHP2 (audio_pulse_detector.cpp:29-55), Q = 0.7071: {b0, b1, b2, a1, a2}
void design_pulse_sos(float fs, float fc, bool highpass, float c[5]);
StatsGeometry stats_geometry(uint32_t sample_rate, uint32_t center_frequency, int n, int focus_khz);

}  // namespace sdrg
