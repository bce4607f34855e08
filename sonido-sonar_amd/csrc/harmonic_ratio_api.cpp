// harmonic_ratio_api.cpp -- sonar_hratio_frames, sonar_hratio_from_spectrum, sonar_hratio and their host-only
// companions: HarmonicRatioAnalyzer (algorithms/tonal/harmonic_ratio.go) for every method of AnalyzeFrame's
// switch.  The host side: NewHarmonicRatioAnalyzer's defaults (:130-161), the argument checks, the Hann
// window and the transform's twiddles as the pitch entries' cached tables, the staged arrays (staging.h),
// the composition of the pitch kernels for ACF and YIN over chunks of windowed frames, and
// postProcessResult + updateTemporalTracking over the raw rows (host::HratioTracker).  The kernels are
// harmonic_ratio_kernels.hip's and pitch_kernels.hip's.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"
#include "host_dsp.h"
#include "harmonic_ratio_kernels.h"
#include "kernels.h"
#include "pitch_kernels.h"
#include "staging.h"

using sonar::HratioOut;
using sonar::detail::fail;
using sonar::detail::Staging;
using sonar::detail::timed_begin;
using sonar::detail::timed_end;

namespace {

constexpr int64_t kChunkFrames = 2048;   // windowed frames (and their correlations) held at once by ACF / YIN

struct Plan {
  int method = 0;                  // HNR (COMB and every unknown value), ACF, HPS, SPECTRAL or YIN
  int nf_method = 0;
  int min_dist = 1;                // the detector's minDistanceBins (spectral_peaks.go:41-43)
  int hps_lo = 0, hps_hi = 0;
  int pct_ok = 1;
};

int check_params(const sonar_hratio_params* p, Plan* pl, std::string& msg) {
  if (!p) { msg = "harmonic ratio: null params"; return SONAR_ERR_INVALID; }
  switch (p->method) {                                               // AnalyzeFrame's switch :228-243
    case SONAR_HRATIO_ACF: case SONAR_HRATIO_HPS: case SONAR_HRATIO_SPECTRAL: case SONAR_HRATIO_YIN:
      pl->method = p->method;
      break;
    default: pl->method = SONAR_HRATIO_HNR; break;
  }
  switch (p->noise_floor_method) {                                   // estimateNoiseFloor's switch :633-642
    case SONAR_HRATIO_NOISE_MEDIAN: case SONAR_HRATIO_NOISE_MINIMUM: pl->nf_method = p->noise_floor_method; break;
    default: pl->nf_method = SONAR_HRATIO_NOISE_PERCENTILE; break;
  }
  if (p->sample_rate < 1 || p->hop_size < 1) {
    msg = "harmonic ratio: hop_size and sample_rate must be at least 1";
    return SONAR_ERR_INVALID;
  }
  if (!(std::isfinite(p->min_freq) && std::isfinite(p->max_freq) && std::isfinite(p->harmonic_tolerance) &&
        std::isfinite(p->min_peak_height))) {
    msg = "harmonic ratio: min_freq, max_freq, harmonic_tolerance and min_peak_height must be finite";
    return SONAR_ERR_INVALID;
  }
  const double pct = p->noise_floor_percentile;
  if (pl->nf_method == SONAR_HRATIO_NOISE_PERCENTILE && pct != pct) {
    msg = "stat: percentile out of bounds";                          // gonum's Quantile, past math.go:39
    return SONAR_ERR_PANIC;
  }
  pl->pct_ok = !(pct < 0 || pct > 1);
  const int W = p->window_size;
  if (!(W >= sonar::PITCH_MIN_W && W <= sonar::PITCH_MAX_W && (W & (W - 1)) == 0)) {
    msg = "harmonic ratio: window_size must be a power of two in [64, 2048]";
    return SONAR_ERR_UNSUPPORTED;
  }
  const double sr = (double)p->sample_rate;
  const double lo = p->min_freq * (double)W / sr, hi = p->max_freq * (double)W / sr;
  if (!(std::fabs(lo) < 2147483648.0 && std::fabs(hi) < 2147483648.0)) {
    msg = "harmonic ratio: the frequency range does not fit an int32 of bins";
    return SONAR_ERR_UNSUPPORTED;
  }
  pl->hps_lo = (int)lo; pl->hps_hi = (int)hi;
  if (pl->method == SONAR_HRATIO_HPS && pl->hps_lo < 0 && pl->hps_hi > pl->hps_lo) {
    msg = "runtime error: index out of range [" + std::to_string(pl->hps_lo) + "]";   // hps[i] :434
    return SONAR_ERR_PANIC;
  }
  if (p->max_harmonics > SONAR_HRATIO_MAX_HARMONICS) {
    msg = "harmonic ratio: max_harmonics above 64";
    return SONAR_ERR_UNSUPPORTED;
  }
  if (p->autocorr_max_lag < W - 1) {
    msg = "harmonic ratio: autocorr_max_lag below window_size - 1";
    return SONAR_ERR_UNSUPPORTED;
  }
  pl->min_dist = std::max((int)(20.0 / (sr / (double)W)), 1);
  return SONAR_OK;
}

// 1 + 2 |len| : 1, the bounds of hrHistory[len(hrHistory) - maxHistory:] at the first frame (:996)
std::string track_panic(int len) {
  return "runtime error: slice bounds out of range [" + std::to_string(1 + 2 * (int64_t)(-(int64_t)len)) + ":1]";
}

struct UserOut {
  double *ratio, *harm_e, *noise_e, *total_e, *f0, *f0_conf, *snr, *periodicity, *harmonicity, *voicing, *roughness;
  int32_t *num, *h_bin;
  double *h_freq, *h_amp, *h_phase, *noise_floor;
};

// the caller's arrays, or scratch that finish() copies to them
HratioOut stage_out(Staging& o, const UserOut& u, int64_t F, int mh, int K) {
  HratioOut d{};
  const size_t f = (size_t)F;
  d.ratio = o.out("r", u.ratio, f); d.harm_e = o.out("he", u.harm_e, f); d.noise_e = o.out("ne", u.noise_e, f);
  d.total_e = o.out("te", u.total_e, f); d.f0 = o.out("f0", u.f0, f); d.f0_conf = o.out("fc", u.f0_conf, f);
  d.snr = o.out("snr", u.snr, f); d.periodicity = o.out("per", u.periodicity, f);
  d.harmonicity = o.out("hty", u.harmonicity, f); d.voicing = o.out("v", u.voicing, f);
  d.roughness = o.out("rg", u.roughness, f); d.num = o.out("num", u.num, f);
  d.h_bin = mh ? o.out("hb", u.h_bin, f * mh) : nullptr;
  d.h_freq = mh ? o.out("hf", u.h_freq, f * mh) : nullptr;
  d.h_amp = mh ? o.out("ha", u.h_amp, f * mh) : nullptr;
  d.h_phase = mh ? o.out("hp", u.h_phase, f * mh) : nullptr;
  d.noise_floor = o.out("nf", u.noise_floor, f * (size_t)K);
  return d;
}

void fill_args(sonar::HratioArgs& a, const sonar_hratio_params* p, const Plan& pl, int64_t F) {
  a.F = F;
  a.W = p->window_size; a.K = p->window_size / 2; a.sr = p->sample_rate; a.method = pl.method;
  a.min_freq = p->min_freq; a.max_freq = p->max_freq; a.tol = p->harmonic_tolerance; a.min_height = p->min_peak_height;
  a.pct = p->noise_floor_percentile; a.pct_ok = pl.pct_ok;
  a.max_h = std::max(p->max_harmonics, 0); a.width = p->peak_detection_width; a.smooth = p->spectral_smoothing_len;
  a.nf_method = pl.nf_method; a.nf_smooth = p->noise_floor_smoothing_len; a.min_dist = pl.min_dist;
  a.hps_lo = pl.hps_lo; a.hps_hi = pl.hps_hi;
}

int launch_rc(sonar_ctx* c, int rc) {
  if (rc == -1) return fail(c, SONAR_ERR_UNSUPPORTED, "harmonic ratio: a shape the kernels do not take");
  if (rc != 0) return fail(c, SONAR_ERR_DEVICE, "harmonic ratio launch failed");
  return SONAR_OK;
}

// ACF and YIN: the outputs the method leaves unset are zeros; the rest comes from the pitch kernels on
// chunks of windowed frames laid out with hop = W
int lag_methods(sonar_ctx* c, const double* dpcm, const sonar_hratio_params* p, const Plan& pl, int64_t F, const HratioOut& d,
                Staging& o) {
  const int W = p->window_size, K = W / 2, mh = std::max(p->max_harmonics, 0);
  const bool acf = pl.method == SONAR_HRATIO_ACF;
  const int64_t CH = std::min<int64_t>(F, kChunkFrames);
  const int width = 2 * W - 1;
  double* frames = o.tmp<double>("frames", (size_t)CH * W);
  double* rp = o.tmp<double>("rawp", (size_t)CH);
  double* rc_ = o.tmp<double>("rawc", (size_t)CH);
  double* curve = acf ? o.tmp<double>("corr", (size_t)CH * width) : nullptr;
  double* stats = acf ? o.tmp<double>("stats", (size_t)CH * 2) : nullptr;
  if (o.nomem) return fail(c, SONAR_ERR_NOMEM, "device allocation failed (harmonic ratio)");
  const double* hann = sonar::detail::pitch_window(c, SONAR_PITCH_WIN_HANN, W);
  // the ACF reads the windowed frame as it is: the rectangular table's x * 1.0 is x
  const double* win2 = acf ? sonar::detail::pitch_window(c, SONAR_PITCH_WIN_RECTANGULAR, W) : hann;
  if (!hann || !win2) return SONAR_ERR_NOMEM;
  const double2* tw = nullptr;
  if (acf && W > 1000) {
    tw = sonar::detail::pitch_twiddles(c, 2 * W);
    if (!tw) return SONAR_ERR_NOMEM;
  }
  struct Z { void* p; size_t bytes; };
  const size_t f = (size_t)F;
  const Z zeros[] = {{d.harm_e, f * 8}, {d.noise_e, f * 8}, {d.total_e, f * 8}, {d.snr, f * 8}, {d.harmonicity, f * 8},
                     {d.roughness, f * 8}, {d.num, f * 4}, {d.h_freq, f * mh * 8}, {d.h_amp, f * mh * 8},
                     {d.h_phase, f * mh * 8}, {d.noise_floor, f * K * 8}, {acf ? d.f0 : nullptr, f * 8},
                     {acf ? d.f0_conf : nullptr, f * 8}};
  for (const Z& z : zeros)
    if (z.p && z.bytes) HIP_TRY(c, hipMemsetAsync(z.p, 0, z.bytes, c->stream));
  if (d.h_bin && mh) HIP_TRY(c, hipMemsetAsync(d.h_bin, 0xff, f * mh * 4, c->stream));   // -1
  for (int64_t f0 = 0; f0 < F; f0 += CH) {
    const int64_t nf = std::min(CH, F - f0);
    int rc = launch_rc(c, sonar::launch_hratio_window(dpcm, p->hop_size, W, hann, f0, nf, frames, c->stream));
    if (rc != SONAR_OK) return rc;
    sonar::PitchArgs a{};
    a.pcm = frames; a.n = nf * W; a.F = nf; a.hop = W;
    a.W = W; a.sr = p->sample_rate; a.method = acf ? SONAR_PITCH_ACF : SONAR_PITCH_YIN; a.pre = 0; a.zp = 0; a.K = 0;
    a.win = win2; a.tw = tw;
    a.min_freq = p->min_freq; a.max_freq = p->max_freq; a.yin_thr = 0.0; a.ac_thr = 0.0;
    a.pitch = rp; a.conf = rc_;
    a.stats = stats; a.curve = curve; a.width = acf ? width : W / 2;
    rc = launch_rc(c, sonar::launch_pitch_frames(a, c->stream));
    if (rc != SONAR_OK) return rc;
    rc = launch_rc(c, acf ? sonar::launch_hratio_acf_tail(curve, width, f0, nf, d, c->stream)
                          : sonar::launch_hratio_yin_tail(rp, rc_, f0, nf, d, c->stream));
    if (rc != SONAR_OK) return rc;
  }
  return SONAR_OK;
}

int frames_impl(sonar_ctx* c, const double* pcm, int64_t n, const sonar_hratio_params* p, const UserOut& u, bool pcm_dev,
                bool out_dev, int64_t* frames) {
  Plan pl;
  std::string msg;
  const int prc = check_params(p, &pl, msg);
  if (prc != SONAR_OK) return fail(c, prc, msg);
  if (n < 0) return fail(c, SONAR_ERR_INVALID, "harmonic ratio: negative sample count");
  const int W = p->window_size;
  const int64_t F = sonar_pitch_detect_frames(n, W, p->hop_size);
  if (frames) *frames = F;
  if (F == 0) return SONAR_OK;
  if (F > 2147483647) return fail(c, SONAR_ERR_UNSUPPORTED, "harmonic ratio: more than 2^31 - 1 frames");
  if (!pcm) return fail(c, SONAR_ERR_INVALID, "harmonic ratio: null pcm pointer");
  HIP_TRY(c, hipSetDevice(c->device));
  Staging in{c, "hratio.", pcm_dev}, o{c, "hratio.", out_dev};
  const double* dpcm = in.in("pcm", pcm, (size_t)n);
  const HratioOut d = stage_out(o, u, F, std::max(p->max_harmonics, 0), W / 2);
  if (in.nomem || o.nomem) return fail(c, SONAR_ERR_NOMEM, "device allocation failed (harmonic ratio)");
  int rc = SONAR_OK;
  if (pl.method == SONAR_HRATIO_ACF || pl.method == SONAR_HRATIO_YIN) {
    rc = in.ready("device allocation failed (harmonic ratio)");
    if (rc != SONAR_OK) return rc;
    hipEvent_t tend = timed_begin(c, c->stream);
    rc = lag_methods(c, dpcm, p, pl, F, d, o);
    if (rc != SONAR_OK) return rc;
    timed_end(c, c->stream, tend);
    return o.finish();
  }
  sonar::HratioArgs a{};
  fill_args(a, p, pl, F);
  a.pcm = dpcm; a.n = n; a.hop = p->hop_size;
  a.o = d;
  a.win = sonar::detail::pitch_window(c, SONAR_PITCH_WIN_HANN, W);
  a.tw = sonar::detail::pitch_twiddles(c, W);
  if (!a.win || !a.tw) return SONAR_ERR_NOMEM;
  rc = in.ready("device allocation failed (harmonic ratio)");
  if (rc != SONAR_OK) return rc;
  hipEvent_t tend = timed_begin(c, c->stream);
  rc = launch_rc(c, sonar::launch_hratio(a, c->stream));
  if (rc != SONAR_OK) return rc;
  timed_end(c, c->stream, tend);
  return o.finish();
}

UserOut user_out(double* ratio, double* harm_e, double* noise_e, double* total_e, double* f0, double* f0_conf, double* snr,
                 double* periodicity, double* harmonicity, double* voicing, double* roughness, int32_t* num, int32_t* h_bin,
                 double* h_freq, double* h_amp, double* h_phase, double* noise_floor) {
  return UserOut{ratio, harm_e, noise_e, total_e, f0, f0_conf, snr, periodicity, harmonicity, voicing, roughness, num, h_bin,
                 h_freq, h_amp, h_phase, noise_floor};
}

}  // namespace

extern "C" {

void sonar_hratio_params_default(sonar_hratio_params* p, int32_t sample_rate) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->method = SONAR_HRATIO_HNR;
  p->sample_rate = sample_rate;
  p->window_size = 2048;
  p->hop_size = 512;
  p->min_freq = 80.0;
  p->max_freq = 8000.0;
  p->max_harmonics = 20;
  p->harmonic_tolerance = 0.1;
  p->min_peak_height = 0.001;
  p->peak_detection_width = 3;
  p->spectral_smoothing_len = 5;
  p->noise_floor_method = SONAR_HRATIO_NOISE_PERCENTILE;
  p->noise_floor_percentile = 0.1;
  p->noise_floor_smoothing_len = 10;
  p->use_temporal_smoothing = 1;
  p->temporal_smoothing_len = 5;
  p->autocorr_max_lag = 2048;
}

int sonar_hratio_check(const sonar_hratio_params* p) {
  Plan pl;
  std::string msg;
  return check_params(p, &pl, msg);
}

int sonar_hratio_from_spectrum(sonar_ctx* c, const double* mag, const double* phase, int64_t F, int32_t K,
                               const sonar_hratio_params* p, double* harmonic_ratio, double* harmonic_energy,
                               double* noise_energy, double* total_energy, double* f0, double* f0_confidence, double* snr,
                               double* periodicity, double* harmonicity, double* voicing, double* roughness,
                               int32_t* num_harmonics, int32_t* h_bin, double* h_freq, double* h_amp, double* h_phase,
                               double* noise_floor, int32_t device_ptrs) {
  if (!c) return SONAR_ERR_INVALID;
  Plan pl;
  std::string msg;
  const int prc = check_params(p, &pl, msg);
  if (prc != SONAR_OK) return fail(c, prc, msg);
  if (pl.method == SONAR_HRATIO_ACF || pl.method == SONAR_HRATIO_YIN)
    return fail(c, SONAR_ERR_INVALID, "harmonic ratio: the ACF and YIN methods need the samples (sonar_hratio_frames)");
  if (K != p->window_size / 2) return fail(c, SONAR_ERR_INVALID, "harmonic ratio: K must be window_size / 2");
  if (F < 0) return fail(c, SONAR_ERR_INVALID, "harmonic ratio: negative frame count");
  if (F == 0) return SONAR_OK;
  if (F > 2147483647) return fail(c, SONAR_ERR_UNSUPPORTED, "harmonic ratio: more than 2^31 - 1 frames");
  if (!mag) return fail(c, SONAR_ERR_INVALID, "harmonic ratio: null magnitude pointer");
  HIP_TRY(c, hipSetDevice(c->device));
  const bool dev = device_ptrs != 0;
  Staging in{c, "hratio.", dev}, o{c, "hratio.", dev};
  sonar::HratioArgs a{};
  fill_args(a, p, pl, F);
  a.mag = in.in("mag", mag, (size_t)F * K);
  a.phase = in.in("phase", phase, (size_t)F * K);
  a.o = stage_out(o, user_out(harmonic_ratio, harmonic_energy, noise_energy, total_energy, f0, f0_confidence, snr,
                              periodicity, harmonicity, voicing, roughness, num_harmonics, h_bin, h_freq, h_amp, h_phase,
                              noise_floor),
                  F, a.max_h, K);
  int rc = in.nomem || o.nomem ? fail(c, SONAR_ERR_NOMEM, "device allocation failed (harmonic ratio)")
                               : in.ready("device allocation failed (harmonic ratio)");
  if (rc != SONAR_OK) return rc;
  hipEvent_t tend = timed_begin(c, c->stream);
  rc = launch_rc(c, sonar::launch_hratio(a, c->stream));
  if (rc != SONAR_OK) return rc;
  timed_end(c, c->stream, tend);
  return o.finish();
}

int sonar_hratio_frames(sonar_ctx* c, const double* pcm, int64_t n, const sonar_hratio_params* p, double* harmonic_ratio,
                        double* harmonic_energy, double* noise_energy, double* total_energy, double* f0,
                        double* f0_confidence, double* snr, double* periodicity, double* harmonicity, double* voicing,
                        double* roughness, int32_t* num_harmonics, int32_t* h_bin, double* h_freq, double* h_amp,
                        double* h_phase, double* noise_floor, int32_t device_ptrs) {
  if (!c) return SONAR_ERR_INVALID;
  const UserOut u = user_out(harmonic_ratio, harmonic_energy, noise_energy, total_energy, f0, f0_confidence, snr, periodicity,
                             harmonicity, voicing, roughness, num_harmonics, h_bin, h_freq, h_amp, h_phase, noise_floor);
  return frames_impl(c, pcm, n, p, u, device_ptrs != 0, device_ptrs != 0, nullptr);
}

int sonar_hratio_track(const sonar_hratio_params* p, int64_t F, const double* raw_harmonic_ratio, const double* raw_f0,
                       double* harmonic_ratio, double* temporal_stability, double* temporal_coherence) {
  (void)raw_f0;                                                        // f0History (:991) is never read
  if (!p || F < 0) return SONAR_ERR_INVALID;
  if (F == 0) return SONAR_OK;
  if (!raw_harmonic_ratio) return SONAR_ERR_INVALID;
  if (p->temporal_smoothing_len < 0) return SONAR_ERR_PANIC;           // :996 at the first frame
  sonar::host::HratioTracker tr;
  for (int64_t f = 0; f < F; ++f) {
    const sonar::host::HratioRow r = tr.step(p->use_temporal_smoothing != 0, p->temporal_smoothing_len, raw_harmonic_ratio[f]);
    if (harmonic_ratio) harmonic_ratio[f] = r.ratio;
    if (temporal_stability) temporal_stability[f] = r.stability;
    if (temporal_coherence) temporal_coherence[f] = r.coherence;
  }
  return SONAR_OK;
}

int sonar_hratio(sonar_ctx* c, const double* pcm, int64_t n, const sonar_hratio_params* p, double* harmonic_ratio,
                 double* temporal_stability, double* temporal_coherence, double* harmonic_energy, double* noise_energy,
                 double* total_energy, double* f0, double* f0_confidence, double* snr, double* periodicity,
                 double* harmonicity, double* voicing, double* roughness, int32_t* num_harmonics, int32_t* h_bin,
                 double* h_freq, double* h_amp, double* h_phase, double* noise_floor, int64_t* frames, int32_t device_ptrs) {
  if (!c) return SONAR_ERR_INVALID;
  if (frames) *frames = 0;
  Plan pl;
  std::string msg;
  const int prc = check_params(p, &pl, msg);
  if (prc != SONAR_OK) return fail(c, prc, msg);
  if (n < 0) return fail(c, SONAR_ERR_INVALID, "harmonic ratio: negative sample count");
  const int64_t F0 = sonar_pitch_detect_frames(n, p->window_size, p->hop_size);
  if (F0 > 0 && p->temporal_smoothing_len < 0) return fail(c, SONAR_ERR_PANIC, track_panic(p->temporal_smoothing_len));
  const bool dev = device_ptrs != 0;
  // the raw ratios come to the host for the tracker (with device pointers through library scratch); every
  // other output goes where the caller wants it
  std::vector<double> raw((size_t)F0);
  int64_t F = 0;
  UserOut u = user_out(nullptr, harmonic_energy, noise_energy, total_energy, f0, f0_confidence, snr, periodicity, harmonicity,
                       voicing, roughness, num_harmonics, h_bin, h_freq, h_amp, h_phase, noise_floor);
  double* dr = nullptr;
  if (dev && F0) {
    dr = (double*)sonar::detail::dbuf(c, "hratio.rawratio", (size_t)F0 * sizeof(double));
    if (!dr) return fail(c, SONAR_ERR_NOMEM, "device allocation failed (harmonic ratio)");
  }
  u.ratio = dev ? dr : raw.data();
  int rc = frames_impl(c, pcm, n, p, u, dev, dev, &F);
  if (rc != SONAR_OK) return rc;
  if (dev && F) {
    HIP_TRY(c, hipMemcpyAsync(raw.data(), dr, (size_t)F * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  if (frames) *frames = F;
  if (F == 0) return SONAR_OK;
  std::vector<double> h((size_t)F * 3);
  rc = sonar_hratio_track(p, F, raw.data(), nullptr, h.data(), h.data() + F, h.data() + 2 * F);
  if (rc != SONAR_OK) return fail(c, rc, "harmonic ratio: tracker arguments");
  double* outs[3] = {harmonic_ratio, temporal_stability, temporal_coherence};
  Staging o{c, "hratio.", dev};
  for (int k = 0; k < 3 && rc == SONAR_OK; ++k) rc = o.put(outs[k], h.data() + (size_t)k * F, (size_t)F * 8);
  return rc != SONAR_OK || !o.dev ? rc : o.finish();
}

double sonar_hratio_average(const double* hr, int64_t n) {
  if (!hr || n <= 0) return 0.0;
  double sum = 0.0;
  int64_t count = 0;
  for (int64_t i = 0; i < n; ++i)
    if (hr[i] > -60.0) { sum += hr[i]; ++count; }
  return count > 0 ? sum / (double)count : 0.0;
}

int32_t sonar_hratio_classify(double hr) {
  if (hr >= 20.0) return SONAR_HRATIO_VERY_HIGH;
  if (hr >= 10.0) return SONAR_HRATIO_HIGH;
  if (hr >= 5.0) return SONAR_HRATIO_MEDIUM;
  if (hr >= 0.0) return SONAR_HRATIO_LOW;
  return SONAR_HRATIO_VERY_LOW;
}

const char* sonar_hratio_category_name(int32_t category) {
  static const char* const names[] = {"Very Low", "Low", "Medium", "High", "Very High"};
  return category >= 0 && category <= SONAR_HRATIO_VERY_HIGH ? names[category] : nullptr;
}

double sonar_hratio_voicing_quality(double hr) { return 1.0 / (1.0 + std::exp(-0.1 * (hr - 5.0))); }

}  // extern "C"
