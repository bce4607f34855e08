// inharmonicity_api.cpp -- sonar_inharm_from_spectrum, sonar_inharm_frames, sonar_inharm and their host-only
// companions: InharmonicityAnalyzer (algorithms/tonal/inharmonicity.go).  The host side:
// NewInharmonicityAnalyzer's defaults (:147-172), the argument checks, fitRailsbackCurve's grid of B as a
// cached table, the f0 of each frame from the default PitchDetector (sonar_pitch_detect on the staged
// samples), the staged arrays (staging.h), and postProcessResult + updateTemporalTracking over the raw rows
// (host::InharmTracker).  The kernel is inharmonicity_kernels.hip's.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"
#include "harmonic_ratio_kernels.h"
#include "host_dsp.h"
#include "inharmonicity_kernels.h"
#include "kernels.h"
#include "pitch_kernels.h"
#include "staging.h"

using sonar::InharmOut;
using sonar::detail::fail;
using sonar::detail::Staging;
using sonar::detail::timed_begin;
using sonar::detail::timed_end;

namespace {

constexpr int64_t kChunkFrames = 2048;   // raw frames (and their correlations) held at once by BeatPattern
constexpr int kDetectorWindow = 1024;    // NewPitchDetector's WindowSize (pitch_detection.go:163)

int check_params(const sonar_inharm_params* p, int W, int* method, std::string& msg) {
  if (!p) { msg = "inharmonicity: null params"; return SONAR_ERR_INVALID; }
  switch (p->method) {                                               // AnalyzeFrame's switch :252-267
    case SONAR_INHARM_RAILSBACK: case SONAR_INHARM_FLETCHER_MUNSON: case SONAR_INHARM_STATISTICAL:
    case SONAR_INHARM_BEAT_PATTERN:
      *method = p->method;
      break;
    default: *method = SONAR_INHARM_SPECTRAL_DEVIATION; break;
  }
  if (p->sample_rate < 1) { msg = "inharmonicity: sample_rate must be at least 1"; return SONAR_ERR_INVALID; }
  if (!(std::isfinite(p->min_freq) && std::isfinite(p->max_freq) && std::isfinite(p->harmonic_tolerance) &&
        std::isfinite(p->min_harmonic_strength))) {
    msg = "inharmonicity: min_freq, max_freq, harmonic_tolerance and min_harmonic_strength must be finite";
    return SONAR_ERR_INVALID;
  }
  if (p->max_harmonics > SONAR_INHARM_MAX_HARMONICS) {
    msg = "inharmonicity: max_harmonics above 64";
    return SONAR_ERR_UNSUPPORTED;
  }
  const double reach = p->max_freq * (1.0 + std::fabs(p->harmonic_tolerance)) * (double)W / (double)p->sample_rate;
  if (!(std::fabs(reach) < 2147483648.0)) {
    msg = "inharmonicity: the search window does not fit an int32 of bins";
    return SONAR_ERR_UNSUPPORTED;
  }
  return SONAR_OK;
}

// inharmonicityHistory[len - maxHistory:] at the first tracked frame (:1098): len is 1
std::string track_panic(int window) {
  return "runtime error: slice bounds out of range [" + std::to_string(1 - (int64_t)window) + ":1]";
}

// for b := -0.01; b <= 0.01; b += 0.0001 (:640): the 201 values the float64 additions give
const double* railsback_grid(sonar_ctx* c) {
  const unsigned char* t = nullptr;
  const int rc = sonar::detail::cached_table(c, "inharm.grid", "inharmonicity grid",
      [&](std::vector<unsigned char>& img, int64_t&) {
        img.resize((size_t)sonar::INHARM_GRID * sizeof(double));
        double* g = (double*)img.data();
        int k = 0;
        for (double b = -0.01; b <= 0.01 && k < sonar::INHARM_GRID; b += 0.0001) g[k++] = b;
        return k == sonar::INHARM_GRID ? SONAR_OK : SONAR_ERR_DEVICE;
      }, &t);
  return rc == SONAR_OK ? (const double*)t : nullptr;
}

struct UserOut {
  int32_t* status;
  double *inh, *std_dev, *conf, *f0, *f0_conf;
  int32_t *num, *ndev, *h_number;
  double *h_freq, *h_ideal, *h_amp, *h_dev, *stiffness, *fit, *clarity, *purity, *coherence, *r2, *chi2, *pval;
  int32_t* quality;
};

// the caller's arrays, or scratch that finish() copies to them
InharmOut stage_out(Staging& o, const UserOut& u, int64_t F, int mh) {
  InharmOut d{};
  const size_t f = (size_t)F;
  d.status = o.out("st", u.status, f); d.inh = o.out("inh", u.inh, f); d.std_dev = o.out("sd", u.std_dev, f);
  d.conf = o.out("cf", u.conf, f); d.f0 = o.out("f0", u.f0, f); d.f0_conf = o.out("fc", u.f0_conf, f);
  d.num = o.out("num", u.num, f); d.ndev = o.out("nd", u.ndev, f);
  d.h_number = mh ? o.out("hn", u.h_number, f * mh) : nullptr;
  d.h_freq = mh ? o.out("hf", u.h_freq, f * mh) : nullptr;
  d.h_ideal = mh ? o.out("hi", u.h_ideal, f * mh) : nullptr;
  d.h_amp = mh ? o.out("ha", u.h_amp, f * mh) : nullptr;
  d.h_dev = mh ? o.out("hd", u.h_dev, f * mh) : nullptr;
  d.stiffness = o.out("es", u.stiffness, f); d.fit = o.out("fit", u.fit, f); d.clarity = o.out("cl", u.clarity, f);
  d.purity = o.out("pu", u.purity, f); d.coherence = o.out("co", u.coherence, f); d.r2 = o.out("r2", u.r2, f);
  d.chi2 = o.out("chi", u.chi2, f); d.pval = o.out("pv", u.pval, f); d.quality = o.out("q", u.quality, f);
  return d;
}

void fill_args(sonar::InharmArgs& a, const sonar_inharm_params* p, int method, int W, int64_t F) {
  a.F = F;
  a.W = W; a.K = W / 2; a.sr = p->sample_rate; a.method = method; a.model = p->model;
  a.max_h = p->max_harmonics; a.min_h = p->min_harmonics; a.slots = std::max(p->max_harmonics, 0);
  a.tol = p->harmonic_tolerance; a.strength = p->min_harmonic_strength; a.min_freq = p->min_freq; a.max_freq = p->max_freq;
  a.tension = p->string_tension; a.length = p->string_length; a.outlier = p->outlier_threshold;
  a.weight = p->weight_by_amplitude != 0; a.robust = p->use_robust_estimation != 0;
}

int launch_rc(sonar_ctx* c, int rc) {
  if (rc == -1) return fail(c, SONAR_ERR_UNSUPPORTED, "inharmonicity: a shape the kernel does not take");
  if (rc != 0) return fail(c, SONAR_ERR_DEVICE, "inharmonicity launch failed");
  return SONAR_OK;
}

// calculateBeatPatternInharmonicity (:552-573): NewAutoCorrelation(W).Compute of the raw frame (the pitch ACF
// kernels on chunks of frames laid out with hop = W, the rectangular table's x * 1.0 being x), then the tail
int beat_pattern(sonar_ctx* c, const double* dpcm, int64_t hop, int W, int sr, int64_t F, double* beat, Staging& o) {
  const int64_t CH = std::min<int64_t>(F, kChunkFrames);
  const int width = 2 * W - 1;
  double* frames = o.tmp<double>("frames", (size_t)CH * W);
  double* rp = o.tmp<double>("rawp", (size_t)CH);
  double* rc_ = o.tmp<double>("rawc", (size_t)CH);
  double* curve = o.tmp<double>("corr", (size_t)CH * width);
  double* stats = o.tmp<double>("stats", (size_t)CH * 2);
  if (o.nomem) return fail(c, SONAR_ERR_NOMEM, "device allocation failed (inharmonicity)");
  const double* rect = sonar::detail::pitch_window(c, SONAR_PITCH_WIN_RECTANGULAR, W);
  const double2* tw = W > 1000 ? sonar::detail::pitch_twiddles(c, 2 * W) : nullptr;
  if (!rect || (W > 1000 && !tw)) return SONAR_ERR_NOMEM;
  for (int64_t f0 = 0; f0 < F; f0 += CH) {
    const int64_t nf = std::min(CH, F - f0);
    int rc = launch_rc(c, sonar::launch_hratio_window(dpcm, hop, W, rect, f0, nf, frames, c->stream));
    if (rc != SONAR_OK) return rc;
    sonar::PitchArgs a{};
    a.pcm = frames; a.n = nf * W; a.F = nf; a.hop = W;
    a.W = W; a.sr = sr; a.method = SONAR_PITCH_ACF; a.pre = 0; a.zp = 0; a.K = 0;
    a.win = rect; a.tw = tw;
    a.min_freq = 80.0; a.max_freq = 1000.0; a.yin_thr = 0.0; a.ac_thr = 0.0;   // of the peak pick, which nothing reads
    a.pitch = rp; a.conf = rc_;
    a.stats = stats; a.curve = curve; a.width = width;
    rc = launch_rc(c, sonar::launch_pitch_frames(a, c->stream));
    if (rc != SONAR_OK) return rc;
    rc = launch_rc(c, sonar::launch_inharm_beat_tail(curve, width, f0, nf, beat, c->stream));
    if (rc != SONAR_OK) return rc;
  }
  return SONAR_OK;
}

int frames_impl(sonar_ctx* c, const double* pcm, int64_t n, int32_t hop, const sonar_inharm_params* p, const UserOut& u,
                bool dev, int64_t* frames) {
  int method = 0;
  std::string msg;
  const int prc = check_params(p, p ? p->window_size : 0, &method, msg);
  if (prc != SONAR_OK) return fail(c, prc, msg);
  if (n < 0) return fail(c, SONAR_ERR_INVALID, "inharmonicity: negative sample count");
  if (hop < 1) return fail(c, SONAR_ERR_INVALID, "inharmonicity: hop_size must be at least 1");
  const int W = p->window_size;
  const int64_t F = sonar_pitch_detect_frames(n, W, hop);
  if (frames) *frames = F;
  if (F == 0) return SONAR_OK;
  if (W != kDetectorWindow)                                            // pitch_detection.go:226 under :231
    return fail(c, SONAR_ERR_INVALID, "audio frame size (" + std::to_string(W) + ") doesn't match window size (" +
                                          std::to_string(kDetectorWindow) + ")");
  if (F > 2147483647) return fail(c, SONAR_ERR_UNSUPPORTED, "inharmonicity: more than 2^31 - 1 frames");
  if (!pcm) return fail(c, SONAR_ERR_INVALID, "inharmonicity: null pcm pointer");
  HIP_TRY(c, hipSetDevice(c->device));
  Staging in{c, "inharm.", dev}, o{c, "inharm.", dev};
  const double* dpcm = in.in("pcm", pcm, (size_t)n);
  double* df0 = in.tmp<double>("pitch", (size_t)F);
  double* dfc = in.tmp<double>("pitchconf", (size_t)F);
  sonar::InharmArgs a{};
  fill_args(a, p, method, W, F);
  a.o = stage_out(o, u, F, a.slots);
  if (in.nomem || o.nomem) return fail(c, SONAR_ERR_NOMEM, "device allocation failed (inharmonicity)");
  a.tw = sonar::detail::pitch_twiddles(c, W);
  a.grid = railsback_grid(c);
  if (!a.tw || !a.grid) return SONAR_ERR_NOMEM;
  int rc = in.ready("device allocation failed (inharmonicity)");
  if (rc != SONAR_OK) return rc;
  // detectFundamentalFrequency (:308-316): the analyzer's own detector at NewPitchDetector's parameters, its
  // history running over every frame
  sonar_pitch_params pp;
  sonar_pitch_params_default(&pp, p->sample_rate);
  pp.hop_size = hop;
  int64_t Fp = 0;
  rc = sonar_pitch_detect(c, dpcm, n, &pp, df0, dfc, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &Fp, 1);
  if (rc != SONAR_OK) return rc;
  if (Fp != F) return fail(c, SONAR_ERR_DEVICE, "inharmonicity: the detector's frame count differs");
  a.pcm = dpcm; a.n = n; a.hop = hop;
  a.f0 = df0; a.f0_conf = dfc;
  hipEvent_t tend = timed_begin(c, c->stream);
  if (method == SONAR_INHARM_BEAT_PATTERN) {
    double* beat = in.tmp<double>("beat", (size_t)F);
    if (!beat) return fail(c, SONAR_ERR_NOMEM, "device allocation failed (inharmonicity)");
    rc = beat_pattern(c, dpcm, hop, W, p->sample_rate, F, beat, in);
    if (rc != SONAR_OK) return rc;
    a.beat = beat;
  }
  rc = launch_rc(c, sonar::launch_inharm(a, c->stream));
  if (rc != SONAR_OK) return rc;
  timed_end(c, c->stream, tend);
  return o.finish();
}

}  // namespace

extern "C" {

void sonar_inharm_params_default(sonar_inharm_params* p, int32_t sample_rate) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->method = SONAR_INHARM_SPECTRAL_DEVIATION;
  p->model = SONAR_INHARM_MODEL_GENERAL;
  p->sample_rate = sample_rate;
  p->window_size = 4096;
  p->max_harmonics = 20;
  p->min_harmonics = 3;
  p->harmonic_tolerance = 0.05;
  p->min_harmonic_strength = 0.01;
  p->min_freq = 80.0;
  p->max_freq = 2000.0;
  p->freq_resolution = 1.0;
  p->reference_harmonic = 1;
  p->weight_by_amplitude = 1;
  p->use_log_frequency = 0;
  p->string_tension = 1.0;
  p->string_length = 1.0;
  p->string_stiffness = 0.001;
  p->outlier_threshold = 2.0;
  p->confidence_level = 0.95;
  p->use_robust_estimation = 1;
  p->use_temporal_tracking = 0;
  p->temporal_window = 10;
}

int sonar_inharm_check(const sonar_inharm_params* p) {
  int method = 0;
  std::string msg;
  return check_params(p, p ? p->window_size : 0, &method, msg);
}

int sonar_inharm_from_spectrum(sonar_ctx* c, const double* mag, const double* f0, const double* f0_confidence, int64_t F,
                               int32_t K, const sonar_inharm_params* p, int32_t* status, double* inharmonicity,
                               double* std_dev, double* confidence, double* f0_out, double* f0_confidence_out,
                               int32_t* num_harmonics, int32_t* n_deviations, int32_t* h_number, double* h_freq,
                               double* h_ideal, double* h_amp, double* h_deviation, double* estimated_stiffness,
                               double* model_fit_quality, double* harmonic_clarity, double* spectral_purity,
                               double* partial_coherence, double* r_squared, double* chi_squared, double* p_value,
                               int32_t* quality, int32_t device_ptrs) {
  if (!c) return SONAR_ERR_INVALID;
  if (K < 4 || K > sonar::INHARM_MAX_K) return fail(c, SONAR_ERR_INVALID, "inharmonicity: K must be in [4, 4096]");
  int method = 0;
  std::string msg;
  const int prc = check_params(p, 2 * K, &method, msg);
  if (prc != SONAR_OK) return fail(c, prc, msg);
  if (method == SONAR_INHARM_BEAT_PATTERN)
    return fail(c, SONAR_ERR_INVALID, "inharmonicity: the BeatPattern method needs the samples (sonar_inharm_frames)");
  if (F < 0) return fail(c, SONAR_ERR_INVALID, "inharmonicity: negative frame count");
  if (F == 0) return SONAR_OK;
  if (F > 2147483647) return fail(c, SONAR_ERR_UNSUPPORTED, "inharmonicity: more than 2^31 - 1 frames");
  if (!mag || !f0 || !f0_confidence) return fail(c, SONAR_ERR_INVALID, "inharmonicity: null input pointer");
  const bool dev = device_ptrs != 0;
  if (!dev)
    for (int64_t f = 0; f < F; ++f)
      if (!std::isfinite(f0[f])) return fail(c, SONAR_ERR_INVALID, "inharmonicity: non-finite f0");
  HIP_TRY(c, hipSetDevice(c->device));
  Staging in{c, "inharm.", dev}, o{c, "inharm.", dev};
  sonar::InharmArgs a{};
  fill_args(a, p, method, 2 * K, F);
  a.mag = in.in("mag", mag, (size_t)F * K);
  a.f0 = in.in("f0in", f0, (size_t)F);
  a.f0_conf = in.in("fcin", f0_confidence, (size_t)F);
  const UserOut u{status, inharmonicity, std_dev, confidence, f0_out, f0_confidence_out, num_harmonics, n_deviations,
                  h_number, h_freq, h_ideal, h_amp, h_deviation, estimated_stiffness, model_fit_quality, harmonic_clarity,
                  spectral_purity, partial_coherence, r_squared, chi_squared, p_value, quality};
  a.o = stage_out(o, u, F, a.slots);
  if (in.nomem || o.nomem) return fail(c, SONAR_ERR_NOMEM, "device allocation failed (inharmonicity)");
  a.grid = railsback_grid(c);
  if (!a.grid) return SONAR_ERR_NOMEM;
  int rc = in.ready("device allocation failed (inharmonicity)");
  if (rc != SONAR_OK) return rc;
  hipEvent_t tend = timed_begin(c, c->stream);
  rc = launch_rc(c, sonar::launch_inharm(a, c->stream));
  if (rc != SONAR_OK) return rc;
  timed_end(c, c->stream, tend);
  return o.finish();
}

int sonar_inharm_frames(sonar_ctx* c, const double* pcm, int64_t n, int32_t hop_size, const sonar_inharm_params* p,
                        int32_t* status, double* inharmonicity, double* std_dev, double* confidence, double* f0,
                        double* f0_confidence, int32_t* num_harmonics, int32_t* n_deviations, int32_t* h_number,
                        double* h_freq, double* h_ideal, double* h_amp, double* h_deviation, double* estimated_stiffness,
                        double* model_fit_quality, double* harmonic_clarity, double* spectral_purity,
                        double* partial_coherence, double* r_squared, double* chi_squared, double* p_value,
                        int32_t* quality, int32_t device_ptrs) {
  if (!c) return SONAR_ERR_INVALID;
  const UserOut u{status, inharmonicity, std_dev, confidence, f0, f0_confidence, num_harmonics, n_deviations, h_number,
                  h_freq, h_ideal, h_amp, h_deviation, estimated_stiffness, model_fit_quality, harmonic_clarity,
                  spectral_purity, partial_coherence, r_squared, chi_squared, p_value, quality};
  return frames_impl(c, pcm, n, hop_size, p, u, device_ptrs != 0, nullptr);
}

int sonar_inharm_track(const sonar_inharm_params* p, int64_t F, const int32_t* status, const double* raw_inharmonicity,
                       const double* f0, double* inharmonicity, double* temporal_stability, double* inharmonicity_trend,
                       double* f0_stability) {
  if (!p || F < 0) return SONAR_ERR_INVALID;
  if (F == 0) return SONAR_OK;
  if (!raw_inharmonicity || !f0) return SONAR_ERR_INVALID;
  sonar::host::InharmTracker tr;
  const bool tracking = p->use_temporal_tracking != 0;
  for (int64_t f = 0; f < F; ++f) {
    sonar::host::InharmRow r;
    r.inharmonicity = raw_inharmonicity[f];
    if (!status || status[f] == SONAR_INHARM_STATUS_OK) {
      if (tracking && p->temporal_window < 0) return SONAR_ERR_PANIC;  // :1098 at the first tracked frame
      r = tr.step(tracking, p->temporal_window, raw_inharmonicity[f], f0[f]);
    }
    if (inharmonicity) inharmonicity[f] = r.inharmonicity;
    if (temporal_stability) temporal_stability[f] = r.stability;
    if (inharmonicity_trend) inharmonicity_trend[f] = r.trend;
    if (f0_stability) f0_stability[f] = r.f0_stability;
  }
  return SONAR_OK;
}

int sonar_inharm(sonar_ctx* c, const double* pcm, int64_t n, int32_t hop_size, const sonar_inharm_params* p,
                 int32_t* status, double* inharmonicity, double* temporal_stability, double* inharmonicity_trend,
                 double* f0_stability, double* std_dev, double* confidence, double* f0, double* f0_confidence,
                 int32_t* num_harmonics, int32_t* n_deviations, int32_t* h_number, double* h_freq, double* h_ideal,
                 double* h_amp, double* h_deviation, double* estimated_stiffness, double* model_fit_quality,
                 double* harmonic_clarity, double* spectral_purity, double* partial_coherence, double* r_squared,
                 double* chi_squared, double* p_value, int32_t* quality, int64_t* frames, int64_t* error_frame,
                 int32_t device_ptrs) {
  if (!c) return SONAR_ERR_INVALID;
  if (frames) *frames = 0;
  if (error_frame) *error_frame = -1;
  const bool dev = device_ptrs != 0;
  {                                                                    // frames_impl's checks, before anything is sized
    int method = 0;
    std::string msg;
    const int prc = check_params(p, p ? p->window_size : 0, &method, msg);
    if (prc != SONAR_OK) return fail(c, prc, msg);
    if (n < 0) return fail(c, SONAR_ERR_INVALID, "inharmonicity: negative sample count");
    if (hop_size < 1) return fail(c, SONAR_ERR_INVALID, "inharmonicity: hop_size must be at least 1");
  }
  int64_t F0 = sonar_pitch_detect_frames(n, p->window_size, hop_size);
  if (p->window_size != kDetectorWindow) F0 = 0;                       // frames_impl refuses it with a frame due
  // the status, raw inharmonicity, f0 and harmonic count come to the host for the tracker and the error (with
  // device pointers through library scratch); every other output goes where the caller wants it
  std::vector<double> raw((size_t)F0), hf0((size_t)F0);
  std::vector<int32_t> st((size_t)F0), num((size_t)F0);
  UserOut u{nullptr, nullptr, std_dev, confidence, nullptr, f0_confidence, nullptr, n_deviations, h_number, h_freq, h_ideal,
            h_amp, h_deviation, estimated_stiffness, model_fit_quality, harmonic_clarity, spectral_purity, partial_coherence,
            r_squared, chi_squared, p_value, quality};
  double *dr = nullptr, *df = nullptr;
  int32_t *ds = nullptr, *dn = nullptr;
  if (dev && F0) {
    dr = (double*)sonar::detail::dbuf(c, "inharm.rawinh", (size_t)F0 * sizeof(double));
    df = (double*)sonar::detail::dbuf(c, "inharm.rawf0", (size_t)F0 * sizeof(double));
    ds = (int32_t*)sonar::detail::dbuf(c, "inharm.rawst", (size_t)F0 * sizeof(int32_t));
    dn = (int32_t*)sonar::detail::dbuf(c, "inharm.rawnum", (size_t)F0 * sizeof(int32_t));
    if (!dr || !df || !ds || !dn) return fail(c, SONAR_ERR_NOMEM, "device allocation failed (inharmonicity)");
  }
  u.inh = dev ? dr : raw.data(); u.f0 = dev ? df : hf0.data();
  u.status = dev ? ds : st.data(); u.num = dev ? dn : num.data();
  int64_t F = 0;
  int rc = frames_impl(c, pcm, n, hop_size, p, u, dev, &F);
  if (rc != SONAR_OK) return rc;
  if (frames) *frames = F;
  if (F == 0) return SONAR_OK;
  if (dev) {
    HIP_TRY(c, hipMemcpyAsync(raw.data(), dr, (size_t)F * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(hf0.data(), df, (size_t)F * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(st.data(), ds, (size_t)F * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(num.data(), dn, (size_t)F * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  int64_t bad = -1;                                                    // AnalyzeSequence's return nil, err :1186-1188
  for (int64_t f = 0; f < F && bad < 0; ++f)
    if (st[(size_t)f] == SONAR_INHARM_STATUS_INSUFFICIENT) bad = f;
  const int64_t Ft = bad < 0 ? F : bad;                                // the frames Go analysed without an error
  std::vector<double> h((size_t)F * 4, 0.0);
  rc = sonar_inharm_track(p, Ft, st.data(), raw.data(), hf0.data(), h.data(), h.data() + F, h.data() + 2 * F,
                          h.data() + 3 * F);
  if (rc == SONAR_ERR_PANIC) return fail(c, rc, track_panic(p->temporal_window));
  if (rc != SONAR_OK) return fail(c, rc, "inharmonicity: tracker arguments");
  for (int64_t f = Ft; f < F; ++f) h[(size_t)f] = raw[(size_t)f];
  Staging o{c, "inharm.", dev};
  double* outs[4] = {inharmonicity, temporal_stability, inharmonicity_trend, f0_stability};
  for (int k = 0; k < 4 && rc == SONAR_OK; ++k) rc = o.put(outs[k], h.data() + (size_t)k * F, (size_t)F * 8);
  if (rc == SONAR_OK) rc = o.put(f0, hf0.data(), (size_t)F * 8);
  if (rc == SONAR_OK) rc = o.put(status, st.data(), (size_t)F * 4);
  if (rc == SONAR_OK) rc = o.put(num_harmonics, num.data(), (size_t)F * 4);
  if (rc == SONAR_OK && o.dev) rc = o.finish();
  if (rc != SONAR_OK) return rc;
  if (bad >= 0) {
    if (error_frame) *error_frame = bad;
    return fail(c, SONAR_ERR_INVALID, "insufficient harmonics found: " + std::to_string(num[(size_t)bad]) + " < " +
                                          std::to_string(p->min_harmonics));
  }
  return SONAR_OK;
}

double sonar_inharm_average(const double* inh, const double* conf, int64_t n) {
  if (!inh || !conf || n <= 0) return 0.0;
  double sum = 0.0;
  int64_t count = 0;
  for (int64_t i = 0; i < n; ++i)
    if (conf[i] > 0.5) { sum += inh[i]; ++count; }
  return count > 0 ? sum / (double)count : 0.0;
}

int32_t sonar_inharm_classify(double inharmonicity) {
  const double a = std::fabs(inharmonicity);
  if (a < 0.0001) return SONAR_INHARM_VERY_LOW;
  if (a < 0.001) return SONAR_INHARM_LOW;
  if (a < 0.005) return SONAR_INHARM_MODERATE;
  if (a < 0.01) return SONAR_INHARM_HIGH;
  return SONAR_INHARM_VERY_HIGH;
}

const char* sonar_inharm_class_name(int32_t cls) {
  static const char* const names[] = {"Very Low", "Low", "Moderate", "High", "Very High"};
  return cls >= 0 && cls <= SONAR_INHARM_VERY_HIGH ? names[cls] : nullptr;
}

int32_t sonar_inharm_instrument_type(double inharmonicity, double f0) {
  const double a = std::fabs(inharmonicity);
  if (a > 0.002 && f0 < 500) return SONAR_INHARM_INSTRUMENT_PIANO_STRING;
  if (a < 0.0005) return SONAR_INHARM_INSTRUMENT_WIND_BRASS;
  if (a > 0.0005 && a < 0.002) return SONAR_INHARM_INSTRUMENT_PLUCKED_STRING;
  if (a < 0.001 && f0 > 100 && f0 < 800) return SONAR_INHARM_INSTRUMENT_VOCAL_HARMONIC;
  return SONAR_INHARM_INSTRUMENT_UNKNOWN;
}

const char* sonar_inharm_instrument_name(int32_t type) {
  static const char* const names[] = {"Piano/String", "Wind/Brass", "Plucked String", "Vocal/Harmonic", "Unknown"};
  return type >= 0 && type <= SONAR_INHARM_INSTRUMENT_UNKNOWN ? names[type] : nullptr;
}

const char* sonar_inharm_method_name(int32_t method) {
  static const char* const names[] = {"Railsback Curve", "Fletcher-Munson Weighted", "Spectral Deviation",
                                      "Partial Tracking", "Beat Pattern Analysis", "Statistical Analysis"};
  return method >= 0 && method <= SONAR_INHARM_STATISTICAL ? names[method] : "Unknown";
}

const char* sonar_inharm_model_name(int32_t model) {
  static const char* const names[] = {"String Instrument", "Pipe/Wind Instrument", "Membrane/Percussion", "General"};
  return model >= 0 && model <= SONAR_INHARM_MODEL_GENERAL ? names[model] : "Unknown";
}

const char* sonar_inharm_quality_name(int32_t quality) {
  static const char* const names[] = {"Very Poor", "Poor", "Fair", "Good", "Excellent", "Poor - Invalid F0"};
  return quality >= 0 && quality <= SONAR_INHARM_QUALITY_INVALID_F0 ? names[quality] : nullptr;
}

}  // extern "C"
