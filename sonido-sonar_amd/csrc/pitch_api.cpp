// pitch_api.cpp -- sonar_pitch_frames_raw, sonar_pitch_detect and their host-only companions:
// PitchDetector (algorithms/tonal/pitch_detection.go) for every method of DetectPitch's switch.  The host
// side: NewPitchDetector's defaults (:159-193), the argument checks, the scan ranges of the HPS (:582-583)
// and the cepstrum (:646-647), createWindowFunction's window (:317-345) and the transform's twiddles as
// cached tables, the staged arrays (staging.h), and postProcessResult + updateTemporalTracking over the
// raw rows (host::PitchTracker).  The kernels are pitch_kernels.hip's.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"
#include "host_dsp.h"
#include "kernels.h"
#include "pitch_kernels.h"
#include "staging.h"

using sonar::detail::fail;
using sonar::detail::pitch_twiddles;
using sonar::detail::pitch_window;
using sonar::detail::Staging;
using sonar::detail::timed_begin;
using sonar::detail::timed_end;

// createWindowFunction (:317-345), cached per (type, W)
const double* sonar::detail::pitch_window(sonar_ctx* c, int type, int W) {
  const unsigned char* t = nullptr;
  const int rc = sonar::detail::cached_table(c, "pitch.win." + std::to_string(type) + "." + std::to_string(W), "pitch window",
      [&](std::vector<unsigned char>& img, int64_t&) {
        img.resize((size_t)W * sizeof(double));
        double* w = (double*)img.data();
        const double d = (double)(W - 1);
        for (int i = 0; i < W; ++i) {
          const double x = (double)i;
          switch (type) {
            case SONAR_PITCH_WIN_HAMMING: w[i] = 0.54 - 0.46 * std::cos(2.0 * M_PI * x / d); break;
            case SONAR_PITCH_WIN_BLACKMAN:
              w[i] = 0.42 - 0.5 * std::cos(2.0 * M_PI * x / d) + 0.08 * std::cos(4.0 * M_PI * x / d);
              break;
            case SONAR_PITCH_WIN_RECTANGULAR: w[i] = 1.0; break;
            default: w[i] = 0.5 * (1.0 - std::cos(2.0 * M_PI * x / d)); break;
          }
        }
        return SONAR_OK;
      }, &t);
  return rc == SONAR_OK ? (const double*)t : nullptr;
}

// the N / 2 (cos, sin) pairs of -2 pi m / N: the table of sonar_xcorr_params' transform, under its key
const double2* sonar::detail::pitch_twiddles(sonar_ctx* c, int64_t N) {
  const unsigned char* tw = nullptr;
  const int rc = sonar::detail::cached_table(c, "xcorr.tw." + std::to_string(N), "correlation FFT",
      [&](std::vector<unsigned char>& img, int64_t&) {
        const int64_t half = N / 2;
        img.resize((size_t)half * sizeof(double2));
        double2* h = (double2*)img.data();
        for (int64_t m = 0; m < half; ++m) ::sincos(-2.0 * M_PI * (double)m / (double)N, &h[m].y, &h[m].x);
        return SONAR_OK;
      }, &tw);
  return rc == SONAR_OK ? (const double2*)tw : nullptr;
}

namespace {

struct Plan {
  int method = 0;                  // the switch's target: YIN, ACF, NSDF, HPS, CEPSTRUM or ZERO_CROSSING
  int width = 0;                   // of a frame's curve
  int fft_n = 0;                   // points of the method's transform, 0 without one
  int lo = 0, hi = 0;              // HPS bins / cepstrum quefrencies, before the clip to the length
};

// int(x) of a finite x >= 0 that fits an int32
bool go_int32(double q, int* out) {
  if (!(q >= 0.0 && q < 2147483648.0)) return false;
  *out = (int)q;
  return true;
}

int check_params(const sonar_pitch_params* p, Plan* pl, std::string& msg) {
  if (!p) { msg = "pitch detection: null params"; return SONAR_ERR_INVALID; }
  switch (p->method) {                                             // DetectPitch's switch :239-260
    case SONAR_PITCH_YIN: case SONAR_PITCH_YIN_FFT: pl->method = SONAR_PITCH_YIN; break;
    case SONAR_PITCH_NSDF: case SONAR_PITCH_MPM: pl->method = SONAR_PITCH_NSDF; break;
    case SONAR_PITCH_HPS: case SONAR_PITCH_PEAKS: pl->method = SONAR_PITCH_HPS; break;
    case SONAR_PITCH_ACF: case SONAR_PITCH_CEPSTRUM: case SONAR_PITCH_ZERO_CROSSING: pl->method = p->method; break;
    default:
      msg = "unsupported pitch detection method: " + std::to_string(p->method);
      return SONAR_ERR_INVALID;
  }
  if (p->hop_size < 1 || p->sample_rate < 1) {
    msg = "pitch detection: hop_size and sample_rate must be at least 1";
    return SONAR_ERR_INVALID;
  }
  if (!(std::isfinite(p->min_freq) && std::isfinite(p->max_freq) && 0.0 < p->min_freq && p->min_freq < p->max_freq)) {
    msg = "pitch detection: 0 < min_freq < max_freq, both finite, is required";
    return SONAR_ERR_INVALID;
  }
  const int W = p->window_size;
  const bool w_ok = W >= sonar::PITCH_MIN_W && W <= sonar::PITCH_MAX_W && (W & (W - 1)) == 0;
  if (pl->method == SONAR_PITCH_HPS && p->zero_padding < 1) {
    msg = "runtime error: index out of range [0] with length 0";   // hps[0] :580
    return SONAR_ERR_PANIC;
  }
  if (pl->method == SONAR_PITCH_CEPSTRUM && W >= 0) {
    int q = 0;
    if (!go_int32((double)p->sample_rate / p->max_freq, &q) || q >= W) {   // realCepstrum[minQuefrency] :650
      msg = "runtime error: index out of range [" + std::to_string(q) + "] with length " + std::to_string(W);
      return SONAR_ERR_PANIC;
    }
  }
  if (!w_ok) {
    msg = "pitch detection: window_size must be a power of two in [64, 2048]";
    return SONAR_ERR_UNSUPPORTED;
  }
  if (p->window_function < SONAR_PITCH_WIN_HANN || p->window_function > SONAR_PITCH_WIN_RECTANGULAR) {
    msg = "pitch detection: window_function outside the enum";
    return SONAR_ERR_UNSUPPORTED;
  }
  const double sr = (double)p->sample_rate;
  switch (pl->method) {
    case SONAR_PITCH_YIN: case SONAR_PITCH_NSDF: pl->width = W / 2; break;
    case SONAR_PITCH_ACF:
      pl->width = 2 * W - 1;
      pl->fft_n = W > 1000 ? 2 * W : 0;                            // fftThreshold, correlation.go:139-142
      break;
    case SONAR_PITCH_HPS: {
      const int zp = p->zero_padding;
      if ((zp != 1 && zp != 2 && zp != 4) || W * zp > sonar::PITCH_MAX_FFT) {
        msg = "pitch detection: zero_padding must be 1, 2 or 4 with window_size * zero_padding <= 4096";
        return SONAR_ERR_UNSUPPORTED;
      }
      pl->fft_n = W * zp;
      pl->width = pl->fft_n / 2;
      if (!go_int32(p->min_freq * (double)pl->fft_n / sr, &pl->lo) || !go_int32(p->max_freq * (double)pl->fft_n / sr, &pl->hi)) {
        msg = "pitch detection: the HPS scan range does not fit an int32";
        return SONAR_ERR_UNSUPPORTED;
      }
      break;
    }
    case SONAR_PITCH_CEPSTRUM:
      pl->fft_n = W;
      pl->width = W;
      if (!go_int32(sr / p->max_freq, &pl->lo) || !go_int32(sr / p->min_freq, &pl->hi)) {
        msg = "pitch detection: the cepstrum scan range does not fit an int32";
        return SONAR_ERR_UNSUPPORTED;
      }
      break;
    default: pl->width = 0; break;
  }
  return SONAR_OK;
}

struct RawOut {
  double *pitch, *conf;
  int32_t *index, *ncand;
  double* second;
  int32_t* cand_index;
  double *cand_conf, *curve;
};

// The raw rows of every frame.  pcm is a host or device array (pcm_dev); the outputs are host or device
// arrays (out_dev).  Waits for the stream before it returns.
int raw_impl(sonar_ctx* c, const double* pcm, int64_t n, const sonar_pitch_params* p, int32_t K, const RawOut& u,
             bool pcm_dev, bool out_dev, int64_t* frames) {
  Plan pl;
  std::string msg;
  const int prc = check_params(p, &pl, msg);
  if (prc != SONAR_OK) return fail(c, prc, msg);
  if (K < 0 || K > sonar::PITCH_MAX_CANDIDATES) return fail(c, SONAR_ERR_INVALID, "pitch detection: max_candidates outside 0..8");
  if (n < 0) return fail(c, SONAR_ERR_INVALID, "pitch detection: negative sample count");
  const int W = p->window_size;
  const int64_t F = sonar_pitch_detect_frames(n, W, p->hop_size);
  if (frames) *frames = F;
  if (F == 0) return SONAR_OK;
  if (F > 2147483647) return fail(c, SONAR_ERR_UNSUPPORTED, "pitch detection: more than 2^31 - 1 frames");
  if (!pcm) return fail(c, SONAR_ERR_INVALID, "pitch detection: null pcm pointer");
  if (!u.pitch || !u.conf) return fail(c, SONAR_ERR_INVALID, "pitch detection: null pitch or confidence pointer");
  HIP_TRY(c, hipSetDevice(c->device));
  Staging in{c, "pitch.", pcm_dev}, o{c, "pitch.", out_dev};
  sonar::PitchArgs a{};
  a.pcm = in.in("pcm", pcm, (size_t)n);
  a.n = n; a.F = F; a.hop = p->hop_size;
  a.W = W; a.sr = p->sample_rate; a.method = pl.method; a.pre = p->pre_emphasis != 0; a.zp = p->zero_padding; a.K = K;
  a.min_freq = p->min_freq; a.max_freq = p->max_freq; a.yin_thr = p->yin_threshold; a.ac_thr = p->autocorr_threshold;
  a.lo = pl.lo; a.hi = pl.hi; a.width = pl.width;
  a.pitch = o.out("p", u.pitch, (size_t)F);
  a.conf = o.out("c", u.conf, (size_t)F);
  a.index = o.out("i", u.index, (size_t)F);
  a.ncand = o.out("nc", u.ncand, (size_t)F);
  a.second = o.out("sc", u.second, (size_t)F);
  a.cand_index = K ? o.out("ci", u.cand_index, (size_t)F * K) : nullptr;
  a.cand_conf = K ? o.out("cc", u.cand_conf, (size_t)F * K) : nullptr;
  a.curve = pl.width ? o.out("curve", u.curve, (size_t)F * (size_t)pl.width) : nullptr;
  if (pl.method == SONAR_PITCH_ACF) a.stats = o.tmp<double>("stats", (size_t)F * 2);
  if (in.nomem || o.nomem) return fail(c, SONAR_ERR_NOMEM, "device allocation failed (pitch detection)");
  a.win = pitch_window(c, p->window_function, W);
  if (!a.win) return SONAR_ERR_NOMEM;
  if (pl.fft_n) {
    a.tw = pitch_twiddles(c, pl.fft_n);
    if (!a.tw) return SONAR_ERR_NOMEM;
  }
  int rc = in.ready("device allocation failed (pitch detection)");
  if (rc != SONAR_OK) return rc;
  hipEvent_t tend = timed_begin(c, c->stream);
  rc = sonar::launch_pitch_frames(a, c->stream);
  if (rc == -1) return fail(c, SONAR_ERR_UNSUPPORTED, "pitch detection: a shape the kernels do not take");
  if (rc != 0) return fail(c, SONAR_ERR_DEVICE, "pitch detection launch failed");
  timed_end(c, c->stream, tend);
  return o.finish();
}

sonar::host::PitchTrackParams track_params(const sonar_pitch_params* p) {
  sonar::host::PitchTrackParams t;
  t.octave_correction = p->octave_correction != 0;
  t.temporal_smoothing = p->temporal_smoothing != 0;
  t.median_filter = p->median_filter;
  t.min_confidence = p->min_confidence;
  return t;
}

}  // namespace

extern "C" {

void sonar_pitch_params_default(sonar_pitch_params* p, int32_t sample_rate) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->method = SONAR_PITCH_YIN;
  p->sample_rate = sample_rate;
  p->window_size = 1024;
  p->hop_size = 512;
  p->min_freq = 80.0;
  p->max_freq = 1000.0;
  p->yin_threshold = 0.15;
  p->autocorr_threshold = 0.3;
  p->cepstral_threshold = 0.3;
  p->min_confidence = 0.5;
  p->min_salience = 0.1;
  p->voicing_threshold = 0.45;
  p->max_harmonics = 10;
  p->harmonic_tolerance = 0.1;
  p->pre_emphasis = 1;
  p->window_function = SONAR_PITCH_WIN_HANN;
  p->zero_padding = 2;
  p->median_filter = 3;
  p->temporal_smoothing = 1;
  p->octave_correction = 1;
}

int64_t sonar_pitch_detect_frames(int64_t n, int32_t window_size, int32_t hop_size) {
  if (window_size < 1 || hop_size < 1 || n < window_size) return 0;
  return (n - window_size) / hop_size + 1;
}

int64_t sonar_pitch_curve_width(const sonar_pitch_params* p) {
  Plan pl;
  std::string msg;
  const int rc = check_params(p, &pl, msg);
  return rc != SONAR_OK ? rc : pl.width;
}

int sonar_pitch_frames_raw(sonar_ctx* c, const double* pcm, int64_t n, const sonar_pitch_params* p, int32_t max_candidates,
                           double* pitch, double* confidence, int32_t* index, int32_t* n_candidates,
                           double* second_confidence, int32_t* cand_index, double* cand_conf, double* curve,
                           int32_t device_ptrs) {
  if (!c) return SONAR_ERR_INVALID;
  const RawOut u{pitch, confidence, index, n_candidates, second_confidence, cand_index, cand_conf, curve};
  return raw_impl(c, pcm, n, p, max_candidates, u, device_ptrs != 0, device_ptrs != 0, nullptr);
}

int sonar_pitch_track(const sonar_pitch_params* p, int64_t F, const double* raw_pitch, const double* raw_confidence,
                      const int32_t* n_candidates, const double* second_confidence, double* pitch, double* confidence,
                      double* voicing, double* periodicity, double* clarity, double* strength, double* salience,
                      double* stability, double* f0_multiple) {
  if (!p || F < 0) return SONAR_ERR_INVALID;
  if (F == 0) return SONAR_OK;
  if (!raw_pitch || !raw_confidence) return SONAR_ERR_INVALID;
  const sonar::host::PitchTrackParams t = track_params(p);
  sonar::host::PitchTracker tr;
  for (int64_t f = 0; f < F; ++f) {
    const int nc = n_candidates ? n_candidates[f] : (raw_confidence[f] != 0.0 ? 1 : 0);
    const sonar::host::PitchRow r = tr.step(t, raw_pitch[f], raw_confidence[f], nc, second_confidence ? second_confidence[f] : 0.0);
    if (pitch) pitch[f] = r.pitch;
    if (confidence) confidence[f] = r.confidence;
    if (voicing) voicing[f] = r.voicing;
    if (periodicity) periodicity[f] = r.periodicity;
    if (clarity) clarity[f] = r.clarity;
    if (strength) strength[f] = r.strength;
    if (salience) salience[f] = r.salience;
    if (stability) stability[f] = r.stability;
    if (f0_multiple) f0_multiple[f] = r.f0_multiple;
  }
  return SONAR_OK;
}

int sonar_pitch_detect(sonar_ctx* c, const double* pcm, int64_t n, const sonar_pitch_params* p, double* pitch,
                       double* confidence, double* voicing, double* periodicity, double* clarity, double* strength,
                       double* salience, double* stability, double* f0_multiple, int64_t* frames, int32_t device_ptrs) {
  if (!c) return SONAR_ERR_INVALID;
  if (frames) *frames = 0;
  if (!p) return fail(c, SONAR_ERR_INVALID, "pitch detection: null params");
  if (n < 0) return fail(c, SONAR_ERR_INVALID, "pitch detection: negative sample count");
  const int64_t F0 = sonar_pitch_detect_frames(n, p->window_size, p->hop_size);
  std::vector<double> rp((size_t)F0), rc_((size_t)F0), sc((size_t)F0);
  std::vector<int32_t> nc((size_t)F0);
  const RawOut u{rp.data(), rc_.data(), nullptr, nc.data(), sc.data(), nullptr, nullptr, nullptr};
  int64_t F = 0;
  int rc = raw_impl(c, pcm, n, p, 0, u, device_ptrs != 0, false, &F);
  if (rc != SONAR_OK) return rc;
  if (frames) *frames = F;
  if (F == 0) return SONAR_OK;
  double* outs[9] = {pitch, confidence, voicing, periodicity, clarity, strength, salience, stability, f0_multiple};
  std::vector<double> h((size_t)F * 9);
  double* hp[9];
  for (int k = 0; k < 9; ++k) hp[k] = h.data() + (size_t)k * F;
  rc = sonar_pitch_track(p, F, rp.data(), rc_.data(), nc.data(), sc.data(), hp[0], hp[1], hp[2], hp[3], hp[4], hp[5], hp[6],
                         hp[7], hp[8]);
  if (rc != SONAR_OK) return fail(c, rc, "pitch detection: tracker arguments");
  Staging o{c, "pitch.", device_ptrs != 0};
  for (int k = 0; k < 9 && rc == SONAR_OK; ++k) rc = o.put(outs[k], hp[k], (size_t)F * 8);
  return rc != SONAR_OK || !o.dev ? rc : o.finish();
}

int sonar_pitch_stability(const double* pitch, int64_t n, int32_t sample_rate, int32_t hop_size, double* out7,
                          int32_t* empty) {
  if (n < 0 || (n > 0 && !pitch) || !out7) return SONAR_ERR_INVALID;
  const bool ok = sonar::host::pitch_stability(pitch, n, sample_rate, hop_size, out7);
  if (empty) *empty = ok ? 0 : 1;
  return SONAR_OK;
}

}  // extern "C"
