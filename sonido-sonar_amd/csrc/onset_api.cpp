// onset_api.cpp -- the onset and tempo entries: OnsetDetection (algorithms/temporal/onset_detection.go)
// and TempoEstimation (tempo_estimation.go) over SpectralFlux (spectral/spectral_flux.go) and
// Envelope.ComputeRMS (temporal/envelope.go).  The host side: the argument checks, Go's truncating
// conversions (minIntervalFrames, the 100 ms frame, the lag range), the staged arrays of each entry
// (staging.h), the flux detector over the chunked walk of the float64 transform with no window, and the
// short serial tails that act on a few values per second of audio: combineOnsets, the interval
// histogram and the peak search over the 30-odd lags the reference reads.  The kernels are
// onset_kernels.hip's.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"
#include "go_math.h"
#include "kernels.h"
#include "magnitude_walk.h"
#include "staging.h"

using sonar::detail::fail;
using sonar::detail::Staging;
using sonar::detail::timed_begin;
using sonar::detail::timed_end;

namespace {

// DetectOnsetsComplex's parameters (:129-131)
constexpr double kFluxThreshold = 0.3, kEnergyThreshold = 0.1, kComplexMinInterval = 0.05;
// findTempoFromIntervals' bins (tempo_estimation.go:83)
constexpr int kTempoBins = 14;
const double kTempoRange[kTempoBins] = {60, 70, 80, 90, 100, 110, 120, 130, 140, 150, 160, 170, 180, 200};
const char* const kCategoryNames[5] = {"very_slow", "slow", "moderate", "fast", "very_fast"};

int64_t peaks_width(int64_t n) { return n > 1 ? (n - 1) / 2 : 0; }

// len(ComputeRMS(...)) (envelope.go:19-23)
int64_t rms_frames(int64_t n, int32_t frame, int32_t hop) {
  if (frame <= 0 || hop <= 0 || n < frame) return 0;
  return (n - frame) / hop + 1;
}

// int(minInterval * float64(sampleRate) / float64(hopSize)) (:103), where Go's conversion is defined
int min_interval_frames(double min_interval, int32_t sample_rate, int32_t hop, int32_t* out, std::string& msg) {
  if (sample_rate <= 0) { msg = "onsets: sample_rate <= 0 is not reproduced"; return SONAR_ERR_UNSUPPORTED; }
  if (hop <= 0) { msg = "onsets: hop_size <= 0 is not reproduced"; return SONAR_ERR_UNSUPPORTED; }
  const double q = min_interval * (double)sample_rate / (double)hop;
  if (!(q > -2147483649.0 && q < 2147483648.0)) {
    msg = "onsets: a min_interval whose frame count is NaN or does not fit an int32 is not reproduced";
    return SONAR_ERR_UNSUPPORTED;
  }
  *out = (int32_t)q;
  return SONAR_OK;
}

// findFluxPeaks of n device values into index (width slots, the unused ones 0) and *dcount, queued
int pick(sonar_ctx* c, const double* v, int64_t n, double threshold, int32_t mif, int64_t scale, uint64_t* mask,
         int64_t* index, int64_t width, int64_t* dcount) {
  if (width > 0) HIP_TRY(c, hipMemsetAsync(index, 0, (size_t)width * 8, c->stream));
  hipEvent_t tend = timed_begin(c, c->stream);
  const int rc = sonar::launch_onset_peaks(v, n, threshold, mif, scale, mask, index, width, dcount, c->stream);
  if (rc == -1) return fail(c, SONAR_ERR_UNSUPPORTED, "onsets: a shape the peak kernels do not take");
  if (rc != 0) return fail(c, SONAR_ERR_DEVICE, "onset peak launch failed");
  timed_end(c, c->stream, tend);
  return SONAR_OK;
}

std::string tagged(const char* tag, const char* name) { return std::string(tag) + name; }

// DetectOnsets (:26-56) on device samples: the spectrogram in chunks through a bounded scratch, the
// flux of every chunk with the last row of the chunk before it carried across, then the peaks
struct FluxDetector {
  sonar::detail::MagnitudeWalk walk;
  int64_t n = 0, width = 0;
  int32_t mif = 0;
  double threshold = 0.0;
  double* flux = nullptr;
  uint64_t* mask = nullptr;
  int64_t *onsets = nullptr, *dcount = nullptr;

  // the transform's checks (Go's error texts) and minIntervalFrames
  int plan(int64_t samples, bool have_pcm, int32_t sample_rate, int32_t window_size, int32_t hop_size, double thr,
           double min_interval, std::string& msg) {
    n = samples;
    threshold = thr;
    // a nil window is no window (stft.go:112): the rectangular table is all ones, x * 1.0 is x
    int rc = walk.plan(sample_rate, window_size ? window_size : SONAR_ONSET_WINDOW, hop_size ? hop_size : SONAR_ONSET_HOP,
                       SONAR_WIN_RECTANGULAR, n, have_pcm, &msg);
    if (rc != SONAR_OK) return rc;
    rc = min_interval_frames(min_interval, sample_rate, walk.H, &mif, msg);
    if (rc != SONAR_OK) return rc;
    width = peaks_width(walk.F - 1);
    return SONAR_OK;
  }
  void alloc(Staging& o, const char* tag, double* user_flux, int64_t* user_onsets) {
    const int64_t F = walk.F;
    const size_t nflux = (size_t)std::max<int64_t>(F - 1, 1);
    flux = user_flux ? o.out(tagged(tag, "flux").c_str(), user_flux, nflux) : o.tmp<double>(tagged(tag, "flux").c_str(), nflux);
    walk.alloc(o, 1, tagged(tag, "chunk").c_str());   // one row before the chunk's: the last row of the chunk before it
    mask = o.tmp<uint64_t>(tagged(tag, "mask").c_str(), (size_t)std::max<int64_t>(sonar::onset_mask_words(F - 1), 1));
    const size_t slots = (size_t)std::max<int64_t>(width, 1);
    onsets = user_onsets ? o.out(tagged(tag, "onsets").c_str(), user_onsets, slots)
                         : o.tmp<int64_t>(tagged(tag, "onsets").c_str(), slots);
    dcount = o.tmp<int64_t>(tagged(tag, "count").c_str(), 1);
  }
  int run(sonar_ctx* c, Staging& o, const double* dx, double* user_magnitude) {
    const int64_t F = walk.F, K = walk.K, cf = walk.chunk_frames;
    double* carried = walk.rows - K;
    const int rc = walk.each(c, dx, n, false, [&](const double* rows, int64_t s0, int64_t nf) -> int {
      hipEvent_t tend = timed_begin(c, c->stream);
      const int lrc = s0 == 0 ? sonar::launch_onset_flux(rows, nf, K, false, flux, c->stream)
                              : sonar::launch_onset_flux(carried, nf + 1, K, false, flux + (s0 - 1), c->stream);
      if (lrc != 0) return fail(c, SONAR_ERR_DEVICE, "spectral flux launch failed");
      timed_end(c, c->stream, tend);
      const int grc = o.give(user_magnitude ? user_magnitude + s0 * K : nullptr, rows, (size_t)nf * (size_t)K * 8);
      if (grc != SONAR_OK) return grc;
      if (s0 + cf < F)
        HIP_TRY(c, hipMemcpyAsync(carried, rows + (nf - 1) * K, (size_t)K * 8, hipMemcpyDeviceToDevice, c->stream));
      return SONAR_OK;
    });
    if (rc != SONAR_OK) return rc;
    // onset sample = index in the flux array * hop (:50-53)
    return pick(c, flux, F - 1, threshold, mif, walk.H, mask, onsets, width, dcount);
  }
};

// DetectOnsetsEnergy (:59-94) on device samples
struct EnergyDetector {
  int64_t Fe = 0, ncurve = 0, width = 0;
  int32_t frame = 0, hop = 0, mif = 0;
  double threshold = 0.0;
  double *env = nullptr, *curve = nullptr;
  uint64_t* mask = nullptr;
  int64_t *onsets = nullptr, *dcount = nullptr;

  int plan(int64_t n, int32_t sample_rate, int32_t frame_size, int32_t hop_size, double thr, double min_interval,
           std::string& msg) {
    frame = frame_size ? frame_size : SONAR_ONSET_ENERGY_FRAME;
    hop = hop_size ? hop_size : SONAR_ONSET_ENERGY_HOP;
    threshold = thr;
    if (frame < 0) { msg = "onsets: frame_size < 0 is not reproduced"; return SONAR_ERR_UNSUPPORTED; }
    const int rc = min_interval_frames(min_interval, sample_rate, hop, &mif, msg);
    if (rc != SONAR_OK) return rc;
    Fe = rms_frames(n, frame, hop);
    ncurve = std::max<int64_t>(Fe - 1, 0);
    width = peaks_width(ncurve);
    return SONAR_OK;
  }
  void alloc(Staging& o, const char* tag, double* user_curve, int64_t* user_onsets) {
    env = o.tmp<double>(tagged(tag, "env").c_str(), (size_t)std::max<int64_t>(Fe, 1));
    const size_t nc = (size_t)std::max<int64_t>(ncurve, 1);
    curve = user_curve ? o.out(tagged(tag, "curve").c_str(), user_curve, nc) : o.tmp<double>(tagged(tag, "curve").c_str(), nc);
    mask = o.tmp<uint64_t>(tagged(tag, "mask").c_str(), (size_t)std::max<int64_t>(sonar::onset_mask_words(ncurve), 1));
    const size_t slots = (size_t)std::max<int64_t>(width, 1);
    onsets = user_onsets ? o.out(tagged(tag, "onsets").c_str(), user_onsets, slots)
                         : o.tmp<int64_t>(tagged(tag, "onsets").c_str(), slots);
    dcount = o.tmp<int64_t>(tagged(tag, "count").c_str(), 1);
  }
  int run(sonar_ctx* c, const double* dx) {
    hipEvent_t tend = timed_begin(c, c->stream);
    if (sonar::launch_onset_rms(dx, Fe, frame, hop, env, c->stream) != 0 ||
        sonar::launch_onset_posdiff(env, ncurve, curve, c->stream) != 0)
      return fail(c, SONAR_ERR_DEVICE, "energy onset launch failed");
    timed_end(c, c->stream, tend);
    return pick(c, curve, ncurve, threshold, mif, hop, mask, onsets, width, dcount);
  }
};

// combineOnsets (:149-182).  The list is sorted ascending, so the kept values are ascending too and the
// kept value nearest to the next one is the last kept: |onset - existing| <= tolerance for any
// existing one implies it for the last.  One comparison per value.
std::vector<int64_t> combine(const int64_t* a, int64_t na, const int64_t* b, int64_t nb, int64_t tolerance) {
  std::vector<int64_t> all(a, a + na);
  all.insert(all.end(), b, b + nb);
  std::sort(all.begin(), all.end());
  std::vector<int64_t> kept;
  for (int64_t v : all)
    if (kept.empty() || v - kept.back() > tolerance) kept.push_back(v);
  return kept;
}

// EstimateTempo's tail (tempo_estimation.go:33-47) and findTempoFromIntervals (:77-118)
double tempo_from_onsets(const int64_t* onsets, int64_t count, int32_t sample_rate, int32_t* counts) {
  int32_t local[kTempoBins];
  if (!counts) counts = local;
  std::fill(counts, counts + kTempoBins, 0);
  if (count < 2) return 0.0;
  for (int64_t i = 0; i + 1 < count; ++i) {
    const double interval = (double)(onsets[i + 1] - onsets[i]) / (double)sample_rate;
    if (!(interval > 0.2 && interval < 2.0)) continue;
    const double tempo = 60.0 / interval;
    int best = 0;
    double best_diff = std::fabs(tempo - kTempoRange[0]);
    for (int k = 0; k < kTempoBins; ++k) {
      const double diff = std::fabs(tempo - kTempoRange[k]);
      if (diff < best_diff) { best_diff = diff; best = k; }
    }
    if (best_diff < 10.0) counts[best]++;
  }
  int32_t max_count = 0;
  double best_tempo = 120.0;
  for (int k = 0; k < kTempoBins; ++k)
    if (counts[k] > max_count) { max_count = counts[k]; best_tempo = kTempoRange[k]; }
  return best_tempo;
}

int32_t tempo_category(double tempo) {   // ClassifyTempoCategory (:220-232); a NaN falls through to the last
  return tempo < 60 ? 0 : tempo < 90 ? 1 : tempo < 120 ? 2 : tempo < 150 ? 3 : 4;
}

// EstimateTempoAutocorrelation's integer side (:57-58, :62, :67, :154, :160-174)
struct AcPlan {
  int32_t frame = 0, hop = 0;
  int64_t L = 0;         // envelope values
  int64_t nac = 0;       // len(autocorr): L / 2, 0 when the envelope has fewer than 10 values
  int64_t min_lag = 0, max_lag = 0;   // the search's range after its clamps (nac >= 10 only)
  double tpf = 0.0;
};

AcPlan ac_plan(int64_t n, int32_t sample_rate) {
  AcPlan p;
  p.frame = (int32_t)(0.1 * (double)sample_rate);
  p.hop = p.frame / 4;
  p.L = rms_frames(n, p.frame, p.hop);
  if (p.L < 10) return p;
  p.nac = p.L / 2;
  if (p.nac < 10) return p;
  p.tpf = (double)p.hop / (double)sample_rate;
  p.min_lag = (int64_t)((60.0 / 180.0) / p.tpf);
  p.max_lag = (int64_t)(1.0 / p.tpf);
  if (p.min_lag < 1) p.min_lag = 1;
  if (p.max_lag >= p.nac) p.max_lag = p.nac - 1;
  return p;
}

// EstimateTempoAutocorrelation on device samples.  The search (:176-200) reads lags min_lag - 1 ..
// min(max_lag, nac - 2) + 1 and lag 0 (the divisor of the normalisation), so those are what is always
// computed and searched; the whole curve is computed besides when the caller wants it.
struct AcEstimator {
  AcPlan p;
  int64_t wlo = 0, nwin = 0;   // the window of lags the search reads: wlo .. wlo + nwin - 1
  double *env = nullptr, *narrow = nullptr, *raw = nullptr, *curve = nullptr;

  void plan(int64_t n, int32_t sample_rate) {
    p = ac_plan(n, sample_rate);
    if (p.nac >= 10) {
      const int64_t hi = std::min(p.max_lag, p.nac - 2);
      if (p.min_lag <= hi) { wlo = p.min_lag - 1; nwin = hi + 1 - wlo + 1; }
    }
  }
  void alloc(Staging& o, const char* tag, double* user_curve) {
    if (p.L < 10) return;
    env = o.tmp<double>(tagged(tag, "env").c_str(), (size_t)p.L);
    narrow = o.tmp<double>(tagged(tag, "narrow").c_str(), (size_t)nwin + 1);
    if (user_curve && p.nac > 0) {
      raw = o.tmp<double>(tagged(tag, "raw").c_str(), (size_t)p.nac);
      curve = o.out(tagged(tag, "curve").c_str(), user_curve, (size_t)p.nac);
    }
  }
  // waits for the stream once, for the window's values
  int run(sonar_ctx* c, Staging& o, const double* dx, double* tempo, int64_t* best_lag) {
    *tempo = 0.0;
    *best_lag = 0;
    if (p.L < 10) return SONAR_OK;   // :62-64
    hipStream_t s = c->stream;
    hipEvent_t tend = timed_begin(c, s);
    if (sonar::launch_onset_rms(dx, p.L, p.frame, p.hop, env, s) != 0)
      return fail(c, SONAR_ERR_DEVICE, "tempo: envelope launch failed");
    if (curve && (sonar::launch_onset_autocorr(env, p.L, 0, p.nac, false, raw, s) != 0 ||
                  sonar::launch_onset_autocorr_norm(raw, p.nac, curve, s) != 0))
      return fail(c, SONAR_ERR_DEVICE, "tempo: autocorrelation launch failed");
    if (p.nac < 10) { timed_end(c, s, tend); return SONAR_OK; }   // :154-156
    if (sonar::launch_onset_autocorr(env, p.L, wlo, nwin + 1, true, narrow, s) != 0)
      return fail(c, SONAR_ERR_DEVICE, "tempo: autocorrelation launch failed");
    timed_end(c, s, tend);
    const double* h = o.back(narrow, (size_t)nwin + 1);
    const int rc = o.fetch();
    if (rc != SONAR_OK) return rc;
    // the in-place normalisation (:143-147): autocorr[0] becomes its own quotient, the rest is divided by that
    const double a0 = h[0];
    const bool norm = a0 > 0.0;
    const double q = a0 / a0;
    auto at = [&](int64_t lag) {
      const double r = lag == 0 ? a0 : h[(size_t)(1 + lag - wlo)];
      return !norm ? r : lag == 0 ? q : r / q;
    };
    double max_val = 0.0;
    int64_t best = 0;
    for (int64_t lag = p.min_lag; lag <= p.max_lag; ++lag) {
      if (!(lag > 0 && lag < p.nac - 1)) continue;
      const double v = at(lag);
      if (v > at(lag - 1) && v > at(lag + 1) && v > max_val) { max_val = v; best = lag; }
    }
    *best_lag = best;
    *tempo = best == 0 ? 120.0 : 60.0 / ((double)best * p.tpf);
    return SONAR_OK;
  }
};

// DetectOnsetsComplex (:123-146) on device samples: both detectors, then combineOnsets on the host
// after one copy of the two lists.  rc is the flux detector's plan error, which ends the call (:135-137).
int complex_onsets(sonar_ctx* c, Staging& o, const double* dx, FluxDetector& fd, EnergyDetector& ed,
                   int32_t sample_rate, std::vector<int64_t>* out) {
  int rc = fd.run(c, o, dx, nullptr);
  if (rc == SONAR_OK) rc = ed.run(c, dx);
  if (rc != SONAR_OK) return rc;
  const int64_t *cf = o.back(fd.dcount, 1), *ce = o.back(ed.dcount, 1);
  const int64_t *hf = o.back(fd.onsets, (size_t)fd.width), *he = o.back(ed.onsets, (size_t)ed.width);
  rc = o.fetch();
  if (rc != SONAR_OK) return rc;
  *out = combine(hf, std::min(*cf, fd.width), he, std::min(*ce, ed.width),
                 (int64_t)(kComplexMinInterval * (double)sample_rate));
  return SONAR_OK;
}

int64_t complex_width(int64_t n) {
  const int64_t F = n >= SONAR_ONSET_WINDOW ? (n - SONAR_ONSET_WINDOW) / SONAR_ONSET_HOP + 1 : 0;
  const int64_t Fe = rms_frames(n, SONAR_ONSET_ENERGY_FRAME, SONAR_ONSET_ENERGY_HOP);
  return peaks_width(F - 1) + peaks_width(Fe - 1);
}

}  // namespace

extern "C" {

int64_t sonar_onset_peaks_width(int64_t n) { return peaks_width(n); }

int64_t sonar_rms_envelope_frames(int64_t n, int32_t frame_size, int32_t hop_size) {
  return rms_frames(n, frame_size, hop_size);
}

int64_t sonar_onsets_complex_width(int64_t n) { return complex_width(n); }

int sonar_onset_min_interval_frames(double min_interval, int32_t sample_rate, int32_t hop_size, int32_t* frames) {
  std::string msg;
  int32_t v = 0;
  const int rc = min_interval_frames(min_interval, sample_rate, hop_size, &v, msg);
  if (rc == SONAR_OK && frames) *frames = v;
  return rc;
}

int sonar_spectral_flux(sonar_ctx* c, const double* mag, int64_t F, int32_t K, int32_t all_changes, double* flux,
                        int32_t device_ptrs) {
  if (!c) return SONAR_ERR_INVALID;
  if (F < 0 || K < 0) return fail(c, SONAR_ERR_INVALID, "spectral flux: negative row count or row length");
  if (F < 2) return SONAR_OK;                                // :18-20
  if (K > sonar::ONSET_MAX_K)
    return fail(c, SONAR_ERR_UNSUPPORTED, "spectral flux: rows of more than " + std::to_string(sonar::ONSET_MAX_K) +
                                              " bins are not supported");
  if (!flux) return fail(c, SONAR_ERR_INVALID, "spectral flux: null flux pointer");
  HIP_TRY(c, hipSetDevice(c->device));
  Staging o{c, "flux.", device_ptrs != 0};
  if (K == 0) return o.zero({{flux, (size_t)(F - 1) * 8}});   // sqrt(0.0)
  if (!mag) return fail(c, SONAR_ERR_INVALID, "spectral flux: null magnitude pointer");
  const double* dm = o.in("mag", mag, (size_t)F * (size_t)K);
  double* df = o.out("out", flux, (size_t)(F - 1));
  int rc = o.ready("device allocation failed");
  if (rc != SONAR_OK) return rc;
  hipEvent_t tend = timed_begin(c, c->stream);
  if (sonar::launch_onset_flux(dm, F, K, all_changes != 0, df, c->stream) != 0)
    return fail(c, SONAR_ERR_DEVICE, "spectral flux launch failed");
  timed_end(c, c->stream, tend);
  return o.finish();
}

int sonar_rms_envelope(sonar_ctx* c, const double* pcm, int64_t n, int32_t frame_size, int32_t hop_size, double* env,
                       int64_t* frames, int32_t device_ptrs) {
  if (!c) return SONAR_ERR_INVALID;
  if (n < 0) return fail(c, SONAR_ERR_INVALID, "rms envelope: negative length");
  const int64_t Fe = rms_frames(n, frame_size, hop_size);
  if (frames) *frames = Fe;
  if (Fe == 0) return SONAR_OK;                              // :19-21
  if (!pcm || !env) return fail(c, SONAR_ERR_INVALID, "rms envelope: null pcm or env pointer");
  HIP_TRY(c, hipSetDevice(c->device));
  Staging o{c, "rms.", device_ptrs != 0};
  const double* dx = o.in("pcm", pcm, (size_t)n);
  double* de = o.out("env", env, (size_t)Fe);
  int rc = o.ready("device allocation failed");
  if (rc != SONAR_OK) return rc;
  hipEvent_t tend = timed_begin(c, c->stream);
  if (sonar::launch_onset_rms(dx, Fe, frame_size, hop_size, de, c->stream) != 0)
    return fail(c, SONAR_ERR_DEVICE, "rms envelope launch failed");
  timed_end(c, c->stream, tend);
  return o.finish();
}

int sonar_onset_peaks(sonar_ctx* c, const double* curve, int64_t n, double threshold, double min_interval,
                      int32_t hop_size, int32_t sample_rate, int64_t* index, int64_t* count, int32_t device_ptrs) {
  if (!c) return SONAR_ERR_INVALID;
  if (n < 0) return fail(c, SONAR_ERR_INVALID, "onset peaks: negative length");
  if (!count) return fail(c, SONAR_ERR_INVALID, "onset peaks: null count pointer");
  *count = 0;
  if (n < 3) return SONAR_OK;                                // :98-100, before the conversion
  std::string msg;
  int32_t mif = 0;
  int rc = min_interval_frames(min_interval, sample_rate, hop_size, &mif, msg);
  if (rc != SONAR_OK) return fail(c, rc, msg);
  if (!curve || !index) return fail(c, SONAR_ERR_INVALID, "onset peaks: null curve or index pointer");
  HIP_TRY(c, hipSetDevice(c->device));
  Staging o{c, "peaks1d.", device_ptrs != 0};
  const int64_t width = peaks_width(n);
  const double* dv = o.in("curve", curve, (size_t)n);
  int64_t* di = o.out("index", index, (size_t)width);
  uint64_t* mask = o.tmp<uint64_t>("mask", (size_t)sonar::onset_mask_words(n));
  int64_t* dc = o.tmp<int64_t>("count", 1);
  o.host_out(count, dc, 1);
  rc = o.ready("device allocation failed");
  if (rc != SONAR_OK) return rc;
  rc = pick(c, dv, n, threshold, mif, 1, mask, di, width, dc);
  return rc != SONAR_OK ? rc : o.finish();
}

int sonar_onset_adaptive_threshold(sonar_ctx* c, const double* curve, int64_t n, double* value, int32_t device_ptrs) {
  if (!c) return SONAR_ERR_INVALID;
  if (n < 0 || !value) return fail(c, SONAR_ERR_INVALID, "adaptive threshold: negative length or null value pointer");
  HIP_TRY(c, hipSetDevice(c->device));
  Staging o{c, "athr.", device_ptrs != 0};
  if (n == 0) return o.zero({{value, 8}});                    // :201-203
  if (!curve) return fail(c, SONAR_ERR_INVALID, "adaptive threshold: null curve pointer");
  const double* dv = o.in("curve", curve, (size_t)n);
  double* dout = o.out("value", value, 1);
  int rc = o.ready("device allocation failed");
  if (rc != SONAR_OK) return rc;
  hipEvent_t tend = timed_begin(c, c->stream);
  if (sonar::launch_onset_threshold(dv, n, dout, c->stream) != 0)
    return fail(c, SONAR_ERR_DEVICE, "adaptive threshold launch failed");
  timed_end(c, c->stream, tend);
  return o.finish();
}

int sonar_onsets_flux(sonar_ctx* c, const double* pcm, int64_t n, int32_t sample_rate, int32_t window_size,
                      int32_t hop_size, double threshold, double min_interval, int64_t* onsets, int64_t* count,
                      double* flux, double* magnitude, int64_t* frames, int32_t device_ptrs) {
  if (!c) return SONAR_ERR_INVALID;
  if (n < 0) return fail(c, SONAR_ERR_INVALID, "onsets: negative length");
  if (!count) return fail(c, SONAR_ERR_INVALID, "onsets: null count pointer");
  *count = 0;
  if (frames) *frames = 0;
  if (n == 0) return SONAR_OK;                               // :27-29
  if (sample_rate <= 0) return fail(c, SONAR_ERR_UNSUPPORTED, "onsets: sample_rate <= 0 is not reproduced");
  FluxDetector fd;
  std::string msg;
  int rc = fd.plan(n, pcm != nullptr, sample_rate, window_size, hop_size, threshold, min_interval, msg);
  if (rc != SONAR_OK) return fail(c, rc, msg);
  if (frames) *frames = fd.walk.F;
  if (fd.width > 0 && !onsets) return fail(c, SONAR_ERR_INVALID, "onsets: null onsets pointer");
  HIP_TRY(c, hipSetDevice(c->device));
  Staging o{c, "onsets.", device_ptrs != 0};
  const double* dx = o.in("pcm", pcm, (size_t)n);
  fd.alloc(o, "f.", fd.walk.F > 1 ? flux : nullptr, fd.width > 0 ? onsets : nullptr);
  o.host_out(count, fd.dcount, 1);
  rc = o.ready("device allocation failed");
  if (rc != SONAR_OK) return rc;
  rc = fd.run(c, o, dx, magnitude);
  return rc != SONAR_OK ? rc : o.finish();
}

int sonar_onsets_energy(sonar_ctx* c, const double* pcm, int64_t n, int32_t sample_rate, int32_t frame_size,
                        int32_t hop_size, double threshold, double min_interval, int64_t* onsets, int64_t* count,
                        double* curve, int64_t* n_curve, int32_t device_ptrs) {
  if (!c) return SONAR_ERR_INVALID;
  if (n < 0) return fail(c, SONAR_ERR_INVALID, "onsets: negative length");
  if (!count) return fail(c, SONAR_ERR_INVALID, "onsets: null count pointer");
  *count = 0;
  if (n_curve) *n_curve = 0;
  if (n == 0) return SONAR_OK;                               // :60-62
  EnergyDetector ed;
  std::string msg;
  int rc = ed.plan(n, sample_rate, frame_size, hop_size, threshold, min_interval, msg);
  if (rc != SONAR_OK) return fail(c, rc, msg);
  if (n_curve) *n_curve = ed.ncurve;
  if (ed.Fe == 0) return SONAR_OK;                           // :69-71
  if (!pcm) return fail(c, SONAR_ERR_INVALID, "onsets: null pcm pointer");
  if (ed.width > 0 && !onsets) return fail(c, SONAR_ERR_INVALID, "onsets: null onsets pointer");
  HIP_TRY(c, hipSetDevice(c->device));
  Staging o{c, "onsets.", device_ptrs != 0};
  const double* dx = o.in("pcm", pcm, (size_t)n);
  ed.alloc(o, "e.", ed.ncurve > 0 ? curve : nullptr, ed.width > 0 ? onsets : nullptr);
  o.host_out(count, ed.dcount, 1);
  rc = o.ready("device allocation failed");
  if (rc != SONAR_OK) return rc;
  rc = ed.run(c, dx);
  return rc != SONAR_OK ? rc : o.finish();
}

int sonar_onsets_complex(sonar_ctx* c, const double* pcm, int64_t n, int32_t sample_rate, int64_t* onsets,
                         int64_t* count, double* density, int32_t device_ptrs) {
  if (!c) return SONAR_ERR_INVALID;
  if (n < 0) return fail(c, SONAR_ERR_INVALID, "onsets: negative length");
  if (!count) return fail(c, SONAR_ERR_INVALID, "onsets: null count pointer");
  *count = 0;
  if (density) *density = 0.0;
  if (sample_rate <= 0) return fail(c, SONAR_ERR_UNSUPPORTED, "onsets: sample_rate <= 0 is not reproduced");
  if (n == 0) return SONAR_OK;                               // :124-126; the duration is 0 (:191-194)
  FluxDetector fd;
  EnergyDetector ed;
  std::string msg;
  int rc = fd.plan(n, pcm != nullptr, sample_rate, 0, 0, kFluxThreshold, kComplexMinInterval, msg);
  if (rc == SONAR_OK) rc = ed.plan(n, sample_rate, 0, 0, kEnergyThreshold, kComplexMinInterval, msg);
  if (rc != SONAR_OK) return fail(c, rc, msg);
  const int64_t width = complex_width(n);
  if (width > 0 && !onsets) return fail(c, SONAR_ERR_INVALID, "onsets: null onsets pointer");
  HIP_TRY(c, hipSetDevice(c->device));
  Staging o{c, "onsets.", device_ptrs != 0};
  const double* dx = o.in("pcm", pcm, (size_t)n);
  fd.alloc(o, "f.", nullptr, nullptr);
  ed.alloc(o, "e.", nullptr, nullptr);
  rc = o.ready("device allocation failed");
  if (rc != SONAR_OK) return rc;
  std::vector<int64_t> kept;
  rc = complex_onsets(c, o, dx, fd, ed, sample_rate, &kept);
  if (rc != SONAR_OK) return rc;
  *count = (int64_t)kept.size();
  kept.resize((size_t)width, 0);                             // the slots past count are 0
  rc = o.put(onsets, kept.data(), (size_t)width * 8);
  if (rc == SONAR_OK) rc = o.settle();
  if (rc != SONAR_OK) return rc;
  const double duration = (double)n / (double)sample_rate;   // ComputeOnsetDensity (:191-196)
  if (density) *density = duration == 0 ? 0.0 : (double)*count / duration;
  return SONAR_OK;
}

int sonar_tempo_from_onsets(const int64_t* onsets, int64_t count, int32_t sample_rate, double* tempo,
                            int32_t* bin_counts) {
  if (count < 0 || (count > 0 && !onsets) || !tempo) return SONAR_ERR_INVALID;
  if (sample_rate <= 0) return SONAR_ERR_UNSUPPORTED;
  *tempo = tempo_from_onsets(onsets, count, sample_rate, bin_counts);
  return SONAR_OK;
}

int32_t sonar_tempo_category(double tempo) { return tempo_category(tempo); }

const char* sonar_tempo_category_name(int32_t category) {
  return category >= 0 && category < 5 ? kCategoryNames[category] : "";
}

int sonar_tempo_autocorr_plan(int64_t n, int32_t sample_rate, int32_t* frame_size, int32_t* hop_size,
                              int64_t* envelope_len, int64_t* n_autocorr, int64_t* min_lag, int64_t* max_lag) {
  if (n < 0) return SONAR_ERR_INVALID;
  if (sample_rate <= 0) return SONAR_ERR_UNSUPPORTED;
  const AcPlan p = ac_plan(n, sample_rate);
  if (frame_size) *frame_size = p.frame;
  if (hop_size) *hop_size = p.hop;
  if (envelope_len) *envelope_len = p.L;
  if (n_autocorr) *n_autocorr = p.nac;
  if (min_lag) *min_lag = p.min_lag;
  if (max_lag) *max_lag = p.max_lag;
  return SONAR_OK;
}

int sonar_tempo_autocorrelation(sonar_ctx* c, const double* pcm, int64_t n, int32_t sample_rate, double* tempo,
                                int64_t* best_lag, double* autocorr, int64_t* n_autocorr, int32_t device_ptrs) {
  if (!c) return SONAR_ERR_INVALID;
  if (n < 0 || !tempo) return fail(c, SONAR_ERR_INVALID, "tempo: negative length or null tempo pointer");
  if (sample_rate <= 0) return fail(c, SONAR_ERR_UNSUPPORTED, "tempo: sample_rate <= 0 is not reproduced");
  if (n > 0 && !pcm) return fail(c, SONAR_ERR_INVALID, "tempo: null pcm pointer");
  HIP_TRY(c, hipSetDevice(c->device));
  AcEstimator ac;
  ac.plan(n, sample_rate);
  if (n_autocorr) *n_autocorr = ac.p.nac;
  Staging o{c, "tempo.", device_ptrs != 0};
  const double* dx = ac.p.L >= 10 ? o.in("pcm", pcm, (size_t)n) : nullptr;
  ac.alloc(o, "a.", autocorr);
  int rc = o.ready("device allocation failed");
  if (rc != SONAR_OK) return rc;
  double t = 0.0;
  int64_t lag = 0;
  rc = ac.run(c, o, dx, &t, &lag);
  if (rc == SONAR_OK) rc = o.put(tempo, &t, 8);
  if (rc == SONAR_OK) rc = o.put(best_lag, &lag, 8);
  return rc != SONAR_OK ? rc : o.finish();
}

int sonar_tempo(sonar_ctx* c, const double* pcm, int64_t n, int32_t sample_rate, sonar_tempo_result* result,
                int32_t device_ptrs) {
  if (!c) return SONAR_ERR_INVALID;
  if (n < 0 || !result) return fail(c, SONAR_ERR_INVALID, "tempo: negative length or null result pointer");
  if (sample_rate <= 0) return fail(c, SONAR_ERR_UNSUPPORTED, "tempo: sample_rate <= 0 is not reproduced");
  if (n > 0 && !pcm) return fail(c, SONAR_ERR_INVALID, "tempo: null pcm pointer");
  std::memset(result, 0, sizeof *result);
  HIP_TRY(c, hipSetDevice(c->device));
  FluxDetector fd;
  EnergyDetector ed;
  AcEstimator ac;
  std::string msg;
  // EstimateTempoRange drops EstimateTempo's error (:206): the STFT's "too short" leaves the onset tempo 0
  int onset_rc = SONAR_OK;
  if (n > 0) {
    onset_rc = fd.plan(n, true, sample_rate, 0, 0, kFluxThreshold, kComplexMinInterval, msg);
    if (onset_rc != SONAR_OK && onset_rc != SONAR_ERR_TOO_SHORT) return fail(c, onset_rc, msg);
    if (onset_rc == SONAR_OK) {
      const int rc = ed.plan(n, sample_rate, 0, 0, kEnergyThreshold, kComplexMinInterval, msg);
      if (rc != SONAR_OK) return fail(c, rc, msg);
    }
  }
  const bool onsets_run = n > 0 && onset_rc == SONAR_OK;
  ac.plan(n, sample_rate);
  Staging o{c, "tempo.", device_ptrs != 0};
  const double* dx = n > 0 ? o.in("pcm", pcm, (size_t)n) : nullptr;   // staged once for both estimates
  if (onsets_run) {
    fd.alloc(o, "f.", nullptr, nullptr);
    ed.alloc(o, "e.", nullptr, nullptr);
  }
  ac.alloc(o, "a.", nullptr);
  int rc = o.ready("device allocation failed");
  if (rc != SONAR_OK) return rc;
  if (onsets_run) {
    std::vector<int64_t> kept;
    rc = complex_onsets(c, o, dx, fd, ed, sample_rate, &kept);
    if (rc != SONAR_OK) return rc;
    result->onset_count = (int64_t)kept.size();
    result->onset_tempo = tempo_from_onsets(kept.data(), (int64_t)kept.size(), sample_rate, nullptr);
  }
  result->onset_error = onset_rc;
  rc = ac.run(c, o, dx, &result->autocorr_tempo, &result->best_lag);
  if (rc != SONAR_OK) return rc;
  rc = o.finish();
  if (rc != SONAR_OK) return rc;
  // EstimateTempoRange (:204-217) and ClassifyTempoCategory of the average
  result->tempo = (result->onset_tempo + result->autocorr_tempo) / 2.0;
  result->difference = std::fabs(result->onset_tempo - result->autocorr_tempo);
  result->confidence = sonar::go_max(0.0, 1.0 - result->difference / 50.0);
  result->category = tempo_category(result->tempo);
  return SONAR_OK;
}

}  // extern "C"
