// voice_api.cpp -- VoiceQualityAnalyzer.AnalyzeVoiceQuality (algorithms/speech/voice_quality.go:56-111)
// above the HIP kernels.
//
//   device: the YIN scan of 1024-sample frames at hop 256 (yin_kernel, :114-127), the RMS of every
//           extracted pitch period (period_rms_kernel, :200-207) and the 2048-lag autocorrelation
//           of calculateHNR (hnr_autocorr_kernel, :255-267);
//   host:   what Go runs sequentially on O(frames) data, in host_dsp.cpp -- the PitchDetector temporal
//           tracking (pitch_detection.go:767-921) and the period walk whose start depends on the
//           previous period's end (period_walk, :133-151), and the scalar formulas
//           (voice_quality_from, :160-451).
// The second device pass needs the walk's periods, so a call synchronises twice.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"
#include "host_dsp.h"
#include "kernels.h"
#include "staging.h"

using sonar::detail::fail;
using sonar::detail::Staging;
using sonar::host::PitchPeriods;

namespace {

constexpr const char* kNoMem = "device allocation failed (voice quality)";

// extractPitchPeriodsAndF0's device half (:114-127): the raw YIN rows of frames i = 0, 256, ... while
// i < n - 1024 (Fl of them: with exactly 1024 samples calculateVoicingStrength's DetectPitch(signal),
// :363-371, reads frame 0 too), and the first min(n, 1024) samples; queued, not waited for
int yin_pass(sonar_ctx* c, const double* dy, int64_t n, int32_t sr, int64_t Fl, std::vector<double>& praw,
             std::vector<double>& craw, std::vector<double>& head) {
  hipStream_t s = c->stream;
  praw.resize(Fl); craw.resize(Fl); head.resize(std::min<int64_t>(n, 1024));
  if (Fl > 0) {
    Staging st{c, "vq.", true};
    double* dp = st.tmp<double>("pitch", Fl);
    double* dc = st.tmp<double>("conf", Fl);
    if (const int rc = st.ready(kNoMem)) return rc;
    if (sonar::launch_yin(dy, n, Fl, 256, sr, dp, dc, nullptr, s) != 0)
      return fail(c, SONAR_ERR_DEVICE, "yin launch failed");
    HIP_TRY(c, hipMemcpyAsync(praw.data(), dp, Fl * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(craw.data(), dc, Fl * 8, hipMemcpyDeviceToHost, s));
  }
  if (!head.empty()) HIP_TRY(c, hipMemcpyAsync(head.data(), dy, head.size() * 8, hipMemcpyDeviceToHost, s));
  return SONAR_OK;
}

// the RMS of every period (:200-207) and, for n >= 2048, the autocorrelation of the 2048 samples around
// the middle (calculateHNR :245-267); queued, not waited for.  ac stays empty without that frame.
int period_pass(sonar_ctx* c, const double* dy, int64_t n, const PitchPeriods& w, std::vector<double>& amp,
                std::vector<double>& ac) {
  hipStream_t s = c->stream;
  const size_t np = w.st.size();
  Staging st{c, "vq.", false};
  const int64_t* dst = st.in("start", w.st.data(), np);
  const int64_t* dln = st.in("len", w.ln.data(), np);
  double* damp = st.tmp<double>("amp", np);
  double* dac = st.tmp<double>("ac", 2048);
  if (const int rc = st.ready(kNoMem)) return rc;
  if (sonar::launch_period_rms(dy, dst, dln, np, damp, s) != 0) return fail(c, SONAR_ERR_DEVICE, "period rms launch failed");
  const bool hnr_frame = n >= 2048;
  if (hnr_frame && sonar::launch_hnr_autocorr(dy + std::max<int64_t>(n / 2 - 1024, 0), dac, s) != 0)
    return fail(c, SONAR_ERR_DEVICE, "hnr launch failed");
  amp.resize(np); ac.resize(hnr_frame ? 2048 : 0);
  HIP_TRY(c, hipMemcpyAsync(amp.data(), damp, np * 8, hipMemcpyDeviceToHost, s));
  if (hnr_frame) HIP_TRY(c, hipMemcpyAsync(ac.data(), dac, 2048 * 8, hipMemcpyDeviceToHost, s));
  return SONAR_OK;
}

}  // namespace

namespace sonar {
namespace detail {

int voice_quality(sonar_ctx* c, const double* dy, int64_t n, int32_t sr, sonar_voice_quality_result* q) {
  std::memset(q, 0, sizeof(*q));
  if (n < (int64_t)sr)                                             // :57-59
    return fail(c, SONAR_ERR_TOO_SHORT, "signal too short for voice quality analysis (need at least 1 second)");
  HIP_TRY(c, hipSetDevice(c->device));
  const int64_t Fv = n > 1024 ? (n - 1025) / 256 + 1 : 0;
  const int64_t Fl = std::max<int64_t>(Fv, n == 1024 ? 1 : 0);
  std::vector<double> praw, craw, head, amp, ac;
  DrainOnExit drain{c};            // declared after the host arrays: an early exit waits for the copies into them
  if (const int rc = yin_pass(c, dy, n, sr, Fl, praw, craw, head)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const PitchPeriods w = sonar::host::period_walk(praw.data(), craw.data(), Fv, n, sr);
  const int64_t np = (int64_t)w.st.size();
  if (np < 3) {                                                    // :67-69
    drain.armed = false;
    return fail(c, SONAR_ERR_TOO_SHORT, "insufficient pitch periods for analysis (found " + std::to_string(np) +
                                            ", need at least 3)");
  }
  if (const int rc = period_pass(c, dy, n, w, amp, ac)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  drain.armed = false;
  *q = sonar::host::voice_quality_from(w.ln.data(), amp.data(), w.f0.data(), np, ac.empty() ? nullptr : ac.data(),
                                       head.data(), n, sr, w.voicing);
  return SONAR_OK;
}

}  // namespace detail
}  // namespace sonar

extern "C" int sonar_voice_quality(sonar_ctx* c, const double* pcm, int64_t n, int32_t sample_rate,
                                   sonar_voice_quality_result* out) {
  if (!c || !out) return fail(c, SONAR_ERR_INVALID, "null argument");
  std::memset(out, 0, sizeof(*out));
  if (n < (int64_t)sample_rate)
    return fail(c, SONAR_ERR_TOO_SHORT, "signal too short for voice quality analysis (need at least 1 second)");
  if (n > 0 && !pcm) return fail(c, SONAR_ERR_INVALID, "null buffer");
  HIP_TRY(c, hipSetDevice(c->device));
  Staging st{c, "vq.", false};
  const double* d = n > 0 ? st.in("pcm", pcm, n) : st.tmp<double>("pcm", 1);
  if (const int rc = st.ready(kNoMem)) return rc;
  return sonar::detail::voice_quality(c, d, n, sample_rate, out);
}
