// content_api.cpp -- ContentDetector (fingerprint/content_detector.go) behind the C ABI.
// The whole-PCM passes and the direct DFT run on the device (content_kernels.hip); the
// metadata rules are string matching on the host, and the per-frame sums come back to the
// host for the scalar reductions in Go's order (frames are 1/512 of the samples).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cctype>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"
#include "host_dsp.h"
#include "kernels.h"
#include "staging.h"

using sonar::detail::fail;
using sonar::detail::Staging;

namespace {

std::string lower(std::string s) {            // strings.ToLower (ASCII)
  for (char& ch : s) ch = (char)std::tolower((unsigned char)ch);
  return s;
}
std::string trim(const std::string& s) {      // strings.TrimSpace (ASCII whitespace)
  size_t a = 0, b = s.size();
  while (a < b && std::isspace((unsigned char)s[a])) a++;
  while (b > a && std::isspace((unsigned char)s[b - 1])) b--;
  return s.substr(a, b - a);
}
bool has(const std::string& s, const char* sub) { return s.find(sub) != std::string::npos; }
bool any_of(const std::string& s, const char* const* list) {
  for (; *list; ++list)
    if (has(s, *list)) return true;
  return false;
}

// parseContentType (:615-626)
int parse_content_type(const std::string& ct) {
  const std::string v = lower(ct);
  if (v == "music" || v == "audio/music") return SONAR_CT_MUSIC;
  if (v == "news" || v == "talk" || v == "spoken") return SONAR_CT_NEWS;
  if (v == "sports") return SONAR_CT_SPORTS;
  return SONAR_CT_UNKNOWN;
}

// inferFromGenre (:501-551)
int infer_from_genre(const std::string& g0) {
  static const char* const music[] = {"rock", "pop", "jazz", "classical", "hip-hop", "hip hop", "country",
                                      "electronic", "blues", "reggae", "folk", "metal", "punk", "r&b", "soul",
                                      "funk", "dance", "techno", "house", "ambient", "indie", "alternative",
                                      "grunge", "ska", "latin", "world", "gospel", nullptr};
  static const char* const news[] = {"news", "talk", "politics", "current affairs", "public radio", "discussion",
                                     "interview", "call-in", "spoken word", "commentary", "analysis", "reporting",
                                     "journalism", "public affairs", nullptr};
  static const char* const sports[] = {"sports", "football", "basketball", "baseball", "soccer", "hockey",
                                       "tennis", "golf", "racing", "motorsports", "athletics", "cricket", "rugby",
                                       "boxing", "mma", "sports talk", "sports news", nullptr};
  const std::string g = lower(trim(g0));
  if (any_of(g, music)) return SONAR_CT_MUSIC;
  if (any_of(g, news)) return SONAR_CT_NEWS;
  if (any_of(g, sports)) return SONAR_CT_SPORTS;
  if (has(g, "talk") && !has(g, "sports")) return SONAR_CT_TALK;
  return SONAR_CT_UNKNOWN;
}

// inferFromStation (:554-599)
int infer_from_station(const std::string& station, const std::string& url) {
  static const char* const news[] = {"news", "npr", "bbc", "cnn", "cbc", "abc news", "nbc news", "fox news",
                                     "public radio", "current affairs", "talk radio", nullptr};
  static const char* const sports[] = {"sports", "espn", "fox sports", "sports radio", "the fan", "sport",
                                       "athletic", "game", "stadium", nullptr};
  static const char* const music[] = {"fm", "music", "hits", "rock", "pop", "jazz", "country", "classic", "radio",
                                      "mix", "beat", "sound", "groove", nullptr};
  const std::string combined = lower(trim(station)) + " " + lower(url);
  if (any_of(combined, news)) return SONAR_CT_NEWS;
  if (any_of(combined, sports)) return SONAR_CT_SPORTS;
  if (any_of(combined, music)) return SONAR_CT_MUSIC;
  if (has(combined, "talk") && !has(combined, "sports")) return SONAR_CT_TALK;
  return SONAR_CT_UNKNOWN;
}

// detectContentTypeFromMetadata (:602-613)
int from_metadata(const char* ct, const char* genre, const char* station, const char* url) {
  const std::string c = ct ? ct : "", g = genre ? genre : "";
  if (!c.empty()) return parse_content_type(c);
  if (!g.empty()) return infer_from_genre(g);
  return infer_from_station(station ? station : "", url ? url : "");
}

// What detect_from_audio derives from the sample count and rate: the DFT's size, the frame counts, and the
// sections of its one scratch block, the same on the device and in its host copy: the scan's three 64-bit
// words (sign changes, max |x|, min |x|) in 64 bytes, the K magnitudes, the fe sums of squares of frames
// 1024 / 512 and the ft of frames of 100 ms.
struct ContentPlan {
  static constexpr size_t kWords = 8;         // doubles
  int N, K;
  int64_t fe, ts, ft;
  ContentPlan(int64_t n, int32_t sr)
      : N((int)std::min<int64_t>(2048, n)), K(N / 2 + 1),
        fe(n > 1024 ? (n - 1024 + 511) / 512 : 0),                 // i < n - 1024, i += 512
        ts(sr / 10), ft(n > ts ? (n - ts + ts - 1) / ts : 0) {}    // i < n - ts, i += ts
  size_t doubles() const { return kWords + (size_t)(K + fe + ft); }
  template <typename D> D* mag(D* block) const { return block + kWords; }
  template <typename D> D* esum(D* block) const { return mag(block) + K; }
  template <typename D> D* tsum(D* block) const { return esum(block) + fe; }
};

// the PCM to the device, the four launches, and the block's copy into `host`, all queued on c->stream
int scan(sonar_ctx* c, const double* pcm, int64_t n, const ContentPlan& p, double* host) {
  hipStream_t s = c->stream;
  Staging st{c, "cd.", false};
  const double* x = st.in("pcm", pcm, n);
  double* w = st.tmp<double>("work", p.doubles());
  if (const int rc = st.ready("device allocation failed")) return rc;
  hipEvent_t tend = sonar::detail::timed_begin(c, s);
  if (sonar::launch_detect_scan(x, n, reinterpret_cast<unsigned long long*>(w), s) ||
      sonar::launch_frame_sums(x, n, p.fe, 512, 1024, p.esum(w), s) ||
      sonar::launch_frame_sums(x, n, p.ft, p.ts, p.ts, p.tsum(w), s) || sonar::launch_dft_mag(x, p.N, p.mag(w), s))
    return fail(c, SONAR_ERR_DEVICE, "content detection launch failed");
  sonar::detail::timed_end(c, s, tend);
  HIP_TRY(c, hipMemcpyAsync(host, w, p.doubles() * sizeof(double), hipMemcpyDeviceToHost, s));
  return SONAR_OK;
}

}  // namespace

namespace sonar {
namespace detail {

// DetectFromAudio (:72-101): extractAcousticFeatures (:118-150) and classifyFromFeatures (:153-217) are
// host_dsp.cpp's, over what the four launches below leave in the scratch block
int detect_from_audio(sonar_ctx* c, const double* pcm, int64_t n, int32_t sr, double thr, int32_t* out,
                      sonar_acoustic_features* feat) {
  sonar_acoustic_features f;
  std::memset(&f, 0, sizeof(f));
  if (n <= 0 || !pcm) {                       // :73-75
    *out = SONAR_CT_UNKNOWN;
    if (feat) *feat = f;
    return SONAR_OK;
  }
  if (sr < 10) return fail(c, SONAR_ERR_INVALID, "sample rate below 10 Hz: the 100 ms frame loop of "
                                                 "calculateTemporalStability never ends (content_detector.go:392-402)");
  const ContentPlan p(n, sr);
  std::vector<double> h(p.doubles());         // the block on the host
  sonar::detail::DrainOnExit drain{c};        // declared after h: an early exit waits for the copy into it
  if (const int rc = scan(c, pcm, n, p, h.data())) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  drain.armed = false;
  unsigned long long crossings;
  double mx, mn;
  std::memcpy(&crossings, h.data(), 8);
  std::memcpy(&mx, h.data() + 1, 8);
  std::memcpy(&mn, h.data() + 2, 8);
  f = sonar::host::content_features(crossings, mx, mn, p.mag(h.data()), p.K, p.esum(h.data()), p.fe,
                                    p.tsum(h.data()), p.ft, n, sr);
  const sonar::host::ContentClass cls = sonar::host::classify_content(f, thr);
  f.classification_confidence = cls.confidence;
  *out = cls.type;
  if (feat) *feat = f;
  return SONAR_OK;
}

// DetectContentType (:31-69)
int detect_content_type(sonar_ctx* c, const double* pcm, int64_t n, int32_t sr, int32_t has_md, const char* ct,
                        const char* genre, const char* station, const char* url, int32_t acoustic,
                        int32_t dflt, double thr, int32_t* out) {
  if (has_md) {
    const int m = from_metadata(ct, genre, station, url);
    if (m != SONAR_CT_UNKNOWN) { *out = m; return SONAR_OK; }
  }
  if (acoustic && n > 0) {
    int32_t a = SONAR_CT_UNKNOWN;
    const int rc = detect_from_audio(c, pcm, n, sr, thr, &a, nullptr);
    if (rc != SONAR_OK) return rc;
    if (a != SONAR_CT_UNKNOWN) { *out = a; return SONAR_OK; }
  }
  *out = dflt;
  return SONAR_OK;
}

}  // namespace detail
}  // namespace sonar

extern "C" {

int sonar_detect_from_audio(sonar_ctx* c, const double* pcm, int64_t n, int32_t sample_rate,
                            double auto_detect_threshold, int32_t* content_type, sonar_acoustic_features* features) {
  if (!c || !content_type) return fail(c, SONAR_ERR_INVALID, "null argument");
  if (n < 0) return fail(c, SONAR_ERR_INVALID, "negative length");
  return sonar::detail::detect_from_audio(c, pcm, n, sample_rate, auto_detect_threshold, content_type, features);
}

int sonar_detect_content_type(sonar_ctx* c, const double* pcm, int64_t n, int32_t sample_rate, int32_t has_metadata,
                              const char* content_type, const char* genre, const char* station, const char* url,
                              int32_t acoustic_detection, int32_t default_content_type, double auto_detect_threshold,
                              int32_t* out_content_type) {
  if (!c || !out_content_type) return fail(c, SONAR_ERR_INVALID, "null argument");
  if (n < 0) return fail(c, SONAR_ERR_INVALID, "negative length");
  return sonar::detail::detect_content_type(c, pcm, n, sample_rate, has_metadata, content_type, genre, station, url,
                                            acoustic_detection, default_content_type, auto_detect_threshold,
                                            out_content_type);
}

}  // extern "C"
