// cqt_api.cpp -- sonar_chroma_cqt_plan / sonar_chroma_cqt: ChromaCQT.ComputeChroma
// (algorithms/chroma/chroma_cqt.go:69-92).  The host side of computeCQTKernel (:95-165): the bin
// frequencies, kernel lengths, FFT size and the taps in the reference's order of operations; the
// chroma class of every bin (:224-230, :245-252); the frame count (:169-172).  Taps and classes are one
// cached table per parameter set (ctx.h, cached_table); the PCM and the outputs are staged by
// staging.h.  The kernels are cqt_kernels.hip's.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"
#include "go_math.h"
#include "kernels.h"
#include "staging.h"

using sonar::go_log2;
using sonar::detail::fail;
using sonar::detail::Staging;
using sonar::detail::timed_begin;
using sonar::detail::timed_end;

namespace {

constexpr int64_t kMaxBins = 65536;                 // bins (Go has no limit; the table would not fit long before)
constexpr int64_t kMaxTableDoubles = int64_t(1) << 27;   // 1 GiB of padded taps

struct CqtPlan {
  int64_t K = 0, N = 0, F = 0, sum_taps = 0;
  std::vector<double> freq;
  std::vector<int32_t> len, cls;
};

// calculateKernelLength (:147-165)
int32_t kernel_len(double q, int32_t sr, double f) {
  const double v = q * (double)sr / f;
  int64_t L = v >= 4.0e18 ? (int64_t)4e18 : (int64_t)v;   // beyond int64 Go's conversion is not defined; the cap below takes it
  if (L % 2 == 0) L++;
  if (L < 3) L = 3;
  if (L > sr / 2) L = sr / 2;
  return (int32_t)L;
}

// The parameter side (want_frames: and the frame count).  msg: Go's panic text or what is unsupported.
int cqt_plan(int32_t sr, double minf, double maxf, int32_t bpo, double q, double tuning, int64_t n, int64_t hop,
             CqtPlan& p, std::string& msg) {
  auto bad = [](double v) { return !std::isfinite(v) || v <= 0.0; };
  if (bad(minf) || bad(maxf) || bad(q) || bad(tuning)) {
    msg = "chroma CQT: a non-finite or non-positive min_freq, max_freq, q_factor or tuning_freq is not reproduced";
    return SONAR_ERR_UNSUPPORTED;
  }
  if (bpo < 1) { msg = "chroma CQT: bins_per_octave < 1 is not reproduced"; return SONAR_ERR_UNSUPPORTED; }
  if (sr < 6) { msg = "chroma CQT: sample_rate < 6 is not reproduced"; return SONAR_ERR_UNSUPPORTED; }
  const double nb = go_log2(maxf / minf) * (double)bpo;    // :97-98
  if (nb <= -9.2e18) p.K = INT64_MIN;                       // amd64's conversion of an out-of-range value
  else if (nb >= (double)(kMaxBins + 1)) {
    msg = "chroma CQT: more than " + std::to_string(kMaxBins) + " bins are not supported";
    return SONAR_ERR_UNSUPPORTED;
  } else p.K = (int64_t)nb;
  if (p.K < 0) { msg = "runtime error: makeslice: len out of range"; return SONAR_ERR_PANIC; }             // :101
  if (p.K == 0) { msg = "runtime error: index out of range [0] with length 0"; return SONAR_ERR_PANIC; }   // :107
  p.freq.resize((size_t)p.K);
  p.len.resize((size_t)p.K);
  p.cls.resize((size_t)p.K);
  p.sum_taps = 0;
  for (int64_t k = 0; k < p.K; ++k) {
    const double f = minf * std::pow(2.0, (double)k / (double)bpo);   // :103
    p.freq[(size_t)k] = f;
    p.len[(size_t)k] = kernel_len(q, sr, f);
    p.sum_taps += p.len[(size_t)k];
    // frequencyToMIDI (:245-252), math.Round (half away from zero), Go's % (sign of the dividend)
    const double midi = f <= 0.0 ? 0.0 : 69.0 + 12.0 * go_log2(f / tuning);
    const double r = std::round(midi);
    int64_t c = (std::isfinite(r) && std::fabs(r) < 9.0e18) ? (int64_t)r % 12 : 0;
    if (c < 0) c += 12;
    p.cls[(size_t)k] = (int32_t)c;
  }
  p.N = 1;                                                  // nextPowerOfTwo(maxKernelLength * 2) :107-108
  while (p.N < 2 * (int64_t)p.len[0]) p.N <<= 1;
  if (n == 0) { p.F = 0; return SONAR_OK; }                 // ComputeChroma returns before the division (:70-72)
  if (hop == 0) { msg = "runtime error: integer divide by zero"; return SONAR_ERR_PANIC; }   // :169
  p.F = (n - hop) / hop;                                    // truncating, as Go's
  if (p.F <= 0) p.F = 1;
  return SONAR_OK;
}

// The device table of one parameter set, cached in the context under the set's bits until sonar_trim:
// the padded taps by bin group (kernels.h, CqtArgs), the groups' offsets and padded lengths, the classes.
struct CqtTables {
  const double* tab;
  const int64_t* goff;
  const int32_t* lpad;
  const int32_t* cls;
};

int cqt_tables(sonar_ctx* c, const CqtPlan& p, int32_t sr, double q, double minf, double maxf, int32_t bpo,
               double tuning, CqtTables* out) {
  char key[160];
  uint64_t b[4];
  std::memcpy(&b[0], &minf, 8); std::memcpy(&b[1], &maxf, 8); std::memcpy(&b[2], &q, 8); std::memcpy(&b[3], &tuning, 8);
  std::snprintf(key, sizeof key, "cqt.%d.%d.%016llx.%016llx.%016llx.%016llx", sr, bpo, (unsigned long long)b[0],
                (unsigned long long)b[1], (unsigned long long)b[2], (unsigned long long)b[3]);
  const int ng = (int)((p.K + sonar::CQT_BK - 1) / sonar::CQT_BK);
  std::vector<int64_t> goff((size_t)ng);
  std::vector<int32_t> lpad((size_t)ng);
  int64_t total = 0;
  for (int g = 0; g < ng; ++g) {
    int32_t L = 0;                                          // the group's longest (its first: lengths fall with the bin index)
    for (int64_t k = (int64_t)g * sonar::CQT_BK; k < std::min<int64_t>(p.K, (int64_t)(g + 1) * sonar::CQT_BK); ++k)
      L = std::max(L, p.len[(size_t)k]);
    lpad[(size_t)g] = (L + 63) / 64 * 64;
    goff[(size_t)g] = total;
    total += (int64_t)sonar::CQT_BK * lpad[(size_t)g];
  }
  if (total > kMaxTableDoubles) return fail(c, SONAR_ERR_UNSUPPORTED, "chroma CQT: the tap table of this configuration exceeds 1 GiB");
  // one image: the taps, then the groups' offsets and padded lengths and the bins' classes
  const size_t tab_bytes = (size_t)total * 8, meta_bytes = (size_t)ng * 8 + (size_t)ng * 4 + (size_t)p.K * 4;
  const unsigned char* img = nullptr;
  const int rc = sonar::detail::cached_table(c, key, "chroma CQT tap table", [&](std::vector<unsigned char>& image, int64_t&) {
    image.assign(tab_bytes + meta_bytes, 0);
    double* tab = (double*)image.data();
    for (int64_t k = 0; k < p.K; ++k) {
      const int g = (int)(k / sonar::CQT_BK);
      double* row = tab + goff[(size_t)g] + (k % sonar::CQT_BK) * (int64_t)lpad[(size_t)g];
      const double freq = p.freq[(size_t)k];
      const int32_t L = p.len[(size_t)k];
      const double bandwidth = freq / q;                                  // :120
      const double sigma = (double)sr / (2.0 * M_PI * bandwidth);         // :121
      const int32_t center = L / 2;                                       // :123
      for (int32_t i = 0; i < L; ++i) {
        const double t = (double)(i - center);
        const double window = std::exp(-(t * t) / (2.0 * sigma * sigma)); // :128
        const double phase = 2.0 * M_PI * freq * t / (double)sr;          // :131
        double sn, cs;
        ::sincos(phase, &sn, &cs);                                        // cmplx.Exp(complex(0, phase)) :132
        row[i] = std::hypot(window * cs, window * sn);                    // cmplx.Abs of the product :135, :309
      }
    }
    unsigned char* meta = image.data() + tab_bytes;
    std::memcpy(meta, goff.data(), (size_t)ng * 8);
    std::memcpy(meta + (size_t)ng * 8, lpad.data(), (size_t)ng * 4);
    std::memcpy(meta + (size_t)ng * 12, p.cls.data(), (size_t)p.K * 4);
    return SONAR_OK;
  }, &img);
  // an upload that failed is reported like an allocation that failed, as before
  if (rc != SONAR_OK) return fail(c, SONAR_ERR_NOMEM, "device allocation failed (chroma CQT tap table)");
  const unsigned char* m = img + tab_bytes;
  out->tab = (const double*)img;
  out->goff = (const int64_t*)m;
  out->lpad = (const int32_t*)(m + (size_t)ng * 8);
  out->cls = (const int32_t*)(m + (size_t)ng * 12);
  return SONAR_OK;
}

}  // namespace

extern "C" {

int sonar_chroma_cqt_plan(int32_t sample_rate, double min_freq, double max_freq, int32_t bins_per_octave,
                          double q_factor, double tuning_freq, int64_t n, int64_t hop, int64_t* total_bins,
                          int64_t* fft_size, int64_t* n_frames, int64_t* sum_taps, int32_t* kernel_len,
                          int32_t* chroma_bin) {
  if (n < 0) return SONAR_ERR_INVALID;
  CqtPlan p;
  std::string msg;
  const int rc = cqt_plan(sample_rate, min_freq, max_freq, bins_per_octave, q_factor, tuning_freq, n, hop, p, msg);
  if (total_bins) *total_bins = p.K;
  if (p.K <= 0 || p.len.empty()) return rc;
  if (fft_size) *fft_size = p.N;
  if (sum_taps) *sum_taps = p.sum_taps;
  if (kernel_len) std::memcpy(kernel_len, p.len.data(), (size_t)p.K * 4);
  if (chroma_bin) std::memcpy(chroma_bin, p.cls.data(), (size_t)p.K * 4);
  if (rc == SONAR_OK && n_frames) *n_frames = p.F;
  return rc;
}

int sonar_chroma_cqt(sonar_ctx* c, const double* pcm, int64_t n, int64_t hop, int32_t sample_rate, double min_freq,
                     double max_freq, int32_t bins_per_octave, double q_factor, double tuning_freq, double* chroma,
                     double* cqt, int32_t device_ptrs) {
  if (!c || n < 0) return SONAR_ERR_INVALID;
  if (n == 0) return SONAR_OK;                              // :70-72: nil, nil
  if (!pcm || !chroma) return fail(c, SONAR_ERR_INVALID, "chroma CQT: null pcm or chroma pointer");
  CqtPlan p;
  std::string msg;
  const int prc = cqt_plan(sample_rate, min_freq, max_freq, bins_per_octave, q_factor, tuning_freq, n, hop, p, msg);
  if (prc != SONAR_OK) return fail(c, prc, msg);
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  CqtTables T{};
  const int trc = cqt_tables(c, p, sample_rate, q_factor, min_freq, max_freq, bins_per_octave, tuning_freq, &T);
  if (trc != SONAR_OK) return trc;
  Staging o{c, "cqt.", device_ptrs != 0};
  const double* dx = o.in("pcm", pcm, (size_t)n);
  // the kernel writes the constant-Q rows in every call: scratch when the caller does not take them
  const size_t cqt_count = (size_t)p.F * (size_t)p.K;
  double* dq = cqt ? o.out("out", cqt, cqt_count) : o.tmp<double>("out", cqt_count);
  double* dc = o.out("chroma", chroma, (size_t)p.F * 12);
  int32_t* flag = o.flag();
  const int src = o.ready("device allocation failed");
  if (src != SONAR_OK) return src;
  // non-finite PCM is refused before any output is written
  if (sonar::launch_nonfinite(dx, n, flag, s) != 0) return fail(c, SONAR_ERR_DEVICE, "chroma CQT launch failed");
  const int frc = o.fetch();
  if (frc != SONAR_OK) return frc;
  if (o.flags())
    return fail(c, SONAR_ERR_UNSUPPORTED, "chroma CQT: non-finite PCM is not reproduced (the reference spreads it through its FFT)");
  sonar::CqtArgs a{};
  a.x = dx; a.n = n; a.hop = hop; a.F = p.F;
  a.K = (int)p.K; a.ngroups = (int)((p.K + sonar::CQT_BK - 1) / sonar::CQT_BK);
  a.N = (double)p.N;
  a.tab = T.tab; a.goff = T.goff; a.lpad = T.lpad; a.cls = T.cls;
  a.cqt = dq; a.chroma = dc;
  hipEvent_t tend = timed_begin(c, s);
  const int rc = sonar::launch_chroma_cqt(a, s);
  if (rc == -1) return fail(c, SONAR_ERR_UNSUPPORTED, "chroma CQT: more frames or bins than one launch takes");
  if (rc != 0) return fail(c, SONAR_ERR_DEVICE, "chroma CQT launch failed");
  timed_end(c, s, tend);
  return o.finish();
}

}  // extern "C"
