// xcorr_api.cpp -- sonar_xcorr_params / sonar_autocorr: CrossCorrelation.Compute and
// AutoCorrelation.Compute (algorithms/stats/correlation.go:131-200, 669-690) for every correlation
// type, method and constructor.  The kernels are xcorr_kernels.hip's (Pearson per lag, subtractMean,
// the FFT method) and ncc_kernels.hip's (z-score, NCC lag sums); the peak, p-value and quality
// metrics are host::ncc_metrics, as in sonar_ncc.  The signals and the scratch are staged by staging.h;
// the FFT twiddles are a cached table (ctx.h, cached_table).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"
#include "host_dsp.h"
#include "kernels.h"
#include "staging.h"

using sonar::detail::fail;
using sonar::detail::Staging;
using sonar::detail::timed_begin;
using sonar::detail::timed_end;

namespace {

// nextPowerOf2 (correlation.go:713-723)
int64_t next_pow2(int64_t n) {
  int64_t p = 1;
  while (p < n) p <<= 1;
  return p;
}

// The (cos, sin) pairs of -2 pi m / N, m < N / 2, on the device: the twiddles of fft's top level
// (:748), which serve every level by stride (xcorr_kernels.hip).  libm on the host, as the checker and the oracle.
// One cached table per N and context (ctx.h, cached_table); sonar_trim releases it.  Null on failure.
const double2* xcorr_twiddles(sonar_ctx* c, int64_t N) {
  const unsigned char* tw = nullptr;
  const int rc = sonar::detail::cached_table(c, "xcorr.tw." + std::to_string(N), "correlation FFT", [&](std::vector<unsigned char>& img, int64_t&) {
    const int64_t half = N / 2;
    img.resize((size_t)half * sizeof(double2));
    double2* h = (double2*)img.data();
    for (int64_t m = 0; m < half; ++m) {
      // one sincos call, as the oracle's cos(th), sin(th) pair compiles to: glibc's sincos and its
      // sin / cos differ in the last bit for a few angles
      ::sincos(-2.0 * M_PI * (double)m / (double)N, &h[m].y, &h[m].x);
    }
    return SONAR_OK;
  }, &tw);
  return rc == SONAR_OK ? (const double2*)tw : nullptr;
}

// Compute (:131-200).  same: signal2 is signal1 (AutoCorrelation.Compute :682-684)
int xcorr_run(sonar_ctx* c, const double* a, int64_t na, const double* b, int64_t nb, int32_t max_lag, int32_t corr_type,
              int32_t method, int32_t use_fft, double* corr, double* metrics, int32_t device_ptrs, bool same) {
  if (!c) return SONAR_ERR_INVALID;
  if (na <= 0 || nb <= 0 || !a || !b) return fail(c, SONAR_ERR_EMPTY, "empty signals provided");
  constexpr int64_t kFftThreshold = 1000;                         // fftThreshold in every constructor
  if (use_fft && (na > kFftThreshold || nb > kFftThreshold)) method = SONAR_CORR_FREQUENCY_DOMAIN;   // :139-142
  if (method != SONAR_CORR_TIME_DOMAIN && method != SONAR_CORR_FREQUENCY_DOMAIN && method != SONAR_CORR_SLIDING_WINDOW)
    return fail(c, SONAR_ERR_INVALID, "unsupported correlation method");
  const bool fft = method == SONAR_CORR_FREQUENCY_DOMAIN;
  int64_t N = 0;
  if (fft) {
    if (na + nb - 1 > sonar::XCORR_FFT_MAX_N)
      return fail(c, SONAR_ERR_UNSUPPORTED, "frequency-domain correlation: len(signal1) + len(signal2) - 1 = " +
                                                std::to_string(na + nb - 1) + " exceeds the FFT limit of " +
                                                std::to_string(sonar::XCORR_FFT_MAX_N) + " points");
    N = next_pow2(na + nb - 1);
  }
  const int64_t L = sonar::detail::ncc_max_lag(max_lag, na, nb), nl = 2 * L + 1;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  Staging o{c, "xcorr.", device_ptrs != 0};
  const double* da = o.in("a", a, (size_t)na);
  const double* db = same ? da : o.in("b", b, (size_t)nb);
  double* xa = o.tmp<double>("xa", (size_t)na);
  double* xb = o.tmp<double>("xb", (size_t)nb);
  double* st = o.tmp<double>("stats", 16);                        // [0..3] z-score, [8..11] subtractMean
  // the correlation also goes to the host for the metrics, so a host array is filled from that copy
  double* dc = (o.dev && corr) ? corr : o.tmp<double>("corr", (size_t)nl);
  const int src = o.ready("device allocation failed");
  if (src != SONAR_OK) return src;
  const double2* tw = nullptr;
  double2 *A = nullptr, *B = nullptr, *C = nullptr;
  if (fft) {
    tw = xcorr_twiddles(c, N);
    A = o.tmp<double2>("fa", (size_t)N);
    B = same ? A : o.tmp<double2>("fb", (size_t)N);
    C = o.tmp<double2>("fc", (size_t)N);
    if (!tw || o.nomem) return fail(c, SONAR_ERR_NOMEM, "device allocation failed (correlation FFT)");
  }
  hipEvent_t tend = timed_begin(c, s);
  int rc = sonar::launch_ncc_zscore(da, na, db, nb, xa, xb, st, s);   // normalizeInputs is true in every constructor
  if (rc == 0) {
    if (fft) {                                                    // computeFFT: the type is not consulted
      rc = sonar::launch_xcorr_fft(xa, na, same ? xa : xb, nb, N, tw, A, B, C, L, dc, s);
    } else if (corr_type == SONAR_CORR_NCC) {
      rc = sonar::launch_ncc_lags(xa, na, xb, nb, L, dc, s);
    } else if (corr_type == SONAR_CORR_ZNCC) {
      rc = sonar::launch_ncc_stats(xa, na, xb, nb, st + 8, s);
      if (rc == 0) rc = sonar::launch_xcorr_center(xa, na, xb, nb, st + 8, s);
      if (rc == 0) rc = sonar::launch_ncc_lags(xa, na, xb, nb, L, dc, s);
    } else {                                                      // Pearson, Spearman, Kendall, unknown (:301-310)
      rc = sonar::launch_xcorr_pearson(xa, na, xb, nb, L, dc, s);
    }
  }
  if (rc != 0) return fail(c, SONAR_ERR_DEVICE, "correlation launch failed");
  timed_end(c, s, tend);
  const double* hc = o.back(dc, (size_t)nl);
  const int frc = o.finish();
  if (frc != SONAR_OK) return frc;
  if (corr && !o.dev) std::memcpy(corr, hc, nl * 8);
  if (metrics) {
    sonar::detail::ncc_metrics_host(hc, L, na, nb, metrics);   // [0..9], as sonar_ncc
    metrics[10] = (double)method;
    metrics[11] = (double)corr_type;
  }
  return SONAR_OK;
}

}  // namespace

extern "C" {

int sonar_xcorr_params(sonar_ctx* c, const double* a, int64_t na, const double* b, int64_t nb, int32_t max_lag,
                       int32_t corr_type, int32_t method, int32_t use_fft, double* corr, double* metrics,
                       int32_t device_ptrs) {
  return xcorr_run(c, a, na, b, nb, max_lag, corr_type, method, use_fft, corr, metrics, device_ptrs,
                   a == b && na == nb);
}

int sonar_autocorr(sonar_ctx* c, const double* x, int64_t n, int32_t max_lag, int32_t corr_type, int32_t method,
                   double* corr, double* metrics, int32_t device_ptrs) {
  return xcorr_run(c, x, n, x, n, max_lag, corr_type, method, 1, corr, metrics, device_ptrs, true);
}

}  // extern "C"
