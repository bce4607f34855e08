// hps_api.cpp -- sonar_hps_from_spectrum, sonar_hps and their host-only companions: HarmonicProduct
// (algorithms/harmonic/harmonic_product.go).  The host side: the argument checks, findF0Peak's scan
// range (:128-139, a function of the parameters alone), GetOptimalNumHarmonics (:301-314), the staged
// arrays of each entry (staging.h) and sonar_hps's estimate over the chunked walk of the float64
// transform (magnitude_walk.h) with applyWindow's window (:212-221).  The kernels are hps_kernels.hip's.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

#include "ctx.h"
#include "kernels.h"
#include "magnitude_walk.h"
#include "staging.h"

using sonar::detail::fail;
using sonar::detail::Staging;
using sonar::detail::timed_begin;
using sonar::detail::timed_end;

// The ordered sum of mag^2 behind the confidence (ComputeHarmonicity :263-266) has two layouts with the
// same bits: a row per lane in hps_energy_kernel before the row kernel, or lane 0 of the row's wave
// walking the row in LDS.  The first runs 64 chains per wave but only F / 64 waves, so it pays from
// about two waves per CU on (Kernel 4g, has the timings on both sides of the rule).
// SONAR_HPS_CHAIN_ROWS_PER_LANE=0 builds a library that always walks (A/B builds).
#ifndef SONAR_HPS_CHAIN_ROWS_PER_LANE
#define SONAR_HPS_CHAIN_ROWS_PER_LANE 1
#endif

namespace {

struct Range { int32_t min_bin, max_bin; };   // before the clamps

constexpr int64_t kRowsPerLaneMinRows = 32768;   // 512 waves of 64 rows
bool rows_per_lane(int64_t F) { return SONAR_HPS_CHAIN_ROWS_PER_LANE && F >= kRowsPerLaneMinRows; }

// int(x) of a quotient that is >= 0 or NaN; false where Go's conversion is implementation-defined
// or the value does not fit an int32
bool go_int32(double q, int32_t* out) {
  if (!(q < 2147483648.0)) return false;
  *out = (int32_t)q;
  return true;
}

// findF0Peak's minBin and maxBin (:128-132)
int scan_range(int32_t sample_rate, int32_t window_size, double min_f0, double max_f0, Range* r, std::string& msg) {
  if (sample_rate <= 0 || window_size <= 0) {
    msg = "harmonic product: sample_rate or window_size <= 0 is not reproduced";
    return SONAR_ERR_UNSUPPORTED;
  }
  if (!std::isfinite(min_f0) || !std::isfinite(max_f0) || min_f0 < 0.0 || max_f0 < 0.0) {
    msg = "harmonic product: a non-finite or negative min_f0 or max_f0 is not reproduced";
    return SONAR_ERR_UNSUPPORTED;
  }
  const double freq_res = (double)sample_rate / (double)window_size;
  if (!go_int32(min_f0 / freq_res, &r->min_bin) || !go_int32(max_f0 / freq_res, &r->max_bin)) {
    msg = "harmonic product: min_f0 or max_f0 over the frequency resolution does not fit an int32";
    return SONAR_ERR_UNSUPPORTED;
  }
  return SONAR_OK;
}

// the clamps (:134-139); K == 0 leaves max_bin -1, an empty range
Range clamp_range(Range r, int32_t K) {
  if (r.min_bin < 1) r.min_bin = 1;
  if (r.max_bin >= K) r.max_bin = K - 1;
  return r;
}

int check_shape(int32_t K, int32_t num_harmonics, bool strengths_wanted, std::string& msg) {
  if (K > sonar::HPS_MAX_K) {
    msg = "harmonic product: rows of more than " + std::to_string(sonar::HPS_MAX_K) + " bins are not supported";
    return SONAR_ERR_UNSUPPORTED;
  }
  if (num_harmonics > sonar::HPS_MAX_HARMONICS) {
    msg = "harmonic product: num_harmonics above " + std::to_string(sonar::HPS_MAX_HARMONICS) + " is not supported";
    return SONAR_ERR_UNSUPPORTED;
  }
  if (num_harmonics < 0 && strengths_wanted) {   // make([]float64, numHarmonics) :230, only on rows with f0 > 0
    msg = "harmonic product: a negative num_harmonics with confidence or strengths is not reproduced";
    return SONAR_ERR_UNSUPPORTED;
  }
  return SONAR_OK;
}

struct RowOut {
  int32_t* f0_bin;
  double *f0, *confidence, *strengths, *hps;
};

// the estimate of F device rows into device outputs (queued on the context's stream); total is the
// scratch of the rows-per-lane chain (F doubles, used when rows_per_lane(F)) or null
int estimate_rows(sonar_ctx* c, const double* dmag, int64_t F, int32_t K, int32_t window_size, int32_t sample_rate,
                  int32_t num_harmonics, Range r, int32_t interpolated, const RowOut& out, double* total) {
  sonar::HpsArgs a{};
  a.mag = dmag; a.F = F; a.K = K;
  a.nh = num_harmonics;
  a.min_bin = r.min_bin; a.max_bin = r.max_bin;
  a.freq_res = (double)sample_rate / (double)window_size;
  a.interpolated = interpolated != 0;
  a.f0_bin = out.f0_bin; a.f0 = out.f0; a.confidence = out.confidence; a.strengths = out.strengths; a.hps = out.hps;
  a.total = out.confidence && rows_per_lane(F) ? total : nullptr;
  hipEvent_t tend = timed_begin(c, c->stream);
  if (a.total && sonar::launch_hps_energy(dmag, F, K, total, c->stream) != 0)
    return fail(c, SONAR_ERR_DEVICE, "harmonic product: energy launch failed");
  const int rc = sonar::launch_hps(a, c->stream);
  if (rc == -1) return fail(c, SONAR_ERR_UNSUPPORTED, "harmonic product: a shape the kernel does not take");
  if (rc != 0) return fail(c, SONAR_ERR_DEVICE, "harmonic product launch failed");
  timed_end(c, c->stream, tend);
  return SONAR_OK;
}

}  // namespace

extern "C" {

int sonar_hps_bins(int32_t sample_rate, int32_t window_size, int32_t K, double min_f0, double max_f0,
                   int32_t* min_bin, int32_t* max_bin) {
  if (K < 0) return SONAR_ERR_INVALID;
  Range r{};
  std::string msg;
  const int rc = scan_range(sample_rate, window_size, min_f0, max_f0, &r, msg);
  if (rc != SONAR_OK) return rc;
  r = clamp_range(r, K);
  if (min_bin) *min_bin = r.min_bin;
  if (max_bin) *max_bin = r.max_bin;
  return SONAR_OK;
}

int sonar_hps_optimal_harmonics(int32_t sample_rate, double min_f0, int32_t* num_harmonics) {
  if (sample_rate <= 0 || !std::isfinite(min_f0) || min_f0 < 0.0) return SONAR_ERR_UNSUPPORTED;
  int32_t m = 0;
  if (!go_int32(((double)sample_rate / 2.0) / min_f0, &m)) return SONAR_ERR_UNSUPPORTED;   // :303-304
  if (num_harmonics) *num_harmonics = m > 7 ? 5 : m > 3 ? m - 1 : 2;                       // :307-313
  return SONAR_OK;
}

int sonar_hps_from_spectrum(sonar_ctx* c, const double* mag, int64_t F, int32_t K, int32_t window_size,
                            int32_t sample_rate, int32_t num_harmonics, double min_f0, double max_f0,
                            int32_t interpolated, int32_t* f0_bin, double* f0, double* confidence, double* strengths,
                            double* hps, int32_t device_ptrs) {
  if (!c) return SONAR_ERR_INVALID;
  if (F < 0 || K < 0) return fail(c, SONAR_ERR_INVALID, "harmonic product: negative row count or row length");
  if (F == 0) return SONAR_OK;
  if (!f0_bin || !f0) return fail(c, SONAR_ERR_INVALID, "harmonic product: null f0_bin or f0 pointer");
  HIP_TRY(c, hipSetDevice(c->device));
  Staging o{c, "hps.", device_ptrs != 0};
  const size_t nh = (size_t)std::max(num_harmonics, 0);
  if (K == 0)                                               // :33-35, then findF0Peak's empty range: bin 0
    return o.zero({{f0_bin, (size_t)F * 4}, {f0, (size_t)F * 8}, {confidence, (size_t)F * 8},
                   {strengths, (size_t)F * nh * 8}});
  Range r{};
  std::string msg;
  int rc = scan_range(sample_rate, window_size, min_f0, max_f0, &r, msg);
  if (rc == SONAR_OK) rc = check_shape(K, num_harmonics, confidence || strengths, msg);
  if (rc != SONAR_OK) return fail(c, rc, msg);
  if (!mag) return fail(c, SONAR_ERR_INVALID, "harmonic product: null magnitude pointer");
  const double* dm = o.in("mag", mag, (size_t)F * (size_t)K);
  RowOut out{};
  out.f0_bin = o.out("bin", f0_bin, (size_t)F);
  out.f0 = o.out("f0", f0, (size_t)F);
  out.confidence = o.out("confidence", confidence, (size_t)F);
  out.strengths = nh ? o.out("strengths", strengths, (size_t)F * nh) : nullptr;
  out.hps = o.out("rows", hps, (size_t)F * (size_t)K);
  double* total = confidence && rows_per_lane(F) ? o.tmp<double>("total", (size_t)F) : nullptr;
  rc = o.ready("device allocation failed");
  if (rc != SONAR_OK) return rc;
  rc = estimate_rows(c, dm, F, K, window_size, sample_rate, num_harmonics, clamp_range(r, K), interpolated, out, total);
  return rc != SONAR_OK ? rc : o.finish();
}

int sonar_hps_plan(int64_t n, int32_t window_size, int32_t hop_size, int64_t* frames, int64_t* chunk_frames,
                   int64_t* n_chunks) {
  const int rc = sonar_hpcp_plan(n, window_size, hop_size, frames, chunk_frames, n_chunks);
  if (rc != SONAR_OK) return rc;
  return window_size < 2 ? SONAR_ERR_UNSUPPORTED : SONAR_OK;   // applyWindow divides by N - 1 (:216)
}

int sonar_hps(sonar_ctx* c, const double* pcm, int64_t n, int32_t sample_rate, int32_t window_size, int32_t hop_size,
              int32_t num_harmonics, double min_f0, double max_f0, int32_t interpolated, int32_t* f0_bin, double* f0,
              double* confidence, double* strengths, double* magnitude, int64_t* frames, int32_t device_ptrs) {
  if (!c) return SONAR_ERR_INVALID;
  sonar::detail::MagnitudeWalk walk;
  std::string msg;
  // the transform's checks first, as sonar_hpcp
  int rc = walk.plan(sample_rate, window_size, hop_size, SONAR_WIN_HANN, n, pcm != nullptr, &msg);
  if (rc != SONAR_OK) return fail(c, rc, msg);
  if (window_size < 2)
    return fail(c, SONAR_ERR_UNSUPPORTED, "harmonic product: a window of fewer than 2 samples is not reproduced");
  const int64_t F = walk.F;
  const int32_t K = walk.K;
  Range r{};
  rc = scan_range(sample_rate, window_size, min_f0, max_f0, &r, msg);
  if (rc == SONAR_OK) rc = check_shape(K, num_harmonics, confidence || strengths, msg);
  if (rc != SONAR_OK) return fail(c, rc, msg);
  if (!f0_bin || !f0) return fail(c, SONAR_ERR_INVALID, "harmonic product: null f0_bin or f0 pointer");
  if (frames) *frames = F;
  HIP_TRY(c, hipSetDevice(c->device));
  Staging o{c, "hps.", device_ptrs != 0};
  const size_t nh = (size_t)std::max(num_harmonics, 0);
  const double* dx = o.in("pcm", pcm, (size_t)n);
  RowOut out{};
  out.f0_bin = o.out("bin", f0_bin, (size_t)F);
  out.f0 = o.out("f0", f0, (size_t)F);
  out.confidence = o.out("confidence", confidence, (size_t)F);
  out.strengths = nh ? o.out("strengths", strengths, (size_t)F * nh) : nullptr;
  walk.alloc(o);
  const int64_t chunk = std::min(walk.chunk_frames, F);
  double* total = confidence && rows_per_lane(chunk) ? o.tmp<double>("total", (size_t)chunk) : nullptr;
  rc = o.ready("device allocation failed");
  if (rc != SONAR_OK) return rc;
  r = clamp_range(r, K);
  // under applyWindow's window: every chunk's estimate and, if wanted, its rows' copy out; one wait, at the end
  rc = walk.each(c, dx, n, true, [&](const double* rows, int64_t s0, int64_t nf) {
    RowOut part{out.f0_bin + s0, out.f0 + s0, out.confidence ? out.confidence + s0 : nullptr,
                out.strengths ? out.strengths + s0 * (int64_t)nh : nullptr, nullptr};
    const int erc = estimate_rows(c, rows, nf, K, window_size, sample_rate, num_harmonics, r, interpolated, part, total);
    return erc != SONAR_OK ? erc : o.give(magnitude ? magnitude + s0 * K : nullptr, rows, (size_t)nf * (size_t)K * 8);
  });
  return rc != SONAR_OK ? rc : o.finish();
}

}  // extern "C"
