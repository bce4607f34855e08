// hpcp_api.cpp -- sonar_spectral_peaks, sonar_hpcp_from_spectrum, sonar_hpcp and their host-only
// companions: SpectralPeaks.DetectPeaks (algorithms/harmonic/spectral_peaks.go:36-100) and
// HPCP.ComputeFromSpectrum (algorithms/chroma/hpcp.go:205-221).  The host side: the argument checks,
// the contribution table (frequencyToPitchClass :224-236, addPeakContribution :254-281,
// computeWindowWeight :284-300, addHarmonicContributions :303-321, evaluated per FFT bin with libm)
// as one cached table per parameter set (ctx.h, cached_table), the staged arrays of each entry
// (staging.h), and sonar_hpcp's profile over the chunked walk of the float64 transform
// (magnitude_walk.h).  The kernel is hpcp_kernels.hip's.
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
#include "magnitude_walk.h"
#include "staging.h"

using sonar::go_log2;
using sonar::detail::fail;
using sonar::detail::MagnitudeWalk;
using sonar::detail::Staging;
using sonar::detail::timed_begin;
using sonar::detail::timed_end;

namespace {

constexpr int64_t kMaxEntries = int64_t(1) << 24;
constexpr int32_t kMaxHarmonics = 16;
constexpr double kMaxWindowSemitones = 12.0;
// ComputeFromSpectrum's detector (:211-216)
constexpr double kHpcpMinHeight = 0.00001, kHpcpMinDistanceHz = 20.0;
constexpr int32_t kHpcpMaxPeaks = 60;

// max(int(min_distance_hz / freq_res), 1) (:41-43).  Out of int64's range (or NaN) amd64's conversion
// gives the most negative value, so 1; a distance of K bins or more acts like K.
int min_distance_bins(double min_distance_hz, double freq_res, int K) {
  const double v = min_distance_hz / freq_res;
  if (!(v > -9.2e18 && v < 9.2e18)) return 1;
  const int64_t d = (int64_t)v;
  return (int)std::min<int64_t>(std::max<int64_t>(d, 1), std::max(K, 1));
}

int64_t peaks_width(int64_t K, int64_t max_peaks) {
  return std::max<int64_t>(std::min<int64_t>(max_peaks, std::max<int64_t>((K - 1) / 2, 0)), 0);
}

int check_rates(int32_t sample_rate, int32_t window_size, int32_t K, std::string& msg) {
  if (sample_rate <= 0 || window_size <= 0) {
    msg = "spectral peaks: sample_rate or window_size <= 0 is not reproduced";
    return SONAR_ERR_UNSUPPORTED;
  }
  if (K > sonar::HPCP_MAX_K) {
    msg = "spectral peaks: rows of more than " + std::to_string(sonar::HPCP_MAX_K) + " bins are not supported";
    return SONAR_ERR_UNSUPPORTED;
  }
  return SONAR_OK;
}

int check_params(const sonar_hpcp_params& p, std::string& msg) {
  if (p.size < 0) { msg = "runtime error: makeslice: len out of range"; return SONAR_ERR_PANIC; }   // :93
  if (!std::isfinite(p.reference_freq) || p.reference_freq <= 0.0) {
    msg = "HPCP: a non-finite or non-positive reference_freq is not reproduced";
    return SONAR_ERR_UNSUPPORTED;
  }
  if (!std::isfinite(p.window_size) || p.window_size < 0.0) {
    msg = "HPCP: a non-finite or negative window_size (semitones) is not reproduced";
    return SONAR_ERR_UNSUPPORTED;
  }
  if (p.size > sonar::HPCP_MAX_SIZE) {
    msg = "HPCP: size above " + std::to_string(sonar::HPCP_MAX_SIZE) + " is not supported";
    return SONAR_ERR_UNSUPPORTED;
  }
  if (p.max_harmonics > kMaxHarmonics) {
    msg = "HPCP: max_harmonics above " + std::to_string(kMaxHarmonics) + " is not supported";
    return SONAR_ERR_UNSUPPORTED;
  }
  if (p.window_size > kMaxWindowSemitones) {
    msg = "HPCP: a window_size above 12 semitones is not supported";
    return SONAR_ERR_UNSUPPORTED;
  }
  return SONAR_OK;
}

struct HpcpTable {
  std::vector<int64_t> row_start;
  std::vector<int32_t> wbin;
  std::vector<double> factor, weight;
};

// frequencyToPitchClass (:224-236)
double pitch_class(const sonar_hpcp_params& p, double freq) {
  const double midi = 69.0 + 12.0 * go_log2(freq / p.reference_freq);
  double pc = std::fmod(midi, 12.0);
  if (pc < 0.0) pc += 12.0;
  return pc * (double)p.size / 12.0;
}

// computeWindowWeight (:284-300)
double window_weight(const sonar_hpcp_params& p, double distance, double window_bins) {
  if (window_bins == 0.0) return 1.0;
  if (p.weight_type == SONAR_HPCP_WEIGHT_COSINE || p.weight_type == SONAR_HPCP_WEIGHT_SQUARED_COSINE) {
    const double angle = M_PI * distance / window_bins;
    const double c = std::cos(angle);
    const double v = c > 0.0 ? c : 0.0;                  // math.Max(0, c) of a finite c
    return p.weight_type == SONAR_HPCP_WEIGHT_COSINE ? v : v * v;
  }
  return 1.0;
}

// addPeakContribution (:254-281) with the weight left symbolic: hpcp[wrapped] += (magnitude * factor) * ww
void add_contribution(const sonar_hpcp_params& p, double pc, double factor, HpcpTable& t) {
  const double window_bins = p.window_size * (double)p.size / 12.0;
  const int64_t start = (int64_t)std::floor(pc - window_bins / 2);
  const int64_t end = (int64_t)std::ceil(pc + window_bins / 2);
  for (int64_t bin = start; bin <= end; ++bin) {
    int64_t wrapped = bin;
    while (wrapped < 0) wrapped += p.size;
    wrapped %= p.size;
    double distance = std::fabs((double)bin - pc);
    if (distance > (double)p.size / 2) distance = (double)p.size - distance;
    if (distance <= window_bins / 2) {
      t.wbin.push_back((int32_t)wrapped);
      t.factor.push_back(factor);
      t.weight.push_back(window_weight(p, distance, window_bins));
    }
  }
}

// The rows of bins 1 .. K - 2 (the only bins DetectPeaks can return) inside [min_freq, max_freq]
int build_table(int32_t sample_rate, int32_t window_size, int32_t K, const sonar_hpcp_params& p, HpcpTable& t,
                std::string& msg) {
  t.row_start.assign((size_t)K + 1, 0);
  const double freq_res = (double)sample_rate / (double)window_size;
  for (int32_t i = 0; i < K; ++i) {
    t.row_start[(size_t)i] = (int64_t)t.wbin.size();
    if (i < 1 || i > K - 2 || p.size == 0) continue;
    const double f = (double)i * freq_res;
    if (f < p.min_freq || f > p.max_freq) continue;                                      // :156
    add_contribution(p, pitch_class(p, f), (p.band_preset && f < p.split_freq) ? 2.0 : 1.0, t);   // :166-172, :239-251
    if (p.max_harmonics > 0 && !p.harmonics_removal) {                                   // :175, :303-321
      for (int32_t h = 2; h <= p.max_harmonics; ++h) {
        const double hf = f * (double)h;
        if (hf > p.max_freq) break;
        add_contribution(p, pitch_class(p, hf), p.harmonics_strength / (double)h, t);
      }
    }
    if ((int64_t)t.wbin.size() > kMaxEntries) {
      msg = "HPCP: the contribution table of this configuration exceeds 2^24 entries";
      return SONAR_ERR_UNSUPPORTED;
    }
  }
  t.row_start[(size_t)K] = (int64_t)t.wbin.size();
  return SONAR_OK;
}

struct DevTable {
  const int32_t* row_start;
  const int32_t* wbin;
  const double* factor;
  const double* weight;
};

// The device copy of one parameter set's table, cached in the context until sonar_trim.
int device_table(sonar_ctx* c, int32_t sample_rate, int32_t window_size, int32_t K, const sonar_hpcp_params& p,
                 DevTable* out) {
  uint64_t b[6];
  const double d[6] = {p.reference_freq, p.window_size, p.min_freq, p.max_freq, p.split_freq, p.harmonics_strength};
  std::memcpy(b, d, sizeof b);
  char key[320];
  std::snprintf(key, sizeof key, "hpcp.tab.%d.%d.%d.%d.%d.%d.%d.%d.%016llx.%016llx.%016llx.%016llx.%016llx.%016llx",
                sample_rate, window_size, K, p.size, p.harmonics_removal != 0,
                p.weight_type == SONAR_HPCP_WEIGHT_COSINE || p.weight_type == SONAR_HPCP_WEIGHT_SQUARED_COSINE
                    ? p.weight_type : 0,
                p.band_preset != 0, std::max(p.max_harmonics, 0), (unsigned long long)b[0], (unsigned long long)b[1],
                (unsigned long long)b[2], (unsigned long long)b[3], (unsigned long long)b[4], (unsigned long long)b[5]);
  auto layout = [&](int64_t n, size_t off[4]) {
    off[0] = 0;
    off[1] = ((size_t)K + 2) / 2 * 8;                       // row_start: K + 1 int32, padded to 8 bytes
    off[2] = off[1] + ((size_t)n + 1) / 2 * 8;             // wbin
    off[3] = off[2] + (size_t)n * 8;                       // factor
    return off[3] + (size_t)n * 8;                         // weight
  };
  size_t off[4];
  const unsigned char* base = nullptr;
  int64_t entries = 0;                                      // kept with the cached entry: it lays the arrays out
  const int trc = sonar::detail::cached_table(c, key, "HPCP contribution table", [&](std::vector<unsigned char>& img, int64_t& n) {
    HpcpTable t;
    std::string msg;
    const int rc = build_table(sample_rate, window_size, K, p, t, msg);
    if (rc != SONAR_OK) return fail(c, rc, msg);
    n = (int64_t)t.wbin.size();
    img.assign(layout(n, off), 0);
    int32_t* rs = (int32_t*)img.data();
    for (int32_t i = 0; i <= K; ++i) rs[i] = (int32_t)t.row_start[(size_t)i];
    if (n > 0) {
      std::memcpy(img.data() + off[1], t.wbin.data(), (size_t)n * 4);
      std::memcpy(img.data() + off[2], t.factor.data(), (size_t)n * 8);
      std::memcpy(img.data() + off[3], t.weight.data(), (size_t)n * 8);
    }
    return (int)SONAR_OK;
  }, &base, &entries);
  if (trc != SONAR_OK) return trc;
  layout(entries, off);
  out->row_start = (const int32_t*)base;
  out->wbin = (const int32_t*)(base + off[1]);
  out->factor = (const double*)(base + off[2]);
  out->weight = (const double*)(base + off[3]);
  return SONAR_OK;
}

// the profile of F device rows into device outputs (queued on the context's stream)
int profile_rows(sonar_ctx* c, const double* dmag, int64_t F, int32_t K, int32_t window_size, int32_t sample_rate,
                 const sonar_hpcp_params& p, const DevTable& T, double* dh, double* de, double* dn) {
  sonar::HpcpArgs a{};
  a.mag = dmag; a.F = F; a.K = K;
  a.freq_res = (double)sample_rate / (double)window_size;
  a.min_height = kHpcpMinHeight;
  a.min_dist = min_distance_bins(kHpcpMinDistanceHz, a.freq_res, K);
  a.P = (int)peaks_width(K, kHpcpMaxPeaks);
  a.row_start = T.row_start; a.wbin = T.wbin; a.factor = T.factor; a.weight = T.weight;
  a.size = p.size; a.non_linear = p.non_linear != 0; a.normalized = p.normalized != 0;
  a.max_shifted = p.max_shifted != 0;
  a.hpcp = dh; a.energy = de; a.entropy = dn;
  hipEvent_t tend = timed_begin(c, c->stream);
  const int rc = sonar::launch_hpcp(a, c->stream);
  if (rc == -1) return fail(c, SONAR_ERR_UNSUPPORTED, "HPCP: a shape the kernel does not take");
  if (rc != 0) return fail(c, SONAR_ERR_DEVICE, "HPCP launch failed");
  timed_end(c, c->stream, tend);
  return SONAR_OK;
}

}  // namespace

extern "C" {

int64_t sonar_spectral_peaks_width(int64_t K, int64_t max_peaks) { return peaks_width(K, max_peaks); }

void sonar_hpcp_params_default(sonar_hpcp_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->size = 12;
  p->reference_freq = 440.0;
  p->normalized = 1;
  p->weight_type = SONAR_HPCP_WEIGHT_COSINE;
  p->window_size = 1.0;
  p->band_preset = 1;
  p->min_freq = 40.0;
  p->max_freq = 5000.0;
  p->split_freq = 500.0;
  p->harmonics_strength = 1.0;
}

int sonar_spectral_peaks(sonar_ctx* c, const double* mag, int64_t F, int32_t K, int32_t window_size,
                         int32_t sample_rate, double min_height, double min_distance_hz, int32_t max_peaks,
                         int32_t* count, int32_t* bin, double* magnitude, double* frequency, int32_t device_ptrs) {
  if (!c) return SONAR_ERR_INVALID;
  if (F < 0 || K < 0) return fail(c, SONAR_ERR_INVALID, "spectral peaks: negative row count or row length");
  if (F == 0) return SONAR_OK;
  if (!count) return fail(c, SONAR_ERR_INVALID, "spectral peaks: null count pointer");
  HIP_TRY(c, hipSetDevice(c->device));
  Staging o{c, "peaks.", device_ptrs != 0};
  if (K == 0) return o.zero({{count, (size_t)F * 4}});      // :37-39
  if (max_peaks < 0)                                        // peaks[:maxPeaks] :95-97
    return fail(c, SONAR_ERR_PANIC, "runtime error: slice bounds out of range [:" + std::to_string(max_peaks) + "]");
  std::string msg;
  const int crc = check_rates(sample_rate, window_size, K, msg);
  if (crc != SONAR_OK) return fail(c, crc, msg);
  if (!mag) return fail(c, SONAR_ERR_INVALID, "spectral peaks: null magnitude pointer");
  const int64_t P = peaks_width(K, max_peaks);
  if (P > 0 && (!bin || !magnitude)) return fail(c, SONAR_ERR_INVALID, "spectral peaks: null bin or magnitude pointer");
  hipStream_t s = c->stream;
  const size_t slots = (size_t)F * (size_t)P;
  sonar::HpcpArgs a{};
  a.mag = o.in("mag", mag, (size_t)F * (size_t)K);
  a.F = F; a.K = K;
  a.freq_res = (double)sample_rate / (double)window_size;   // :41
  a.min_height = min_height;
  a.min_dist = min_distance_bins(min_distance_hz, a.freq_res, K);
  a.P = (int)P;
  a.count = o.out("count", count, (size_t)F);
  if (P > 0) {
    a.bin = o.out("bin", bin, slots);
    a.pmag = o.out("pmag", magnitude, slots);
    a.pfreq = o.out("pfreq", frequency, slots);
  }
  const int src = o.ready("device allocation failed");
  if (src != SONAR_OK) return src;
  hipEvent_t tend = timed_begin(c, s);
  const int rc = sonar::launch_hpcp(a, s);
  if (rc == -1) return fail(c, SONAR_ERR_UNSUPPORTED, "spectral peaks: a shape the kernel does not take");
  if (rc != 0) return fail(c, SONAR_ERR_DEVICE, "spectral peaks launch failed");
  timed_end(c, s, tend);
  return o.finish();
}

int sonar_hpcp_table(int32_t sample_rate, int32_t window_size, int32_t K, const sonar_hpcp_params* params,
                     int64_t* n_entries, int64_t* row_start, int32_t* wrapped_bin, double* factor,
                     double* window_weight) {
  if (!params || K < 0) return SONAR_ERR_INVALID;
  std::string msg;
  int rc = check_params(*params, msg);
  if (rc == SONAR_OK) rc = check_rates(sample_rate, window_size, K, msg);
  if (rc != SONAR_OK) return rc;
  HpcpTable t;
  rc = build_table(sample_rate, window_size, K, *params, t, msg);
  if (rc != SONAR_OK) return rc;
  const size_t n = t.wbin.size();
  if (n_entries) *n_entries = (int64_t)n;
  if (row_start) std::memcpy(row_start, t.row_start.data(), ((size_t)K + 1) * 8);
  if (wrapped_bin && n) std::memcpy(wrapped_bin, t.wbin.data(), n * 4);
  if (factor && n) std::memcpy(factor, t.factor.data(), n * 8);
  if (window_weight && n) std::memcpy(window_weight, t.weight.data(), n * 8);
  return SONAR_OK;
}

int sonar_hpcp_from_spectrum(sonar_ctx* c, const double* mag, int64_t F, int32_t K, int32_t window_size,
                             int32_t sample_rate, const sonar_hpcp_params* params, double* hpcp, double* energy,
                             double* entropy, int32_t device_ptrs) {
  if (!c) return SONAR_ERR_INVALID;
  if (F < 0 || K < 0 || !params) return fail(c, SONAR_ERR_INVALID, "HPCP: negative row count or row length, or null params");
  if (F == 0) return SONAR_OK;
  const sonar_hpcp_params& p = *params;
  std::string msg;
  int rc = check_params(p, msg);
  if (rc == SONAR_OK) rc = check_rates(sample_rate, window_size, K, msg);
  if (rc != SONAR_OK) return fail(c, rc, msg);
  HIP_TRY(c, hipSetDevice(c->device));
  Staging o{c, "hpcp.", device_ptrs != 0};
  const size_t prof = (size_t)F * (size_t)p.size;
  if (p.size == 0 || K == 0) {                              // no bins, or no peaks: zeros all through
    if (p.size > 0 && !hpcp) return fail(c, SONAR_ERR_INVALID, "HPCP: null hpcp pointer");
    return o.zero({{hpcp, prof * 8}, {energy, (size_t)F * 8}, {entropy, (size_t)F * 8}});
  }
  if (!mag || !hpcp) return fail(c, SONAR_ERR_INVALID, "HPCP: null magnitude or hpcp pointer");
  DevTable T{};
  rc = device_table(c, sample_rate, window_size, K, p, &T);
  if (rc != SONAR_OK) return rc;
  const double* dm = o.in("mag", mag, (size_t)F * (size_t)K);
  double* dh = o.out("out", hpcp, prof);
  double* de = o.out("energy", energy, (size_t)F);
  double* dn = o.out("entropy", entropy, (size_t)F);
  rc = o.ready("device allocation failed");
  if (rc != SONAR_OK) return rc;
  rc = profile_rows(c, dm, F, K, window_size, sample_rate, p, T, dh, de, dn);
  return rc != SONAR_OK ? rc : o.finish();
}

int sonar_hpcp_plan(int64_t n, int32_t window_size, int32_t hop_size, int64_t* frames, int64_t* chunk_frames,
                    int64_t* n_chunks) {
  MagnitudeWalk walk;
  std::string msg;
  const int rc = walk.plan(44100, window_size, hop_size, SONAR_WIN_HANN, n, true, &msg);
  if (rc != SONAR_OK) return rc;
  if (frames) *frames = walk.F;
  if (chunk_frames) *chunk_frames = walk.chunk_frames;
  if (n_chunks) *n_chunks = (walk.F + walk.chunk_frames - 1) / walk.chunk_frames;
  return SONAR_OK;
}

int sonar_hpcp(sonar_ctx* c, const double* pcm, int64_t n, int32_t sample_rate, int32_t window_size, int32_t hop_size,
               int32_t window_type, const sonar_hpcp_params* params, double* hpcp, double* energy, double* entropy,
               int32_t device_ptrs) {
  if (!c) return SONAR_ERR_INVALID;
  if (!params) return fail(c, SONAR_ERR_INVALID, "HPCP: null params");
  MagnitudeWalk walk;
  std::string msg;
  // ComputeSTFTWithWindow's checks first
  int rc = walk.plan(sample_rate, window_size, hop_size, window_type, n, pcm != nullptr, &msg);
  if (rc != SONAR_OK) return fail(c, rc, msg);
  const sonar_hpcp_params& p = *params;
  const int64_t F = walk.F;
  const int32_t K = walk.K;
  rc = check_params(p, msg);
  if (rc == SONAR_OK) rc = check_rates(sample_rate, window_size, K, msg);
  if (rc != SONAR_OK) return fail(c, rc, msg);
  HIP_TRY(c, hipSetDevice(c->device));
  Staging o{c, "hpcp.", device_ptrs != 0};
  if (p.size > 0 && !hpcp) return fail(c, SONAR_ERR_INVALID, "HPCP: null hpcp pointer");
  DevTable T{};
  if (p.size > 0) {
    rc = device_table(c, sample_rate, window_size, K, p, &T);
    if (rc != SONAR_OK) return rc;
  }
  const double* dx = o.in("pcm", pcm, (size_t)n);
  double* dh = o.out("out", hpcp, (size_t)F * (size_t)p.size);
  double* de = o.out("energy", energy, (size_t)F);
  double* dn = o.out("entropy", entropy, (size_t)F);
  walk.alloc(o);
  rc = o.ready("device allocation failed");
  if (rc != SONAR_OK) return rc;
  // the profile of every chunk's rows; the host waits once, at the end
  if (p.size > 0)
    rc = walk.each(c, dx, n, false, [&](const double* rows, int64_t f0, int64_t nf) {
      return profile_rows(c, rows, nf, K, window_size, sample_rate, p, T, dh + f0 * p.size, de ? de + f0 : nullptr,
                          dn ? dn + f0 : nullptr);
    });
  if (rc != SONAR_OK) return rc;
  if (p.size == 0) {                                        // the staged copies are device memory in both modes
    for (double* z : {de, dn}) {
      const int zrc = sonar::detail::zero_out(c, z, (size_t)F * 8, true);
      if (zrc != SONAR_OK) return zrc;
    }
  }
  return o.finish();
}

}  // extern "C"
