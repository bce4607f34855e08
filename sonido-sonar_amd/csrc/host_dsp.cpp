// host_dsp.cpp -- see host_dsp.h.  Go semantics restated (file:line cited per
// function); float64 throughout, evaluation order as in the Go source.
#include "host_dsp.h"

#include <algorithm>
#include <cmath>
#include <limits>

#include "go_math.h"

namespace sonar {
namespace host {

namespace {
constexpr double kPi = 3.14159265358979323846;

// Go int(float64) on amd64: NaN / out-of-range -> MinInt64 (CVTTSD2SQ)
int64_t go_trunc(double x) {
  if (!(x >= -9.2233720368547758e18 && x < 9.2233720368547758e18)) return std::numeric_limits<int64_t>::min();
  return static_cast<int64_t>(x);
}
double bessel_i0(double x) {   // windowing.go:425-441
  double sum = 1.0, term = 1.0;
  for (int k = 1; k < 50; k++) {
    const double t = x / (2.0 * (double)k);
    term *= t * t;
    sum += term;
    if (term < 1e-12) break;
  }
  return sum;
}
}  // namespace

bool make_window(int type, int size, bool symmetric, bool normalize, double beta, double alpha,
                 std::vector<double>& c) {
  if (size <= 0 || size > 1048576) return false;                 // validateConfig :177-199
  const int N = size;
  c.assign(N, 0.0);
  const double den = symmetric ? (double)(N - 1) : (double)N;
  switch (type) {
    case 0: for (int i = 0; i < N; i++) c[i] = 0.5 * (1.0 - std::cos(2 * kPi * (double)i / den)); break;   // :246
    case 1: for (int i = 0; i < N; i++) c[i] = 0.54 - 0.46 * std::cos(2 * kPi * (double)i / den); break;   // :259
    case 2: for (int i = 0; i < N; i++) {                                                                  // :272
        const double a = 2 * kPi * (double)i / den; c[i] = 0.42 - 0.5 * std::cos(a) + 0.08 * std::cos(2 * a); }
      break;
    case 3: for (int i = 0; i < N; i++) {                                                                  // :288
        const double a = 2 * kPi * (double)i / den;
        c[i] = 0.35875 - 0.48829 * std::cos(a) + 0.14128 * std::cos(2 * a) - 0.01168 * std::cos(3 * a); }
      break;
    case 4: {                                                                                              // :304
      if (beta < 0) return false;
      const double i0b = bessel_i0(beta);
      for (int i = 0; i < N; i++) { const double a = 2.0 * (double)i / den - 1.0;
        c[i] = bessel_i0(beta * std::sqrt(1 - a * a)) / i0b; }
      break; }
    case 5: {                                                                                              // :321
      if (alpha < 0 || alpha > 1) return false;
      const int taper = (int)(alpha * (double)N / 2.0);
      for (int i = 0; i < N; i++) {
        if (i < taper) c[i] = 0.5 * (1 + std::cos(kPi * (double)i / (double)taper - kPi));
        else if (i >= N - taper) c[i] = 0.5 * (1 + std::cos(kPi * (double)(i - (N - taper)) / (double)taper));
        else c[i] = 1.0;
      }
      break; }
    case 6: for (int i = 0; i < N; i++) c[i] = 1.0; break;
    case 7: for (int i = 0; i < N; i++)                                                                    // :350
        c[i] = (i <= N / 2) ? 2.0 * (double)i / (double)(N - 1) : 2.0 - 2.0 * (double)i / (double)(N - 1);
      break;
    case 8: for (int i = 0; i < N; i++) {                                                                  // :363
        const double a = ((double)i - (double)(N - 1) / 2.0) / ((double)(N - 1) / 2.0); c[i] = 1.0 - a * a; }
      break;
    default: return false;
  }
  if (normalize) {                                                // calculateWindowProperties + normalizeWindow :393-437
    double energy = 0.0;
    for (double v : c) energy += v * v;
    const double nf = 1.0 / std::sqrt(energy / (double)N);
    for (double& v : c) v *= nf;
  }
  return true;
}

bool make_filterbank(int kind, int nf, int fft_size, int sr, double low, double high, std::vector<double>& fb) {
  if (nf <= 0 || fft_size <= 0) return false;
  const int K = fft_size / 2 + 1;
  fb.assign((size_t)nf * K, 0.0);
  auto fwd = [kind](double hz) {
    return kind ? (26.81 * hz / (1960.0 + hz)) - 0.53 : 2595.0 * std::log10(1.0 + hz / 700.0);
  };
  auto inv = [kind](double v) {
    return kind ? 1960.0 * (v + 0.53) / (26.28 - v) : 700.0 * (std::pow(10.0, v / 2595.0) - 1.0);
  };
  const double lo = fwd(low), hi = fwd(high);
  const double step = (hi - lo) / (double)(nf + 1);
  std::vector<int64_t> bins(nf + 2);
  for (int i = 0; i < nf + 2; i++) {
    const double hz = inv(lo + (double)i * step);
    int64_t b = go_trunc(std::floor(((double)fft_size + 1.0) * hz / (double)sr + 0.5));
    bins[i] = std::min<int64_t>(b, fft_size / 2);
  }
  for (int m = 1; m <= nf; m++) {
    const int64_t l = bins[m - 1], c = bins[m], r = bins[m + 1];
    double* row = fb.data() + (size_t)(m - 1) * K;
    for (int64_t k = l; k < c && k < K; k++)
      if (c != l && k >= 0) row[k] = (double)(k - l) / (double)(c - l);
    for (int64_t k = c; k < r && k < K; k++)
      if (r != c && k >= 0) row[k] = (double)(r - k) / (double)(r - c);
  }
  return true;
}

bool make_mfcc_tables(int sr, int n_mfcc, int n_filters, int fb_kind, double low, double high, bool use_lifter,
                      double lifter, int fft_size, MfccTables& t) {
  if (n_mfcc <= 0) n_mfcc = 13;                                   // NewMFCCWithParams :58-70
  if (n_filters <= 0) n_filters = 26;
  if (high <= 0) high = (double)sr / 2.0;
  if (lifter <= 0) lifter = 22.0;
  std::vector<double> fb;
  if (!make_filterbank(fb_kind, n_filters, fft_size, sr, low, high, fb)) return false;
  t.n_mfcc = n_mfcc; t.n_mels = n_filters; t.K = fft_size / 2 + 1;
  t.lo.assign(n_filters, 0); t.hi.assign(n_filters, 0); t.woff.assign(n_filters, 0); t.w.clear();
  for (int m = 0; m < n_filters; m++) {
    const double* row = fb.data() + (size_t)m * t.K;
    int lo = -1, hi = -1;
    for (int k = 0; k < t.K; k++) if (row[k] != 0.0) { if (lo < 0) lo = k; hi = k + 1; }
    if (lo < 0) { lo = 0; hi = 0; }
    t.lo[m] = lo; t.hi[m] = hi; t.woff[m] = (int)t.w.size();
    for (int k = lo; k < hi; k++) t.w.push_back(row[k]);    // zeros inside the range kept: same sum order
  }
  t.dct.assign((size_t)n_mfcc * n_filters, 0.0);
  for (int k = 0; k < n_mfcc; k++)
    for (int n = 0; n < n_filters; n++) {
      double v = std::cos(kPi * (double)k * ((double)n + 0.5) / (double)n_filters);
      v *= (k == 0) ? std::sqrt(1.0 / (double)n_filters) : std::sqrt(2.0 / (double)n_filters);
      t.dct[(size_t)k * n_filters + n] = v;
    }
  t.lift.assign(n_mfcc, 1.0);
  if (use_lifter)
    for (int i = 1; i < n_mfcc; i++) t.lift[i] = 1.0 + (lifter / 2.0) * std::sin(kPi * (double)i / lifter);
  return true;
}

void balance_groups(const MfccTables& t, int groups, std::vector<int>& off, std::vector<int>& mels) {
  std::vector<std::vector<int>> g(groups);
  std::vector<long> load(groups, 0);
  std::vector<int> order(t.n_mels);
  for (int m = 0; m < t.n_mels; m++) order[m] = m;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return (t.hi[a] - t.lo[a]) > (t.hi[b] - t.lo[b]); });
  for (int m : order) {   // longest-processing-time first
    int best = 0;
    for (int k = 1; k < groups; k++) if (load[k] < load[best]) best = k;
    g[best].push_back(m);
    load[best] += (t.hi[m] - t.lo[m]) + 8;
  }
  off.assign(groups + 1, 0); mels.clear();
  for (int k = 0; k < groups; k++) { off[k] = (int)mels.size(); for (int m : g[k]) mels.push_back(m); }
  off[groups] = (int)mels.size();
}

std::vector<int> chroma_map(int fs, int sr) {
  const int K = fs / 2 + 1;
  std::vector<int> map(K, -1);
  const double res = (double)sr / (double)fs;                    // stft.go:158
  for (int f = 0; f < K; f++) {
    const double fr = (double)f * res;
    if (fr < 80.0 || fr > 8000.0) continue;
    const double midi = fr <= 0 ? 0.0 : 69.0 + 12.0 * std::log2(fr / 440.0);
    map[f] = (int)(go_trunc(std::round(midi)) % 12);
  }
  return map;
}

static double median_positive(const double* v, int n) {           // calculateMedian :975-1004
  double tmp[8];                                                  // n <= 5
  int m = 0;
  for (int i = 0; i < n; i++)
    if (v[i] > 0) {                                               // insertion sort of the positives
      int j = m++;
      while (j > 0 && tmp[j - 1] > v[i]) { tmp[j] = tmp[j - 1]; --j; }
      tmp[j] = v[i];
    }
  if (m == 0) return 0.0;
  return (m % 2 == 0) ? (tmp[m / 2 - 1] + tmp[m / 2]) / 2.0 : tmp[m / 2];
}

void YinTracker::step(double& pitch, double& conf, double& voicing) {
  double p = pitch, c = conf, v = conf;
  if (p != 0.0 && count > 0) {                                    // applyOctaveCorrection :789-827
    const int cnt = std::min(count, 5);
    if (cnt >= 3) {
      const double med = median_positive(hist + count - cnt, cnt);
      const double ratios[4] = {0.5, 2.0, 1.0 / 3.0, 3.0};
      for (double r : ratios) {
        const double ex = med * r;
        if (std::fabs(p - ex) / ex < 0.1) {
          if (std::fabs(p - med) > std::fabs(ex - med)) p = ex;
          break;
        }
      }
    }
  }
  if (c < 0.5) { p = 0; c = 0; v = 0; }                          // MinConfidence :781-785
  if (count == 20) {                                              // updateTemporalTracking :876-899
    for (int i = 1; i < 20; i++) hist[i - 1] = hist[i];
    hist[19] = p;
  } else {
    hist[count++] = p;
  }
  if (count > 1) {                                                // applyTemporalSmoothing :903-921
    const int cnt = std::min(count, 3);
    if (cnt >= 3) p = median_positive(hist + count - cnt, cnt);
    else p = 0.3 * p + (1 - 0.3) * prev;
  }
  prev = p;
  pitch = p; conf = c; voicing = v;
}

void track_rows(YinTracker& t, const double* raw_pitch, const double* raw_conf, int64_t lo, int64_t hi, int64_t n,
                double* pitch, double* conf, double* voicing) {
  for (int64_t i = lo; i < hi; i++) {
    double p = 0.0, q = 0.0, v = 0.0;
    if (i * 512 + 1024 <= n) {
      p = raw_pitch[i]; q = raw_conf[i];
      t.step(p, q, v);
    }
    if (pitch) pitch[i] = p;
    if (conf) conf[i] = q;
    voicing[i] = v;
  }
}

CorrSums corr_sums(const double* corr, int64_t nl) {
  CorrSums c;
  c.num_lags = nl;
  if (nl <= 0) return c;
  double pk = corr[0]; int64_t pidx = 0;                          // findPeak :526-544
  for (int64_t i = 0; i < nl; i++) if (std::fabs(corr[i]) > std::fabs(pk)) { pk = corr[i]; pidx = i; }
  c.peak = pk; c.peak_index = pidx;
  for (int64_t i = 0; i < nl; i++)                                // calculateSNR :572-601
    if (std::llabs(i - pidx) > 5) { c.noise_sum += corr[i] * corr[i]; c.noise_count++; }
  if (nl >= 3 && pidx > 0 && pidx < nl - 1)                        // calculateSharpness :611-619
    c.sharpness = -(corr[pidx + 1] - 2 * corr[pidx] + corr[pidx - 1]);
  for (int64_t i = 0; i < nl; i++)                                // findSecondPeak :622-636
    if (i != pidx && std::fabs(corr[i]) > std::fabs(c.second_peak)) c.second_peak = corr[i];
  for (int64_t i = 0; i < nl; i++)                                // calculatePeakToSidelobe :639-661
    if (std::llabs(i - pidx) > 10 && std::fabs(corr[i]) > c.max_sidelobe) c.max_sidelobe = std::fabs(corr[i]);
  return c;
}

NccMetrics ncc_metrics(const CorrSums& c, int64_t L, int64_t na, int64_t nb) {
  NccMetrics m;
  m.num_lags = c.num_lags;
  if (c.num_lags <= 0) return m;
  const double pk = c.peak;
  const int64_t pidx = c.peak_index;
  m.peak_corr = pk; m.peak_index = pidx; m.peak_lag = pidx - L;
  const int64_t n = std::min(na, nb);                              // calculatePValue :547-569
  m.p_value = 1.0;
  if (n > 2) {
    const double t = std::fabs(pk) * std::sqrt((double)(n - 2)) / std::sqrt(1.0 - pk * pk);
    m.p_value = t > 2.0 ? 0.01 : t > 1.5 ? 0.05 : t > 1.0 ? 0.1 : 0.5;
  }
  {                                                               // calculateSNR :572-601
    const double pv = std::fabs(pk);
    if (c.noise_count > 0) {
      const double lvl = std::sqrt(c.noise_sum / (double)c.noise_count);
      m.snr = lvl < 1e-10 ? INFINITY : 20.0 * std::log10(pv / lvl);
    }
  }
  m.sharpness = c.sharpness;
  m.second_peak = c.second_peak;
  {                                                               // calculatePeakToSidelobe :639-661
    const double pv = std::fabs(pk), ms = c.max_sidelobe;
    m.psl = ms < 1e-10 ? INFINITY : 20.0 * std::log10(pv / ms);
  }
  const int64_t lag = m.peak_lag;                                  // calculateOverlapLength :664-667
  int64_t s1, e1, s2, e2;
  if (lag >= 0) { s1 = 0; e1 = na; s2 = lag; e2 = nb; if (e1 > nb - lag) e1 = nb - lag; if (e2 > nb) e2 = nb; }
  else { s1 = -lag; e1 = na; s2 = 0; e2 = nb; if (e1 > na) e1 = na; if (e2 > na + lag) e2 = na + lag; }
  m.overlap = std::min(e1 - s1, e2 - s2);
  return m;
}

NccMetrics ncc_metrics(const double* corr, int64_t nl, int64_t L, int64_t na, int64_t nb) {
  return ncc_metrics(corr_sums(corr, nl), L, na, nb);
}

AlignScores xcorr_scores(const NccMetrics& m, int hop, int sr, int max_lag) {
  AlignScores s;                                                  // alignWithCrossCorrelation :151-181
  s.offset = m.peak_lag * hop;
  s.offset_seconds = (double)s.offset / (double)sr;
  s.similarity = go_min(1.0, go_max(0.0, std::fabs(m.peak_corr)));
  const double pm = std::fabs(m.peak_corr);
  if (pm >= 0.1) {                                                // calculateCorrelationConfidence :183-243
    double ps = pm; if (pm >= 0.6) ps = pm + (pm - 0.6) * 0.5;
    const double ss = go_min(0.9, m.sharpness * 8.0);
    double sl = 0.0; if (m.psl > 0 && !std::isinf(m.psl)) sl = go_min(0.8, m.psl / 15.0);
    double sn = 0.0; if (m.snr > 0) sn = go_min(0.7, m.snr / 25.0);
    double pen = 0.0;
    if (m.second_peak != 0 && pm > 0) { const double r = std::fabs(m.second_peak) / pm; if (r > 0.7) pen = (r - 0.7) * 0.25; }
    const double bonus = pm >= 0.75 ? 0.12 : pm >= 0.6 ? 0.08 : 0.0;
    const double c = 0.55 * ps + 0.22 * ss + 0.12 * sl + 0.06 * sn + 0.05 * 0.15 + bonus - pen;
    s.confidence = go_min(0.95, go_max(0.0, c));
  }
  if (pm >= 0.08) {                                               // calculateCorrelationQuality :245-305
    double pq = pm; if (pm >= 0.6) pq = pm + (pm - 0.6) * 0.4;
    const double sq = go_min(0.85, m.sharpness * 5.0);
    double slq = 0.0; if (m.psl > 0 && !std::isinf(m.psl)) slq = go_min(0.7, m.psl / 20.0);
    double snq = 0.0; if (m.snr > 0) snq = go_min(0.6, m.snr / 30.0);
    double lp = 0.0;
    if (max_lag > 0 && m.peak_lag < 0) {
      const double nr = std::fabs((double)m.peak_lag) / (double)max_lag;
      if (nr > 0.90) lp = (nr - 0.90) * 4.0;
    }
    const double qb = pm >= 0.7 ? 0.10 : pm >= 0.55 ? 0.06 : 0.0;
    s.quality = go_min(1.0, go_max(0.0, 0.50 * pq + 0.25 * sq + 0.15 * slq + 0.10 * snq + qb - lp));
  }
  s.noise_level = 1.0 - m.snr / 20.0;
  return s;
}

PathSums path_sums(const int32_t* pq, const int32_t* pr, const double* pc, int64_t P) {
  PathSums s;
  s.P = P;
  if (P <= 0) return s;
  s.p0q = pq[0]; s.p0r = pr[0]; s.p1q = pq[P - 1]; s.p1r = pr[P - 1];
  for (int64_t i = 0; i < P; i++) { s.offset_sum += pr[i] - pq[i]; s.sum_cost += pc[i]; }   // :530-541, :380-406
  int pd0 = 0, pd1 = 0;
  for (int64_t i = 1; i < P; i++) {
    const int d0 = pq[i] - pq[i - 1], d1 = pr[i] - pr[i - 1];
    if (d0 > 0 && d1 > 0) s.diag_steps++;                         // calculateDiagonalBias :514-540
    if (i > 1 && (d0 != pd0 || d1 != pd1)) s.changes++;           // calculatePathChanges :569-603
    pd0 = d0; pd1 = d1;
  }
  if (P > 1) {                                                    // calculateCostConsistency :466-512
    int64_t w = std::min<int64_t>(5, P / 4);
    w = std::max<int64_t>(w, 2);
    std::vector<double> sm(P);
    for (int64_t i = 0; i < P; i++) {
      double t = 0; int64_t c = 0;
      for (int64_t j = std::max<int64_t>(0, i - w / 2); j <= std::min<int64_t>(P - 1, i + w / 2); j++) { t += pc[j]; c++; }
      sm[i] = t / (double)c;
    }
    for (double v : sm) s.sum_smooth += v;
    const double mean = s.sum_smooth / (double)P;
    for (double v : sm) { const double d = v - mean; s.var_smooth += d * d; }
  }
  return s;
}

namespace {
double cost_consistency(const PathSums& s) {                      // alignment.go:466-512
  if (s.P <= 1) return 0.0;
  const double mean = s.sum_smooth / (double)s.P;
  if (mean <= 1e-10) return 1.0;
  const double var = s.var_smooth / (double)s.P;
  return 1.0 / (1.0 + std::sqrt(var) / mean);
}
double diagonal_bias(const PathSums& s) {                         // :514-540
  if (s.P <= 1) return 1.0;
  const double ratio = (double)s.diag_steps / (double)(s.P - 1);
  return 1.0 / (1.0 + std::exp(-10.0 * (ratio - 0.3)));
}
double path_changes_ratio(const PathSums& s) {                    // :569-603 / :620-643
  return (double)s.changes / (double)(s.P - 1);
}
double dtw_quality(const PathSums& s, int64_t nq, int64_t nr) {
  if (s.P == 0) return 0.0;                                       // calculateDTWQuality :543-566
  double eff = (double)std::max(nq, nr) / (double)s.P;
  eff = go_min(1.0, eff);
  const double smooth = s.P <= 2 ? 1.0 : go_max(0.0, 1.0 - path_changes_ratio(s));
  const double q = 0.3 * eff + 0.3 * diagonal_bias(s) + 0.2 * smooth + 0.2 * cost_consistency(s);
  return go_min(1.0, go_max(0.0, q));
}
}  // namespace

AlignScores dtw_scores(const PathSums& ps, int64_t nq, int64_t nr, double dist, int sr) {
  AlignScores s;                                                  // alignWithDTW :129-148
  const int64_t P = ps.P;
  const double avg = (double)(nq + nr) / 2.0;
  if (avg != 0) {                                                 // calculateSimilarityFromDTW :380-406
    const double ds = 1.0 / (1.0 + dist / avg);
    double mc = 0; if (P > 0) mc = ps.sum_cost / (double)P;
    s.similarity = go_min(1.0, go_max(0.0, 0.5 * ds + 0.3 * dtw_quality(ps, nq, nr) + 0.2 * (1.0 / (1.0 + mc))));
  }
  if (P > 0 && avg != 0) {                                        // calculateDTWConfidence :420-463
    const double c1 = std::exp(-(dist / avg) * 2.0);
    const double pe = go_min(1.0, (double)std::max(nq, nr) / (double)P);
    s.confidence = go_min(1.0, go_max(0.0, 0.4 * c1 + 0.25 * pe + 0.2 * cost_consistency(ps) +
                                               0.15 * diagonal_bias(ps)));
  }
  if (P > 0) s.offset = ps.offset_sum / P;                        // calculateAverageOffset :530-541
  s.offset_seconds = (double)s.offset / (double)sr;               // F9: frames / sample rate
  s.quality = dtw_quality(ps, nq, nr);
  if (P >= 3) s.stability = go_max(0.0, 1.0 - path_changes_ratio(ps));   // :620-643
  return s;
}

AlignScores dtw_scores(const int32_t* pq, const int32_t* pr, const double* pc, int64_t P, int64_t nq, int64_t nr,
                       double dist, int sr) {
  return dtw_scores(path_sums(pq, pr, pc, P), nq, nr, dist, sr);
}

double energy_variance(const double* e, size_t n) {               // energy.go:96-117
  if (n < 2) return 0.0;
  double mean = 0.0;
  for (size_t i = 0; i < n; i++) mean += e[i];
  mean /= (double)n;
  double var = 0.0;
  for (size_t i = 0; i < n; i++) { const double d = e[i] - mean; var += d * d; }
  return var / (double)(n - 1);
}

double loudness_range_from_rms(std::vector<double> v) {           // energy.go:145-205
  if (v.empty()) return 0.0;
  for (double& x : v) x = x > 0 ? -0.691 + 10.0 * std::log10(x * x) : -70.0;
  std::sort(v.begin(), v.end());
  const int64_t lo = (int64_t)(0.10 * (double)(v.size() - 1));
  const int64_t hi = (int64_t)(0.95 * (double)(v.size() - 1));
  double lv = v[lo], hv = v[hi];
  if (lv <= 0.0) lv = 1e-10;
  if (hv <= 0.0) return 0.0;
  return 20.0 * std::log10(hv / lv);
}

double percentile10_threshold(const double* e, size_t n) {        // speech.go:594-605 (bubble sort)
  // the element at index n/10 of the sorted order; a selection gives the same value in O(n)
  std::vector<double> v(e, e + n);
  std::nth_element(v.begin(), v.begin() + n / 10, v.end());
  return v[n / 10];
}

double silence_ratio(const double* e, size_t n, double thr) {
  if (!n) return 0.0;
  int64_t k = 0;
  for (size_t i = 0; i < n; i++) if (e[i] <= thr) k++;
  return (double)k / (double)n;
}

std::vector<double> pause_durations(const double* e, size_t n, double thr, int hop, int rate) {
  std::vector<double> pauses;
  const double fts = (double)hop / (double)rate;
  bool in = false; size_t st = 0;
  auto close = [&](size_t end) { const double d = (double)(int64_t)(end - st) * fts; if (d > 0.1) pauses.push_back(d); };
  for (size_t i = 0; i < n; i++) {
    if (e[i] <= thr) { if (!in) { in = true; st = i; } }
    else if (in) { close(i); in = false; }
  }
  if (in) close(n);                                               // the signal ends in a pause
  return pauses;
}

std::vector<int64_t> detect_onsets(const double* e, size_t n) {   // with calculateAdaptiveThreshold :695-716
  std::vector<int64_t> onsets;
  if (n < 3) return onsets;
  std::vector<double> der(n - 1);
  for (size_t i = 0; i + 1 < n; i++) der[i] = e[i + 1] - e[i];
  double sum = 0; for (double v : der) sum += v;
  const double mean = sum / (double)der.size();
  double var = 0; for (double v : der) { const double d = v - mean; var += d * d; }
  const double thr = mean + 2 * std::sqrt(var / (double)der.size());
  for (size_t i = 1; i + 1 < der.size(); i++)
    if (der[i] > der[i - 1] && der[i] > der[i + 1] && der[i] > thr) onsets.push_back((int64_t)i);
  return onsets;
}

std::vector<double> attack_times(const std::vector<int64_t>& onsets, const double* e, int hop, int rate) {
  std::vector<double> att(onsets.size());
  const double fts = (double)hop / (double)rate;
  for (size_t i = 0; i < onsets.size(); i++) {
    const int64_t on = onsets[i];
    const double pk = e[on];
    int64_t st = on;
    for (int64_t j = on - 1; j >= 0 && j > on - 10; j--) if (e[j] < 0.1 * pk) { st = j; break; }
    att[i] = (double)(on - st) * fts;
    if (att[i] > 0.1) att[i] = 0.1;
  }
  return att;
}

double speech_rate(double silence, int64_t n_samples, int rate) {
  const double dur = (double)n_samples / (double)rate;
  const double speech_time = dur * (1.0 - silence);
  return speech_time > 0 ? 4.0 * speech_time / dur : 3.0;
}

static bool check_periodicity(const double* fr, int64_t n) {      // speech_analysis.go:165-202, first 1024 samples
  if (n < 1024) return false;
  double mc = 0.0;
  for (int lag = 20; lag < 400 && lag < 512; lag++) {
    double corr = 0.0; int cnt = 0;
    for (int i = 0; i < 1024 - lag; i++) { corr += fr[i] * fr[i + lag]; cnt++; }
    if (cnt > 0) { corr /= (double)cnt; if (corr > mc) mc = corr; }
  }
  double en = 0.0;
  for (int i = 0; i < 1024; i++) en += fr[i] * fr[i];
  en /= 1024.0;
  if (en > 0) mc /= en;
  return mc > 0.1;
}

bool detect_speech(int64_t n_samples, int rate, double crossings, double sum_sq, const double* head, int64_t head_n) {
  if (n_samples < (int64_t)(rate / 4)) return false;
  const double z = n_samples <= 1 ? 0.0 : crossings / (double)(n_samples - 1);
  if (z < 0.01 || z > 0.3) return false;
  if (std::sqrt(sum_sq / (double)n_samples) < 0.001) return false;
  return check_periodicity(head, head_n);
}

// ---- MusicFeatureExtractor.ExtractFeatures' scalar tail (fingerprint/extractors/music.go) ----------

int64_t go_int(double x) {
  if (!(x >= -9.2233720368547758e18 && x < 9.2233720368547758e18)) return std::numeric_limits<int64_t>::min();
  return (int64_t)x;
}

std::vector<int> contrast_edges(int sample_rate, int K, int nb) {
  std::vector<int> e(nb + 1);
  const double nyquist = (double)sample_rate / 2.0;
  const double minf = 200.0;
  double maxf = nyquist;
  if (maxf <= minf) maxf = minf * 2;
  const double lmin = std::log10(minf), lmax = std::log10(maxf);
  const double step = (lmax - lmin) / (double)nb;
  for (int i = 0; i <= nb; i++) {
    const double f = std::pow(10.0, lmin + (double)i * step);
    int64_t b = go_int(f * (double)(K - 1) / nyquist);
    if (b >= K) b = K - 1;
    if (b < 0) b = 0;
    e[i] = (int)b;
  }
  for (int i = 1; i <= nb; i++)
    if (e[i] <= e[i - 1]) e[i] = e[i - 1] + 1;
  return e;
}

double gonum_variance(const double* x, size_t n) {                // common/math.go:22-27
  if (n < 2) return 0.0;
  double s = 0.0;
  for (size_t i = 0; i < n; i++) s += x[i];
  const double mean = s / (double)n;
  double ss = 0.0, comp = 0.0;
  for (size_t i = 0; i < n; i++) { const double d = x[i] - mean; ss += d * d; comp += d; }
  return (ss - comp * comp / (double)n) / (double)(n - 1);
}

std::vector<double> crest_factors(const double* peaks, const double* energy, size_t n) {   // :428-444
  std::vector<double> crest(n, 0.0);
  for (size_t i = 0; i < n; i++) if (energy[i] > 0) crest[i] = peaks[i] / energy[i];
  return crest;
}

std::vector<double> energy_entropy(const double* e, size_t n, double* loudness_range) {     // :481-510
  std::vector<double> ent(n, 0.0);
  double mx = 0.0, mn = std::numeric_limits<double>::infinity();
  for (size_t i = 0; i < n; i++) {
    if (e[i] > 0) ent[i] = -e[i] * std::log2(e[i]);
    if (e[i] > mx) mx = e[i];
    if (e[i] < mn && e[i] > 0) mn = e[i];
  }
  *loudness_range = (mn != std::numeric_limits<double>::infinity() && mn > 0) ? 20 * std::log10(mx / mn) : 0.0;
  return ent;
}

bool chroma_slice_panics(int64_t F, int64_t hop, int64_t n, int64_t* frame) {
  if (!((F - 1) * hop > n)) return false;
  *frame = n / hop + 1;
  return true;
}

bool percentile_panics(int64_t n, int64_t* index, int64_t* L) {
  *L = n >= 1024 ? (n - 1024) / 512 + 1 : 0;
  if (*L < 2) return false;
  *index = go_int(10.0 * (double)(*L - 1));
  return true;
}

// ---- ContentDetector (fingerprint/content_detector.go) ---------------------------------------------

sonar_acoustic_features content_features(uint64_t crossings, double max, double min, const double* spec, int K,
                                         const double* es, int64_t fe, const double* tsm, int64_t ft, int64_t n,
                                         int sr) {
  sonar_acoustic_features f = {};
  // calculateZeroCrossingRate (:220-233)
  f.zero_crossing_rate = n <= 1 ? 0.0 : (double)crossings / (double)(n - 1);
  // calculateSpectralCentroid (:236-252)
  {
    double ws = 0.0, ms = 0.0;
    for (int i = 0; i < K; i++) {
      const double fr = (double)i * (double)sr / (double)(K * 2);
      ws += fr * spec[i];
      ms += spec[i];
    }
    f.spectral_centroid = ms == 0 ? 0.0 : ws / ms;
  }
  // calculateEnergyVariance (:255-290)
  if (n >= 2048 && fe > 1) {
    double mean = 0.0;
    for (int64_t i = 0; i < fe; i++) mean += es[i] / 1024.0;
    mean /= (double)fe;
    double var = 0.0;
    for (int64_t i = 0; i < fe; i++) {
      const double d = es[i] / 1024.0 - mean;
      var += d * d;
    }
    f.energy_variance = var / (double)fe;
  }
  // calculateSilenceRatio (:293-317)
  if (fe > 0) {
    int64_t silent = 0;
    for (int64_t i = 0; i < fe; i++) silent += std::sqrt(es[i] / 1024.0) < 0.01;
    f.silence_ratio = (double)silent / (double)fe;
  }
  // calculateDynamicRange (:320-343)
  f.dynamic_range = (min == 0 || std::isinf(min)) ? 0.0 : 20.0 * std::log10(max / min);
  // calculateFreqEnergyRatio (:346-369)
  {
    const int split = K / 4;
    double lo = 0.0, hi = 0.0;
    for (int i = 0; i < split && i < K; i++) lo += spec[i] * spec[i];
    for (int i = split; i < K; i++) hi += spec[i] * spec[i];
    const double tot = lo + hi;
    if (tot != 0) { f.low_freq_energy = lo / tot; f.high_freq_energy = hi / tot; }
  }
  // calculateHarmonicRatio (:372-401)
  if (K >= 10) {
    std::vector<int> peaks;
    for (int i = 2; i < K - 2; i++)
      if (spec[i] > spec[i - 1] && spec[i] > spec[i + 1] && spec[i] > spec[i - 2] && spec[i] > spec[i + 2])
        peaks.push_back(i);
    if (peaks.size() >= 2) {
      int harm = 0;
      for (size_t q = 1; q < peaks.size(); q++) {
        const double r = (double)peaks[q] / (double)peaks[0];
        if (std::fabs(r - std::round(r)) < 0.1) harm++;
      }
      f.harmonic_ratio = (double)harm / (double)(peaks.size() - 1);
    }
  }
  // calculateTemporalStability (:404-447)
  const int64_t ts = sr / 10;
  if (n >= 3 * ts && ft > 1) {
    double mean = 0.0;
    for (int64_t i = 0; i < ft; i++) mean += tsm[i];
    mean /= (double)ft;
    if (mean != 0) {
      double var = 0.0;
      for (int64_t i = 0; i < ft; i++) {
        const double d = tsm[i] - mean;
        var += d * d;
      }
      var /= (double)ft;
      f.temporal_stability = go_max(0.0, 1.0 - std::sqrt(var) / mean);
    }
  }
  return f;
}

ContentClass classify_content(const sonar_acoustic_features& f, double thr) {
  double music = 0.0, speech = 0.0, sports = 0.0;
  if (f.zero_crossing_rate < 0.1) music += 2.0;
  if (f.harmonic_ratio > 0.3) music += 2.0;
  if (f.temporal_stability > 0.5) music += 1.0;
  if (f.dynamic_range > 20) music += 1.0;
  if (f.zero_crossing_rate > 0.05 && f.zero_crossing_rate < 0.3) speech += 2.0;
  if (f.spectral_centroid > 800 && f.spectral_centroid < 3000) speech += 2.0;
  if (f.harmonic_ratio < 0.2) speech += 1.0;
  if (f.silence_ratio > 0.1 && f.silence_ratio < 0.4) speech += 1.0;
  if (f.energy_variance > 0.3) sports += 2.0;
  if (f.dynamic_range > 30) sports += 1.5;
  if (f.temporal_stability < 0.4) sports += 1.0;
  const int types[4] = {SONAR_CT_MUSIC, SONAR_CT_NEWS, SONAR_CT_TALK, SONAR_CT_SPORTS};
  const double scores[4] = {music, speech, speech * 0.9, sports};
  ContentClass best = {SONAR_CT_UNKNOWN, 0.0};
  double bs = thr;
  for (int i = 0; i < 4; i++)
    if (scores[i] > bs) { bs = scores[i]; best.type = types[i]; }
  best.confidence = bs / 6.0;
  return best;
}

// ---- VoiceQualityAnalyzer.AnalyzeVoiceQuality (algorithms/speech/voice_quality.go) -----------------

PitchPeriods period_walk(const double* raw_pitch, const double* raw_conf, int64_t Fv, int64_t n, int sr) {
  PitchPeriods w;
  YinTracker tr;
  int64_t last_end = 0;
  for (int64_t i = 0; i < Fv; i++) {
    double p = raw_pitch[i], cf = raw_conf[i], v = 0.0;
    tr.step(p, cf, v);
    if (v > 0.5 && cf > 0.5 && p >= 50.0 && p <= 500.0) {
      const int64_t len = (int64_t)((double)sr / p);
      const int64_t s0 = std::max<int64_t>(i * 256, last_end), e0 = s0 + len;
      if (e0 < n) { w.st.push_back(s0); w.ln.push_back(len); w.f0.push_back(p); last_end = e0; }
    }
  }
  if (n == 1024) { double p = raw_pitch[0], cf = raw_conf[0]; tr.step(p, cf, w.voicing); }
  return w;
}

sonar_voice_quality_result voice_quality_from(const int64_t* ln, const double* amp, const double* f0, int64_t np,
                                              const double* ac, const double* head, int64_t n, int sr, double vstr) {
  // calculateJitter (:160-191) and calculateShimmer (:194-229)
  double avg = 0.0, js = 0.0;
  for (int64_t k = 0; k < np; k++) avg += (double)ln[k];
  avg /= (double)np;
  for (int64_t k = 1; k < np; k++) js += std::fabs((double)ln[k] - (double)ln[k - 1]);
  const double jitter = avg == 0 ? 0.0 : (js / (double)(np - 1)) / avg * 100.0;
  double aavg = 0.0, ss = 0.0;
  for (int64_t k = 0; k < np; k++) aavg += amp[k];
  aavg /= (double)np;
  for (int64_t k = 1; k < np; k++) ss += std::fabs(amp[k] - amp[k - 1]);
  const double shimmer = aavg == 0 ? 0.0 : (ss / (double)(np - 1)) / aavg * 100.0;
  // calculateHNR (:232-294): peak of the autocorrelation within +-25 % of the mean-F0 lag
  double mf = 0.0, hnr = 0.0;
  for (int64_t k = 0; k < np; k++) mf += f0[k];
  mf /= (double)np;
  if (ac) {
    const int64_t el = (int64_t)((double)sr / mf);
    if (el < 2048) {
      const int64_t r = el / 4, a = std::max<int64_t>(1, el - r), b = std::min<int64_t>(2047, el + r);
      double mc = 0.0;
      for (int64_t i = a; i <= b; i++) if (ac[i] > mc) mc = ac[i];
      if (mc > 0 && mc < ac[0]) hnr = 10.0 * std::log10(mc / (ac[0] - mc));
    }
  }
  // calculateF0Stability (:297-322), calculateAmplitudeStability (:325-360)
  double var = 0.0;
  for (int64_t k = 0; k < np; k++) { const double d = f0[k] - mf; var += d * d; }
  var /= (double)np;
  const double f0s = mf == 0 ? 0.0 : go_max(0.0, 1.0 - std::sqrt(var) / mf);
  double av = 0.0;
  for (int64_t k = 0; k < np; k++) { const double d = amp[k] - aavg; av += d * d; }
  av /= (double)np;
  const double ams = aavg == 0 ? 0.0 : go_max(0.0, 1.0 - std::sqrt(av) / aavg);
  // calculateNoiseMeasure (:374-398) on the first 1024 samples
  double nm = 0.0;
  if (n >= 1024) {
    double hf = 0.0, te = 0.0;
    for (int i = 1; i < 1024; i++) { const double d = head[i] - head[i - 1]; hf += d * d; te += head[i] * head[i]; }
    nm = te == 0 ? 0.0 : hf / te;
  }
  // calculateF0Statistics (:401-426), calculateOverallQuality (:429-437), calculateAnalysisQuality (:440-451)
  double lo = f0[0], hi = f0[0];
  for (int64_t k = 0; k < np; k++) { if (f0[k] < lo) lo = f0[k]; if (f0[k] > hi) hi = f0[k]; }
  sonar_voice_quality_result q = {};
  q.jitter = jitter;
  q.shimmer = shimmer;
  q.hnr = hnr;
  q.noise_measure = nm;
  q.f0_stability = f0s;
  q.amplitude_stability = ams;
  q.voicing_strength = vstr;
  q.overall_quality = (go_max(0, 1.0 - jitter / 5.0) + go_max(0, 1.0 - shimmer / 10.0) +
                       go_min(1.0, go_max(0, hnr / 20.0)) + f0s) / 4.0;
  q.num_periods = np;
  q.mean_f0 = mf;
  q.f0_range = hi - lo;
  q.analysis_quality = (go_min(1.0, (double)np / 10.0) + f0s + go_min(1.0, go_max(0, hnr / 15.0))) / 3.0;
  return q;
}

// ---- PitchDetector post-processing for every method and parameter set (pitch_detection.go:767-1160)
static double median_positive_n(const double* v, int n) {        // calculateMedian :978-1007, n <= 20
  double tmp[20];
  int m = 0;
  for (int i = 0; i < n; i++)
    if (v[i] > 0) {
      int j = m++;
      while (j > 0 && tmp[j - 1] > v[i]) { tmp[j] = tmp[j - 1]; --j; }
      tmp[j] = v[i];
    }
  if (m == 0) return 0.0;
  return (m % 2 == 0) ? (tmp[m / 2 - 1] + tmp[m / 2]) / 2.0 : tmp[m / 2];
}

PitchRow PitchTracker::step(const PitchTrackParams& prm, double raw_pitch, double raw_conf, int n_candidates,
                            double second_conf) {
  PitchRow r;
  r.pitch = raw_pitch; r.confidence = raw_conf; r.voicing = raw_conf; r.periodicity = raw_conf;
  if (prm.octave_correction && r.pitch != 0.0 && count > 0) {     // applyOctaveCorrection :793-827
    const int cnt = std::min(count, 5);
    if (cnt >= 3) {
      const double med = median_positive_n(hist + count - cnt, cnt);
      const double ratios[4] = {0.5, 2.0, 1.0 / 3.0, 3.0};
      for (double q : ratios) {
        const double ex = med * q;
        if (std::fabs(r.pitch - ex) / ex < 0.1) {
          if (std::fabs(r.pitch - med) > std::fabs(ex - med)) { r.pitch = ex; r.f0_multiple = q; }
          break;
        }
      }
    }
  }
  if (n_candidates == 1) r.clarity = raw_conf;                     // calculateClarity :830-849
  else if (n_candidates > 1 && raw_conf > 0) r.clarity = (raw_conf - second_conf) / raw_conf;
  r.strength = (r.periodicity + r.voicing) / 2.0;                  // calculateStrength :852-855
  double base = r.confidence;                                      // calculateSalience :858-873
  if (r.pitch >= 200 && r.pitch <= 800) base *= 1.2;
  if (r.pitch < 100 || r.pitch > 1000) base *= 0.8;
  r.salience = go_min(base, 1.0);
  if (r.confidence < prm.min_confidence) { r.pitch = 0.0; r.confidence = 0.0; r.voicing = 0.0; }   // :783-787
  if (count == 20) {                                               // updateTemporalTracking :876-902
    for (int i = 1; i < 20; i++) hist[i - 1] = hist[i];
    hist[19] = r.pitch;
  } else {
    hist[count++] = r.pitch;
  }
  if (prm.temporal_smoothing && count > 1) {                       // applyTemporalSmoothing :905-921
    const int cnt = prm.median_filter > 0 ? std::min(count, prm.median_filter) : 0;
    if (cnt >= 3) r.pitch = median_positive_n(hist + count - cnt, cnt);
    else r.pitch = 0.3 * r.pitch + (1 - 0.3) * prev;
  }
  if (count >= 3) {                                                // calculateStability :924-963
    int m = 0;
    double mean = 0.0;
    for (int i = 0; i < count; i++) if (hist[i] > 0) { mean += hist[i]; ++m; }
    if (m >= 2) {
      mean /= (double)m;
      double var = 0.0;
      for (int i = 0; i < count; i++) if (hist[i] > 0) { const double d = hist[i] - mean; var += d * d; }
      var /= (double)(m - 1);
      if (mean > 0) r.stability = go_max(0.0, 1.0 - std::sqrt(var) / mean);
    }
  }
  prev = r.pitch;
  return r;
}

bool pitch_stability(const double* pitch, int64_t n, int sample_rate, int hop_size, double out7[7]) {
  for (int k = 0; k < 7; k++) out7[k] = 0.0;
  if (n < 2) return false;
  std::vector<double> v;
  for (int64_t i = 0; i < n; i++) if (pitch[i] > 0) v.push_back(pitch[i]);
  const size_t m = v.size();
  if (m < 2) return false;
  double mean = 0.0;
  for (double x : v) mean += x;
  mean /= (double)m;
  double var = 0.0;
  for (double x : v) { const double d = x - mean; var += d * d; }
  var /= (double)(m - 1);
  const double sd = std::sqrt(var);
  double jitter = 0.0;
  for (size_t i = 1; i < m; i++) jitter += std::fabs(v[i] - v[i - 1]);
  jitter /= (double)(m - 1);
  double vib = 0.0;                                                // estimateVibratoRate :1116-1160
  if (m >= 10) {
    const double nn = (double)m;
    const double sx = nn * (nn - 1) / 2, sx2 = (nn - 1) * nn * (2 * nn - 1) / 6;
    double sy = 0.0, sxy = 0.0;
    for (size_t i = 0; i < m; i++) { sy += v[i]; sxy += (double)i * v[i]; }
    const double slope = (nn * sxy - sx * sy) / (nn * sx2 - sx * sx);
    const double icpt = (sy - slope * sx) / nn;
    int64_t cross = 0;
    double prevd = 0.0;
    for (size_t i = 0; i < m; i++) {
      const double d = v[i] - (icpt + slope * (double)i);
      if (i > 0 && ((d > 0 && prevd <= 0) || (d <= 0 && prevd > 0))) ++cross;
      prevd = d;
    }
    const double hop_rate = (double)sample_rate / (double)hop_size;
    vib = (double)cross / (2.0 * nn / hop_rate);
  }
  out7[0] = mean; out7[1] = sd; out7[2] = sd / mean; out7[3] = jitter;
  out7[4] = 1.0 / (1.0 + sd / mean); out7[5] = vib; out7[6] = (double)m / (double)n;
  return true;
}

HratioRow HratioTracker::step(bool smoothing, int len, double raw) {
  HratioRow r;
  r.ratio = raw;
  if (smoothing && !hist.empty()) r.ratio = 0.3 * raw + (1.0 - 0.3) * prev;    // applyTemporalSmoothing :939-947
  const size_t n = hist.size();
  if (n >= 3) {                                                                // calculateTemporalStability :949-964
    double s = 0.0;
    for (double v : hist) s += v;
    const double mean = s / (double)n;
    if (mean > 0) {
      const double q = 1.0 - std::sqrt(gonum_variance(hist.data(), n)) / mean;
      r.stability = q != q ? q : std::max(0.0, q);                             // math.Max: a NaN stays
    }
  }
  if (n >= 2) {                                                                // calculateTemporalCoherence :966-986
    double total = 0.0;
    for (size_t i = 1; i < n; ++i) total += std::fabs(hist[i] - hist[i - 1]);
    r.coherence = std::exp(-(total / (double)(n - 1)) / 10.0);
  }
  hist.push_back(r.ratio);                                                     // updateTemporalTracking :988-1002
  const size_t keep = (size_t)std::max(len, 0) * 2;
  if (hist.size() > keep) hist.erase(hist.begin(), hist.end() - (std::ptrdiff_t)keep);
  prev = r.ratio;
  return r;
}

double gonum_linear_regression(const double* x, const double* y, size_t n) {   // common/math.go:237-262, the slope
  double sx = 0.0, sy = 0.0;
  for (size_t i = 0; i < n; i++) { sx += x[i]; sy += y[i]; }
  const double xu = sx / (double)n, yu = sy / (double)n;
  double ss = 0.0, xc = 0.0, yc = 0.0;
  for (size_t i = 0; i < n; i++) {
    const double xd = x[i] - xu, yd = y[i] - yu;
    ss += xd * yd; xc += xd; yc += yd;
  }
  const double cov = (ss - xc * yc / (double)n) / (double)(n - 1);
  return cov / gonum_variance(x, n);
}

InharmRow InharmTracker::step(bool tracking, int window, double raw, double f0) {
  InharmRow r;
  r.inharmonicity = raw;
  if (tracking && !hist.empty()) r.inharmonicity = 0.3 * raw + (1.0 - 0.3) * hist.back();   // :1009-1011, :1023-1032
  const size_t n = hist.size();
  if (n >= 3) {
    double s = 0.0;
    for (double v : hist) s += v;
    const double mean = s / (double)n;
    if (mean != 0) r.stability = 1.0 / (1.0 + std::sqrt(gonum_variance(hist.data(), n)) / std::fabs(mean));   // :1034-1050
    std::vector<double> x(n);
    for (size_t i = 0; i < n; i++) x[i] = (double)i;
    r.trend = gonum_linear_regression(x.data(), hist.data(), n);                              // :1052-1066
  }
  if (f0_hist.size() >= 3) {                                                                  // :1068-1084
    const size_t m = f0_hist.size();
    double s = 0.0;
    for (double v : f0_hist) s += v;
    const double mean = s / (double)m;
    if (mean > 0) r.f0_stability = 1.0 / (1.0 + std::sqrt(gonum_variance(f0_hist.data(), m)) / mean);
  }
  if (tracking) {                                                                             // :1086-1101
    hist.push_back(r.inharmonicity);
    f0_hist.push_back(f0);
    const size_t keep = (size_t)std::max(window, 0);
    if (hist.size() > keep) {
      hist.erase(hist.begin(), hist.end() - (std::ptrdiff_t)keep);
      f0_hist.erase(f0_hist.begin(), f0_hist.end() - (std::ptrdiff_t)keep);
    }
  }
  return r;
}

}  // namespace host
}  // namespace sonar
