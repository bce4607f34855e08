// inharmonicity_kernels.hip -- InharmonicityAnalyzer.AnalyzeFrame per frame (algorithms/tonal/inharmonicity.go:236-292),
// without postProcessResult's tracking, float64 like the Go reference.
//
//  inharm_kernel<PCM>   one block of 256 threads per frame.  PCM: the raw frame (no window, no pre-emphasis)
//                       is transformed in LDS (hratio_kernel's butterfly, table and level order), |X| of the
//                       first W / 2 bins; else the row of K magnitudes is loaded.
//  inharm_beat_tail_kernel   calculateBeatPatternInharmonicity's tail (:563-567) over rows of correlations: one
//                       wave per row; FindPeaks(corr, 0.1, 1.0) (common/math.go:265: strict local maxima
//                       >= 0.1, the distance of 1.0 never binds) compacted in order, the lags' mean (exact:
//                       they are integers) and gonum's two-pass variance in index order.
//
// The stage of inharm_kernel, in order (Kernel 4k):
//  1. analyzeHarmonicStructure (:341-365): one lane of wave 0 per harmonic runs findHarmonicPeak (:376-416)
//     and the two acceptance tests; the kept lanes are compacted in h order (ballot + prefix count) into
//     five 64-entry LDS arrays.  The count decides the row's status.
//  2. Railsback only: fitRailsbackCurve's 201 errors (:640-654), one grid value per thread of the block, each
//     a sum over the harmonics in order; wave 0 then takes the first strict minimum, which skips the NaN of a
//     negative 1 + B n^2 because a NaN is never below anything.
//  3. the method, the String model, the three quality metrics and the quality class by wave 0, every lane
//     running the same ordered loops over the <= 64 harmonics (LDS broadcasts, no divergence); Statistical's
//     quartiles are rank selections by comparison counts, one value per lane, as hratio_kernel's noise floor.
//  4. the scalars through sqrt / log10 / exp last, then the stores.
// Every comparison and every sum here decides an output bit: built without FMA contraction.
#include <cstdint>

#include "go_math.h"
#include "inharmonicity_kernels.h"
#include "lds_fft.h"
#include "wave.h"
#include "../../include/sonar_gpu.h"

#pragma clang fp contract(off)

namespace sonar {

namespace {

constexpr int kNone = 0x7fffffff;

// Go's int(float64) on amd64 (CVTTSD2SQ): a NaN or a value out of range is the minimum int64
__device__ __forceinline__ int64_t go_int(double x) {
  return (x >= -9223372036854775808.0 && x < 9223372036854775808.0) ? (int64_t)x : INT64_MIN;
}

// common.Mean / common.Variance (common/math.go:14-27) as host::gonum_variance states them: the mean's sum
// sequential, the variance compensated two-pass over n - 1
__device__ double mean_of(const double* x, int n) {
  if (n == 0) return 0.0;
  double s = 0.0;
  for (int i = 0; i < n; ++i) s = s + x[i];
  return s / (double)n;
}
__device__ double variance_of(const double* x, int n) {
  if (n < 2) return 0.0;
  const double mean = mean_of(x, n);
  double ss = 0.0, comp = 0.0;
  for (int i = 0; i < n; ++i) { const double d = x[i] - mean; ss = ss + d * d; comp = comp + d; }
  return (ss - comp * comp / (double)n) / (double)(n - 1);
}

// n f0 sqrt(1 + B n^2) as :485, :645, :668 and :909 spell it
__device__ __forceinline__ double stretched(double n, double f0, double B) { return n * f0 * sqrt(1.0 + B * n * n); }

// calculateFletcherMunsonWeight (:682-704)
__device__ double fm_weight(double freq) {
  if (freq < 20.0 || freq > 20000.0) return 0.0;
  double w = 1.0;
  if (freq < 1000.0) w = 0.5 + 0.5 * (freq / 1000.0);
  else if (freq > 4000.0) w = 1.0 - 0.3 * log10(freq / 4000.0);
  return go_max(0.1, w);
}

// stat.Quantile(p, stat.Empirical, sorted, nil) of x[0, n), n >= 1, by the wave: lane j holds x[j]; the
// value with fewer than c smaller and at least c not larger, c the first count that reaches p n
__device__ double quantile_of(const double* x, int n, double p, int lane, double* slot) {
  const double fidx = p * (double)n;
  int c = 1;
  while (c < n && (double)c < fidx) ++c;
  const double v = lane < n ? x[lane] : 0.0;
  int less = 0, leq = 0;
  for (int k = 0; k < n; ++k) {
    const double xk = x[k];
    less += xk < v ? 1 : 0;
    leq += xk <= v ? 1 : 0;
  }
  const uint64_t b = __ballot(lane < n && less < c && c <= leq);
  const int src = b ? __ffsll((long long)b) - 1 : 0;
  if (lane == src) *slot = v;
  wave_lds_sync();
  return *slot;
}

}  // namespace

// LDS, in doubles: PCM  re[W] | im[W] | M[K];  spectrum  M[K].  Then hf[64] | hi[64] | ha[64] | hd[64] (the
// kept harmonics: frequency, ideal frequency, amplitude, deviation) | dv[64] (HarmonicDeviations) |
// sp[64] (spacings) | E[256] (the grid's errors) | sc[8] | hn[64] (int) | misc[8] (int)
size_t inharm_lds_bytes(int K, bool pcm) {
  return 8 * ((size_t)(pcm ? 5 : 1) * K + 6 * 64 + 256 + 8) + 4 * (64 + 8);
}

template <bool PCM>
__global__ __launch_bounds__(256) void inharm_kernel(const InharmArgs a) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int K = a.K, W = a.W, sr = a.sr;
  const int64_t fi = blockIdx.x;
  double* M = PCM ? lds + 2 * W : lds;
  double* hf = M + K;
  double* hi = hf + 64;
  double* ha = hi + 64;
  double* hd = ha + 64;
  double* dv = hd + 64;
  double* sp = dv + 64;
  double* E = sp + 64;
  double* sc = E + 256;
  int* hn = (int*)(sc + 8);
  int* misc = hn + 64;
  const uint64_t below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  const InharmOut& o = a.o;

  const double f0 = a.f0[fi], f0c = a.f0_conf[fi];
  // :236, and a non-finite f0 (the host refuses it where it can read it): no bin can be formed from one
  const bool valid = !(f0 <= 0.0 || f0 < a.min_freq || f0 > a.max_freq) && f0 - f0 == 0.0;

  // ---- the spectrum (:321-328)
  if (valid) {                                                          // block-uniform
    if constexpr (PCM) {
      double *sre = lds, *sim = lds + W;
      const int logN = fft_log2i(W);
      const int64_t s = fi * a.hop;
      for (int j = tid; j < W; j += 256) {
        sre[j] = a.pcm[s + fft_bitrev(j, logN)];
        sim[j] = 0.0;
      }
      lds_fft_256(sre, sim, W, logN, a.tw);
      for (int i = tid; i < K; i += 256) M[i] = sqrt(sre[i] * sre[i] + sim[i] * sim[i]);
    } else {
      for (int i = tid; i < K; i += 256) M[i] = a.mag[fi * K + i];
    }
  }
  __syncthreads();

  // ---- 1. analyzeHarmonicStructure :341-365 -> hn / hf / hi / ha / hd[0, n)
  if (tid < 64) {
    bool keep = false;
    double freq = 0.0, ideal = 0.0, amp = 0.0, dev = 0.0;
    const int h = lane + 1;
    if (valid && h <= a.max_h) {
      ideal = f0 * (double)h;
      if (!(ideal > a.max_freq)) {                                      // the break of :345: h f0 grows with h
        const double eb = ideal * (double)W / (double)sr;               // findHarmonicPeak :378-385
        const double tb = a.tol * ideal * (double)W / (double)sr;
        const int64_t sb = go_int(go_max(0.0, eb - tb));
        const int64_t eb2 = go_int(go_min((double)(K - 1), eb + tb));
        if (sb >= 0) {
          double mx = 0.0;
          int64_t mb = sb;
          for (int64_t i = sb; i <= eb2; ++i) {
            const double m = M[i];
            if (m > mx) { mx = m; mb = i; }
          }
          if (mb > 0 && mb < K - 1 && M[mb] > M[mb - 1] && M[mb] > M[mb + 1]) {
            freq = (double)mb * (double)sr / (double)W;                 // freqBins[maxBin] :211
            amp = mx;
            if (amp > a.strength) {
              dev = (freq - ideal) / ideal;
              keep = fabs(dev) < a.tol;
            }
          }
        }
      }
    }
    const uint64_t b = __ballot(keep);
    const int slot = __popcll(b & below);
    if (keep) { hn[slot] = h; hf[slot] = freq; hi[slot] = ideal; ha[slot] = amp; hd[slot] = dev; }
    if (lane == 0) misc[0] = __popcll(b);
  }
  __syncthreads();
  const int n = misc[0];
  const int status = !valid ? SONAR_INHARM_STATUS_INVALID_F0
                            : n < a.min_h ? SONAR_INHARM_STATUS_INSUFFICIENT : SONAR_INHARM_STATUS_OK;
  const bool ok = status == SONAR_INHARM_STATUS_OK;

  // ---- 2. fitRailsbackCurve's errors :640-654
  const bool rails = ok && a.method == SONAR_INHARM_RAILSBACK && n >= 3;
  if (rails) {                                                          // block-uniform
    double err = __builtin_nan("");
    if (tid < INHARM_GRID) {
      const double B = a.grid[tid];
      err = 0.0;
      for (int i = 0; i < n; ++i) {
        const double diff = hf[i] - stretched((double)hn[i], f0, B);
        err = err + diff * diff;
      }
    }
    E[tid] = err;
    __syncthreads();
  }
  if (tid >= 64) return;

  // ---- 3. the method
  double inh = 0.0, sd = 0.0, conf = 0.0, r2 = 0.0, fit = 0.0, chi2 = 0.0, pval = 0.0, stiff = 0.0;
  double clarity = 0.0, purity = 0.0, coherence = 0.0;
  int ndev = 0, quality = -1;
  bool arrays = false;                                                  // the result carries the harmonic arrays
  if (ok) {
    if (a.method == SONAR_INHARM_RAILSBACK) {
      if (rails) {                                                      // :467-510
        double bv = __builtin_huge_val();
        int bi = kNone;
        for (int t = lane; t < INHARM_GRID; t += 64) {
          const double e = E[t];
          if (e < bv) { bv = e; bi = t; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const double ov = __shfl_xor(bv, off, 64);
          const int oi = __shfl_xor(bi, off, 64);
          if (ov < bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        const double B = bi != kNone ? a.grid[bi] : 0.0;                // bestB := 0.0 when no error is below +Inf
        const double mean_obs = mean_of(hf, n);                         // calculateRSquared :659-680
        double ss_res = 0.0, ss_tot = 0.0;
        for (int i = 0; i < n; ++i) {
          const double pred = stretched((double)hn[i], f0, B), obs = hf[i];
          ss_res = ss_res + (obs - pred) * (obs - pred);
          ss_tot = ss_tot + (obs - mean_obs) * (obs - mean_obs);
        }
        r2 = ss_tot > 0 ? 1.0 - (ss_res / ss_tot) : 0.0;
        if (lane < n) {
          const double ex = stretched((double)hn[lane], f0, B);
          dv[lane] = (hf[lane] - ex) / ex;
        }
        wave_lds_sync();
        ndev = n;
        inh = B;
        sd = sqrt(variance_of(dv, n));
        conf = go_max(0.0, r2);
        fit = r2;
        arrays = true;
      }
    } else if (a.method == SONAR_INHARM_FLETCHER_MUNSON) {              // :513-542
      if (lane < n) dv[lane] = hd[lane] * fm_weight(hf[lane]);
      wave_lds_sync();
      ndev = n;
      inh = mean_of(dv, n);
      sd = sqrt(variance_of(dv, n));
      conf = go_min(1.0, ((double)n / (double)a.max_h) * mean_of(ha, n));   // calculateConfidence :620-630
      arrays = true;
    } else if (a.method == SONAR_INHARM_STATISTICAL) {                  // :576-610
      if (n > 0) {
        bool in = lane < n;
        if (a.robust && n >= 3) {                                       // removeOutliers :735-762
          const double q1 = quantile_of(hd, n, 0.25, lane, sc + 0);
          const double q3 = quantile_of(hd, n, 0.75, lane, sc + 1);
          const double iqr = q3 - q1;
          const double lo = q1 - a.outlier * iqr, up = q3 + a.outlier * iqr;
          in = lane < n && hd[lane] >= lo && hd[lane] <= up;
        }
        const uint64_t b = __ballot(in);
        if (in) dv[__popcll(b & below)] = hd[lane];
        wave_lds_sync();
        const int m = __popcll(b);
        ndev = m;
        const double mean = mean_of(dv, m), var = variance_of(dv, m);
        inh = mean;
        sd = sqrt(var);
        if (m >= 2) {                                                   // calculateStatisticalConfidence :764-791
          const double moe = 2.0 * sqrt(var / (double)m);
          conf = mean != 0 ? go_min(1.0, 1.0 / (1.0 + moe / fabs(mean))) : 0.5;
        }
        pval = 1.0;                                                     // performGoodnessOfFitTest :793-845
        if (m >= 5) {
          const int nb = (int)go_int(go_min(10.0, (double)m / 2.0));
          const double lo = mean - 3.0 * sd, hi2 = mean + 3.0 * sd;
          const double bw = (hi2 - lo) / (double)nb;
          int64_t mybin = -1;
          if (lane < m) mybin = go_int((dv[lane] - lo) / bw);
          for (int i = 0; i < nb; ++i) {
            const int observed = __popcll(__ballot(mybin == i));
            const double center = lo + ((double)i + 0.5) * bw;
            const double z = (center - mean) / sd;
            const double density = exp(-0.5 * z * z) / (sd * sqrt(2.0 * 3.14159265358979323846264338327950288));
            const double expected = density * bw * (double)m;
            if (expected > 0) {
              const double diff = (double)observed - expected;
              chi2 = chi2 + (diff * diff) / expected;
            }
          }
          const double dof = (double)(nb - 3);
          pval = go_max(0.0, go_min(1.0, 1.0 - (chi2 / (dof * 2.0))));
        }
        arrays = true;
      }
    } else if (a.method == SONAR_INHARM_BEAT_PATTERN) {                 // :552-573: no confidence, no arrays
      inh = a.beat[fi];
    } else if (n > 0) {                                                 // SpectralDeviation :419-464
      double num = 0.0, den = 0.0;
      for (int i = 0; i < n; ++i) {
        const double hnum = (double)hn[i];
        const double w = a.weight ? ha[i] : 1.0;
        num = num + w * (hd[i] - 0.0) * hnum * hnum;
        den = den + w * hnum * hnum * hnum * hnum;
      }
      inh = den > 0 ? num / den : 0.0;
      if (lane < n) dv[lane] = hd[lane];
      wave_lds_sync();
      ndev = n;
      sd = sqrt(variance_of(hd, n));
      conf = go_min(1.0, ((double)n / (double)a.max_h) * mean_of(ha, n));
      arrays = true;
    }

    // applyStringModel :860-884, calculateStringModelFit :898-919
    if (a.model == SONAR_INHARM_MODEL_STRING) {
      stiff = inh * a.tension * a.length * a.length;
      fit = 0.0;
      if (n > 0) {
        const double f0m = hi[0] / (double)hn[0];
        double total = 0.0;
        for (int i = 0; i < n; ++i) total = total + fabs(hf[i] - stretched((double)hn[i], f0m, inh));
        fit = exp(-(total / (double)n) / f0m);
      }
    }

    // calculateQualityMetrics :921-1005
    if (n > 0) {
      double mx = 0.0;
      for (int i = 0; i < n; ++i)
        if (ha[i] > mx) mx = ha[i];
      double mn = mx;
      for (int i = 0; i < n; ++i)
        if (ha[i] < mn && ha[i] > 0) mn = ha[i];
      if (mn > 0) clarity = go_min(1.0, (20.0 * log10(mx / mn)) / 60.0);
      double ad = 0.0;
      for (int i = 0; i < n; ++i) ad = ad + fabs(hd[i]);
      ad = ad / (double)n;
      purity = exp(-ad * 20.0);
    }
    if (n >= 2) {
      if (lane >= 1 && lane < n) sp[lane - 1] = hf[lane] - hf[lane - 1];
      wave_lds_sync();
      const double mean = mean_of(sp, n - 1);
      if (mean > 0) coherence = 1.0 / (1.0 + sqrt(variance_of(sp, n - 1)) / mean);
    }

    // assessAnalysisQuality :1103-1137
    double score = 0.0;
    score = score + ((double)n / (double)a.max_h) * 0.3;
    score = score + f0c * 0.3;
    score = score + conf * 0.2;
    score = fit > 0 ? score + fit * 0.2 : score + 0.1;
    quality = score >= 0.8 ? SONAR_INHARM_QUALITY_EXCELLENT
              : score >= 0.6 ? SONAR_INHARM_QUALITY_GOOD
              : score >= 0.4 ? SONAR_INHARM_QUALITY_FAIR
              : score >= 0.2 ? SONAR_INHARM_QUALITY_POOR : SONAR_INHARM_QUALITY_VERY_POOR;
  } else if (!valid) {
    quality = SONAR_INHARM_QUALITY_INVALID_F0;
  }

  // ---- 4. the stores
  if (lane < a.slots) {
    const int64_t oi = fi * a.slots + lane;
    const bool on = arrays && lane < n;
    if (o.h_number) o.h_number[oi] = on ? hn[lane] : -1;
    if (o.h_freq) o.h_freq[oi] = on ? hf[lane] : 0.0;
    if (o.h_ideal) o.h_ideal[oi] = on ? hi[lane] : 0.0;
    if (o.h_amp) o.h_amp[oi] = on ? ha[lane] : 0.0;
    if (o.h_dev) o.h_dev[oi] = arrays && lane < ndev ? dv[lane] : 0.0;
  }
  if (lane == 0) {
    if (o.status) o.status[fi] = status;
    if (o.inh) o.inh[fi] = inh;
    if (o.std_dev) o.std_dev[fi] = sd;
    if (o.conf) o.conf[fi] = conf;
    if (o.f0) o.f0[fi] = f0;
    if (o.f0_conf) o.f0_conf[fi] = f0c;
    if (o.num) o.num[fi] = valid ? n : 0;
    if (o.ndev) o.ndev[fi] = ndev;
    if (o.stiffness) o.stiffness[fi] = stiff;
    if (o.fit) o.fit[fi] = fit;
    if (o.clarity) o.clarity[fi] = clarity;
    if (o.purity) o.purity[fi] = purity;
    if (o.coherence) o.coherence[fi] = coherence;
    if (o.r2) o.r2[fi] = r2;
    if (o.chi2) o.chi2[fi] = chi2;
    if (o.pval) o.pval[fi] = pval;
    if (o.quality) o.quality[fi] = quality;
  }
}

__global__ __launch_bounds__(64) void inharm_beat_tail_kernel(const double* corr, int width, int64_t f0, double* beat) {
  __shared__ int lag[INHARM_MAX_BEAT_WIDTH / 2];                         // strict maxima are 2 entries apart
  __shared__ double dl[INHARM_MAX_BEAT_WIDTH / 2];
  const int lane = threadIdx.x;
  const uint64_t below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  const int64_t f = blockIdx.x;
  const double* row = corr + f * (int64_t)width;
  const int max_lag = (width - 1) / 2;
  double v = 0.0;
  if (width >= 10) {                                                    // :707
    int np = 0;
    for (int b0 = 1; b0 < width - 1; b0 += 64) {
      const int i = b0 + lane;
      bool cand = false;
      if (i < width - 1) {
        const double m = row[i];
        cand = m > row[i - 1] && m > row[i + 1] && m >= 0.1;
      }
      const uint64_t b = __ballot(cand);
      if (cand) lag[np + __popcll(b & below)] = i - max_lag;
      np += __popcll(b);
    }
    wave_lds_sync();
    if (np >= 2) {                                                      // :714
      for (int k = lane; k < np; k += 64) dl[k] = (double)lag[k];
      wave_lds_sync();
      const double mean = mean_of(dl, np);
      if (mean > 0) v = sqrt(variance_of(dl, np)) / mean;               // :725-730
    }
  }
  if (lane == 0) beat[f0 + f] = v * 0.001;                              // :567
}

int launch_inharm(const InharmArgs& a, hipStream_t s) {
  if (a.F < 1) return 0;
  const int W = a.W, K = a.K;
  if (K < 4 || K > INHARM_MAX_K || W != 2 * K || a.F > 2147483647 || a.sr < 1 || a.max_h > INHARM_MAX_HARMONICS ||
      a.slots != (a.max_h > 0 ? a.max_h : 0) || !a.f0 || !a.f0_conf || !a.grid)
    return -1;
  if (a.method != SONAR_INHARM_RAILSBACK && a.method != SONAR_INHARM_FLETCHER_MUNSON &&
      a.method != SONAR_INHARM_SPECTRAL_DEVIATION && a.method != SONAR_INHARM_STATISTICAL &&
      a.method != SONAR_INHARM_BEAT_PATTERN)
    return -1;
  if (a.method == SONAR_INHARM_BEAT_PATTERN && !a.beat) return -1;
  if (a.pcm) {
    if ((W & (W - 1)) || W < 64 || W > 2048 || !a.tw || a.hop < 1 || (a.F - 1) * a.hop + W > a.n) return -1;
    hipLaunchKernelGGL((inharm_kernel<true>), dim3((unsigned)a.F), dim3(256), inharm_lds_bytes(K, true), s, a);
  } else {
    if (!a.mag) return -1;
    hipLaunchKernelGGL((inharm_kernel<false>), dim3((unsigned)a.F), dim3(256), inharm_lds_bytes(K, false), s, a);
  }
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

int launch_inharm_beat_tail(const double* corr, int width, int64_t f0, int64_t nf, double* beat, hipStream_t s) {
  if (nf < 1) return 0;
  if (!corr || !beat || width < 1 || width > INHARM_MAX_BEAT_WIDTH || nf > 2147483647) return -1;
  hipLaunchKernelGGL(inharm_beat_tail_kernel, dim3((unsigned)nf), dim3(64), 0, s, corr, width, f0, beat);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // namespace sonar
