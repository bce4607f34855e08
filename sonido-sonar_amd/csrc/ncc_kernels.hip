// ncc_kernels.hip -- path B of the hot path on gfx950: normalized cross-correlation, float64
// like the Go reference (the DTW of the same path is dtw_kernels.hip).
//
//  NCC  CrossCorrelation.Compute with NormalizedCrossCorrelation / TimeDomain
//       (algorithms/stats/correlation.go:131-228, 373-409, 452-501) as configured by
//       NewAlignmentAnalyzer (algorithms/stats/alignment.go:60-81).
//       One thread per lag; every sum runs in Go's index order with unfused
//       mul/add (__d*_rn), so correlations -- and therefore the peak lag -- are
//       bit-identical to a sequential float64 evaluation.
//  perturb_kernel / first_column_kernel: the alignment analyzer's addNoise and flatten2DFeatures.
#include <algorithm>
#include <cstdint>

#include "kernels.h"
#include "wave.h"

#pragma clang fp contract(off)

namespace sonar {

// ---------------------------------------------------------------- NCC ----
// stats[0..3] = mean_a, sd_a, mean_b, sd_b  (correlation.go:464-501, sequential sums)
// Global z-score statistics (normalize :464-501): mean and population std of each input, every
// sum sequential in Go's index order (bit-exact).  One wave per input: the wave loads 64
// consecutive values per step (coalesced, the next step in flight), and every lane runs the
// same sequential add chain over them through v_readlane broadcasts (readlane_f64, wave.h).
// BJ (this and the two NCC kernels below): one pair per blockIdx.y, its arguments from jobs[]
template <bool BJ = false>
__global__ __launch_bounds__(64) void ncc_stats_kernel(const double* a, int64_t na, const double* b, int64_t nb,
                                                       double* stats, const NccJob* jobs) {
  SONAR_FEAT_PRIO();
  if constexpr (BJ) {
    const NccJob j = load_job(jobs + blockIdx.y);
    a = j.a; na = j.na; b = j.b; nb = j.nb; stats = j.stats;
  }
  const int w = blockIdx.x;
  const int lane = threadIdx.x;
  const double* s = w ? b : a;
  const int64_t n = w ? nb : na;
  // full 64-value steps are unrolled (constant readlane indices, broadcasts issued ahead of the
  // add chain); the tail runs the same chain with a runtime index
  double mean = 0.0;
  {
    double cur = lane < n ? s[lane] : 0.0;
    int64_t i = 0;
    for (; i + 64 <= n; i += 64) {
      const double nxt = i + 64 + lane < n ? s[i + 64 + lane] : 0.0;
#pragma unroll
      for (int j = 0; j < 64; j++) mean = __dadd_rn(mean, readlane_f64(cur, j));
      cur = nxt;
    }
    for (int j = 0; j < (int)(n - i); j++) mean = __dadd_rn(mean, readlane_f64(cur, j));
  }
  mean = __ddiv_rn(mean, (double)n);
  double var = 0.0;
  {
    double cur = lane < n ? __dsub_rn(s[lane], mean) : 0.0;
    int64_t i = 0;
    for (; i + 64 <= n; i += 64) {
      const double nxt = i + 64 + lane < n ? __dsub_rn(s[i + 64 + lane], mean) : 0.0;
#pragma unroll
      for (int j = 0; j < 64; j++) {
        const double d = readlane_f64(cur, j);
        var = __dadd_rn(var, __dmul_rn(d, d));
      }
      cur = nxt;
    }
    for (int j = 0; j < (int)(n - i); j++) {
      const double d = readlane_f64(cur, j);
      var = __dadd_rn(var, __dmul_rn(d, d));
    }
  }
  var = __ddiv_rn(var, (double)n);
  if (lane == 0) {
    stats[2 * w] = mean;
    stats[2 * w + 1] = sqrt(var);
  }
}

template <bool BJ = false>
__global__ void ncc_norm_kernel(const double* a, int64_t na, const double* b, int64_t nb, const double* stats,
                                double* xa, double* xb, const NccJob* jobs) {
  SONAR_FEAT_PRIO();
  if constexpr (BJ) {
    const NccJob j = load_job(jobs + blockIdx.y);
    a = j.a; na = j.na; b = j.b; nb = j.nb; stats = j.stats; xa = j.xa; xb = j.xb;
  }
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < na) {
    const double d = __dsub_rn(a[i], stats[0]);
    xa[i] = stats[1] < 1e-10 ? d : __ddiv_rn(d, stats[1]);
  }
  if (i < nb) {
    const double d = __dsub_rn(b[i], stats[2]);
    xb[i] = stats[3] < 1e-10 ? d : __ddiv_rn(d, stats[3]);
  }
}

// one lag per thread (normalizedCrossCorrelation, correlation.go:373-409), sums in Go's index
// order (bit-exact).  A block owns 256 consecutive lags; their overlap windows start within 255
// samples of each other (s1 = max(0, -lag), s2 = max(0, lag)), so each k-tile of both inputs is
// staged once in LDS (coalesced) and every thread walks its own offsets there.
constexpr int kNccTile = 1024;
template <bool BJ = false>
__global__ __launch_bounds__(256) void ncc_lag_kernel(const double* x, int64_t na, const double* y, int64_t nb,
                                                      int64_t L, double* corr, const NccJob* jobs) {
  SONAR_FEAT_PRIO();
  __shared__ double xs[kNccTile + 256], ys[kNccTile + 256];
  __shared__ int64_t ovmax_s;
  if constexpr (BJ) {
    const NccJob j = load_job(jobs + blockIdx.y);
    x = j.xa; na = j.na; y = j.xb; nb = j.nb; L = j.L; corr = j.corr;
  }
  const int64_t nl = 2 * L + 1;
  const int64_t idx0 = (int64_t)blockIdx.x * 256;
  if (idx0 >= nl) return;
  const int64_t idx = idx0 + threadIdx.x;
  const bool active = idx < nl;
  const int64_t lag = idx - L;
  int64_t s1 = 0, e1 = 0, s2 = 0, e2 = 0;         // calculateOverlapRegion :421-449
  if (lag >= 0) { s1 = 0; e1 = na; s2 = lag; e2 = nb; if (e1 > nb - lag) e1 = nb - lag; if (e2 > nb) e2 = nb; }
  else { s1 = -lag; e1 = na; s2 = 0; e2 = nb; if (e1 > na) e1 = na; if (e2 > na + lag) e2 = na + lag; }
  int64_t ov = (e1 - s1) < (e2 - s2) ? (e1 - s1) : (e2 - s2);
  if (!active || ov < 0) ov = 0;
  // window origins over the block's lags [idx0 - L, last - L]
  const int64_t lastlag = (idx0 + 255 < nl ? idx0 + 255 : nl - 1) - L;
  const int64_t x0 = lastlag < 0 ? -lastlag : 0;   // min s1
  const int64_t y0 = idx0 - L > 0 ? idx0 - L : 0;   // min s2
  if (threadIdx.x == 0) ovmax_s = 0;
  __syncthreads();
  atomicMax(reinterpret_cast<unsigned long long*>(&ovmax_s), (unsigned long long)ov);
  __syncthreads();
  const int64_t ovmax = ovmax_s;
  const int ox = (int)(s1 - x0), oy = (int)(s2 - y0);   // 0..255 for active lags
  double sm = 0.0, q1 = 0.0, q2 = 0.0;
  for (int64_t k0 = 0; k0 < ovmax; k0 += kNccTile) {
    for (int j = threadIdx.x; j < kNccTile + 256; j += 256) {
      const int64_t gx = x0 + k0 + j, gy = y0 + k0 + j;
      xs[j] = gx < na ? x[gx] : 0.0;
      ys[j] = gy < nb ? y[gy] : 0.0;
    }
    __syncthreads();
    int kend = ov - k0 < kNccTile ? (int)(ov - k0) : kNccTile;
    if (kend < 0) kend = 0;
    const double* px = xs + ox;
    const double* py = ys + oy;
    int k = 0;
    for (; k + 4 <= kend; k += 4) {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const double c1 = px[k + j], c2 = py[k + j];
        sm = __dadd_rn(sm, __dmul_rn(c1, c2));
        q1 = __dadd_rn(q1, __dmul_rn(c1, c1));
        q2 = __dadd_rn(q2, __dmul_rn(c2, c2));
      }
    }
    for (; k < kend; k++) {
      const double c1 = px[k], c2 = py[k];
      sm = __dadd_rn(sm, __dmul_rn(c1, c2));
      q1 = __dadd_rn(q1, __dmul_rn(c1, c1));
      q2 = __dadd_rn(q2, __dmul_rn(c2, c2));
    }
    __syncthreads();
  }
  if (!active) return;
  double c = 0.0;
  if (ov > 0) {
    const double dn = sqrt(__dmul_rn(q1, q2));
    c = dn < 1e-10 ? 0.0 : __ddiv_rn(sm, dn);
  }
  corr[idx] = c;
}

int launch_ncc(const double* a, int64_t na, const double* b, int64_t nb, int64_t L, double* xa, double* xb,
               double* stats, double* corr, hipStream_t s) {
  const NccJob* none = nullptr;
  hipLaunchKernelGGL((ncc_stats_kernel<false>), dim3(2), dim3(64), 0, s, a, na, b, nb, stats, none);
  const int64_t nmax = na > nb ? na : nb;
  hipLaunchKernelGGL((ncc_norm_kernel<false>), dim3((unsigned)((nmax + 255) / 256)), dim3(256), 0, s, a, na, b, nb, stats, xa,
                     xb, none);
  const int64_t nl = 2 * L + 1;
  hipLaunchKernelGGL((ncc_lag_kernel<false>), dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, s, xa, na, xb, nb, L, corr,
                     none);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

// launch_ncc's kernels one by one (sonar_xcorr_params: the same z-score under every type and method)
int launch_ncc_stats(const double* a, int64_t na, const double* b, int64_t nb, double* stats, hipStream_t s) {
  const NccJob* none = nullptr;
  hipLaunchKernelGGL((ncc_stats_kernel<false>), dim3(2), dim3(64), 0, s, a, na, b, nb, stats, none);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

int launch_ncc_zscore(const double* a, int64_t na, const double* b, int64_t nb, double* xa, double* xb, double* stats,
                      hipStream_t s) {
  const NccJob* none = nullptr;
  hipLaunchKernelGGL((ncc_stats_kernel<false>), dim3(2), dim3(64), 0, s, a, na, b, nb, stats, none);
  const int64_t nmax = na > nb ? na : nb;
  hipLaunchKernelGGL((ncc_norm_kernel<false>), dim3((unsigned)((nmax + 255) / 256)), dim3(256), 0, s, a, na, b, nb, stats, xa,
                     xb, none);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

int launch_ncc_lags(const double* xa, int64_t na, const double* xb, int64_t nb, int64_t L, double* corr, hipStream_t s) {
  const NccJob* none = nullptr;
  const int64_t nl = 2 * L + 1;
  hipLaunchKernelGGL((ncc_lag_kernel<false>), dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, s, xa, na, xb, nb, L, corr,
                     none);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

// launch_ncc over many pairs in three launches (blockIdx.y = pair); the same kernels, arithmetic
// and order per pair, so the same bits
int launch_ncc_batch(const NccJob* hjobs, const NccJob* djobs, int nj, hipStream_t s) {
  if (nj <= 0) return 0;
  if (nj > 65535) return -1;
  int64_t nmax = 1, nlmax = 1;
  for (int k = 0; k < nj; ++k) {
    nmax = std::max(nmax, std::max(hjobs[k].na, hjobs[k].nb));
    nlmax = std::max(nlmax, 2 * hjobs[k].L + 1);
  }
  hipLaunchKernelGGL((ncc_stats_kernel<true>), dim3(2, (unsigned)nj), dim3(64), 0, s, nullptr, 0, nullptr, 0, nullptr,
                     djobs);
  hipLaunchKernelGGL((ncc_norm_kernel<true>), dim3((unsigned)((nmax + 255) / 256), (unsigned)nj), dim3(256), 0, s,
                     nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, djobs);
  hipLaunchKernelGGL((ncc_lag_kernel<true>), dim3((unsigned)((nlmax + 255) / 256), (unsigned)nj), dim3(256), 0, s,
                     nullptr, 0, nullptr, 0, 0, nullptr, djobs);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

// AlignmentAnalyzer.addNoise (alignment.go:737-749): out[i][j] = q + (sin(i*j+i+j) * level) * q
__global__ void perturb_kernel(const double* q, int64_t nq, int dim, double level, double* out) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= nq * dim) return;
  const int64_t i = idx / dim, j = idx - i * dim;
  const double v = q[idx];
  out[idx] = __dadd_rn(v, __dmul_rn(__dmul_rn(sin((double)(i * j + i + j)), level), v));
}
// flatten2DFeatures (:363-378): the first component of every frame
__global__ void first_column_kernel(const double* x, int64_t n, int dim, double* out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = x[i * dim];
}
int launch_perturb(const double* q, int64_t nq, int dim, double level, double* out, hipStream_t s) {
  const int64_t n = nq * dim;
  if (n <= 0) return 0;
  hipLaunchKernelGGL(perturb_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, q, nq, dim, level, out);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}
int launch_first_column(const double* x, int64_t n, int dim, double* out, hipStream_t s) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(first_column_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, n, dim, out);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // namespace sonar
