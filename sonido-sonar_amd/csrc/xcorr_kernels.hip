// xcorr_kernels.hip -- the configurations of CrossCorrelation.Compute (algorithms/stats/correlation.go)
// beyond NormalizedCrossCorrelation / TimeDomain (ncc_kernels.hip), float64 like the Go reference:
//
//  xcorr_pearson_kernel   pearsonCorrelation per lag (:314-370): the overlap means in one walk, the
//                         centred sums in a second one, the clamp to [-1, 1] (NaN passes)
//  xcorr_center_kernel    subtractMean (:504-523) of zeroNormalizedCrossCorrelation (:412-418), once
//                         per call (Go repeats it per lag with the same result)
//  xcorr_fft_*_kernel     computeFFT (:231-291) over the in-tree recursive radix-2 fft / ifft
//                         (:726-774) as an iterative decimation-in-time transform
//
// Every sum runs in Go's index order with unfused multiplies and adds (__d*_rn), so the correlations
// are bit-identical to a sequential float64 evaluation.  The z-score of both inputs (normalize
// :464-501) and the NCC lag sums are ncc_kernels.hip's (launch_ncc_zscore, launch_ncc_lags).
#include <cstdint>

#include "kernels.h"

#pragma clang fp contract(off)

namespace sonar {

// ------------------------------------------------------------- Pearson ----
// One lag per thread, 256 consecutive lags per block, both inputs staged in LDS in tiles of 1,024
// samples (+ the 255 the block's window origins spread over), as ncc_lag_kernel.  Two walks over
// the overlap: mean1 / mean2 (:328-344), then numerator / sum1sq / sum2sq of the differences (:349-361).
constexpr int kXcTile = 1024;
__global__ __launch_bounds__(256) void xcorr_pearson_kernel(const double* x, int64_t na, const double* y, int64_t nb,
                                                            int64_t L, double* corr) {
  SONAR_FEAT_PRIO();
  __shared__ double xs[kXcTile + 256], ys[kXcTile + 256];
  __shared__ int64_t ovmax_s;
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
  if (!active || ov <= 1) ov = 0;                  // overlapLen <= 1 -> 0.0 (:320-322): nothing to walk
  const int64_t lastlag = (idx0 + 255 < nl ? idx0 + 255 : nl - 1) - L;
  const int64_t x0 = lastlag < 0 ? -lastlag : 0;   // min s1 over the block's lags
  const int64_t y0 = idx0 - L > 0 ? idx0 - L : 0;   // min s2
  if (threadIdx.x == 0) ovmax_s = 0;
  __syncthreads();
  atomicMax(reinterpret_cast<unsigned long long*>(&ovmax_s), (unsigned long long)ov);
  __syncthreads();
  const int64_t ovmax = ovmax_s;
  const int ox = active ? (int)(s1 - x0) : 0, oy = active ? (int)(s2 - y0) : 0;   // 0..255
  double m1 = 0.0, m2 = 0.0, num = 0.0, q1 = 0.0, q2 = 0.0;
  for (int walk = 0; walk < 2; ++walk) {
    for (int64_t k0 = 0; k0 < ovmax; k0 += kXcTile) {
      for (int j = threadIdx.x; j < kXcTile + 256; j += 256) {
        const int64_t gx = x0 + k0 + j, gy = y0 + k0 + j;
        xs[j] = gx < na ? x[gx] : 0.0;
        ys[j] = gy < nb ? y[gy] : 0.0;
      }
      __syncthreads();
      int kend = ov - k0 < kXcTile ? (int)(ov - k0) : kXcTile;
      if (kend < 0) kend = 0;
      const double* px = xs + ox;
      const double* py = ys + oy;
      if (walk == 0) {
        for (int k = 0; k < kend; k++) {
          m1 = __dadd_rn(m1, px[k]);
          m2 = __dadd_rn(m2, py[k]);
        }
      } else {
        for (int k = 0; k < kend; k++) {
          const double d1 = __dsub_rn(px[k], m1), d2 = __dsub_rn(py[k], m2);
          num = __dadd_rn(num, __dmul_rn(d1, d2));
          q1 = __dadd_rn(q1, __dmul_rn(d1, d1));
          q2 = __dadd_rn(q2, __dmul_rn(d2, d2));
        }
      }
      __syncthreads();
    }
    if (walk == 0 && ov > 0) {
      m1 = __ddiv_rn(m1, (double)ov);                // count == overlapLen: every index is in range
      m2 = __ddiv_rn(m2, (double)ov);
    }
  }
  if (!active) return;
  double c = 0.0;
  if (ov > 0) {
    const double dn = sqrt(__dmul_rn(q1, q2));
    if (!(dn < 1e-10)) {                             // a NaN denominator goes on, as in Go
      c = __ddiv_rn(num, dn);
      if (c > 1.0) c = 1.0;                          // clampCorrelation :695-702 (NaN passes)
      else if (c < -1.0) c = -1.0;
    }
  }
  corr[idx] = c;
}

int launch_xcorr_pearson(const double* xa, int64_t na, const double* xb, int64_t nb, int64_t L, double* corr,
                         hipStream_t s) {
  const int64_t nl = 2 * L + 1;
  hipLaunchKernelGGL(xcorr_pearson_kernel, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, s, xa, na, xb, nb, L, corr);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

// ---------------------------------------------------------- subtractMean ----
__global__ void xcorr_center_kernel(double* xa, int64_t na, double* xb, int64_t nb, const double* stats) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < na) xa[i] = __dsub_rn(xa[i], stats[0]);
  if (i < nb) xb[i] = __dsub_rn(xb[i], stats[2]);
}

int launch_xcorr_center(double* xa, int64_t na, double* xb, int64_t nb, const double* stats, hipStream_t s) {
  const int64_t nmax = na > nb ? na : nb;
  hipLaunchKernelGGL(xcorr_center_kernel, dim3((unsigned)((nmax + 255) / 256)), dim3(256), 0, s, xa, na, xb, nb, stats);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

// ------------------------------------------------------------------ FFT ----
// Go's fft (:726-754) splits into even and odd samples, transforms both and combines
//   t = exp(-2 pi i k / n) * odd[k];  out[k] = even[k] + t;  out[k + n/2] = even[k] - t
// with the complex product (c*or - s*oi, c*oi + s*or).  Unrolled, that is the iterative
// decimation-in-time transform over a bit-reversed load: level s (n = 2^s) combines the finished
// halves of every group of n consecutive points with the same products and sums, so the bits are the
// recursion's.  The level-n twiddle of index k is entry k * (N / n) of the top-level table (the angle
// scales by a power of two, so -2 pi k / n has the same bits either way): one table of N / 2
// (cos, sin) pairs, built by the host with libm, serves every level.
//
// The low levels of XCORR_FFT_TILE consecutive points run in LDS (re and im planes, 64 KB, 256
// threads, 8 butterflies per thread and level); the levels above go through global memory, up to four
// per pass with 16 points per thread in registers.
__device__ __forceinline__ void butterfly(double c, double s, double& er, double& ei, double& odr, double& odi) {
  const double tr = __dsub_rn(__dmul_rn(c, odr), __dmul_rn(s, odi));
  const double ti = __dadd_rn(__dmul_rn(c, odi), __dmul_rn(s, odr));
  const double ar = er, ai = ei;
  er = __dadd_rn(ar, tr); ei = __dadd_rn(ai, ti);
  odr = __dsub_rn(ar, tr); odi = __dsub_rn(ai, ti);
}

// PRODUCT false: blockIdx.y picks (x0, n0) -> out0 or (x1, n1) -> out1, real samples zero-padded to N.
// PRODUCT true: the input point is conj(A * conj(B)) (the cross-power spectrum :261-264 with ifft's
// leading conjugate :761-763 folded in), into out0.
template <bool PRODUCT>
__global__ __launch_bounds__(256) void xcorr_fft_tile_kernel(const double* x0, int64_t n0, const double* x1, int64_t n1,
                                                             const double2* A, const double2* B, int64_t N, int logN,
                                                             int logT, const double2* tw, double2* out0, double2* out1) {
  __shared__ double sre[XCORR_FFT_TILE], sim[XCORR_FFT_TILE];
  const int Tn = 1 << logT;
  const int hb = logN - logT;                        // bits of the tile index
  const int64_t b = blockIdx.x;
  const int64_t brev = hb ? (int64_t)(__brev((unsigned)b) >> (32 - hb)) : 0;
  const double* x = blockIdx.y ? x1 : x0;
  const int64_t n = blockIdx.y ? n1 : n0;
  double2* out = blockIdx.y ? out1 : out0;
  for (int j = threadIdx.x; j < Tn; j += 256) {
    const unsigned jr = logT ? __brev((unsigned)j) >> (32 - logT) : 0u;
    const int64_t src = ((int64_t)jr << hb) + brev;  // bit reversal of b * Tn + j over logN bits
    if constexpr (PRODUCT) {
      const double2 u = A[src], v = B[src];
      const double c = v.x, d = -v.y;
      sre[j] = __dsub_rn(__dmul_rn(u.x, c), __dmul_rn(u.y, d));
      sim[j] = -__dadd_rn(__dmul_rn(u.x, d), __dmul_rn(u.y, c));
    } else {
      sre[j] = src < n ? x[src] : 0.0;
      sim[j] = 0.0;
    }
  }
  for (int s = 1; s <= logT; ++s) {
    __syncthreads();
    const int h = 1 << (s - 1);
    const int64_t stride = N >> s;
    for (int k = threadIdx.x; k < Tn / 2; k += 256) {
      const int i = k & (h - 1);
      const int p = ((k >> (s - 1)) << s) + i, q = p + h;
      const double2 w = tw[(int64_t)i * stride];
      double er = sre[p], ei = sim[p], odr = sre[q], odi = sim[q];
      butterfly(w.x, w.y, er, ei, odr, odi);
      sre[p] = er; sim[p] = ei; sre[q] = odr; sim[q] = odi;
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < Tn; j += 256) out[b * Tn + j] = make_double2(sre[j], sim[j]);
}

// levels s0 + 1 .. s0 + K in place: thread t owns the 2^K points base + r * 2^s0
template <int K>
__global__ __launch_bounds__(256) void xcorr_fft_pass_kernel(double2* X0, double2* X1, int64_t N, int s0,
                                                             const double2* tw) {
  double2* X = blockIdx.y ? X1 : X0;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (N >> K)) return;
  const int64_t h0 = int64_t(1) << s0;
  const int64_t i = t & (h0 - 1);
  const int64_t base = ((t >> s0) << (s0 + K)) + i;
  constexpr int R = 1 << K;
  double2 v[R];
#pragma unroll
  for (int r = 0; r < R; ++r) v[r] = X[base + r * h0];
#pragma unroll
  for (int l = 0; l < K; ++l) {
    const int64_t stride = N >> (s0 + l + 1);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (r & (1 << l)) continue;
      const int64_t il = i + (int64_t)(r & ((1 << l) - 1)) * h0;
      const double2 w = tw[il * stride];
      butterfly(w.x, w.y, v[r].x, v[r].y, v[r | (1 << l)].x, v[r | (1 << l)].y);
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) X[base + r * h0] = v[r];
}

// correlations[i] = real(conj(y[idx]) / N) with idx = lag or N + lag (:275-288, 769-771)
__global__ void xcorr_fft_extract_kernel(const double2* C, int64_t N, int64_t L, double* corr) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k > 2 * L) return;
  const int64_t lag = k - L;
  corr[k] = __ddiv_rn(C[lag >= 0 ? lag : N + lag].x, (double)N);
}

static void fft_passes(double2* X0, double2* X1, int ny, int64_t N, int logN, int logT, const double2* tw,
                       hipStream_t s) {
  for (int s0 = logT; s0 < logN;) {
    const int K = logN - s0 < 4 ? logN - s0 : 4;
    const dim3 grid((unsigned)(((N >> K) + 255) / 256), (unsigned)ny);
    switch (K) {
      case 1: hipLaunchKernelGGL(xcorr_fft_pass_kernel<1>, grid, dim3(256), 0, s, X0, X1, N, s0, tw); break;
      case 2: hipLaunchKernelGGL(xcorr_fft_pass_kernel<2>, grid, dim3(256), 0, s, X0, X1, N, s0, tw); break;
      case 3: hipLaunchKernelGGL(xcorr_fft_pass_kernel<3>, grid, dim3(256), 0, s, X0, X1, N, s0, tw); break;
      default: hipLaunchKernelGGL(xcorr_fft_pass_kernel<4>, grid, dim3(256), 0, s, X0, X1, N, s0, tw); break;
    }
    s0 += K;
  }
}

int launch_xcorr_fft(const double* xa, int64_t na, const double* xb, int64_t nb, int64_t N, const double2* tw,
                     double2* A, double2* B, double2* C, int64_t L, double* corr, hipStream_t s) {
  if (N < 1 || N > XCORR_FFT_MAX_N || (N & (N - 1)) || na + nb - 1 > N || L >= N) return -1;
  int logN = 0;
  while ((int64_t(1) << logN) < N) ++logN;
  const int logT = logN < 12 ? logN : 12;
  static_assert(XCORR_FFT_TILE == 1 << 12, "logT");
  const bool same = xb == xa && nb == na;            // two transforms of the same bits give the same bits
  const int ny = same ? 1 : 2;
  if (same) B = A;
  const unsigned tiles = (unsigned)(N >> logT);
  const double2* none = nullptr;
  hipLaunchKernelGGL((xcorr_fft_tile_kernel<false>), dim3(tiles, ny), dim3(256), 0, s, xa, na, xb, nb, none, none, N, logN,
                     logT, tw, A, B);
  fft_passes(A, B, ny, N, logN, logT, tw, s);
  hipLaunchKernelGGL((xcorr_fft_tile_kernel<true>), dim3(tiles, 1), dim3(256), 0, s, nullptr, 0, nullptr, 0, A, B, N, logN,
                     logT, tw, C, C);
  fft_passes(C, C, 1, N, logN, logT, tw, s);
  const int64_t nl = 2 * L + 1;
  hipLaunchKernelGGL(xcorr_fft_extract_kernel, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, s, C, N, L, corr);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // namespace sonar
