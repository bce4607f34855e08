// hps_kernels.hip -- HarmonicProduct (algorithms/harmonic/harmonic_product.go) per spectrum row,
// float64 like the Go reference: ComputeHPS (:32-58) or ComputeHPSWithInterpolation (:163-191),
// findF0Peak (:127-160), the bin's frequency (:89-90), ComputeHarmonicStrength (:224-247) and
// ComputeHarmonicity (:250-273).
//
// One wave (one block) per row, rows strided over the grid, as hpcp_rows_kernel.  Nothing on the path
// is transcendental: products, comparisons, a two-point interpolation and one quotient per row, and
// every one of them decides an output bit, so this file is built without FMA contraction.
//
//  1. the row's powers p[i] = mag[i] * mag[i] into LDS (8 K bytes), read once, coalesced.
//  2. lane l owns bins l, l + 64, ...: hps = p[i], then harmonic by harmonic one rounding each, the
//     factor gathered from LDS (p[i * h], or the interpolation at float64(i) / float64(h)).  Only the
//     scan range is evaluated unless the HPS rows are an output.
//  3. findF0Peak: each lane keeps its first strict maximum above 0.0; a wave butterfly takes the
//     larger value and, of equal values, the lower bin.  A NaN is never above anything.
//  4. lane h - 1 interpolates the magnitudes at (f0 * h) / freq_res; lane 0 adds the squares in
//     harmonic order and divides by the sum of mag^2 in bin order: its own walk over the LDS row, or
//     the value hps_energy_kernel left (a row per lane, 64 chains per wave).
#include <cstdint>

#include "kernels.h"

namespace sonar {

namespace {

// interpolateSpectrum (:194-209) on K values; index is never NaN here.  rightBin < K always holds
// below K - 1, so the reference's second branch is dead.
template <typename Row>
__device__ inline double interpolate(Row s, int K, double index) {
  if (index < 0.0 || index >= (double)(K - 1)) return 0.0;
  const int l = (int)index;
  const double frac = index - (double)l;
  const double a = s[l], b = s[l + 1];
  return a + frac * (b - a);
}

constexpr int kTileRows = 64, kTileCols = 32;   // hps_energy_kernel: rows per wave, columns per tile

}  // namespace

// LDS: p[K] | strengths[64]
__global__ __launch_bounds__(64) void hps_rows_kernel(HpsArgs a) {
  extern __shared__ double p[];
  const int lane = threadIdx.x;
  const int K = a.K, nh = a.nh;
  double* sq = p + K;
  // ComputeHPS: a harmonic above K downsamples to an empty slice and multiplies nothing (:103-106, :52)
  const int hplain = nh < K ? nh : K;
  const int lo = a.hps ? 0 : a.min_bin, hi = a.hps ? K - 1 : a.max_bin;

  for (int64_t f = blockIdx.x; f < a.F; f += gridDim.x) {
    const double* row = a.mag + f * (int64_t)K;
    for (int i = lane; i < K; i += 64) {
      const double m = row[i];
      p[i] = m * m;
    }
    __syncthreads();
    double bv = 0.0;
    int bb = 0;
    for (int i = lo + lane; i <= hi; i += 64) {
      double v = p[i];
      if (a.interpolated) {
        for (int h = 2; h <= nh; ++h) v = v * interpolate(p, K, __ddiv_rn((double)i, (double)h));
      } else {
        for (int h = 2; h <= hplain; ++h) {
          // i < K / h  <=>  (i + 1) * h <= K.  Past it the factor is 0.0 for this and every later
          // harmonic: x * 0.0 is +0 or NaN, and multiplying that by 0.0 again changes nothing.
          if ((i + 1) * h > K) { v = v * 0.0; break; }
          v = v * p[i * h];
        }
      }
      if (a.hps) a.hps[f * (int64_t)K + i] = v;
      if (i >= a.min_bin && i <= a.max_bin && v > bv) { bv = v; bb = i; }
    }
    for (int off = 32; off > 0; off >>= 1) {
      const double ov = __shfl_xor(bv, off);
      const int ob = __shfl_xor(bb, off);
      if (ov > bv || (ov == bv && ob < bb)) { bv = ov; bb = ob; }
    }
    const double f0 = bb == 0 ? 0.0 : (double)bb * a.freq_res;
    if (lane == 0) {
      a.f0_bin[f] = bb;
      a.f0[f] = f0;
    }
    if (a.confidence || a.strengths) {
      double s = 0.0;
      if (bb > 0 && lane < nh) {   // f0 > 0 (:225)
        const double hb = __ddiv_rn(f0 * (double)(lane + 1), a.freq_res);
        s = hb >= (double)K ? 0.0 : interpolate(row, K, hb);
      }
      if (a.strengths && lane < nh) a.strengths[f * (int64_t)nh + lane] = s;
      if (a.confidence) {
        sq[lane] = s;
        __syncthreads();
        if (lane == 0) {
          double conf = 0.0;
          if (bb > 0 && nh > 0) {
            double he = 0.0, te = 0.0;
            for (int h = 0; h < nh; ++h) he = he + sq[h] * sq[h];
            if (a.total) te = a.total[f];
            else
              for (int i = 0; i < K; ++i) te = te + p[i];
            conf = te == 0.0 ? 0.0 : __ddiv_rn(he, te);
          }
          a.confidence[f] = conf;
        }
      }
    }
    __syncthreads();   // the next row rewrites the powers
  }
}

// A wave owns 64 rows; tiles of 64 rows x 32 columns go through LDS and lane r adds row r's squares
// in bin order.  A half wave loads 32 consecutive doubles of one row (256 contiguous bytes), the two
// halves take neighbouring rows, 32 loads per lane are in flight, and the values are squared on the
// way in.  The tile is padded to 33 columns: lane r reads column c at 33 r + c, 32 distinct 8-byte
// banks per half wave.  There is no prefetch across tiles: other waves of the CU fill the chain time.
__global__ __launch_bounds__(64) void hps_energy_kernel(const double* mag, int64_t F, int K, double* total) {
  __shared__ double tile[kTileRows][kTileCols + 1];
  const int lane = threadIdx.x;
  const int half = lane >> 5, col = lane & 31;
  for (int64_t r0 = (int64_t)blockIdx.x * kTileRows; r0 < F; r0 += (int64_t)gridDim.x * kTileRows) {
    const int rows = F - r0 < kTileRows ? (int)(F - r0) : kTileRows;
    double t = 0.0;
    for (int c0 = 0; c0 < K; c0 += kTileCols) {
      const double* src = mag + (r0 + half) * (int64_t)K + c0 + col;
      const bool in_row = c0 + col < K;
      double v[kTileRows / 2];
#pragma unroll
      for (int j = 0; j < kTileRows / 2; ++j) v[j] = (in_row && 2 * j + half < rows) ? src[(int64_t)(2 * j) * K] : 0.0;
      __syncthreads();   // the previous tile's chains are done
#pragma unroll
      for (int j = 0; j < kTileRows / 2; ++j) tile[2 * j + half][col] = v[j] * v[j];
      __syncthreads();
      const int w = K - c0 < kTileCols ? K - c0 : kTileCols;
      for (int c = 0; c < w; ++c) t = t + tile[lane][c];
    }
    if (lane < rows) total[r0 + lane] = t;
  }
}

int launch_hps(const HpsArgs& a, hipStream_t s) {
  if (a.F < 1) return 0;
  if (a.K < 1 || a.K > HPS_MAX_K || a.nh > HPS_MAX_HARMONICS || a.min_bin < 0 || a.max_bin > a.K - 1) return -1;
  if (!a.f0_bin || !a.f0 || ((a.confidence || a.strengths) && a.nh < 0)) return -1;
  const size_t lds = (size_t)a.K * 8 + 64 * 8;
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute((const void*)hps_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  const unsigned grid = (unsigned)(a.F < (int64_t)(1 << 20) ? a.F : (int64_t)(1 << 20));
  hipLaunchKernelGGL(hps_rows_kernel, dim3(grid), dim3(64), lds, s, a);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

int launch_hps_energy(const double* mag, int64_t F, int K, double* total, hipStream_t s) {
  if (F < 1) return 0;
  if (K < 1 || !mag || !total) return -1;
  const int64_t blocks = (F + kTileRows - 1) / kTileRows;
  const unsigned grid = (unsigned)(blocks < (int64_t)(1 << 20) ? blocks : (int64_t)(1 << 20));
  hipLaunchKernelGGL(hps_energy_kernel, dim3(grid), dim3(64), 0, s, mag, F, K, total);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // namespace sonar
