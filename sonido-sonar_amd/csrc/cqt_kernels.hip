// cqt_kernels.hip -- ChromaCQT.ComputeChroma (algorithms/chroma/chroma_cqt.go), float64 like the Go
// reference:
//
//  cqt_bank_kernel   computeCQTSpectrogram (:168-210).  The reference's kernels have no phase
//                    (complexToReal takes cmplx.Abs of every tap, :306-312), so the sum over all FFT
//                    bins of frameFFT * conj(K_k) (:198-200) is N times the real dot product of the
//                    frame's first L_k samples with g_k: a decimating FIR bank,
//                    out[f][k] = |N * sum_t x[f hop + t] g_k[t]|, a Toeplitz GEMM.
//  cqt_fold_kernel   convertCQTToChroma + normalizeChromaFrame (:213-268)
//
// No decision hangs on a rounding inside the tap sums (the only ones are the 1e-10 test of the fold and
// the bin map, which the host computes), so this file is built with FMA contraction on; the fold's
// sums are written unfused all the same, in Go's order.
#include <cstdint>

#include "kernels.h"

namespace sonar {

// One wave per CQT_FT consecutive frames x one group of CQT_BK consecutive bins; the taps run across
// the lanes (lane l takes t = l, l + 64, ...), so every load of x and of g is 64 consecutive doubles,
// and each lane keeps a CQT_FT x CQT_BK block of partial sums: 64 FMAs per 16 doubles loaded.  The
// four waves of a block take four consecutive frame tiles of the same group, so they read the same
// taps at about the same time.  blockIdx.y is the group: the long groups are dispatched first.
// Nothing is shared between lanes before the end, so the operands come straight from global memory
// (the taps from L2, the PCM tile re-read hop by hop from L1 / L2); LDS only carries the reduction.
constexpr int kCqtWaves = 4;
constexpr int kCqtRedRows = 16;    // partial sums reduced per pass
constexpr int kCqtRedPitch = 65;   // doubles: lane (i, q) reads row i at q * 16 + j -> 32 banks apart

__global__ __launch_bounds__(64 * kCqtWaves) void cqt_bank_kernel(CqtArgs a) {
  __shared__ double red[kCqtWaves][kCqtRedRows][kCqtRedPitch];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int grp = blockIdx.y;
  const int64_t f0 = ((int64_t)blockIdx.x * kCqtWaves + w) * CQT_FT;
  const int lpad = a.lpad[grp];
  const double* g = a.tab + a.goff[grp];
  const bool live = f0 < a.F;            // a wave past the last frame only keeps the barriers company
  // every sample of the tile's CQT_FT frames inside the signal: no bound checks in the loop
  const bool fast = live && a.hop > 0 && f0 + CQT_FT - 1 < a.F && (f0 + CQT_FT - 1) * a.hop + lpad <= a.n;
  double acc[CQT_FT][CQT_BK];
#pragma unroll
  for (int i = 0; i < CQT_FT; ++i)
#pragma unroll
    for (int j = 0; j < CQT_BK; ++j) acc[i][j] = 0.0;
  if (fast) {
    // The operands of a step are loaded two steps ahead (three sets in registers), so a step's 64
    // FMAs run while the next two steps' 32 loads are in flight; past the lane's last tap the
    // prefetch re-reads that tap and is dropped.
    const double* xp = a.x + f0 * a.hop;
    const int64_t hop = a.hop;
    struct Ops { double x[CQT_FT], g[CQT_BK]; };
    auto load = [&](int t) {
      Ops o;
#pragma unroll
      for (int i = 0; i < CQT_FT; ++i) o.x[i] = xp[(int64_t)i * hop + t];
#pragma unroll
      for (int j = 0; j < CQT_BK; ++j) o.g[j] = g[(int64_t)j * lpad + t];
      return o;
    };
    const int tl = lpad - 64 + lane;       // the lane's last tap
    Ops o0 = load(lane), o1 = load(lane + 64 < tl ? lane + 64 : tl);
#pragma unroll 3
    for (int t = lane; t < lpad; t += 64) {
      const Ops o2 = load(t + 128 < tl ? t + 128 : tl);
#pragma unroll
      for (int i = 0; i < CQT_FT; ++i)
#pragma unroll
        for (int j = 0; j < CQT_BK; ++j) acc[i][j] = fma(o0.x[i], o0.g[j], acc[i][j]);
      o0 = o1;
      o1 = o2;
    }
  } else if (live) {
    // the signal's end (zero padding, :183-188), the last frames, a single frame with any hop
    int64_t start[CQT_FT];
#pragma unroll
    for (int i = 0; i < CQT_FT; ++i) start[i] = f0 + i < a.F ? (f0 + i == 0 ? 0 : (f0 + i) * a.hop) : a.n;
    for (int t = lane; t < lpad; t += 64) {
      double xv[CQT_FT], gv[CQT_BK];
#pragma unroll
      for (int i = 0; i < CQT_FT; ++i) xv[i] = start[i] < a.n - t ? a.x[start[i] + t] : 0.0;
#pragma unroll
      for (int j = 0; j < CQT_BK; ++j) gv[j] = g[(int64_t)j * lpad + t];
#pragma unroll
      for (int i = 0; i < CQT_FT; ++i)
#pragma unroll
        for (int j = 0; j < CQT_BK; ++j) acc[i][j] = fma(xv[i], gv[j], acc[i][j]);
    }
  }
  // the 64 lanes' partial sums of each (frame, bin): 16 of the 64 sums per pass through LDS, lane
  // (i, q) adds quarter q of row i in lane order, two exchanges join the quarters (a + b == b + a, so
  // all four lanes hold the same bits)
  const int ri = lane & 15, rq = lane >> 4;
#pragma unroll
  for (int p = 0; p < CQT_FT * CQT_BK / kCqtRedRows; ++p) {
#pragma unroll
    for (int i = 0; i < kCqtRedRows; ++i)
      red[w][i][lane] = acc[(p * kCqtRedRows + i) / CQT_BK][(p * kCqtRedRows + i) % CQT_BK];
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 16; ++j) s += red[w][ri][rq * 16 + j];
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    const int v = p * kCqtRedRows + ri;
    const int64_t f = f0 + v / CQT_BK;
    const int k = grp * CQT_BK + v % CQT_BK;
    if (rq == 0 && f < a.F && k < a.K) a.cqt[f * a.K + k] = fabs(a.N * s);   // cmplx.Abs :203
    __syncthreads();
  }
}

// 16 frames x 12 classes per block.  Thread (frame, c) adds cqt^2 of class c's bins in bin order
// (:224-235), then every thread of a frame adds the 12 sums in class order (:257-260) and divides its
// own when the total is > 1e-10 (:263-267).
__global__ __launch_bounds__(192) void cqt_fold_kernel(const double* cqt, int64_t F, int K, const int32_t* cls,
                                                        double* chroma) {
  __shared__ double e[16][12];
  const int fl = threadIdx.x / 12, c = threadIdx.x % 12;
  const int64_t f = (int64_t)blockIdx.x * 16 + fl;
  double s = 0.0;
  if (f < F) {
    const double* row = cqt + f * K;
    for (int k = 0; k < K; ++k)
      if (cls[k] == c) s = __dadd_rn(s, __dmul_rn(row[k], row[k]));
  }
  e[fl][c] = s;
  __syncthreads();
  if (f >= F) return;
  double total = 0.0;
  for (int j = 0; j < 12; ++j) total = __dadd_rn(total, e[fl][j]);
  chroma[f * 12 + c] = total > 1e-10 ? __ddiv_rn(s, total) : s;
}

int launch_chroma_cqt(const CqtArgs& a, hipStream_t s) {
  if (a.F < 1 || a.K < 1 || a.ngroups != (a.K + CQT_BK - 1) / CQT_BK || a.ngroups > 65535) return -1;
  const int64_t tiles = (a.F + CQT_FT * kCqtWaves - 1) / (CQT_FT * kCqtWaves);
  const int64_t fblocks = (a.F + 15) / 16;
  if (tiles > 0x7fffffff || fblocks > 0x7fffffff) return -1;
  hipLaunchKernelGGL(cqt_bank_kernel, dim3((unsigned)tiles, (unsigned)a.ngroups), dim3(64 * kCqtWaves), 0, s, a);
  hipLaunchKernelGGL(cqt_fold_kernel, dim3((unsigned)fblocks), dim3(192), 0, s, a.cqt, a.F, a.K, a.cls, a.chroma);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // namespace sonar
