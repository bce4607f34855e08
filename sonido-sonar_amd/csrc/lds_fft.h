// lds_fft.h -- the radix-2 transform of a frame held in LDS, shared by the kernel files that must give
// correlation.go's bits for |X| (harmonic_ratio_kernels.hip, inharmonicity_kernels.hip): the butterfly with each
// operation rounded on its own, the level loop over a block of 256 threads, and the bit-reversed load index.
// xcorr_kernels.hip and pitch_kernels.hip keep their own statements of the same order (their tiles and thread
// counts differ).
#pragma once
#include <hip/hip_runtime.h>

namespace sonar {

__device__ __forceinline__ void fft_butterfly(double c, double s, double& er, double& ei, double& odr, double& odi) {
  const double tr = __dsub_rn(__dmul_rn(c, odr), __dmul_rn(s, odi));
  const double ti = __dadd_rn(__dmul_rn(c, odi), __dmul_rn(s, odr));
  const double ar = er, ai = ei;
  er = __dadd_rn(ar, tr); ei = __dadd_rn(ai, ti);
  odr = __dsub_rn(ar, tr); odi = __dsub_rn(ai, ti);
}

// in place over sre / sim[0, N) in bit-reversed order, by a block of 256 threads; tw: (cos, sin) of -2 pi m / N
static __device__ void lds_fft_256(double* sre, double* sim, int N, int logN, const double2* tw) {
  for (int s = 1; s <= logN; ++s) {
    __syncthreads();
    const int h = 1 << (s - 1);
    const int stride = N >> s;
    for (int k = threadIdx.x; k < N / 2; k += 256) {
      const int i = k & (h - 1);
      const int p = ((k >> (s - 1)) << s) + i, q = p + h;
      const double2 w = tw[i * stride];
      double er = sre[p], ei = sim[p], odr = sre[q], odi = sim[q];
      fft_butterfly(w.x, w.y, er, ei, odr, odi);
      sre[p] = er; sim[p] = ei; sre[q] = odr; sim[q] = odi;
    }
  }
  __syncthreads();
}

__device__ __forceinline__ int fft_log2i(int N) { return 31 - __clz(N); }
__device__ __forceinline__ int fft_bitrev(int j, int logN) { return (int)(__brev((unsigned)j) >> (32 - logN)); }

}  // namespace sonar
