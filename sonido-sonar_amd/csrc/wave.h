// wave.h -- the wave-level device helpers every kernel file shares (gfx950, wave64).  Each performs
// one fixed sequence of operations, so a call site that moves here keeps its generated code; what
// reduces in another order or with its own tie rule stays with its kernel.
#pragma once
#include <hip/hip_runtime.h>

namespace sonar {

// Phase boundary of the wave-private LDS exchanges: the fence and wave barrier keep the
// compiler from moving DS ops across it; the explicit lgkmcnt(0) retires every DS op of the
// phase before the next phase reads other lanes' words (defensive; costs < 2 % in mfcc_pair_kernel).
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
#ifndef SONAR_NO_LGKM_SYNC
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
  __builtin_amdgcn_wave_barrier();
}

// lane `lane`'s v in every lane (two v_readlane; a wave-uniform result)
__device__ __forceinline__ double readlane_f64(double v, int lane) {
  const int2 a = __builtin_bit_cast(int2, v);
  return __builtin_bit_cast(double, make_int2(__builtin_amdgcn_readlane(a.x, lane), __builtin_amdgcn_readlane(a.y, lane)));
}

// a batched launch's job, or any argument struct at a wave-uniform address, into SGPRs (every
// field read through readfirstlane)
template <class J>
__device__ __forceinline__ J load_job(const J* p) {
  static_assert(sizeof(J) % 4 == 0, "read as dwords");
  J r;
  const int* src = reinterpret_cast<const int*>(p);
  int* dst = reinterpret_cast<int*>(&r);
#pragma unroll
  for (int k = 0; k < (int)(sizeof(J) / 4); ++k) dst[k] = __builtin_amdgcn_readfirstlane(src[k]);
  return r;
}

// xor-butterfly reductions over aligned groups of N lanes (N = 64: the wave); every lane of a group
// ends with the group's result.  Sum adds in butterfly order; max / min keep the compare-and-select
// form u > v ? u : v (not fmax / fmin, which canonicalise their operands and treat NaN differently).
template <class T, int N = 64>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = N / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
template <class T, int N = 64>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
  for (int o = N / 2; o > 0; o >>= 1) { const T u = __shfl_xor(v, o, 64); v = u > v ? u : v; }
  return v;
}
template <class T, int N = 64>
__device__ __forceinline__ T wave_min(T v) {
#pragma unroll
  for (int o = N / 2; o > 0; o >>= 1) { const T u = __shfl_xor(v, o, 64); v = u < v ? u : v; }
  return v;
}

}  // namespace sonar
