// go_math.h -- Go's math.Max, math.Min and math.Log2, one definition each for the host layer and the
// kernels.  Every caller hangs a decision on them (the NaN / +-0 / +-Inf order of a DTW step or a
// clamped score, the CQT bin count at whole octaves), so they follow Go's source test by test.  A
// plain host compiler without the HIP headers can include this file too.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define SONAR_GO_MATH __host__ __device__ inline __attribute__((always_inline))
#else
#define SONAR_GO_MATH inline
#endif

namespace sonar {

// math.Max (Go's dim.go): +Inf wins, then NaN propagates, then +0 > -0
SONAR_GO_MATH double go_max(double x, double y) {
  if (__builtin_isinf(x) && x > 0) return x;
  if (__builtin_isinf(y) && y > 0) return y;
  if (__builtin_isnan(x) || __builtin_isnan(y)) return __builtin_nan("");
  if (x == 0 && x == y) return __builtin_signbit(x) ? y : x;
  return x > y ? x : y;
}

// math.Min (Go's dim.go): -Inf wins, then NaN propagates, then -0 < +0
SONAR_GO_MATH double go_min(double x, double y) {
  if (__builtin_isinf(x) && x < 0) return x;
  if (__builtin_isinf(y) && y < 0) return y;
  if (__builtin_isnan(x) || __builtin_isnan(y)) return __builtin_nan("");
  if (x == 0 && x == y) return __builtin_signbit(x) ? x : y;
  return x < y ? x : y;
}

// math.Log2 (Go's log10.go): Frexp, an exact answer for powers of two, else exp + Log(frac) * (1 / Ln2).
// int(Log2(max / min) * bins) truncates, so the last bit decides a bin count at whole octaves.
SONAR_GO_MATH double go_log2(double x) {
  int e = 0;
  const double fr = ::frexp(x, &e);
  if (fr == 0.5) return (double)(e - 1);
  return (double)e + ::log(fr) * (1.0 / 0.693147180559945309417232121458176568);
}

}  // namespace sonar
