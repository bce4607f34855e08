// go_math_check -- csrc/go_math.h under a plain host compiler: the known answers of Go's math.Max,
// math.Min and math.Log2 documentation.  Prints one line per failure; exit status 1 if there is any.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../../sonido-sonar_amd/csrc/go_math.h"

using sonar::go_log2;
using sonar::go_max;
using sonar::go_min;

static int failures = 0;

static uint64_t bits(double x) {
  uint64_t b;
  std::memcpy(&b, &x, 8);
  return b;
}
// the same value bit for bit; any NaN equals any NaN
static void same(const char* what, double got, double want) {
  if ((std::isnan(got) && std::isnan(want)) || bits(got) == bits(want)) return;
  std::printf("FAIL %s: got %a (%016llx), want %a (%016llx)\n", what, got, (unsigned long long)bits(got), want,
              (unsigned long long)bits(want));
  failures++;
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double pz = 0.0, nz = -0.0;
  // math.Max: Max(x, +Inf) = Max(+Inf, x) = +Inf; Max(x, NaN) = Max(NaN, x) = NaN; Max(+0, +-0) = Max(+-0, +0) = +0;
  // Max(-0, -0) = -0
  same("Max(+0,-0)", go_max(pz, nz), pz);
  same("Max(-0,+0)", go_max(nz, pz), pz);
  same("Max(-0,-0)", go_max(nz, nz), nz);
  same("Max(1,NaN)", go_max(1.0, nan), nan);
  same("Max(NaN,1)", go_max(nan, 1.0), nan);
  same("Max(+Inf,NaN)", go_max(inf, nan), inf);
  same("Max(NaN,+Inf)", go_max(nan, inf), inf);
  same("Max(-Inf,NaN)", go_max(-inf, nan), nan);
  same("Max(1,2)", go_max(1.0, 2.0), 2.0);
  same("Max(2,1)", go_max(2.0, 1.0), 2.0);
  same("Max(-Inf,-1)", go_max(-inf, -1.0), -1.0);
  // math.Min: Min(x, -Inf) = Min(-Inf, x) = -Inf; Min(x, NaN) = Min(NaN, x) = NaN; Min(-0, +-0) = Min(+-0, -0) = -0
  same("Min(+0,-0)", go_min(pz, nz), nz);
  same("Min(-0,+0)", go_min(nz, pz), nz);
  same("Min(+0,+0)", go_min(pz, pz), pz);
  same("Min(1,NaN)", go_min(1.0, nan), nan);
  same("Min(NaN,1)", go_min(nan, 1.0), nan);
  same("Min(-Inf,NaN)", go_min(-inf, nan), -inf);
  same("Min(NaN,-Inf)", go_min(nan, -inf), -inf);
  same("Min(+Inf,NaN)", go_min(inf, nan), nan);
  same("Min(1,2)", go_min(1.0, 2.0), 1.0);
  same("Min(2,1)", go_min(2.0, 1.0), 1.0);
  same("Min(+Inf,1)", go_min(inf, 1.0), 1.0);
  // math.Log2: exact at every power of two a float64 holds, subnormal ones included
  for (int k = -1074; k <= 1023; ++k) {
    char what[32];
    std::snprintf(what, sizeof what, "Log2(2^%d)", k);
    same(what, go_log2(std::ldexp(1.0, k)), (double)k);
  }
  // Log2(+-0) = -Inf, Log2(x < 0) = NaN, Log2(+Inf) = +Inf, Log2(NaN) = NaN
  same("Log2(+0)", go_log2(pz), -inf);
  same("Log2(-0)", go_log2(nz), -inf);
  same("Log2(-1)", go_log2(-1.0), nan);
  same("Log2(+Inf)", go_log2(inf), inf);
  same("Log2(NaN)", go_log2(nan), nan);
  // elsewhere the value is Frexp's exponent plus Log(fraction) * (1 / Ln2), each operation rounded on its own
  const double xs[] = {3.0, 10.0, 24.0, 0.1, 440.0 / 261.6255653005986, 5000.0 / 40.0, 1.0 / 24.0, 6.02214076e23,
                       4.9406564584124654e-324 * 3.0};
  for (double x : xs) {
    int e = 0;
    const volatile double fr = std::frexp(x, &e);
    const volatile double l = std::log(fr);
    const volatile double inv = 1.0 / 0.693147180559945309417232121458176568;
    const volatile double prod = l * inv;
    const volatile double want = (double)e + prod;
    char what[48];
    std::snprintf(what, sizeof what, "Log2(%a)", x);
    same(what, go_log2(x), want);
  }
  if (failures == 0) std::printf("go_math ok\n");
  return failures ? 1 : 0;
}
