// inharm_track_check.cpp -- the library's inharmonicity tracker and regression (host_dsp.cpp:
// host::InharmTracker, host::gonum_linear_regression) as a stand-alone program, so that
// tests/test_inharm_cpu.py can hold them to the Python checker without a device and run the same code
// under a sanitizer.  Cases on stdin, numbers as C hex floats both ways:
//   T <tracking> <window> <F>   then F rows  <raw_inharmonicity> <f0>
//     -> F lines: inharmonicity, temporal_stability, inharmonicity_trend, f0_stability
//   R <n>   then n rows  <x> <y>
//     -> one line: the slope
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../sonido-sonar_amd/csrc/host_dsp.h"

static bool next_double(double* v) {
  char tok[128];
  if (std::scanf("%127s", tok) != 1) return false;
  *v = std::strtod(tok, nullptr);
  return true;
}

int main() {
  char kind[8];
  while (std::scanf("%7s", kind) == 1) {
    if (kind[0] == 'T') {
      int tracking = 0, window = 0;
      long long F = 0;
      if (std::scanf("%d %d %lld", &tracking, &window, &F) != 3 || window < 0) return 2;
      sonar::host::InharmTracker tr;
      for (long long f = 0; f < F; ++f) {
        double raw, f0;
        if (!next_double(&raw) || !next_double(&f0)) return 2;
        const sonar::host::InharmRow r = tr.step(tracking != 0, window, raw, f0);
        std::printf("%a %a %a %a\n", r.inharmonicity, r.stability, r.trend, r.f0_stability);
      }
    } else if (kind[0] == 'R') {
      long long n = 0;
      if (std::scanf("%lld", &n) != 1 || n < 2) return 2;
      std::vector<double> x((size_t)n), y((size_t)n);
      for (long long i = 0; i < n; ++i)
        if (!next_double(&x[(size_t)i]) || !next_double(&y[(size_t)i])) return 2;
      std::printf("%a\n", sonar::host::gonum_linear_regression(x.data(), y.data(), (size_t)n));
    } else {
      return 2;
    }
  }
  return 0;
}
