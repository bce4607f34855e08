// pitch_track_check.cpp -- the library's pitch tracker and stability analysis (host_dsp.cpp:
// host::PitchTracker, host::pitch_stability, host::YinTracker) as a stand-alone program, so that
// tests/test_pitch_cpu.py can hold them to the Python checker without a device, and so that the same
// code can run under a sanitizer.  Cases on stdin, numbers as C hex floats both ways:
//   T <octave> <smoothing> <median> <min_conf> <F>   then F rows  <raw_pitch> <raw_conf> <n_cand> <second>
//     -> F lines of the nine PitchRow values followed by YinTracker::step's pitch, confidence, voicing
//   S <sample_rate> <hop> <n>   then n pitches
//     -> one line: <ok> and the seven values
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
      int oct = 0, sm = 0, med = 0;
      long long F = 0;
      double mc = 0;
      if (std::scanf("%d %d %d", &oct, &sm, &med) != 3 || !next_double(&mc) || std::scanf("%lld", &F) != 1) return 2;
      sonar::host::PitchTrackParams p;
      p.octave_correction = oct != 0; p.temporal_smoothing = sm != 0; p.median_filter = med; p.min_confidence = mc;
      sonar::host::PitchTracker tr;
      sonar::host::YinTracker yt;
      for (long long f = 0; f < F; ++f) {
        double rp, rc, sc;
        int nc;
        if (!next_double(&rp) || !next_double(&rc) || std::scanf("%d", &nc) != 1 || !next_double(&sc)) return 2;
        const sonar::host::PitchRow r = tr.step(p, rp, rc, nc, sc);
        double yp = rp, yc = rc, yv = 0.0;
        yt.step(yp, yc, yv);
        std::printf("%a %a %a %a %a %a %a %a %a %a %a %a\n", r.pitch, r.confidence, r.voicing, r.periodicity, r.clarity,
                    r.strength, r.salience, r.stability, r.f0_multiple, yp, yc, yv);
      }
    } else if (kind[0] == 'S') {
      int sr = 0, hop = 0;
      long long n = 0;
      if (std::scanf("%d %d %lld", &sr, &hop, &n) != 3) return 2;
      std::vector<double> v((size_t)n);
      for (auto& x : v)
        if (!next_double(&x)) return 2;
      double out[7];
      const bool ok = sonar::host::pitch_stability(v.data(), n, sr, hop, out);
      std::printf("%d %a %a %a %a %a %a %a\n", ok ? 1 : 0, out[0], out[1], out[2], out[3], out[4], out[5], out[6]);
    } else {
      return 2;
    }
  }
  return 0;
}
