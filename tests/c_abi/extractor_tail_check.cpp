// extractor_tail_check -- the scalar host tails of the music, content and voice extractors
// (csrc/host_dsp.cpp) and the music extractor's plan (csrc/music_plan.h) under a plain host compiler.
// Reads cases on stdin and prints every result with %.17g (integers as integers), one labelled line each;
// tests/test_extractor_tail_cpu.py feeds the same cases to the plain-Python restatement and compares exactly.
//   goint X                                   -> goint V
//   edges RATE K NB                           -> edges NB+1 e[0] ..
//   variance N x[0] ..                        -> variance V
//   crest N peak[0] .. energy[0] ..           -> crest N v[0] ..
//   entropy N e[0] ..                         -> entropy N v[0] ..  and  loudness_range V
//   panics F HOP N                            -> chroma_panic FRAME | -1  and  pct_panic INDEX | -1  L
//   plan N F W RATE WINDOW HOP                -> plan F K chroma_bad Fe fse Fenv live L pct_index maxband e[0] .. e[6]
//   content CROSSINGS MAX MIN N SR THR K spec[] FE esum[] FT tsum[]
//                                             -> features (the ten fields)  and  class TYPE
//   walk FV N SR ROWS pitch[] conf[]          -> starts, lengths, f0 (counted lists)  and  voicing V
//   voice N SR VSTR NP ln[] amp[] f0[] NAC ac[] NHEAD head[]
//                                             -> voice (the twelve fields)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sonido-sonar_amd/csrc/host_dsp.h"
#include "../../sonido-sonar_amd/csrc/music_plan.h"

namespace H = sonar::host;

static bool read_doubles(std::vector<double>& v, long long n) {
  if (n < 0) return false;
  v.resize((size_t)n);
  for (double& x : v)
    if (std::scanf("%lf", &x) != 1) return false;
  return true;
}

static bool read_counted(std::vector<double>& v) {
  long long n;
  return std::scanf("%lld", &n) == 1 && read_doubles(v, n);
}

template <typename T>
static void print_list(const char* name, const std::vector<T>& v) {
  std::printf("%s %zu", name, v.size());
  for (T x : v) std::printf(" %.17g", (double)x);
  std::printf("\n");
}

static bool music_case(const char* kind) {
  std::vector<double> a, b;
  long long n, F, hop;
  int rate, K, nb, W, window, ihop;
  double x;
  if (!std::strcmp(kind, "goint")) {
    if (std::scanf("%lf", &x) != 1) return false;
    std::printf("goint %lld\n", (long long)H::go_int(x));
  } else if (!std::strcmp(kind, "edges")) {
    if (std::scanf("%d %d %d", &rate, &K, &nb) != 3 || nb < 0) return false;
    print_list("edges", H::contrast_edges(rate, K, nb));
  } else if (!std::strcmp(kind, "variance")) {
    if (!read_counted(a)) return false;
    std::printf("variance %.17g\n", H::gonum_variance(a.data(), a.size()));
  } else if (!std::strcmp(kind, "crest")) {
    if (std::scanf("%lld", &n) != 1 || !read_doubles(a, n) || !read_doubles(b, n)) return false;
    print_list("crest", H::crest_factors(a.data(), b.data(), a.size()));
  } else if (!std::strcmp(kind, "entropy")) {
    if (!read_counted(a)) return false;
    print_list("entropy", H::energy_entropy(a.data(), a.size(), &x));
    std::printf("loudness_range %.17g\n", x);
  } else if (!std::strcmp(kind, "panics")) {
    if (std::scanf("%lld %lld %lld", &F, &hop, &n) != 3 || hop <= 0) return false;
    int64_t frame = -1, index = -1, L = 0;
    if (!H::chroma_slice_panics(F, hop, n, &frame)) frame = -1;
    if (!H::percentile_panics(n, &index, &L)) index = -1;
    std::printf("chroma_panic %lld\npct_panic %lld %lld\n", (long long)frame, (long long)index, (long long)L);
  } else if (!std::strcmp(kind, "plan")) {
    if (std::scanf("%lld %lld %d %d %d %d", &n, &F, &W, &rate, &window, &ihop) != 6) return false;
    const sonar::MusicPlan p(n, F, W, rate, window, ihop);
    std::printf("plan %lld %d %lld %lld %lld %lld %d %lld %lld %d", (long long)p.F, p.K, (long long)p.chroma_bad,
                (long long)p.Fe, (long long)p.fse, (long long)p.Fenv, p.harmonic_live ? 1 : 0, (long long)p.L,
                (long long)p.pct_index, p.maxband);
    for (int e : p.edges) std::printf(" %d", e);
    std::printf("\n");
  } else {
    return false;
  }
  return true;
}

static bool content_case() {
  unsigned long long crossings;
  long long n;
  int sr;
  double mx, mn, thr;
  std::vector<double> spec, es, ts;
  if (std::scanf("%llu %lf %lf %lld %d %lf", &crossings, &mx, &mn, &n, &sr, &thr) != 6 || !read_counted(spec) ||
      !read_counted(es) || !read_counted(ts))
    return false;
  sonar_acoustic_features f = H::content_features(crossings, mx, mn, spec.data(), (int)spec.size(), es.data(),
                                                  (int64_t)es.size(), ts.data(), (int64_t)ts.size(), n, sr);
  const H::ContentClass c = H::classify_content(f, thr);
  f.classification_confidence = c.confidence;
  std::printf("features %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\nclass %d\n", f.zero_crossing_rate,
              f.spectral_centroid, f.energy_variance, f.silence_ratio, f.harmonic_ratio, f.low_freq_energy,
              f.high_freq_energy, f.dynamic_range, f.temporal_stability, f.classification_confidence, c.type);
  return true;
}

static bool voice_case(const char* kind) {
  long long n, Fv;
  int sr;
  if (!std::strcmp(kind, "walk")) {
    std::vector<double> p, c;
    long long rows;
    if (std::scanf("%lld %lld %d %lld", &Fv, &n, &sr, &rows) != 4 || rows < Fv || (n == 1024 && rows < 1) ||
        !read_doubles(p, rows) || !read_doubles(c, rows))
      return false;
    const H::PitchPeriods w = H::period_walk(p.data(), c.data(), Fv, n, sr);
    print_list("starts", w.st);
    print_list("lengths", w.ln);
    print_list("f0", w.f0);
    std::printf("voicing %.17g\n", w.voicing);
    return true;
  }
  double vstr;
  std::vector<double> lnd, amp, f0, ac, head;
  long long np;
  if (std::scanf("%lld %d %lf %lld", &n, &sr, &vstr, &np) != 4 || np < 3 || !read_doubles(lnd, np) ||
      !read_doubles(amp, np) || !read_doubles(f0, np) || !read_counted(ac) || !read_counted(head))
    return false;
  if ((!ac.empty() && ac.size() != 2048) || (n >= 1024 && head.size() < 1024)) return false;
  const std::vector<int64_t> ln(lnd.begin(), lnd.end());
  const sonar_voice_quality_result q = H::voice_quality_from(ln.data(), amp.data(), f0.data(), np,
                                                             ac.empty() ? nullptr : ac.data(), head.data(), n, sr, vstr);
  std::printf("voice %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %lld %.17g %.17g %.17g\n", q.jitter, q.shimmer, q.hnr,
              q.noise_measure, q.f0_stability, q.amplitude_stability, q.voicing_strength, q.overall_quality,
              (long long)q.num_periods, q.mean_f0, q.f0_range, q.analysis_quality);
  return true;
}

int main() {
  char kind[16];
  while (std::scanf("%15s", kind) == 1) {
    bool ok;
    if (!std::strcmp(kind, "content")) ok = content_case();
    else if (!std::strcmp(kind, "walk") || !std::strcmp(kind, "voice")) ok = voice_case(kind);
    else ok = music_case(kind);
    if (!ok) return 2;
  }
  return 0;
}
