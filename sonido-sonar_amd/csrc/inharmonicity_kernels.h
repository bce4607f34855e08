// inharmonicity_kernels.h -- the launch interface of inharmonicity_kernels.hip (InharmonicityAnalyzer.AnalyzeFrame
// per frame, algorithms/tonal/inharmonicity.go:236-292, without postProcessResult's tracking).
#pragma once
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace sonar {

constexpr int INHARM_MAX_HARMONICS = 64;   // one lane per harmonic of analyzeHarmonicStructure
constexpr int INHARM_GRID = 201;           // fitRailsbackCurve's values of B (:640), one thread each
constexpr int INHARM_MAX_K = 4096;
constexpr int INHARM_MAX_BEAT_WIDTH = 4096;   // of a row of correlations (2 W - 1 at W <= 2048)

// the per-frame outputs of every entry; each may be null
struct InharmOut {
  int32_t* status;
  double *inh, *std_dev, *conf, *f0, *f0_conf;
  int32_t *num, *ndev, *h_number;  // h_*: F x slots
  double *h_freq, *h_ideal, *h_amp, *h_dev;
  double *stiffness, *fit, *clarity, *purity, *coherence, *r2, *chi2, *pval;
  int32_t* quality;
};

struct InharmArgs {
  const double* pcm;               // the PCM path: frames of W every hop, each whole; null for the spectrum path
  int64_t n, hop;
  const double* mag;               // the spectrum path: F x K rows
  const double *f0, *f0_conf;      // F each
  int64_t F;
  int W, K, sr, method, model;     // method: a SONAR_INHARM_* but PARTIAL_TRACKING (which is SPECTRAL_DEVIATION)
  const double2* tw;               // (cos, sin) of -2 pi m / W, m < W / 2 (the PCM path)
  const double* grid;              // INHARM_GRID values of B
  const double* beat;              // BEAT_PATTERN: the F values of launch_inharm_beat_tail
  int max_h, min_h;                // as given: max_h divides in the confidence and the quality score
  int slots;                       // max(max_h, 0): the width of the h_* rows
  double tol, strength, min_freq, max_freq, tension, length, outlier;
  int weight, robust;
  InharmOut o;
};

// LDS bytes of one block (one frame per block)
size_t inharm_lds_bytes(int K, bool pcm);

// 0, -1 for a shape the kernel does not take, -5 for a launch error
int launch_inharm(const InharmArgs& a, hipStream_t s);

// analyzePeriodicityVariation (:706-733) times 0.001 (:567) over nf rows of `width` = 2 maxLag + 1 correlations
// (lag = index - maxLag), into beat[f0 + row]
int launch_inharm_beat_tail(const double* corr, int width, int64_t f0, int64_t nf, double* beat, hipStream_t s);

}  // namespace sonar
