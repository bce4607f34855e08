// harmonic_ratio_kernels.h -- the launch interface of harmonic_ratio_kernels.hip (HarmonicRatioAnalyzer.AnalyzeFrame per
// frame, algorithms/tonal/harmonic_ratio.go:205-924, before postProcessResult).
#pragma once
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace sonar {

constexpr int HRATIO_MAX_HARMONICS = 64;   // one lane per harmonic of findHarmonicPeaks
constexpr int HRATIO_MAX_PEAKS = 100;      // NewSpectralPeaks(sr, height, 20.0, 100) :155, :169
constexpr int HRATIO_PEAK_SLOTS = 128;     // >= HRATIO_MAX_PEAKS, two per lane of a wave
constexpr int HRATIO_NOISE_WINDOW = 20;    // windowSize of the three noise floors :654, :672, :689

// the per-frame outputs of every entry; each may be null
struct HratioOut {
  double *ratio, *harm_e, *noise_e, *total_e, *f0, *f0_conf, *snr, *periodicity, *harmonicity, *voicing, *roughness;
  int32_t *num, *h_bin;            // h_*: F x max_h
  double *h_freq, *h_amp, *h_phase;
  double* noise_floor;             // F x K
};

struct HratioArgs {
  const double* pcm;               // the PCM path: frames of W every hop, each whole; null for the spectrum path
  int64_t n, hop;
  const double *mag, *phase;       // the spectrum path: F x K rows (phase may be null)
  int64_t F;
  int W, K, sr, method;            // method: SONAR_HRATIO_HNR, _HPS or _SPECTRAL (COMB is HNR)
  const double* win;               // W Hann values, denominator W - 1
  const double2* tw;               // (cos, sin) of -2 pi m / W, m < W / 2
  double min_freq, max_freq, tol, min_height, pct;
  int max_h, width, smooth, nf_method, nf_smooth, min_dist;
  int pct_ok;                      // the percentile is in [0, 1] (common.Percentile returns 0 otherwise)
  int hps_lo, hps_hi;              // int(min_freq W / sr), int(max_freq W / sr)
  HratioOut o;
};

// LDS bytes of one block of the per-frame kernel (one frame per block)
size_t hratio_lds_bytes(int K, bool pcm);

// 0, -1 for a shape the kernel does not take, -5 for a launch error
int launch_hratio(const HratioArgs& a, hipStream_t s);

// preprocessFrame of the frames [f0, f0 + nf) of pcm into rows of W: out[(f - f0) W + i] = pcm[f hop + i] win[i]
int launch_hratio_window(const double* pcm, int64_t hop, int W, const double* win, int64_t f0, int64_t nf, double* out,
                         hipStream_t s);
// analyzeACF's tail (:392-410) over nf rows of `width` correlations, into the outputs' rows from f0 on
int launch_hratio_acf_tail(const double* corr, int width, int64_t f0, int64_t nf, const HratioOut& o, hipStream_t s);
// analyzeYin's tail (:532-541) over the temporary detector's raw rows, after its postProcessResult on an
// empty history with min_confidence 0
int launch_hratio_yin_tail(const double* pitch, const double* conf, int64_t f0, int64_t nf, const HratioOut& o,
                           hipStream_t s);

}  // namespace sonar
