// pitch_kernels.h -- the launch interface of pitch_kernels.hip (PitchDetector.DetectPitch per frame,
// algorithms/tonal/pitch_detection.go:225-727, before postProcessResult).
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

struct sonar_ctx;

namespace sonar {

constexpr int PITCH_MIN_W = 64, PITCH_MAX_W = 2048;   // powers of two; W * zero_padding and the ACF's 2 W
constexpr int PITCH_MAX_FFT = 4096;                   // fit the 4096-point LDS tile (XCORR_FFT_TILE)
constexpr int PITCH_MAX_CANDIDATES = 8;
// frames per block of the wave-per-frame kernels (YIN, NSDF, zero crossing) and frames per wave of the
// z-score statistics pass (one frame per lane); the transform kernels take one frame per block
constexpr int PITCH_FRAMES_PER_BLOCK = 4;
constexpr int PITCH_STATS_FRAMES_PER_WAVE = 64;

struct PitchArgs {
  const double* pcm;
  int64_t n, F, hop;             // frames 0 .. F - 1 start at f * hop; every frame is whole
  int W, sr, method, pre, zp, K; // method: SONAR_PITCH_*; K = max_candidates
  const double* win;             // W window values
  const double2* tw;             // (cos, sin) of -2 pi m / N, m < N / 2, of the method's transform (or null)
  double min_freq, max_freq, yin_thr, ac_thr;
  int lo, hi;                    // HPS: [minBin, maxBin); cepstrum: [minQuefrency, maxQuefrency)
  double* stats;                 // ACF: 2 F doubles of scratch (mean, population std per frame)
  // outputs, per frame; all but pitch and conf may be null
  double *pitch, *conf, *second;
  int32_t *index, *ncand, *cand_index;
  double *cand_conf, *curve;
  int width;                     // of a frame's curve
};

// 0, -1 for a shape the kernels do not take, -5 for a launch error
int launch_pitch_frames(const PitchArgs& a, hipStream_t s);

namespace detail {
// The cached device tables of the pitch entries (pitch_api.cpp), which the harmonic-ratio entries share:
// createWindowFunction's window (SONAR_PITCH_WIN_*, denominator W - 1) and the N / 2 (cos, sin) pairs of
// -2 pi m / N.  Null after a failure, whose code and text the context holds.
const double* pitch_window(sonar_ctx* c, int type, int W);
const double2* pitch_twiddles(sonar_ctx* c, int64_t N);
}  // namespace detail

}  // namespace sonar
