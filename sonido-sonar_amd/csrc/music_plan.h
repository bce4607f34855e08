// music_plan.h -- what sonar_extract_music_features (music_api.cpp) derives from its arguments before it
// reserves or launches anything: the frame counts of every group, where Go panics, and the spectral
// contrast's band edges.  No HIP types here, so the plain host compiler can check the arithmetic
// (tests/c_abi/extractor_tail_check.cpp).
#pragma once
#include <algorithm>
#include <cstdint>

#include "host_dsp.h"
#include "speech_layout.h"

namespace sonar {

constexpr int kContrastBands = 6;                                  // NewSpectralContrast(sr, 6), music.go:117

struct MusicPlan {
  int64_t F = 0;             // spectrogram frames (sonar_stft_frames, checked by the caller)
  int K = 0;                 // bins per frame
  int64_t chroma_bad = -1;   // the chroma frame whose slice starts past the signal (Go panics there), or -1
  int64_t Fe = 0;            // ShortTimeEnergy frames (FeatureConfig window / hop); 0 after a chroma panic
  int64_t fse = 0;           // frameSize := len(pcm) / numFrames (:383)
  int64_t Fenv = 0;          // envelope frames of fse samples
  bool harmonic_live = false;   // the harmonic block's one live case: a 1024-sample frame (DetectPitch's window, :539)
  int64_t L = 0, pct_index = 0;   // DynamicRange's RMS frames; L >= 2: the index Go panics on
  int edges[kContrastBands + 1] = {};
  int maxband = 1;           // the widest band, in bins

  MusicPlan() = default;
  // n samples, spectrogram window W; rate, window, hop = FeatureConfig.SampleRate / WindowSize / HopSize.
  // hop <= 0 is ExtractFeatures' chroma error: nothing past the spectrogram's groups is planned then.
  MusicPlan(int64_t n, int64_t F_, int W, int rate, int window, int hop) : F(F_), K(W / 2 + 1) {
    const std::vector<int> e = host::contrast_edges(rate, K, kContrastBands);
    std::copy(e.begin(), e.end(), edges);
    for (int b = 0; b < kContrastBands; b++) maxband = std::max(maxband, std::min(edges[b + 1], K) - edges[b]);
    host::percentile_panics(n, &pct_index, &L);
    if (hop <= 0) return;
    if (host::chroma_slice_panics(F, hop, n, &chroma_bad)) return;
    Fe = energy_frames(n, window, hop);
    fse = Fe > 0 ? n / Fe : 0;
    Fenv = (Fe > 0 && fse > 0 && n >= fse) ? (n - fse) / hop + 1 : 0;
    harmonic_live = F > 0 && n / F == 1024 && n < 1536;
  }
};

}  // namespace sonar
