// speech_layout.h -- the one description of what sonar_extract_speech_features (speech_api.cpp) sizes:
// its frame counts and the sections of its pinned result block.  The block holds float64 values only;
// every section starts on a multiple of 8 doubles, in this order:
//   mfcc      F x nm coefficients (absent with MFCC off)
//   spec      nine descriptor rows of F: centroid, rolloff, bandwidth, flatness, crest, slope, flux,
//             low and high energy ratio
//   zcr       F
//   energy    Fe short-time energies, then  entropy  Fe
//   pitch_raw Fp raw YIN pitches, then  conf_raw  Fp confidences
//   stats     256 block partials of (peak, sum |y|, sum y^2, sign changes)
//   envelope  Fenv RMS frames 512 / 256, then  loudness  Fl RMS frames of 400 ms / 100 ms
//   tilt      Fp (absent with the speech block off)
//   head      the first min(n, 1024) pre-emphasised samples (detectSpeech's periodicity check)
//   track     six tracked rows of Fp: pitch, confidence, voicing, harmonic ratio, inharmonicity, tonal centroid
//   lohi      2 x Fe: the energy ratios padded with zeros, only when Fe > F
// Everything but track and lohi is copied from the device; those two are written on the host.
// No HIP types here, so the plain host compiler can check the arithmetic (tests/c_abi/speech_layout_check.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace sonar {

// ShortTimeEnergy's frame count (energy.go:55-58) and the pitch track's (1024 / 512)
inline int64_t energy_frames(int64_t n, int64_t W, int64_t H) { return (n < W || H <= 0 || W <= 0) ? 0 : (n - W) / H + 1; }
inline int64_t pitch_frames(int64_t n) { return std::max<int64_t>((n - 1024) / 512 + 1, 0); }

constexpr int SPEECH_STAT_BLOCKS = 256;

struct SpeechPlan {
  enum Section { MFCC, SPEC, ZCR, ENERGY, ENTROPY, PITCH_RAW, CONF_RAW, STATS, ENVELOPE, LOUDNESS, TILT, HEAD, TRACK,
                 LOHI, NSEC };
  struct Sec { size_t off, cnt; };   // in doubles
  int64_t F = 0, Fe = 0, Fp = 0, Fenv = 0, Fl = 0;
  int lw = 0, lh = 0, nm = 0;        // loudness window and hop in samples; MFCC coefficients per frame
  Sec sec[NSEC] = {};
  size_t total = 0;                  // the block's size in doubles

  SpeechPlan() = default;
  // n samples, F spectrogram frames (sonar_stft_frames, checked by the caller); rate = FeatureConfig.SampleRate
  SpeechPlan(int64_t n, int64_t F_, int rate, int window, int hop, int mfcc_coefficients, bool mfcc, bool speech)
      : F(F_), Fe(energy_frames(n, window, hop)), Fp(pitch_frames(n)),
        Fenv(energy_frames(n, 512, 256)),                          // extractSimpleEnvelope (speech.go:752-777)
        lw((int)(0.4 * (double)rate)), lh(std::max(1, lw / 4)),      // ComputeLoudnessRange (energy.go:145-178)
        nm(mfcc_coefficients > 0 ? mfcc_coefficients : 13) {
    Fl = rate > 0 ? energy_frames(n, lw, lh) : 0;
    const size_t f = (size_t)F, fe = (size_t)Fe, fp = (size_t)Fp;
    const size_t cnt[NSEC] = {mfcc ? f * nm : 0, f * 9, f, fe, fe, fp, fp, (size_t)SPEECH_STAT_BLOCKS * 4,
                              (size_t)Fenv, (size_t)Fl, speech ? fp : 0, (size_t)std::min<int64_t>(n, 1024), 6 * fp,
                              Fe > F ? 2 * fe : 0};                  // Go pads the ratios past the spectrogram
    for (int i = 0; i < NSEC; i++) {
      sec[i] = {total, cnt[i]};
      total += (cnt[i] + 7) & ~size_t(7);
    }
  }
  bool lohi_copy() const { return sec[LOHI].cnt != 0; }
  double* at(double* base, Section s) const { return base + sec[s].off; }
};

}  // namespace sonar
