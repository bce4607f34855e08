// host_dsp.h -- host-side parts of the hot path that are O(table) or O(path):
// window / filterbank / DCT tables built once per configuration, and the
// sequential scalar epilogues of the Go API (YIN temporal tracking, the speech
// extractor's tail, NCC peak metrics, alignment scorers).  Pure C++17, float64,
// Go evaluation order.
#pragma once
#include "../../include/sonar_gpu.h"

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace sonar {
namespace host {

// analyzers.WindowGenerator.Generate (fingerprint/analyzers/windowing.go:77-136)
bool make_window(int type, int size, bool symmetric, bool normalize, double beta, double alpha,
                 std::vector<double>& out);

// MelScale / BarkScale.CreateXFilterBank (algorithms/spectral/mel_scale.go:29-86,
// bark_scale.go:36-93) as dense rows [n_filters][fft_size/2+1]
bool make_filterbank(int kind, int n_filters, int fft_size, int sample_rate, double low, double high,
                     std::vector<double>& fb);

struct MfccTables {
  int n_mfcc = 13, n_mels = 26, K = 0;
  std::vector<int> lo, hi, woff;   // per filter nonzero range [lo, hi)
  std::vector<double> w;           // packed weights
  std::vector<double> dct;         // [n_mfcc][n_mels] (mfcc.go:194-212)
  std::vector<double> lift;        // [n_mfcc] lifter multipliers (mfcc.go:230-245)
};
// NewMFCCWithParams defaults + Initialize (mfcc.go:58-110)
bool make_mfcc_tables(int sample_rate, int n_mfcc, int n_filters, int fb_kind, double low, double high,
                      bool use_lifter, double lifter, int fft_size, MfccTables& t);
// balanced assignment of filter rows to `groups` epilogue groups (by nonzeros)
void balance_groups(const MfccTables& t, int groups, std::vector<int>& off, std::vector<int>& mels);

// ChromaSTFT.calculateChromaMapping (algorithms/chroma/chroma_stft.go:95-117)
std::vector<int> chroma_map(int fs, int sample_rate);

// PitchDetector post-processing + temporal tracking (pitch_detection.go:767-921)
// The history is Go's pitchHistory capped at 20 entries (only its last 5 are ever read), kept in a
// fixed array: one step allocates nothing (a 1-hour call runs 310,000 steps).
struct YinTracker {
  double hist[20] = {0};
  int count = 0;                   // entries held (<= 20), oldest first
  double prev = 0.0;
  void step(double& pitch, double& conf, double& voicing);
};
// DetectPitch's post-processing over the raw YIN rows [lo, hi) of an n-sample signal (frames of 1024
// every 512; a frame past the end is skipped and gives zeros, pitch_detection.go:226): the tracked
// pitch, confidence and voicing rows; pitch and conf may be null.  The speech extractor runs its voicing
// pass (extractVoicingProbability, speech.go:530-550) and then its harmonic pass (:464-509) through the
// same tracker, whose history carries over: that is the Go behaviour.
void track_rows(YinTracker& t, const double* raw_pitch, const double* raw_conf, int64_t lo, int64_t hi, int64_t n,
                double* pitch, double* conf, double* voicing);

// The speech extractor's sequential tail over its energy frames e[0, n) (speech.go:587-797); rate is
// FeatureConfig.SampleRate, 0 under GenerateFingerprint (F1): the frame time hop / rate is then +Inf.
// The element at index n / 10 of the sorted energies (n > 0): the silence threshold of the next two
double percentile10_threshold(const double* e, size_t n);
double silence_ratio(const double* e, size_t n, double thr);                                  // :641-668
std::vector<double> pause_durations(const double* e, size_t n, double thr, int hop, int rate);   // :587-639
std::vector<int64_t> detect_onsets(const double* e, size_t n);                                // :672-716
std::vector<double> attack_times(const std::vector<int64_t>& onsets, const double* e, int hop, int rate);   // :718-749
double speech_rate(double silence, int64_t n_samples, int rate);                              // :779-797, speech detected
// SpeechAnalyzer.detectSpeech (speech_analysis.go:105-202) from the whole signal's zero-crossing count
// and sum of squares and its first head_n = min(n, 1024) samples (checkPeriodicity reads no more)
bool detect_speech(int64_t n_samples, int rate, double crossings, double sum_sq, const double* head, int64_t head_n);

// CrossCorrelation metrics from the correlation array (correlation.go:526-667)
struct NccMetrics {
  double peak_corr = 0, p_value = 1, snr = 0, sharpness = 0, second_peak = 0, psl = 0;
  int64_t peak_lag = 0, peak_index = 0, overlap = 0, num_lags = 0;
};
// The O(lags) part of those metrics: findPeak's index and value, calculateSNR's noise sum and count
// (|i - peak| > 5), findSecondPeak's value, calculatePeakToSidelobe's sidelobe maximum (|i - peak|
// > 10) and calculateSharpness's second difference (0 at the ends).  corr_sums runs Go's loops; the
// batched pair path computes the same on the device (pair_score_kernel, pair_score_kernels.hip), every
// sum in Go's index order with masked terms added as exact zeros, so the two are bit-identical
// (test_device_scorer_equals_host_scorer).  Plain data, shared with the kernels.
struct CorrSums {
  int64_t num_lags = 0, peak_index = 0, noise_count = 0;
  double peak = 0, noise_sum = 0, second_peak = 0, max_sidelobe = 0, sharpness = 0;
};
CorrSums corr_sums(const double* corr, int64_t nl);
NccMetrics ncc_metrics(const CorrSums& c, int64_t L, int64_t na, int64_t nb);
NccMetrics ncc_metrics(const double* corr, int64_t nl, int64_t L, int64_t na, int64_t nb);
// The O(path) part of the DTW scorers (alignment.go:380-643): the path length and end points,
// diagonal steps and direction changes (calculateDiagonalBias, calculatePathChanges), the offset
// sum (calculateAverageOffset), the cost sum (calculateSimilarityFromDTW's mean cost) and
// calculateCostConsistency's smoothed-cost sum and squared deviations from their mean
struct PathSums {
  int64_t P = 0, diag_steps = 0, changes = 0, offset_sum = 0;
  int32_t p0q = 0, p0r = 0, p1q = 0, p1r = 0;
  double sum_cost = 0, sum_smooth = 0, var_smooth = 0;
};
PathSums path_sums(const int32_t* pq, const int32_t* pr, const double* pc, int64_t P);

// AlignmentAnalyzer scorers (algorithms/stats/alignment.go)
struct AlignScores {
  double similarity = 0, confidence = 0, offset_seconds = 0, quality = 0, stability = 0, noise_level = 0;
  int64_t offset = 0;
};
AlignScores xcorr_scores(const NccMetrics& m, int hop, int sample_rate, int max_lag);
AlignScores dtw_scores(const int32_t* pq, const int32_t* pr, const double* pc, int64_t P, int64_t nq, int64_t nr,
                       double distance, int sample_rate);
AlignScores dtw_scores(const PathSums& s, int64_t nq, int64_t nr, double distance, int sample_rate);

// Energy helpers used by extractEnergyFeatures (algorithms/temporal/energy.go:96-178)
double energy_variance(const double* e, size_t n);
// ComputeLoudnessRange tail: RMS of 400 ms / 100 ms frames -> LU -> 10th..95th percentile range
double loudness_range_from_rms(std::vector<double> rms);

// MusicFeatureExtractor.ExtractFeatures' scalar tail (fingerprint/extractors/music.go:378-525)
// Go int(float64) on amd64 (CVTTSD2SQ): NaN / out of range -> MinInt64
int64_t go_int(double x);
// SpectralContrast.initializeBands (spectral_contrast.go:140-185): nb + 1 bin edges
std::vector<int> contrast_edges(int sample_rate, int K, int nb);
// gonum stat.Variance(x, nil) (v0.16.0 MeanVariance: compensated two-pass, n - 1), with the
// mean's sum sequential (gonum's amd64 kernel pairs terms: agreement to rounding, parity unpinned)
double gonum_variance(const double* x, size_t n);
std::vector<double> crest_factors(const double* peaks, const double* energy, size_t n);      // :428-444
// -e log2 e per frame (:481-497), and 20 log10 of the largest over the smallest positive energy (:499-510)
std::vector<double> energy_entropy(const double* e, size_t n, double* loudness_range);
// Where Go panics, and what its runtime message names.  extractChromaFeatures slices
// processedPCM[f hop : min(f hop + n / F, n)] (:348-352, hop > 0): with (F - 1) hop > n the first frame
// starting past the end is *frame, "slice bounds out of range [*frame hop:n]".
bool chroma_slice_panics(int64_t F, int64_t hop, int64_t n, int64_t* frame);
// DynamicRange.ComputeRange(pcm, 10, 90) (:401-403, dynamic_range.go:58-76) reads sorted[int(10 (L - 1))] of
// the L RMS frames 1024 / 512: "index out of range [*index] with length *L" for every L >= 2
bool percentile_panics(int64_t n, int64_t* index, int64_t* L);

// ContentDetector.extractAcousticFeatures (fingerprint/content_detector.go:118-150) from the whole signal's
// sign changes and extrema of |x|, the K magnitudes of its first 2 (K - 1) samples' DFT, the fe sums of
// squares of frames 1024 / 512 and the ft of frames of 100 ms; classification_confidence is left 0
sonar_acoustic_features content_features(uint64_t crossings, double max, double min, const double* spec, int K,
                                         const double* esum, int64_t fe, const double* tsum, int64_t ft, int64_t n,
                                         int sr);
// classifyFromFeatures (:153-217): the first score strictly above thr and the others (Go iterates a map;
// here music, news, talk, sports); confidence = the winning score, or thr, over 6
struct ContentClass { int type; double confidence; };
ContentClass classify_content(const sonar_acoustic_features& f, double thr);

// VoiceQualityAnalyzer.extractPitchPeriodsAndF0 (algorithms/speech/voice_quality.go:114-157) over the raw
// YIN rows of the Fv frames 1024 / 256 of an n-sample signal: a fresh PitchDetector, voiced frames with
// voicing and confidence > 0.5 and F0 in [50, 500]; each period starts at max(frame start, last end).
// voicing: calculateVoicingStrength (:363-371), which DetectPitch answers only for n == 1024 (row 0 again).
struct PitchPeriods {
  std::vector<int64_t> st, ln;
  std::vector<double> f0;
  double voicing = 0.0;
};
PitchPeriods period_walk(const double* raw_pitch, const double* raw_conf, int64_t Fv, int64_t n, int sr);
// The scalar formulas (:160-451) over np >= 3 periods: their lengths, RMS amplitudes and F0, the 2048-lag
// autocorrelation of the middle frame (null for n < 2048) and the first min(n, 1024) samples
sonar_voice_quality_result voice_quality_from(const int64_t* ln, const double* amp, const double* f0, int64_t np,
                                              const double* ac, const double* head, int64_t n, int sr, double vstr);

// PitchDetector's postProcessResult + updateTemporalTracking (pitch_detection.go:767-963) for any
// method and any post-processing parameters: YinTracker above is this at the constructor's defaults,
// reduced to the three values its callers read.  One step per raw frame, in order; a fresh tracker is a
// fresh detector (or one after Reset).
struct PitchTrackParams {
  bool octave_correction = true, temporal_smoothing = true;
  int median_filter = 3;           // getRecentPitches(n): n > 20 reads the whole history, n < 1 nothing
  double min_confidence = 0.5;
};
struct PitchRow {
  double pitch = 0, confidence = 0, voicing = 0, periodicity = 0, clarity = 0, strength = 0, salience = 0,
         stability = 0, f0_multiple = 0;
};
struct PitchTracker {
  double hist[20] = {0};           // pitchHistory: gated, octave-corrected, unsmoothed; oldest first
  int count = 0;
  double prev = 0.0;               // previousPitch: the last smoothed pitch
  // raw_pitch / raw_conf: what detectPitch* returned (Periodicity = Voicing = Confidence there);
  // n_candidates = len(Candidates), second_conf = Candidates[1].Confidence when there are two
  PitchRow step(const PitchTrackParams& p, double raw_pitch, double raw_conf, int n_candidates, double second_conf);
};
// AnalyzePitchStability + estimateVibratoRate (:1059-1160): out7 = mean_pitch, pitch_std_dev,
// coefficient_of_variation, jitter, stability, vibrato_rate, voiced_frames_ratio; false (and zeros) for
// the empty map of fewer than two entries or fewer than two voiced ones
bool pitch_stability(const double* pitch, int64_t n, int sample_rate, int hop_size, double out7[7]);


// HarmonicRatioAnalyzer's postProcessResult + updateTemporalTracking (harmonic_ratio.go:926-1002).  One step
// per raw frame, in order; a fresh tracker is a fresh analyzer (or one after Reset).  The stability is
// 1 - sqrt(gonum_variance) / mean of the history (stat.Mean's sum sequential), the coherence
// exp(-mean |difference| / 10); both before the frame's own smoothed ratio enters the history, which keeps
// its last 2 len values.  len >= 0 (Go panics at :996 otherwise; the caller refuses it).
struct HratioRow { double ratio = 0, stability = 0, coherence = 0; };
struct HratioTracker {
  std::vector<double> hist;        // hrHistory, oldest first
  double prev = 0.0;               // previousHR
  HratioRow step(bool smoothing, int len, double raw);
};

// gonum stat.LinearRegression(x, y, nil, false)'s slope: the covariance over the variance of x, both
// compensated around stat.Mean's means (sums sequential here: parity unpinned, as gonum_variance); n >= 2
double gonum_linear_regression(const double* x, const double* y, size_t n);

// InharmonicityAnalyzer's postProcessResult + updateTemporalTracking (inharmonicity.go:1007-1101).  One step per
// frame that reaches them (AnalyzeFrame returns before both on an invalid f0), in order; a fresh tracker is a
// fresh analyzer (or one after Reset).  The stability, the trend and the f0 stability are computed before the
// frame's own values enter the histories, which keep their last `window` entries.  window >= 0 (Go panics at
// :1098 otherwise; the caller refuses it).
struct InharmRow { double inharmonicity = 0, stability = 0, trend = 0, f0_stability = 0; };
struct InharmTracker {
  std::vector<double> hist, f0_hist;   // inharmonicityHistory, f0History, oldest first
  InharmRow step(bool tracking, int window, double raw, double f0);
};

}  // namespace host
}  // namespace sonar
