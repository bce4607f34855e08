/*
 * sonar_gpu.h -- C ABI of the MI355X (gfx950) implementation of the
 * sonido-sonar per-frame DSP + alignment hot path.
 *
 * Library: sonido-sonar_amd/lib/libsonar_gpu.so (HIP kernels + C++ host code).
 * Plain C types only: pointers, sizes, POD structs.  No torch, no HIP types.
 *
 * Every entry replaces one seam of the Go reference (RyanBlaney/sonido-sonar,
 * paths relative to the repo root); INTEGRATION.md shows the cgo binding.
 *
 *   sonar_fingerprint          <- SpectralAnalyzer.ComputeSTFTWithWindow
 *                                 (fingerprint/analyzers/spectral.go:385) fused with
 *                                 MFCC.ComputeFrames (algorithms/spectral/mfcc.go:167),
 *                                 the per-frame descriptors of
 *                                 SpeechFeatureExtractor.extractSpectralFeatures
 *                                 (fingerprint/extractors/speech.go:320) and
 *                                 Energy.ComputeShortTimeEnergy (algorithms/temporal/energy.go:25)
 *   sonar_fingerprint_batch    <- SpectralAnalyzer.ComputeSTFTBatch (fingerprint/analyzers/spectral.go:234)
 *   sonar_pitch_yin            <- PitchDetector.DetectPitch per-frame YIN core
 *                                 (algorithms/tonal/pitch_detection.go:225-420)
 *   sonar_pitch_frames_raw, sonar_pitch_detect, sonar_pitch_track, sonar_pitch_stability
 *                              <- PitchDetector.DetectPitch for every method of its switch,
 *                                 ProcessAudioStream, postProcessResult + updateTemporalTracking,
 *                                 AnalyzePitchStability (pitch_detection.go:225-1160)
 *   sonar_chroma_stft          <- MusicFeatureExtractor.extractChromaFeatures
 *                                 (fingerprint/extractors/music.go:327) ->
 *                                 ChromaSTFT.ComputeChroma (algorithms/chroma/chroma_stft.go:45)
 *   sonar_chroma_cqt           <- ChromaCQT.ComputeChroma (algorithms/chroma/chroma_cqt.go:69)
 *   sonar_chroma_cqt_plan      <- computeCQTKernel's bin count, kernel lengths and FFT size
 *                                 (chroma_cqt.go:95-165) and computeCQTSpectrogram's frame count (:169-172)
 *   sonar_chroma_similarity    <- ChromaSequenceSimilarity.ComputeSimilarity, all six methods
 *                                 (algorithms/chroma/chroma_similarity.go:86-538)
 *   sonar_chroma_frame_matrix  <- ChromaVectorAnalyzer.Distance / Similarity / CircularShift for every
 *                                 frame pair (chroma_vector.go:145-216; stats/distance.go)
 *   sonar_chroma_similarity_plan <- its integer side: sample step, OTI ranges, the DTW band rule
 *   sonar_spectral_peaks       <- SpectralPeaks.DetectPeaks per spectrum row
 *                                 (algorithms/harmonic/spectral_peaks.go:36-100)
 *   sonar_hpcp_from_spectrum   <- HPCP.ComputeFromSpectrum per spectrum row (algorithms/chroma/hpcp.go:205-221)
 *   sonar_hpcp                 <- SpectralAnalyzer.ComputeSTFT magnitudes -> HPCP.ComputeFromSpectrum per frame
 *   sonar_hpcp_table           <- frequencyToPitchClass, addPeakContribution, computeWindowWeight and
 *                                 addHarmonicContributions per FFT bin (hpcp.go:224-321)
 *   sonar_hpcp_plan            <- the frame count and the chunks sonar_hpcp works in
 *   sonar_hps_from_spectrum    <- HarmonicProduct.ComputeHPS / ComputeHPSWithInterpolation, findF0Peak,
 *                                 ComputeHarmonicStrength and ComputeHarmonicity per spectrum row
 *                                 (algorithms/harmonic/harmonic_product.go:32-273)
 *   sonar_hps                  <- HarmonicProduct.EstimateF0WithConfidence per frame of PCM (:61-91, :276-298)
 *   sonar_hps_bins             <- findF0Peak's scan range (:128-139)
 *   sonar_hps_optimal_harmonics <- HarmonicProduct.GetOptimalNumHarmonics (:301-314)
 *   sonar_hps_plan             <- the frame count and the chunks sonar_hps works in
 *   sonar_spectral_flux        <- SpectralFlux.Compute / ComputeAllChanges (algorithms/spectral/spectral_flux.go:17-56)
 *   sonar_rms_envelope         <- Envelope.ComputeRMS (algorithms/temporal/envelope.go:18-43)
 *   sonar_onset_peaks          <- OnsetDetection.findFluxPeaks on any curve (algorithms/temporal/onset_detection.go:97-120)
 *   sonar_onset_adaptive_threshold <- OnsetDetection.AdaptiveThreshold (:200-222)
 *   sonar_onsets_flux          <- OnsetDetection.DetectOnsets (:26-56)
 *   sonar_onsets_energy        <- OnsetDetection.DetectOnsetsEnergy (:59-94)
 *   sonar_onsets_complex       <- OnsetDetection.DetectOnsetsComplex, combineOnsets, ComputeOnsetDensity (:123-197)
 *   sonar_tempo_from_onsets    <- TempoEstimation.findTempoFromIntervals (algorithms/temporal/tempo_estimation.go:77-118)
 *   sonar_tempo_autocorrelation <- TempoEstimation.EstimateTempoAutocorrelation (:51-74, :121-201)
 *   sonar_tempo                <- TempoEstimation.EstimateTempo, EstimateTempoRange, ClassifyTempoCategory (:22-48, :204-232)
 *   sonar_key_frames          <- KeyEstimator.EstimateKey / EstimateKeyFromHPCP per chroma row,
 *                                 KeyEstimationBatch.ProcessBatch (algorithms/tonal/key_estimation.go:196-247, 911)
 *   sonar_key_sequence         <- KeyEstimator.EstimateKeySequence (key_estimation.go:250-270)
 *   sonar_key_batch            <- KeyEstimationBatch.ProcessBatch / GetGlobalKey / GetKeyProgression (:896-1005)
 *   sonar_key_transition       <- AnalyzeKeyTransition (:843-894)
 *   sonar_chord_frames         <- ChordDetector.DetectChord from templateMatching on, per chroma row through a
 *                                 fresh detector (algorithms/tonal/chord_detection.go:428-502)
 *   sonar_chord_sequence       <- the same with one detector fed the rows in order (:783-806, :919-926)
 *   sonar_chord_detect         <- ChordDetector.DetectChord per frame of PCM (:408-503, :506-531)
 *   sonar_chord_progression    <- ChordProgressionAnalyzer.AnalyzeProgression (:1128-1173)
 *   sonar_ncc                  <- CrossCorrelation.Compute, NormalizedCrossCorrelation /
 *                                 TimeDomain (algorithms/stats/correlation.go:131)
 *   sonar_xcorr_params         <- CrossCorrelation.Compute for every type, method and constructor
 *                                 (correlation.go:103-128, 131-370, 412-418, 726-774)
 *   sonar_autocorr             <- AutoCorrelation.Compute / SetParameters (correlation.go:669-690)
 *   sonar_dtw                  <- DTWAlignment.Align (algorithms/stats/dtw.go:55)
 *   sonar_dtw_params           <- NewDTWAlignmentWithParams(...).Align (dtw.go:45-52, 137-162; distance.go)
 *   sonar_dtw_quality          <- DTWAlignment.GetAlignmentQuality (dtw.go:253-286)
 *   sonar_dtw_optimize_step_pattern <- DTWAlignment.OptimizeStepPattern (dtw.go:288-311)
 *   sonar_formants             <- FormantAnalyzer.AnalyzeMultipleFrames / AnalyzeFormants
 *                                 (algorithms/speech/format.go:85-449) over LPCAnalyzer.Analyze
 *                                 (algorithms/speech/lpc.go:44-265)
 *   sonar_voice_quality        <- VoiceQualityAnalyzer.AnalyzeVoiceQuality
 *                                 (algorithms/speech/voice_quality.go:56-111)
 *   sonar_generate_fingerprint <- FingerprintGenerator.GenerateFingerprint
 *                                 (fingerprint/fingerprint.go:137)
 *   sonar_extract_speech_features <- SpeechFeatureExtractor.ExtractFeatures
 *                                 (fingerprint/extractors/speech.go:135), the extractor
 *                                 GenerateFingerprint builds for every content type
 *   sonar_align_features       <- AlignmentExtractor.ExtractAlignmentFeatures
 *                                 (fingerprint/extractors/alignment.go:139)
 *   sonar_music_alignment_features <- MusicFeatureExtractor energy + chroma
 *                                 (fingerprint/extractors/music.go:178-376)
 *   sonar_detect_from_audio / sonar_detect_content_type
 *                              <- ContentDetector.DetectFromAudio / DetectContentType
 *                                 (fingerprint/content_detector.go:31-101)
 *   sonar_gallery_* / sonar_compare / sonar_find_best_matches
 *                              <- FingerprintComparator.Compare / BatchCompare /
 *                                 FindBestMatches (fingerprint/comparison.go:133-263, 1107)
 *
 * Conventions
 *  - Every call returns SONAR_OK (0) or a negative SONAR_ERR_*; the message
 *    (same text as the Go error where one exists) is in sonar_last_error(ctx).
 *  - Buffers are owned by the caller.  With cfg->device_ptrs == 0 they are
 *    host memory and the call is synchronous; with device_ptrs == 1 they are
 *    device pointers on the ctx's device and the call is asynchronous on the
 *    ctx stream (sonar_synchronize() waits).
 *  - One ctx per OS thread / goroutine (the Go objects are not goroutine-safe
 *    either).  Several ctxs may share one device.
 */
#ifndef SONAR_GPU_H
#define SONAR_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SONAR_ABI_VERSION 4

enum {
  SONAR_OK = 0,
  SONAR_ERR_INVALID = -1,      /* bad argument (message says which)            */
  SONAR_ERR_TOO_SHORT = -2,    /* "signal too short for given window size ..."  */
  SONAR_ERR_EMPTY = -3,        /* "empty signal" / "empty sequences provided"   */
  SONAR_ERR_UNSUPPORTED = -4,  /* configuration not implemented on the GPU path */
  SONAR_ERR_DEVICE = -5,       /* HIP runtime error                             */
  SONAR_ERR_NOMEM = -6,        /* device allocation failed                      */
  SONAR_ERR_PANIC = -7         /* the Go reference panics on this input (message: Go's runtime
                                  error text); see the entry for what *out then holds */
};

/* window types: analyzers.WindowType (fingerprint/analyzers/windowing.go:13-23) */
enum {
  SONAR_WIN_HANN = 0, SONAR_WIN_HAMMING, SONAR_WIN_BLACKMAN, SONAR_WIN_BLACKMAN_HARRIS,
  SONAR_WIN_KAISER, SONAR_WIN_TUKEY, SONAR_WIN_RECTANGULAR, SONAR_WIN_BARTLETT, SONAR_WIN_WELCH
};

enum { SONAR_F32 = 0, SONAR_F64 = 1 };              /* arithmetic / element types */
enum { SONAR_FB_MEL = 0, SONAR_FB_BARK = 1 };       /* mel_scale.go / bark_scale.go */

/* sonar_fp_cfg.flags: which outputs sonar_fingerprint produces */
enum {
  SONAR_FP_MFCC = 1u << 0,      /* out->mfcc       F x n_mfcc                        */
  SONAR_FP_MAGNITUDE = 1u << 1, /* out->magnitude  F x (W/2+1)  (SpectrogramResult)  */
  SONAR_FP_SPECTRAL = 1u << 2,  /* centroid..slope, flux (F-1), low/high energy ratio */
  SONAR_FP_ZCR = 1u << 3,       /* out->zcr        F, on the pre-emphasised PCM       */
  SONAR_FP_ENERGY = 1u << 4,    /* out->energy     sonar_energy_frames(), pre-emphasised */
  SONAR_FP_COMPLEX = 1u << 5,   /* out->complex    F x (W/2+1) x 2 (re, im)  SpectrogramResult.Complex */
  SONAR_FP_PHASE = 1u << 6,     /* out->phase      F x (W/2+1), atan2(im, re) SpectrogramResult.Phase */
  SONAR_FP_GENERIC = 1u << 30   /* force the general fused kernel (A/B checks of the f32 MFCC path) */
};

typedef struct sonar_ctx sonar_ctx;

/* ---- context ---------------------------------------------------------- */
int sonar_create(int device, sonar_ctx** out);
void sonar_destroy(sonar_ctx* ctx);
const char* sonar_last_error(const sonar_ctx* ctx);
int sonar_abi_version(void);
/* Run on an external hipStream_t (e.g. torch.cuda.current_stream().cuda_stream);
 * NULL restores the ctx-owned stream. */
int sonar_set_stream(sonar_ctx* ctx, void* hip_stream);
int sonar_synchronize(sonar_ctx* ctx);
/* Average duration (ms) of the last `n` launches of the dominant kernel of
 * the last call, measured with HIP events on the stream it ran on (bench). */
int sonar_last_kernel_ms(sonar_ctx* ctx, double* ms);
int sonar_enable_kernel_timing(sonar_ctx* ctx, int on);
/* Name of the fused path-A kernel the last sonar_fingerprint call launched
 * ("mfcc_pair_kernel" or "fp_wave_kernel"; "" if none) -- diagnostics. */
const char* sonar_last_fp_kernel(sonar_ctx* ctx);
/* HIP-event durations (ms) of the kernels of the last sonar_dtw call on this
 * context: ms3[0] the band sweep (dtw_band_kernel), ms3[1] the backtrack walk,
 * ms3[2] the path decode -- diagnostics and the bench's DTW roofline. */
int sonar_dtw_last_timing(sonar_ctx* ctx, double* ms3);
/* Liveness counters of the DTW band pipeline accumulated on this context (and
 * the worker contexts of sonar_align_pairs) since the last reset: out4[0]
 * edge-poll refresh fences (an agent-scope acquire issued after 1 ms without
 * a new value from the band above), out4[1] those after which the next poll
 * found new values, out4[2] DTWs whose pipeline timed out (the call returned
 * SONAR_ERR_DEVICE with a diagnostic text in sonar_last_error), out4[3] waves
 * that timed out.  reset != 0 zeroes them after reading -- diagnostics. */
int sonar_dtw_counters(sonar_ctx* ctx, int64_t* out4, int32_t reset);
/* Frees the device and pinned host buffers this context (and its sonar_align_pairs
 * worker contexts) cache between calls; the tables and streams stay.  The next call
 * allocates what it needs again.  sonar_align_pairs' workers keep up to ~70 % of the
 * device memory that was free when it ran: trim releases it.  No Go counterpart
 * (memory management of this library). */
int sonar_trim(sonar_ctx* ctx);

/* ---- sizes (same integer rules as the Go code) ------------------------ */
/* (n - W)/H + 1, Go truncating division; <= 0 -> SONAR_ERR_TOO_SHORT
 * (fingerprint/analyzers/spectral.go:409-412) */
int64_t sonar_stft_frames(int64_t n, int32_t window_size, int32_t hop_size);
/* Energy.ComputeShortTimeEnergy frame count, 0 when n < W or W,H <= 0 (energy.go:25-31) */
int64_t sonar_energy_frames(int64_t n, int32_t window_size, int32_t hop_size);
/* extractHarmonicFeatures frame count (1024/512), speech.go:469-471 */
int64_t sonar_pitch_frames(int64_t n);

/* ---- path A: fused STFT -> |X| -> filterbank -> ln -> DCT (+ descriptors) */
typedef struct {
  int32_t window_size;     /* STFT W (FFT size)                                     */
  int32_t hop_size;        /* STFT H                                                */
  int32_t window_type;     /* SONAR_WIN_*; always {Normalize, Symmetric} like spectral.go:415 */
  int32_t sample_rate;     /* rate the algorithms see (0 reproduces GenerateFingerprint, F1) */
  /* MFCCParams (mfcc.go:27-34); <=0 fields take the Go defaults of NewMFCCWithParams */
  int32_t n_mfcc;
  int32_t n_filters;
  int32_t filterbank;      /* SONAR_FB_MEL / SONAR_FB_BARK                          */
  int32_t use_lifter;
  double low_freq;
  double high_freq;
  double lifter;
  int32_t mfcc_input_power;/* 0: Compute() is fed |X| (speech.go:257); 1: fed |X|^2 (music.go:311, F5) */
  int32_t energy_window;   /* ShortTimeEnergy frame size (extractor FeatureConfig.WindowSize) */
  int32_t energy_hop;      /* ShortTimeEnergy hop                                   */
  double preemph_alpha;    /* pre-emphasis for ZCR/energy (0.97 speech, pre_emphasis.go:116) */
  uint32_t flags;          /* SONAR_FP_*                                            */
  int32_t precision;       /* SONAR_F32 (throughput) / SONAR_F64 (parity); calls with
                              SONAR_FP_SPECTRAL always run the f64 transform          */
  int32_t pcm_dtype;       /* SONAR_F32 / SONAR_F64                                 */
  int32_t out_dtype;       /* SONAR_F32 / SONAR_F64 element type of every output    */
  int32_t device_ptrs;     /* 0: host buffers (sync); 1: device buffers (async)     */
} sonar_fp_cfg;

typedef struct {
  void* mfcc;       /* F x n_mfcc                     */
  void* magnitude;  /* F x (W/2+1)                    */
  void* centroid;   /* F each ...                     */
  void* rolloff;
  void* bandwidth;
  void* flatness;
  void* crest;
  void* slope;
  void* flux;       /* F-1                            */
  void* low_ratio;  /* F (per STFT frame)             */
  void* high_ratio; /* F                              */
  void* zcr;        /* F                              */
  void* energy;     /* sonar_energy_frames(n, ew, eh) */
  void* complex;    /* F x (W/2+1) x 2, interleaved (re, im)   (spectral.go:491) */
  void* phase;      /* F x (W/2+1)                             (spectral.go:493) */
} sonar_fp_out;

void sonar_fp_cfg_default(sonar_fp_cfg* cfg);
/* Window sizes: 128, 256, 512, 1024 and 2048 run the fused kernels (every flag); any other W up
 * to 8192 runs the generic float64 DFT path (MFCC, magnitude, complex, phase, ZCR, energy; the
 * spectral descriptors -> SONAR_ERR_UNSUPPORTED), as go-dsp's FFTReal takes any length. */
int sonar_fingerprint(sonar_ctx* ctx, const void* pcm, int64_t n, const sonar_fp_cfg* cfg,
                      sonar_fp_out* out);
/* Which transform kernel sonar_fingerprint runs for (cfg, n): pure host logic, the decision the
 * call itself makes (no device needed).  SONAR_PLAN_PAIR: mfcc_pair_kernel (float32 MFCC only,
 * W = 1024, at most SONAR_PAIR_MAX_FRAMES frames -- its frame indices are 32-bit -- and a
 * filterbank that fits its lane chunks, else the call takes fp_wave_kernel); SONAR_PLAN_WAVE:
 * fp_wave_kernel; SONAR_PLAN_DFT: stft_dft_kernel (other W); SONAR_PLAN_NONE: no transform
 * requested (ZCR / energy only).  < 0: the error code the call would return for (cfg, n). */
enum { SONAR_PLAN_NONE = 0, SONAR_PLAN_PAIR = 1, SONAR_PLAN_WAVE = 2, SONAR_PLAN_DFT = 3 };
#define SONAR_PAIR_MAX_FRAMES 2147483646LL
int32_t sonar_fp_kernel_plan(const sonar_fp_cfg* cfg, int64_t n);
/* SpectralAnalyzer.ComputeSTFTBatch (fingerprint/analyzers/spectral.go:234-285): sonar_fingerprint
 * of `count` signals with one configuration; out[i] receives signal i's outputs (sizes as for
 * sonar_fingerprint with n[i]).  count <= 0 -> SONAR_ERR_EMPTY "no signals provided"; the first
 * failing signal by index -> its code with "error processing signal i: <message>" (:276-281), and
 * nothing is launched when a signal fails ComputeSTFTWithWindow's argument checks.  The f32 MFCC
 * configuration at W = 1024 (flags == SONAR_FP_MFCC, precision / pcm_dtype / out_dtype F32) runs
 * every signal's frames in ONE mfcc_pair_kernel launch; other configurations run sonar_fingerprint
 * per signal on the ctx stream.  cfg->device_ptrs applies to every pcm[i] and out[i] buffer. */
int sonar_fingerprint_batch(sonar_ctx* ctx, const void* const* pcm, const int64_t* n, int32_t count,
                            const sonar_fp_cfg* cfg, sonar_fp_out* out);

/* ---- STFTStreamer (fingerprint/analyzers/spectral.go:287-374) ---------------------------------
 * SpectralAnalyzer.ComputeSTFTStreaming(W, H, windowType) + STFTStreamer.ProcessChunk.  The stream
 * keeps Go's buffer (the samples not yet consumed, < W for H <= W) on the device; each push appends
 * a chunk and emits every complete frame in ONE fused STFT launch over [buffer | chunk].  Rows are
 * bit-identical to one sonar_fingerprint call over the concatenated stream with the same cfg plus
 * SONAR_FP_GENERIC (the per-frame kernel; the headline pair kernel's bits depend on a frame's
 * partner, which a push may not have yet).  Frame placement is Go's, including its quirk for
 * H > W: a frame whose hop reaches past the buffered samples clears the buffer (:355-362), so the
 * rest of that skip is not carried into the next chunk. */
typedef struct sonar_stft_stream sonar_stft_stream;
/* cfg: window_size, hop_size, window_type ({Normalize, Symmetric} and Go's zero Beta / Alpha, as
 * :290-295), flags (SONAR_FP_MAGNITUDE / _PHASE / _COMPLEX -- SpectrogramFrame -- and SONAR_FP_MFCC
 * with cfg's MFCC parameters), precision, pcm_dtype, out_dtype, device_ptrs (for every push's chunk
 * and outputs).  Errors: "failed to generate window: window size must be positive: W" / "... too
 * large: W" (windowing.go:180-187); other flags -> SONAR_ERR_UNSUPPORTED. */
int sonar_stft_stream_create(sonar_ctx* ctx, const sonar_fp_cfg* cfg, sonar_stft_stream** out);
/* Frames the next push of n samples will emit: 0 for n <= 0 or while fewer than W samples are held,
 * else (buffered + n - W) / H + 1 (host arithmetic; size the outputs of the push with it). */
int64_t sonar_stft_stream_frames(const sonar_stft_stream* st, int64_t n);
/* STFTStreamer.ProcessChunk(chunk) (:322-366): n <= 0 emits nothing (Go returns nil, nil).  out's
 * requested arrays receive *frames rows (laid out as sonar_fingerprint's for that many frames).
 * H == 0 with a frame due -> SONAR_ERR_INVALID (Go's loop never advances); H < 0 -> SONAR_ERR_PANIC
 * "runtime error: slice bounds out of range [H:]" (:359).  Host buffers: synchronous; device buffers:
 * asynchronous on the ctx stream (the chunk may be reused once the stream has passed the push). */
int sonar_stft_stream_push(sonar_stft_stream* st, const void* chunk, int64_t n, sonar_fp_out* out,
                           int64_t* frames);
int64_t sonar_stft_stream_buffered(const sonar_stft_stream* st);   /* len(s.buffer) */
void sonar_stft_stream_destroy(sonar_stft_stream* st);

/* ---- PCM ingest: the decoder's f64le byte stream -> device samples.
 * Replaces Decoder.bytesToFloat64 + processFFmpegOutput's empty check (transcode/decoder.go:850-871,
 * :782-787; ffmpeg "-f f64le" at :709): nbytes is trimmed to a multiple of 8, zero samples fail with
 * SONAR_ERR_EMPTY "no audio samples decoded".  Samples keep the stream's (interleaved) order, as
 * AudioData.PCM does.  The bytes go through a ring of pinned host slots filled by host_threads
 * threads (0 = OMP_NUM_THREADS or min(16, cores)) while earlier slots DMA on the ctx stream:
 *   SONAR_INGEST_DEVICE_CONVERT  f64 crosses PCIe, a kernel rounds to f32 (if out_dtype F32)
 *   SONAR_INGEST_HOST_CONVERT    the filling threads round to f32 (half the PCIe bytes)
 * Rounding is round-to-nearest-even in both (Go float32(x)).  d_out: device buffer of
 * n_samples * (out_dtype F64 ? 8 : 4) bytes, 16-B aligned; NULL only reports *n_samples.
 * Returns once the host bytes are consumed; the device writes complete in ctx-stream order. */
#define SONAR_INGEST_DEVICE_CONVERT 0
#define SONAR_INGEST_HOST_CONVERT 1
int sonar_ingest_f64le(sonar_ctx* ctx, const void* bytes, int64_t nbytes, int32_t out_dtype, int32_t mode,
                       int32_t host_threads, void* d_out, int64_t* n_samples);
/* Decoder output straight into path A: sonar_ingest_f64le (in cfg->pcm_dtype, `mode`) into a
 * ctx-owned device buffer, then sonar_fingerprint on it; pcm_dtype F64 (the default) keeps Go's
 * []float64 samples end to end, F32 rounds them to nearest even; outputs are host buffers
 * (cfg->device_ptrs must be 0).  Replaces bytesToFloat64 + ComputeSTFTWithWindow's upload of
 * AudioData.PCM (decoder.go:850-871 -> analyzers/spectral.go:385) with one call. */
int sonar_fingerprint_f64le(sonar_ctx* ctx, const void* bytes, int64_t nbytes, int32_t mode,
                            const sonar_fp_cfg* cfg, sonar_fp_out* out);

/* ---- YIN per-frame core (frames of 1024 at hop 512, PitchDetector defaults).
 * Writes the raw YIN result per frame (pitch Hz or 0, confidence 1-cmndf or 0)
 * before the sequential octave-correction / median tracking, which the host
 * layer (sonar_generate_fingerprint) applies.  pcm is float64. ----------- */
int sonar_pitch_yin(sonar_ctx* ctx, const double* pcm, int64_t n, int32_t sample_rate,
                    double* pitch_raw, double* conf_raw, int32_t* tau, int32_t device_ptrs);

/* ---- chroma (music extractor): DC removal + pre-emphasis 0.95, frames of
 * frame_size = n / n_frames at hop, normalised symmetric Hann, |DFT|^2 folded
 * to 12 pitch classes over [80, 8000] Hz, unit-sum normalised. ----------- */
int sonar_chroma_stft(sonar_ctx* ctx, const double* pcm, int64_t n, int64_t n_frames, int32_t hop,
                      int32_t sample_rate, int32_t preprocess, double* chroma /* n_frames x 12 */,
                      int32_t device_ptrs);

/* ---- constant-Q chroma: ChromaCQT.ComputeChroma (algorithms/chroma/chroma_cqt.go:69-92) of
 * NewChromaCQT(sample_rate, min_freq, max_freq, bins_per_octave, q_factor, tuning_freq) (:43-54;
 * NewChromaCQTDefault :57-66 is 65.4, 2093.0, 12, 25.0, 440.0), float64 PCM.
 *   total_bins = int(math.Log2(max_freq / min_freq) * bins_per_octave) (:97-98),
 *   freq_k = min_freq * math.Pow(2, k / bins_per_octave) (:103),
 *   kernel_len(f) = int(q_factor * sample_rate / f), made odd, raised to 3, then capped at
 *   sample_rate / 2 (the capped value may be even); the centre is kernel_len / 2 (:147-165, :123),
 *   fft_size = nextPowerOfTwo(2 * kernel_len(freq_0)) (:107-108, :315-325),
 *   n_frames = (n - hop) / hop truncating, 1 when that is <= 0 (:169-172; a negative hop gives one
 *   frame at sample 0); frame f starts at f * hop and spans fft_size samples, zero-padded past the
 *   end of the signal (:183-188).
 * The reference passes each Gaussian-windowed complex exponential through complexToReal, which takes
 * cmplx.Abs of every tap (:139, :306-312), so kernel k is the FFT of the real sequence
 * g_k[t] = hypot(w cos(phi), w sin(phi)), w = exp(-(t - centre)^2 / (2 sigma^2)),
 * sigma = sample_rate / (2 pi freq_k / q_factor), phi = 2 pi freq_k (t - centre) / sample_rate
 * (:120-135), and the sum of frameFFT[n] * conj(K_k[n]) over all fft_size bins (:198-200) is, by
 * Parseval, fft_size * sum_{t < kernel_len_k} frame[t] g_k[t].  So
 *   cqt[f][k] = |fft_size * sum_t pcm[f hop + t] g_k[t]|                                   (:203)
 * computed as that dot product in float64 (the reference's FFT-domain sum differs from it by its
 * rounding: 1e-15 of fft_size |frame[:L_k]| |g_k|), and the fold (:213-242, :255-268):
 *   chroma_bin_k = int(math.Round(69 + 12 log2(freq_k / tuning_freq))) % 12, + 12 if negative,
 *   chroma[f][c] = sum of cqt[f][k]^2 over the bins of class c, in bin order; each frame is divided
 *   by its sum only when the sum is > 1e-10; classes no bin maps to stay 0.
 * The tap table is built on the host and cached in the context per parameter set until sonar_trim.
 * Results and errors in Go's words: n == 0 -> SONAR_OK with zero frames (Go returns nil, nil) before
 * anything else is looked at; total_bins == 0 -> SONAR_ERR_PANIC "runtime error: index out of range
 * [0] with length 0" (:107); total_bins < 0 -> SONAR_ERR_PANIC "runtime error: makeslice: len out
 * of range" (:101); hop == 0 -> SONAR_ERR_PANIC "runtime error: integer divide by zero" (:169).
 * Not reproduced (SONAR_ERR_UNSUPPORTED, the message says so): a non-finite or non-positive
 * min_freq, max_freq, q_factor or tuning_freq; bins_per_octave < 1; sample_rate < 6; a bin count or
 * tap table beyond the library's limits; non-finite PCM (the reference spreads a NaN through its
 * FFT's butterflies over the whole fft_size-sample frame span). */
/* The integer side, host only (no context, no GPU).  kernel_len and chroma_bin are optional arrays of
 * total_bins entries (call once with both NULL for the count); sum_taps = sum of kernel_len.  n == 0
 * gives n_frames = 0 whatever hop is.  Returns SONAR_OK, SONAR_ERR_PANIC or SONAR_ERR_UNSUPPORTED as
 * above (the outputs computed before the error are set: total_bins for the two bin-count panics). */
int sonar_chroma_cqt_plan(int32_t sample_rate, double min_freq, double max_freq, int32_t bins_per_octave,
                          double q_factor, double tuning_freq, int64_t n, int64_t hop,
                          int64_t* total_bins, int64_t* fft_size, int64_t* n_frames, int64_t* sum_taps,
                          int32_t* kernel_len /* [total_bins] or NULL */,
                          int32_t* chroma_bin /* [total_bins] or NULL */);
/* ComputeChroma.  Host pointers: synchronous.  Device pointers (device_ptrs): pcm, chroma and cqt are
 * device addresses, a null cqt goes to library scratch; the call returns after its kernels have run
 * (the non-finite scan's answer is read first). */
int sonar_chroma_cqt(sonar_ctx* ctx, const double* pcm, int64_t n, int64_t hop, int32_t sample_rate,
                     double min_freq, double max_freq, int32_t bins_per_octave, double q_factor,
                     double tuning_freq, double* chroma /* n_frames x 12 */,
                     double* cqt /* n_frames x total_bins, may be NULL */, int32_t device_ptrs);

/* ---- chroma sequence similarity (float64) --------------------------------
 * ChromaSequenceSimilarity.ComputeSimilarity (algorithms/chroma/chroma_similarity.go:86-538) over
 * ChromaVectorAnalyzer.Distance / Similarity / CircularShift (chroma_vector.go:145-216) and the frame
 * metrics of stats/distance.go (:28-108, :247-294, :341-369).  q and r are nq x dim and nr x dim
 * row-major chroma frames, dim >= 1 (12, 24 and 36 are the reference's sizes).  Every array pointer
 * of a call is of one kind, host or device; the library tells which from q (r when nq == 0).
 * Frame metric: Distance is the metric's DistanceFunc, any value outside 0..6 is Euclidean.
 * Similarity is 1 - d/2 for Cosine and Pearson and exp(-d) for every other value.  Pearson is
 * 1 - |corr|; Cosine is 1 when a norm is 0; KL, JS and Hellinger normalise each frame to a
 * probability vector first (positive values only, an all-non-positive frame becomes uniform), and
 * JS normalises its normalised arguments a second time inside KLDivergenceFunc (:276, :250).
 * CircularShift: value k of the shifted query frame is q[(k + shift) % dim].
 * Never read by the reference, so not carried here: FrameStackSize, FrameStackStride,
 * NormalizeSimilarity, ComputationTime. */
#define SONAR_CHROMA_SIM_DIRECT 0
#define SONAR_CHROMA_SIM_BINARY 1
#define SONAR_CHROMA_SIM_SMITH_WATERMAN 2
#define SONAR_CHROMA_SIM_DTW 3
#define SONAR_CHROMA_SIM_QMAX 4
#define SONAR_CHROMA_SIM_OTI 5
#define SONAR_CHROMA_DIST_EUCLIDEAN 0
#define SONAR_CHROMA_DIST_MANHATTAN 1
#define SONAR_CHROMA_DIST_COSINE 2
#define SONAR_CHROMA_DIST_PEARSON 3
#define SONAR_CHROMA_DIST_KL 4
#define SONAR_CHROMA_DIST_JS 5
#define SONAR_CHROMA_DIST_HELLINGER 6
/* ChromaVectorAnalyzer.Distance (as_similarity = 0) or Similarity of CircularShift(q_i, shift) and
 * r_j for every pair: out[i * nr + j].  shift < 0 is Go's index panic (SONAR_ERR_PANIC). */
int sonar_chroma_frame_matrix(sonar_ctx* ctx, const double* q, int64_t nq, const double* r, int64_t nr,
                              int32_t dim, int32_t metric, int32_t shift, int32_t as_similarity, double* out);
/* ComputeSimilarity.  method outside 0..5 runs Direct, as the reference's default case does.
 *   Direct  matrix = Similarity(q_i, r_j); overall = the sum over the matrix / (nq nr) (the reference
 *           adds serially in row-major order, this adds as a tree: they differ by at most
 *           nq nr 2^-53 mean|sim|).  With transposition_invariant the query is shifted by
 *           findBestTransposition's shift (:450-479: step = int(max(1, nq / 50)) for rows and columns,
 *           12 sampled means added in Go's order, the first strictly greater than the running best
 *           from 0.0 wins, NaN never) and overall = that best mean.
 *   Binary  Direct's matrix > binary_threshold as 1.0 / 0.0; overall = matches / (nq nr).
 *   QMax    Direct's matrix; overall = max(0, largest non-NaN entry) (every cell lies on one diagonal).
 *   OTI     per shift 0..11 the similarities of j in [max(0, i - R), min(nr, i + R + 1)), R =
 *           oti_radius, the rest 0, added in Go's order; avg = total / (nq nr), the full grid; the
 *           first avg strictly greater than the running best from 0.0 wins.  If none does the matrix
 *           is nil (*matrix_is_nil = 1, matrix untouched), overall 0, transposition 0.  Ignores
 *           transposition_invariant.
 *   Smith-Waterman  S = max(0, max(S[i-1][j-1] + sim, max(S[i-1][j] - 0.1, S[i][j-1] - 0.1))) with
 *           math.Max; matrix = S[1:][1:], the scores; the path walks back from the first row-major
 *           maximum > 0 while S > 0, by the codes of `switch maxVal {case match, delete, insert}`
 *           (float equality, 0 when none is equal); points (i - 1, j - 1, S[i][j]); overall =
 *           maxScore / len(path), 0 / 0 = NaN when nothing scores.  No transposition.
 *   DTW     cost = Distance; acc[0][0] = cost[0][0], first row and column cumulative, interior
 *           cost + math.Min(up, math.Min(left, diag)); with dtw_band_radius R > 0 a column j >= 1 with
 *           |j - int(float64(j nq) / float64(nr))| > R is skipped in every row i >= 1 and stays 0
 *           (never with nq == nr); the path walks back from the end with <=, diagonal, up, left, and
 *           does not hold (0, 0); points (i, j, acc[i][j]); overall = exp(-acc[nq-1][nr-1] /
 *           len(path)) (1 x 1: a division by 0); matrix = exp(-cost).
 * matrix (nq x nr) may be NULL: Direct, Binary, QMax and OTI then reduce without storing it and
 * take any size; Smith-Waterman and DTW keep their DP matrix in device scratch and take nq nr <= 2^30
 * cells (SONAR_ERR_UNSUPPORTED beyond).  path_q, path_r, path_score (nq + nr entries each, any may be
 * NULL) and *path_len are written by Smith-Waterman and DTW only.
 * Empty input in Go's words: DTW -> SONAR_ERR_PANIC "runtime error: index out of range [0] with length
 * 0"; the others return SONAR_OK and launch nothing: overall NaN (Direct, Binary, Smith-Waterman),
 * 0 (QMax, Direct with transposition_invariant), OTI nil. */
int sonar_chroma_similarity(sonar_ctx* ctx, const double* q, int64_t nq, const double* r, int64_t nr,
                            int32_t dim, int32_t method, int32_t metric, double binary_threshold,
                            int32_t oti_radius, int32_t dtw_band_radius, int32_t transposition_invariant,
                            double* matrix /* nq*nr, nullable */, int32_t* matrix_is_nil, double* overall,
                            int32_t* best_transposition, int32_t* path_q, int32_t* path_r,
                            double* path_score /* nq+nr each, nullable */, int64_t* path_len);
/* The integer side, host only (no context, no GPU): findBestTransposition's step and its pairs per
 * shift, OTI's computed cells per shift, the columns j >= 1 the DTW band rule skips (0 when
 * dtw_band_radius <= 0 or nq < 2), and the device scratch of a host-pointer call with a matrix. */
int sonar_chroma_similarity_plan(int32_t method, int64_t nq, int64_t nr, int32_t dim, int32_t oti_radius,
                                 int32_t dtw_band_radius, int64_t* sample_step, int64_t* sampled_pairs,
                                 int64_t* oti_cells, int64_t* dtw_skipped_columns, int64_t* scratch_bytes);
/* HIP-event times (ms) of the last chroma similarity or frame matrix call on this context: ms4[0] the
 * frame matrix (with the row preparation), ms4[1] the ordered sums, ms4[2] the Smith-Waterman / DTW
 * fill, ms4[3] the traceback; 0 for a family the call did not run -- diagnostics. */
int sonar_chroma_similarity_last_timing(sonar_ctx* ctx, double* ms4);

/* ---- spectral peaks and the harmonic pitch class profile (float64) --------
 * SpectralPeaks.DetectPeaks (algorithms/harmonic/spectral_peaks.go:36-100) on each of F rows of K
 * magnitudes, for NewSpectralPeaks(sample_rate, min_height, min_distance_hz, max_peaks) and
 * DetectPeaks(row, window_size):
 *   a candidate is a bin 1 <= i <= K - 2 with row[i] > row[i-1], row[i] > row[i+1] and row[i] >=
 *   min_height (a NaN makes every comparison false; +Inf is a magnitude like any other);
 *   min_distance_bins = max(int(min_distance_hz / (sample_rate / window_size)), 1).  Strict local
 *   maxima are 2 bins apart, so the distance rule acts from 3 on.  The reference's loop (:56-73) stops
 *   at the first kept peak closer than that, replaces it when the candidate is strictly larger and
 *   drops the candidate otherwise; kept peaks stay pairwise at least min_distance_bins apart, so that
 *   peak is always the last kept one: a serial greedy, not a cluster maximum.
 *   The kept peaks are sorted by magnitude, descending (:90-92, sort.Slice: Go leaves the order of
 *   equal magnitudes open; here equal magnitudes come in ascending bin order) and cut to max_peaks.
 *   frequency = float64(bin) * (sample_rate / window_size).  Phase (0) and Harmonic (-1) are constants
 *   and are not returned.
 * Outputs: count[F]; bin, magnitude and frequency (frequency may be NULL) have F rows of
 * P = sonar_spectral_peaks_width(K, max_peaks) = min(max_peaks, max((K - 1) / 2, 0)) slots, the slots
 * past count[f] are 0.  F == 0 or K == 0 -> SONAR_OK, zero counts (Go returns before it looks at
 * anything else); max_peaks < 0 -> SONAR_ERR_PANIC "runtime error: slice bounds out of range [:-1]"
 * (:95-97).  Not reproduced (SONAR_ERR_UNSUPPORTED): sample_rate or window_size <= 0; K > 8192. */
int64_t sonar_spectral_peaks_width(int64_t K, int64_t max_peaks);
int sonar_spectral_peaks(sonar_ctx* ctx, const double* mag /* F x K */, int64_t F, int32_t K, int32_t window_size,
                         int32_t sample_rate, double min_height, double min_distance_hz, int32_t max_peaks,
                         int32_t* count /* F */, int32_t* bin /* F x P */, double* magnitude /* F x P */,
                         double* frequency /* F x P or NULL */, int32_t device_ptrs);

/* HPCPParams (algorithms/chroma/hpcp.go:11-26).  weight_type: Go's strings "none", "cosine",
 * "squared_cosine"; any other value is "none", as the reference's default cases are. */
#define SONAR_HPCP_WEIGHT_NONE 0
#define SONAR_HPCP_WEIGHT_COSINE 1
#define SONAR_HPCP_WEIGHT_SQUARED_COSINE 2
typedef struct sonar_hpcp_params {
  int32_t size;               /* Size: bins of the profile (12, 24, 36) */
  int32_t harmonics_removal;  /* HarmonicsRemoval: removes nothing, only switches the harmonic additions off */
  int32_t normalized;         /* Normalized: common.Normalizer(Energy) */
  int32_t weight_type;        /* WeightType */
  int32_t max_shifted;        /* MaxShifted */
  int32_t non_linear;         /* NonLinear: log(1 + x) on positive bins */
  int32_t band_preset;        /* BandPreset: peaks below split_freq weigh double */
  int32_t max_harmonics;      /* MaxHarmonics: harmonics 2..max_harmonics are added */
  double reference_freq;      /* ReferenceFreq */
  double window_size;         /* WindowSize, semitones */
  double min_freq;            /* MinFreq */
  double max_freq;            /* MaxFreq */
  double split_freq;          /* SplitFreq */
  double harmonics_strength;  /* HarmonicsStrength */
} sonar_hpcp_params;
/* NewHPCP's values (hpcp.go:54-75): 12, 440, no removal, normalized, cosine, 1.0, not shifted, linear,
 * band preset, 40, 5000, 500, 1.0, 0 harmonics. */
void sonar_hpcp_params_default(sonar_hpcp_params* p);

/* HPCP.ComputeFromSpectrum(row, window_size) (hpcp.go:205-221) of NewHPCPWithParams(sample_rate,
 * params) on each of F rows of K magnitudes: DetectPeaks with the reference's fixed (1e-5, 20.0 Hz,
 * 60), then ComputeFromSpectralPeaks (:147-202).  K is the row length whatever window_size is (the
 * chord detector passes all window_size bins; the mirror half is cut by max_freq only).
 * Per peak, in sorted order: skipped when f < min_freq || f > max_freq; pc = mod(69 + 12
 * log2(f / reference_freq), 12), + 12 if negative, times size / 12; weight = magnitude, doubled when
 * band_preset and f < split_freq; addPeakContribution (:254-281) over the unwrapped bins
 * floor(pc - w/2) .. ceil(pc + w/2), w = window_size size / 12, each within w/2 (distance folded at
 * size/2) adding weight * window_weight to its wrapped bin; with max_harmonics > 0 and no
 * harmonics_removal the harmonics h = 2.. of f h, weight magnitude * (harmonics_strength / h), until
 * the first above max_freq.  Then non_linear, normalized (divided by sqrt(sum x^2) only when sum x^2
 * >= 1e-10), max_shifted (the identity up to rounding), energy = sqrt(sum x^2),
 * entropy = -sum p log2 p over the positive bins (0 when the sum is 0).
 * A peak's frequency is bin * sample_rate / window_size, so everything transcendental is a function
 * of the bin: the library builds the contribution table of sonar_hpcp_table on the host, caches it in
 * the context per parameter set until sonar_trim, and the device adds (magnitude * factor) *
 * window_weight, two roundings each, in the reference's program order.
 * hpcp is F x size; energy and entropy (F each) may be NULL.
 * size < 0 -> SONAR_ERR_PANIC "runtime error: makeslice: len out of range"; size == 0 -> SONAR_OK, an
 * empty profile, energy 0, entropy 0.  Not reproduced (SONAR_ERR_UNSUPPORTED, the message says which):
 * a non-finite or non-positive reference_freq; a non-finite or negative window_size; sample_rate or
 * the STFT window_size <= 0; size > 120, max_harmonics > 16, K > 8192, window_size > 12 semitones, a
 * table of more than 2^24 entries.  Non-finite magnitudes are no error: they follow IEEE comparisons
 * as in Go. */
int sonar_hpcp_from_spectrum(sonar_ctx* ctx, const double* mag /* F x K */, int64_t F, int32_t K,
                             int32_t window_size, int32_t sample_rate, const sonar_hpcp_params* params,
                             double* hpcp /* F x size */, double* energy /* F or NULL */,
                             double* entropy /* F or NULL */, int32_t device_ptrs);
/* The contribution table, host only (no context, no GPU), in CSR form: row i (row_start[i] ..
 * row_start[i+1]) holds what a peak at bin i adds, in the reference's program order: the main
 * contribution's bins ascending, then harmonic 2's, and so on.  Entry e adds (magnitude * factor[e]) *
 * window_weight[e] to hpcp[wrapped_bin[e]]; factor is 1, 2 (band preset below split_freq) or
 * harmonics_strength / h.  Rows of bins outside [min_freq, max_freq], and of bins 0 and K - 1 (never
 * peaks), are empty.  Call with NULL arrays for *n_entries, then with row_start[K + 1] and three
 * arrays of *n_entries.  Errors as sonar_hpcp_from_spectrum's (no message: there is no context). */
int sonar_hpcp_table(int32_t sample_rate, int32_t window_size, int32_t K, const sonar_hpcp_params* params,
                     int64_t* n_entries, int64_t* row_start /* K + 1 or NULL */,
                     int32_t* wrapped_bin /* n_entries or NULL */, double* factor, double* window_weight);
/* The frames of sonar_hpcp on n samples and how it splits them, host only: chunk_frames rows of
 * window_size / 2 + 1 doubles fill about 64 MiB, n_chunks = ceil(frames / chunk_frames).  Errors are
 * sonar_fingerprint's (empty, non-positive sizes, too short, a window above its limits). */
int sonar_hpcp_plan(int64_t n, int32_t window_size, int32_t hop_size, int64_t* frames, int64_t* chunk_frames,
                    int64_t* n_chunks);
/* SpectralAnalyzer.ComputeSTFTWithWindow's magnitude rows (as sonar_fingerprint with
 * SONAR_FP_MAGNITUDE, float64 PCM, the float64 transform) -> ComputeFromSpectrum per frame, K =
 * window_size / 2 + 1.  The magnitude rows live in a bounded device scratch, chunk_frames at a time
 * (sonar_hpcp_plan); chunks partition the frames and share no state.  The window sizes and errors are
 * sonar_fingerprint's (too short: SONAR_ERR_TOO_SHORT "signal too short for given window size and
 * hop size"), then sonar_hpcp_from_spectrum's.  hpcp is frames x size. */
int sonar_hpcp(sonar_ctx* ctx, const double* pcm, int64_t n, int32_t sample_rate, int32_t window_size,
               int32_t hop_size, int32_t window_type, const sonar_hpcp_params* params, double* hpcp,
               double* energy /* frames or NULL */, double* entropy /* frames or NULL */, int32_t device_ptrs);

/* ---- harmonic product spectrum (float64) -----------------------------------
 * HarmonicProduct (algorithms/harmonic/harmonic_product.go) of NewHarmonicProduct(sample_rate,
 * num_harmonics, min_f0, max_f0) on each of F rows of K magnitudes; window_size is the reference's
 * signalLength and, as in sonar_hpcp_from_spectrum, K is the row length whatever window_size is.
 *   ComputeHPS (:32-58): p[i] = row[i] * row[i]; hps = p; for h = 2 .. num_harmonics in order, with
 *   L = K / h: nothing when L == 0 (h > K: downsampleSpectrum returns an empty slice),
 *   else hps[i] *= (i < L ? p[i * h] : 0.0) for every i < K.  The multiplication by 0.0 happens, so an
 *   Inf or NaN there gives NaN (F63).  One rounding per product, left to right; subnormal products
 *   survive.  num_harmonics <= 1 leaves the power spectrum.
 *   ComputeHPSWithInterpolation (:163-191), interpolated != 0: hps[i] *= interpolateSpectrum(p,
 *   float64(i) / float64(h)) for every bin and every h, h > K included; interpolateSpectrum (:194-209)
 *   is 0.0 at index >= float64(K - 1), else p[l] + frac * (p[l+1] - p[l]), unfused.
 *   findF0Peak (:127-160): sonar_hps_bins' range, a strict > against 0.0 in ascending bin order: the
 *   lowest bin among equal maxima, never a NaN, bin 0 when nothing in the range is above 0 or the
 *   range is empty (the local-maximum check after the loop changes nothing, F65).
 *   f0 = float64(bin) * (float64(sample_rate) / float64(window_size)), 0 for bin 0 (:84-90).
 *   ComputeHarmonicStrength (:224-247) at that f0 and window_size: for h = 1 .. num_harmonics,
 *   harmonicBin = (f0 * float64(h)) / freqResolution as written (bin * h only up to rounding, F66),
 *   0 at harmonicBin >= float64(K), else interpolateSpectrum on the magnitudes.
 *   ComputeHarmonicity (:250-273), the confidence of EstimateF0WithConfidence (:276-298): the sum of
 *   strength^2 in harmonic order over the sum of row[i] * row[i] in bin order, 0 when that is 0 or
 *   num_harmonics is 0.
 * Outputs: f0_bin[F] and f0[F] are required; confidence[F], strengths[F x max(num_harmonics, 0)] and
 * hps[F x K] (the spectrum the peak search ran on) may be NULL.  Rows with f0 == 0 get confidence 0
 * and zero strengths.  F == 0 or K == 0 -> SONAR_OK, zeros where there is anything to write.
 * Not reproduced (SONAR_ERR_UNSUPPORTED, the message says which): sample_rate or window_size <= 0;
 * min_f0 or max_f0 non-finite or negative, or one whose quotient by the frequency resolution does not
 * fit an int32 (Go's conversion is implementation-defined there); K > 8192; num_harmonics > 64;
 * num_harmonics < 0 when confidence or strengths is asked for (Go's make panics, on rows with f0 > 0
 * only).  Non-finite magnitudes are no error: they follow IEEE arithmetic as in Go. */
int sonar_hps_from_spectrum(sonar_ctx* ctx, const double* mag /* F x K */, int64_t F, int32_t K,
                            int32_t window_size, int32_t sample_rate, int32_t num_harmonics,
                            double min_f0, double max_f0, int32_t interpolated,
                            int32_t* f0_bin /* F */, double* f0 /* F */, double* confidence /* F or NULL */,
                            double* strengths /* F x max(num_harmonics,0) or NULL */,
                            double* hps /* F x K or NULL */, int32_t device_ptrs);
/* findF0Peak's scan range for rows of K bins, host only (no context, no GPU): min_bin = int(min_f0 /
 * freqResolution) raised to 1, max_bin = int(max_f0 / freqResolution) lowered to K - 1, both
 * conversions truncating (:128-139).  min_bin > max_bin is an empty range (K == 0: max_bin -1).
 * K < 0 -> SONAR_ERR_INVALID; the range errors of sonar_hps_from_spectrum (no message). */
int sonar_hps_bins(int32_t sample_rate, int32_t window_size, int32_t K, double min_f0, double max_f0,
                   int32_t* min_bin, int32_t* max_bin);
/* GetOptimalNumHarmonics (:301-314), host only: m = int((float64(sample_rate) / 2) / min_f0); 5 when
 * m > 7, m - 1 when m > 3, else 2.  SONAR_ERR_UNSUPPORTED: sample_rate <= 0, min_f0 non-finite or
 * negative, or a quotient that does not fit an int32 (min_f0 == 0). */
int sonar_hps_optimal_harmonics(int32_t sample_rate, double min_f0, int32_t* num_harmonics);
/* The frames of sonar_hps on n samples and how it splits them, host only: sonar_hpcp_plan's values
 * and errors, and SONAR_ERR_UNSUPPORTED for window_size < 2. */
int sonar_hps_plan(int64_t n, int32_t window_size, int32_t hop_size, int64_t* frames,
                   int64_t* chunk_frames, int64_t* n_chunks);
/* EstimateF0WithConfidence (:276-298) on every frame of window_size samples at hop_size, (n -
 * window_size) / hop_size + 1 of them: applyWindow (:212-221), 0.5 (1 - cos(2 pi i / (N - 1))), symmetric
 * and not energy-normalised, the float64 transform's magnitudes with K = window_size / 2 + 1, then
 * sonar_hps_from_spectrum's row estimate with signalLength = window_size.  The rows go through a
 * bounded device scratch, chunk_frames at a time (sonar_hps_plan), as in sonar_hpcp.  magnitude
 * (frames x K or NULL) receives the rows; frames (host memory in both modes, or NULL) the frame count.
 * The window sizes and errors are sonar_hpcp's (the fused transform at 128-2048, the DFT path for
 * other sizes up to 8192); window_size < 2 -> SONAR_ERR_UNSUPPORTED (the window divides by N - 1);
 * then sonar_hps_from_spectrum's. */
int sonar_hps(sonar_ctx* ctx, const double* pcm, int64_t n, int32_t sample_rate, int32_t window_size,
              int32_t hop_size, int32_t num_harmonics, double min_f0, double max_f0, int32_t interpolated,
              int32_t* f0_bin, double* f0, double* confidence /* or NULL */, double* strengths /* or NULL */,
              double* magnitude /* frames x K or NULL */, int64_t* frames /* host, or NULL */,
              int32_t device_ptrs);

/* ---- onsets and tempo (float64) ---------------------------------------------
 * OnsetDetection (algorithms/temporal/onset_detection.go) and TempoEstimation (tempo_estimation.go)
 * over SpectralFlux (algorithms/spectral/spectral_flux.go) and Envelope.ComputeRMS (temporal/envelope.go).
 * Every sum keeps the reference's order and nothing is fused, so the curves are the reference's bit for
 * bit and the decisions made on them (strict maxima, thresholds, votes) are the reference's.  Frame
 * indices, onset samples and counts are int64.  A count, a frame count and a curve length are written
 * to host memory whatever device_ptrs says; arrays (and sonar_tempo_autocorrelation's two scalars)
 * follow device_ptrs.  DESIGN.md F70-F79 list what the reference does that a reader would not guess.
 * Not reproduced (SONAR_ERR_UNSUPPORTED, the message says which): sample_rate <= 0; hop_size <= 0 where
 * a minimum interval is converted; a min_interval whose frame count is NaN or does not fit an int32
 * (Go's conversion is implementation-defined there); rows of more than 8192 bins. */
#define SONAR_ONSET_WINDOW 1024        /* DetectOnsets' windowSize (onset_detection.go:32)       */
#define SONAR_ONSET_HOP 512            /* ... and hopSize (:33)                                   */
#define SONAR_ONSET_ENERGY_FRAME 512   /* DetectOnsetsEnergy's frameSize (:65)                    */
#define SONAR_ONSET_ENERGY_HOP 256     /* ... and hopSize (:66)                                   */
/* SpectralFlux.Compute (spectral_flux.go:17-36), or ComputeAllChanges (:39-56) when all_changes != 0, on
 * F rows of K magnitudes: flux[t] = sqrt(sum over bins, ascending, of d * d), d = mag[t+1][f] - mag[t][f];
 * Compute adds a term only when d > 0, so a NaN difference adds nothing there.  max(F - 1, 0) values;
 * F < 2 writes nothing. */
int sonar_spectral_flux(sonar_ctx* ctx, const double* mag /* F x K */, int64_t F, int32_t K, int32_t all_changes,
                        double* flux /* max(F-1,0) */, int32_t device_ptrs);
/* len(Envelope.ComputeRMS(signal of n, frame_size, hop_size)), host only: (n - frame_size) / hop_size + 1,
 * and 0 when n < frame_size, frame_size <= 0 or hop_size <= 0 (envelope.go:19-23). */
int64_t sonar_rms_envelope_frames(int64_t n, int32_t frame_size, int32_t hop_size);
/* Envelope.ComputeRMS (envelope.go:18-43): env[i] = sqrt((sum of x[j] * x[j] over the frame, in sample
 * order) / float64(frame_size)).  frames (host, or NULL) receives sonar_rms_envelope_frames' value; an
 * empty result is SONAR_OK. */
int sonar_rms_envelope(sonar_ctx* ctx, const double* pcm, int64_t n, int32_t frame_size, int32_t hop_size,
                       double* env, int64_t* frames /* host, or NULL */, int32_t device_ptrs);
/* The most peaks findFluxPeaks can return on n values, host only: max((n - 1) / 2, 0) (strict local
 * maxima inside 1 .. n - 2 are two apart). */
int64_t sonar_onset_peaks_width(int64_t n);
/* findFluxPeaks' minIntervalFrames, host only: int(min_interval * float64(sample_rate) /
 * float64(hop_size)), truncating (:103). */
int sonar_onset_min_interval_frames(double min_interval, int32_t sample_rate, int32_t hop_size, int32_t* frames);
/* findFluxPeaks (onset_detection.go:97-120) on any curve of n values: index i in 1 .. n - 2 is kept when
 * v[i] > v[i-1], v[i] > v[i+1], v[i] >= threshold and i - last >= minIntervalFrames, where last is the
 * index kept before (-minIntervalFrames at the start): a serial greedy over the strict local maxima.  A
 * NaN value or threshold makes its comparisons false; a non-positive minIntervalFrames never rejects.
 * index has sonar_onset_peaks_width(n) slots, the kept indices ascending, the slots past count 0.
 * n < 3 -> SONAR_OK, count 0, before anything else is looked at. */
int sonar_onset_peaks(sonar_ctx* ctx, const double* curve, int64_t n, double threshold, double min_interval,
                      int32_t hop_size, int32_t sample_rate, int64_t* index /* width */,
                      int64_t* count /* host */, int32_t device_ptrs);
/* AdaptiveThreshold (:200-222): mean + 2 * population standard deviation, two passes in index order;
 * 0 for n == 0. */
int sonar_onset_adaptive_threshold(sonar_ctx* ctx, const double* curve, int64_t n, double* value,
                                   int32_t device_ptrs);
/* DetectOnsets (:26-56): the magnitudes of the STFT with no window at all (a nil window, stft.go:112),
 * SpectralFlux.Compute over them, findFluxPeaks on the flux, onset sample = index in the flux array *
 * hop_size (flux index i compares frames i and i + 1 and is reported as i).
 * window_size / hop_size 0 are the reference's SONAR_ONSET_WINDOW / SONAR_ONSET_HOP; other values are
 * the same algorithm on another grid, with sonar_hpcp's window sizes.  The rows go through the
 * bounded device scratch of sonar_hpcp, chunk_frames at a time (sonar_hpcp_plan), the last row of a
 * chunk carried into the next so that the flux at a seam is the whole spectrogram's.
 * onsets has sonar_onset_peaks_width(frames - 1) slots (slots past count 0); flux (frames - 1 values) and
 * magnitude (frames x K) may be NULL; frames (host, or NULL) receives the frame count.
 * n == 0 -> SONAR_OK and nothing (:27-29); then sonar_fingerprint's errors (n <= window_size - hop_size:
 * SONAR_ERR_TOO_SHORT "signal too short for given window size and hop size"; Go's truncating frame
 * count gives window_size - hop_size < n < window_size one frame, left all zero); one
 * frame -> no flux, no onsets, SONAR_OK. */
int sonar_onsets_flux(sonar_ctx* ctx, const double* pcm, int64_t n, int32_t sample_rate, int32_t window_size,
                      int32_t hop_size, double threshold, double min_interval, int64_t* onsets,
                      int64_t* count /* host */, double* flux /* or NULL */,
                      double* magnitude /* frames x K or NULL */, int64_t* frames /* host, or NULL */,
                      int32_t device_ptrs);
/* DetectOnsetsEnergy (:59-94): ComputeRMS at frame_size / hop_size (0: SONAR_ONSET_ENERGY_FRAME /
 * SONAR_ONSET_ENERGY_HOP), energyDiff[i] = env[i+1] - env[i] when that is > 0 and else 0 (a NaN
 * difference gives 0), findFluxPeaks, onset sample = i * hop_size.  curve (the energyDiff, n_curve =
 * max(frames - 1, 0) values, or NULL); onsets has sonar_onset_peaks_width(n_curve) slots.  A signal
 * shorter than a frame gives nothing and no error. */
int sonar_onsets_energy(sonar_ctx* ctx, const double* pcm, int64_t n, int32_t sample_rate, int32_t frame_size,
                        int32_t hop_size, double threshold, double min_interval, int64_t* onsets,
                        int64_t* count /* host */, double* curve /* or NULL */, int64_t* n_curve /* host, or NULL */,
                        int32_t device_ptrs);
/* The slots sonar_onsets_complex needs for n samples, host only: the two detectors' widths added. */
int64_t sonar_onsets_complex_width(int64_t n);
/* DetectOnsetsComplex (:123-146): DetectOnsets at threshold 0.3 and DetectOnsetsEnergy at 0.1, both with
 * a 0.05 s minimum interval, concatenated, sorted ascending, and a value dropped when it lies within
 * int(0.05 * float64(sample_rate)) samples of one already kept (combineOnsets :149-182).  density (host,
 * or NULL) is ComputeOnsetDensity (:185-197): count / (n / sample_rate), 0 when n == 0.  The flux
 * detector's error ends the call even where the energy detector would have run (:135-137). */
int sonar_onsets_complex(sonar_ctx* ctx, const double* pcm, int64_t n, int32_t sample_rate, int64_t* onsets,
                         int64_t* count /* host */, double* density /* host, or NULL */, int32_t device_ptrs);
/* EstimateTempo's tail (tempo_estimation.go:33-47) and findTempoFromIntervals (:77-118) over a list of
 * onset samples, host only: intervals between consecutive onsets in seconds; one strictly inside
 * (0.2, 2.0) votes for the first bin of {60, 70, ..., 180, 200} nearest to 60 / interval when that
 * distance is strictly below 10; the most voted bin wins, the lowest of equals; 120 when nothing voted,
 * 0 with fewer than two onsets.  bin_counts (14 values, or NULL) receives the votes. */
int sonar_tempo_from_onsets(const int64_t* onsets, int64_t count, int32_t sample_rate, double* tempo,
                            int32_t* bin_counts /* 14, or NULL */);
/* EstimateTempoAutocorrelation's integer side, host only: frame_size = int(0.1 * float64(sample_rate)),
 * hop_size = frame_size / 4, the envelope's length, n_autocorr = envelope_len / 2 (0 when the envelope
 * has fewer than 10 values, :62) and, when n_autocorr >= 10, the search's lag range after its clamps
 * (:166-174). */
int sonar_tempo_autocorr_plan(int64_t n, int32_t sample_rate, int32_t* frame_size, int32_t* hop_size,
                              int64_t* envelope_len, int64_t* n_autocorr, int64_t* min_lag, int64_t* max_lag);
/* EstimateTempoAutocorrelation (:51-74): the RMS envelope e at the plan's frame and hop;
 * calculateAutocorrelation (:121-150), ac[lag] = (sum over ascending i of e[i] * e[i+lag]) / float64(len -
 * lag) for lag < len / 2, then the loop `ac[i] /= ac[0]` from i = 0 when ac[0] > 0, which makes ac[0] its
 * own quotient first and divides every other lag by that: the curve stays unnormalised;
 * findTempoFromAutocorrelation (:153-201), the highest strict local maximum above 0.0 inside the lag
 * range, the first of equals, tempo = 60 / (float64(lag) * (float64(hop) / float64(sample_rate))), 120
 * with no maximum, 0 when the envelope has fewer than 10 values or the curve fewer than 10 lags.
 * autocorr == NULL: only lag 0 and the lags the search reads are computed.  With a buffer of
 * n_autocorr values (sonar_tempo_autocorr_plan) the whole curve is computed as well; tempo and best_lag
 * are the same either way.  tempo and best_lag (or NULL) follow device_ptrs; n_autocorr is host. */
int sonar_tempo_autocorrelation(sonar_ctx* ctx, const double* pcm, int64_t n, int32_t sample_rate, double* tempo,
                                int64_t* best_lag, double* autocorr /* n_autocorr, or NULL */,
                                int64_t* n_autocorr /* host, or NULL */, int32_t device_ptrs);
/* ClassifyTempoCategory (:220-232): cut at 60 / 90 / 120 / 150 */
enum {
  SONAR_TEMPO_VERY_SLOW = 0, SONAR_TEMPO_SLOW, SONAR_TEMPO_MODERATE, SONAR_TEMPO_FAST, SONAR_TEMPO_VERY_FAST
};
int32_t sonar_tempo_category(double tempo);
/* "very_slow", "slow", "moderate", "fast", "very_fast"; "" for anything else */
const char* sonar_tempo_category_name(int32_t category);
typedef struct sonar_tempo_result {
  double onset_tempo;      /* EstimateTempo; 0 when its error was dropped (see onset_error)         */
  double autocorr_tempo;   /* EstimateTempoAutocorrelation                                         */
  double tempo;            /* EstimateTempoRange: (onset_tempo + autocorr_tempo) / 2               */
  double confidence;       /* math.Max(0, 1 - difference / 50)                                     */
  double difference;       /* |onset_tempo - autocorr_tempo|                                       */
  int64_t onset_count;     /* len(DetectOnsetsComplex)                                             */
  int64_t best_lag;        /* the autocorrelation's lag, 0 when there was none                     */
  int32_t category;        /* SONAR_TEMPO_* of tempo                                               */
  int32_t onset_error;     /* SONAR_OK, or the SONAR_ERR_TOO_SHORT EstimateTempoRange drops (:206) */
} sonar_tempo_result;
/* EstimateTempo (:22-48), EstimateTempoAutocorrelation, EstimateTempoRange (:204-217) and
 * ClassifyTempoCategory of the average, with the samples staged once.  result is host memory;
 * device_ptrs speaks of pcm.  n == 0 is no error: both tempos are 0 and the confidence 1. */
int sonar_tempo(sonar_ctx* ctx, const double* pcm, int64_t n, int32_t sample_rate, sonar_tempo_result* result,
                int32_t device_ptrs);

/* ---- key estimation over a chromagram (float64) ----------------------------
 * KeyEstimator (algorithms/tonal/key_estimation.go) on F rows of dim chroma values, for example the
 * profile sonar_hpcp leaves on the device.  The entries are stateless: keyHistory, which the
 * reference grows on every internal EstimateKey, is the last 20 first candidates of the per-frame
 * output and is left to the caller.
 *
 * EstimateKey (:196-233) of one row:
 *   preprocessChroma (:273-297): when dim != hpcp_size, resizeChromaVector (:464-485): entry i takes
 *   row[int(float64(i) * (float64(dim) / float64(hpcp_size)))] when that index is < dim, else 0;
 *   normalize_chroma: divided by sqrt(sum x^2) only when sum x^2 >= 1e-10 (common/normalization.go:
 *   113-134); remove_mean: minus the mean (the in-order sum / n); binary_mode: > mean as 1.0 / 0.0.
 *   estimateKeyProfile (:300-370): scores[mode * 12 + key] = stats.PearsonCorrelationFunc(row, shifted)
 *   (stats/distance.go:111-145), shifted[i] = profile[(i + key) % 12], so key k's template has its
 *   tonic at pitch class (12 - k) % 12; 0 when either centred sum of squares is 0,
 *   and every score is 0 when hpcp_size != 12 (correlateWithProfile's length test, F44).  The 24
 *   candidates, created in the order C major, C minor, C# major, ..., are sorted by score, descending;
 *   sort.Slice leaves the order of equal scores open, here they stay in creation order (F45); the first
 *   min(max_candidates, 24) are kept, as codes key * 2 + mode.  key, mode and strength are the first
 *   candidate's, clarity = (s0 - s1) / s0 over the descending scores when s0 > 0, else 0; ambiguity =
 *   the entropy (math.Log2) of the positive scores over their sum, / log2(24), 0 when nothing is
 *   positive; tonality = 1 - computeUniformity(processed row) (chroma/chroma_vector.go:385-408).
 *   postProcessResult (:675-686): confidence = the first candidate's score, or 0 with known = 0 ("Unknown")
 *   when it is < min_confidence; key, mode, strength and the candidates keep their values.
 *   profile outside 0..6 is Krumhansl (:301-305).  There is no method field: every method runs the
 *   profile correlation (F43).
 * Go's panics are SONAR_ERR_PANIC with Go's text, tested in Go's order, only when F > 0 (no row,
 * no EstimateKey): hpcp_size < 0 "runtime error: makeslice:
 * len out of range"; max_candidates < 0 "runtime error: slice bounds out of range [:-1]" (the value);
 * max_candidates == 0, and then hpcp_size == 0 (ComputeStats' values[0]), "runtime error: index out of
 * range [0] with length 0".  dim == 0 with a positive hpcp_size is legal: rows of zeros.
 * Not reproduced (SONAR_ERR_UNSUPPORTED): dim or hpcp_size above 120; F above 2^31 - 1; any non-finite
 * chroma value that is read (a NaN score makes sort.Slice's order undefined; outputs are then
 * unspecified).
 * With device_ptrs = 1 the chromagram and every output, the single values included, are device
 * addresses; the call returns after the stream has drained either way.  Every output may be NULL and
 * then costs nothing. */
#define SONAR_KEY_PROFILE_KRUMHANSL 0
#define SONAR_KEY_PROFILE_TEMPERLEY 1
#define SONAR_KEY_PROFILE_SHAATH 2
#define SONAR_KEY_PROFILE_EDMA 3
#define SONAR_KEY_PROFILE_BGATE 4
#define SONAR_KEY_PROFILE_DIATONIC 5
#define SONAR_KEY_PROFILE_TONIC_TRIAD 6
/* The fields of KeyEstimationParams (:88-113) the reference reads. */
typedef struct sonar_key_params {
  int32_t profile;           /* Profile */
  int32_t hpcp_size;         /* HPCPSize */
  int32_t normalize_chroma;  /* NormalizeChroma */
  int32_t remove_mean;       /* RemoveMean */
  int32_t binary_mode;       /* BinaryMode */
  int32_t max_candidates;    /* MaxCandidates */
  double min_confidence;     /* MinConfidence */
} sonar_key_params;
/* NewKeyEstimator's values (:141-166): Krumhansl, 12, normalized, mean kept, not binary, 5, 0.5. */
void sonar_key_params_default(sonar_key_params* p);

/* EstimateKey per row; also KeyEstimationBatch.ProcessBatch (:911-920) and EstimateKeyFromHPCP
 * (:236-247) per HPCP row.  key, mode, known, confidence, strength, clarity, ambiguity, tonality: F
 * each.  F == 0 -> SONAR_OK, nothing is read or written. */
int sonar_key_frames(sonar_ctx* ctx, const double* chroma /* F x dim */, int64_t F, int32_t dim,
                     const sonar_key_params* params, int32_t* key, int32_t* mode, int32_t* known,
                     double* confidence, double* strength, double* clarity, double* ambiguity, double* tonality,
                     double* scores /* F x 24 */, int32_t* candidates /* F x min(max_candidates, 24) */,
                     double* processed /* F x hpcp_size */, int32_t device_ptrs);
/* EstimateKeySequence (:250-270).  The single result is EstimateKey of computeAverageChroma (:575-596:
 * per bin the sum over the frames in frame order, / F): one value per field, scores[24],
 * processed[hpcp_size].  stability (analyzeTemporalStability :598-622): 0 below 3 frames, else the share
 * of frames whose code key * 2 + mode equals the most frequent one (findMode iterates a map; here the
 * lowest code among the most frequent wins, F45); a frame below min_confidence still votes (F46).
 * modulations (detectModulations :624-655; capacity max(F - 20, 0), ascending, *n_modulations of them):
 * nothing at 20 frames or fewer; for i = 10 .. F - 11 the in-order mean of the 10 rows [i - 5, i + 5) is
 * estimated, and i is reported when its code differs from position i - 1's and its thresholded
 * confidence is > 0.7; position 10 has no predecessor, so nothing is reported below 22 frames (F47).
 * F == 0 -> SONAR_OK, all zeros. */
int sonar_key_sequence(sonar_ctx* ctx, const double* chroma /* F x dim */, int64_t F, int32_t dim,
                       const sonar_key_params* params, int32_t* key, int32_t* mode, int32_t* known,
                       double* confidence, double* strength, double* clarity, double* ambiguity, double* tonality,
                       double* scores /* 24 */, double* processed /* hpcp_size */, double* stability,
                       int32_t* modulations /* max(F - 20, 0) */, int64_t* n_modulations, int32_t device_ptrs);
#define SONAR_KEY_TRANSITION_SAME_KEY 0
#define SONAR_KEY_TRANSITION_PARALLEL 1
#define SONAR_KEY_TRANSITION_RELATIVE 2
#define SONAR_KEY_TRANSITION_DOMINANT 3
#define SONAR_KEY_TRANSITION_SUBDOMINANT 4
#define SONAR_KEY_TRANSITION_DISTANT 5
/* KeyEstimationBatch (:896-1005): ProcessBatch's per-frame outputs as sonar_key_frames', then
 * GetGlobalKey (:923-959): in frame order every frame with confidence > 0.5 adds its confidence to its
 * key's vote (votes[24], by code) and to a total; the largest vote wins (the reference iterates a map;
 * here the lowest code among equal votes, F45); *global_code = its code, -1 when nothing voted (Go's
 * empty name); *global_confidence = best / total (0 / 0 = NaN then); *global_strength = best / F.
 * GetKeyProgression (:962-989): a record for every frame i >= 1 whose confidence and its predecessor's
 * are both > 0.5, the same key included: t_frame = i, t_from / t_to the two codes, t_confidence their
 * mean, t_type AnalyzeKeyTransition's type; capacity max(F - 1, 0), ascending, *n_transitions of them.
 * F == 0 -> SONAR_OK: code -1, confidence 0, strength 0, no votes, no transitions. */
int sonar_key_batch(sonar_ctx* ctx, const double* chroma /* F x dim */, int64_t F, int32_t dim,
                    const sonar_key_params* params, int32_t* key, int32_t* mode, int32_t* known,
                    double* confidence, double* strength, double* clarity, double* ambiguity, double* tonality,
                    double* scores, int32_t* candidates, double* processed, int32_t* global_code,
                    double* global_confidence, double* global_strength, double* votes /* 24 */,
                    int32_t* t_frame, int32_t* t_from, int32_t* t_to, double* t_confidence, int32_t* t_type,
                    int64_t* n_transitions, int32_t device_ptrs);
/* AnalyzeKeyTransition (:843-894), host only: *type (same key, then parallel, relative by
 * GetRelativeKey, dominant (+7), subdominant (-7), else distant), *semitone_distance = (to - from + 12)
 * % 12, *fifths_distance = 0 (same, parallel), 1 (relative, dominant, subdominant), else
 * min(distance, 12 - distance); *strength = 1 / (1 + fifths_distance).  Any output may be NULL. */
int sonar_key_transition(int32_t from_key, int32_t from_mode, int32_t to_key, int32_t to_mode, int32_t* type,
                         int32_t* semitone_distance, int32_t* fifths_distance, double* strength);

/* ---- chord detection over a chromagram (float64) ----------------------------
 * ChordDetector (algorithms/tonal/chord_detection.go) on F rows of dim chroma values, for example the
 * profile sonar_hpcp leaves on the device.  Nothing on the path calls a transcendental function.
 *
 * DetectChord (:408-503) of one row, from templateMatching (:586-641) on:
 *   normalize_templates: the row is divided by sqrt(sum x^2) only when sum x^2 >= 1e-10
 *   (common/normalization.go:113-134).  The 120 template scores are calculateTemplateScore (:721-733) of
 *   the ten templates (Major 0, Minor 1, Diminished 2, Augmented 3, Sus2 4, Sus4 5, Maj7 6, Min7 7, Dom7 8,
 *   PowerChord 23) rotated to the twelve roots, times the template's weight; a candidate's slot is
 *   t * 12 + root with t the template's position in that order (the reference iterates a map there; this
 *   is the order fixed here), and template_scores is indexed by slot.  Every score is 0
 *   when dim is not 12 (F54).  With use_bass_detection and a bass confidence > 0.3 a candidate whose
 *   chord tones hold the bass note gains bass_weight * bass_confidence (:735-750); a slot is a candidate
 *   when its score >= min_chord_strength; with use_inversions and a bass confidence > 0.3,
 *   detectInversion (:752-781: 1.5 at the bass tone) replaces strength and inversion when it scores
 *   higher.  confidence = min(strength, 1).  The methods harmonic_analysis, cqt_based and statistical
 *   match with the bass forced to (0, 0.0); every other value of method matches with the bass (F58).
 *   applyTemporalSmoothing (:783-806, sonar_chord_sequence only): a candidate that is in chordHistory
 *   has its confidence times 1.1, clipped to 1.  chordHistory aliases the candidate slice that is then
 *   sorted in place: after a frame it is that frame's candidate set, minus its first-ranked candidate
 *   when the history was not empty before the frame and the frame has more than temporal_window
 *   candidates (F52); a frame without candidates empties it (F55).
 *   The candidates are sorted by confidence, descending; sort.Slice leaves the order of equal
 *   confidences open, here they stay in slot order (F50); the first max_candidates are kept.  root,
 *   quality (Go's ChordQuality code), inversion, confidence and strength are the first kept candidate's;
 *   clarity = c0 - c1 (c0 with one kept), ambiguity = 1 - clarity, consonance the template's, tension =
 *   calculateHarmonicTension (:1012-1035) of the raw row, stability = max(0, 1 - variance) of
 *   confidenceHistory (the first confidences of the last <= temporal_window earlier frames that kept a
 *   candidate), or the confidence when that history is empty (always in sonar_chord_frames).
 *   extensions (detect_extensions; :840-894) is a mask of 1 << interval over the intervals 2, 5, 9, 10, 11;
 *   role (use_functional_analysis; :896-917) is 0 "", 1 tonic, 2 subdominant, 3 dominant, 4 leading_tone,
 *   5 other.  A row that keeps no candidate is Go's zero result: every per-frame output 0 but n_found (F55).
 * Errors, tested in Go's order and only when F > 0: dim not 12, 24 or 36 -> SONAR_ERR_INVALID "failed to
 * extract chroma features: unsupported chroma size: N" (:416-419); max_candidates < 0 -> SONAR_ERR_PANIC
 * "runtime error: slice bounds out of range [:-1]" (the value; :458-460, even for rows without
 * candidates); a bass note outside 0..11 -> SONAR_ERR_INVALID; in a sequence, temporal_window < 0 at a
 * frame without candidates after one with -> SONAR_ERR_PANIC "runtime error: slice bounds out of range
 * [1:0]" (:802).  Not reproduced (SONAR_ERR_UNSUPPORTED, the message says which): a non-finite chroma
 * value, bass confidence or parameter; temporal_window above 64; F above 2^31 - 1.
 * F == 0 -> SONAR_OK, nothing is read or written.
 * With device_ptrs = 1 the inputs and every output are device addresses; the call returns after the
 * stream has drained either way.  Every output may be NULL and then costs nothing. */
#define SONAR_CHORD_TEMPLATE_MATCHING 0
#define SONAR_CHORD_HARMONIC_ANALYSIS 1
#define SONAR_CHORD_CQT_BASED 2
#define SONAR_CHORD_STATISTICAL 3
#define SONAR_CHORD_ML_BASED 4
#define SONAR_CHORD_HYBRID 5
#define SONAR_CHORD_SLOTS 120
/* The fields of ChordDetectionParams (:136-175) the reference reads (DESIGN.md F51 lists the others);
 * ChromaSize is the row length dim. */
typedef struct sonar_chord_params {
  int32_t method;                  /* Method */
  int32_t normalize_templates;     /* NormalizeTemplates */
  int32_t use_inversions;          /* UseInversions */
  int32_t max_candidates;          /* MaxCandidates */
  int32_t use_bass_detection;      /* UseBassDetection */
  int32_t detect_extensions;       /* DetectExtensions */
  int32_t max_extension;           /* MaxExtension */
  int32_t use_temporal_smoothing;  /* UseTemporalSmoothing */
  int32_t temporal_window;         /* TemporalWindow */
  int32_t use_functional_analysis; /* UseFunctionalAnalysis */
  double min_chord_strength;       /* MinChordStrength */
  double bass_weight;              /* BassWeight */
} sonar_chord_params;
/* NewChordDetector's values (:217-244): template matching, normalized, inversions, 5 candidates, bass
 * detection, extensions up to 13, smoothing over 5, no functional analysis, 0.2, 0.3. */
void sonar_chord_params_default(sonar_chord_params* p);
/* The outputs of the chord entries: F entries each, template_scores F x 120, the candidate arrays
 * F x max_candidates (slots, -1 and zeros beyond the kept ones). */
typedef struct sonar_chord_out {
  int32_t* root;
  int32_t* quality;
  int32_t* inversion;
  int32_t* n_found;           /* candidates before the cut */
  double* confidence;
  double* strength;
  double* clarity;
  double* ambiguity;
  double* consonance;
  double* tension;
  double* stability;
  int32_t* extensions;
  int32_t* role;
  double* template_scores;
  int32_t* candidates;
  int32_t* cand_inversion;
  double* cand_confidence;
  double* cand_strength;
} sonar_chord_out;
/* Every row through a fresh detector: no boost, stability = confidence.  bass_note / bass_confidence: F
 * entries each or NULL, what detectBassNote returned per row (NULL: 0 and 0.0). */
int sonar_chord_frames(sonar_ctx* ctx, const double* chroma /* F x dim */, int64_t F, int32_t dim,
                       const int32_t* bass_note, const double* bass_confidence, const sonar_chord_params* params,
                       const sonar_chord_out* out, int32_t device_ptrs);
/* One detector fed the rows in order: the smoothing chain and the stability history apply. */
int sonar_chord_sequence(sonar_ctx* ctx, const double* chroma /* F x dim */, int64_t F, int32_t dim,
                         const int32_t* bass_note, const double* bass_confidence, const sonar_chord_params* params,
                         const sonar_chord_out* out, int32_t device_ptrs);
/* DetectChord on every frame of frame_len samples at hop: (n - frame_len) / hop + 1 frames (*frames when
 * not NULL; n < frame_len -> SONAR_ERR_TOO_SHORT).  extractChromaFeatures (:506-531) takes the first W =
 * min(2048, frame_len) samples of the frame, unwindowed (F56), their full-length magnitude spectrum
 * (mirror half included, F37) and ComputeFromSpectrum with NewHPCP's defaults; then one detector is fed
 * the profiles in order as in sonar_chord_sequence.  hpcp (frames x 12 or NULL) receives the profiles.
 * W must be a power-of-two window size of the fused STFT path, else SONAR_ERR_UNSUPPORTED.  DetectPitch
 * rejects every frame whose length is not 1024, so the bass is (0, 0.0) there (F53) and the bass arrays
 * are not read; at frame_len 1024 with use_bass_detection the caller supplies both bass arrays or the
 * call is SONAR_ERR_UNSUPPORTED (the pitch detector's stateful post-processing is not reproduced).
 * method cqt_based is SONAR_ERR_UNSUPPORTED here, and so are rows of 24 or 36 bins: the entry computes
 * the 12-bin profile.  frames is a host address in both pointer modes. */
int sonar_chord_detect(sonar_ctx* ctx, const double* pcm, int64_t n, int32_t sample_rate, int32_t frame_len,
                       int32_t hop, const int32_t* bass_note, const double* bass_confidence,
                       const sonar_chord_params* params, const sonar_chord_out* out, double* hpcp, int64_t* frames,
                       int32_t device_ptrs);
/* AnalyzeProgression (:1128-1173) over the per-frame results of F chords.  *num_chords = F;
 * *insufficient_data = 1 below two chords and nothing else is written (decided on the host: ctx may be
 * NULL then, with host pointers).  Else *average_confidence = (the sum of confidence in frame order) / F
 * and *most_common_quality = the most frequent quality code (the reference iterates a map; here the
 * lowest code among equal counts).  root and inversion only name the chords of the reference's
 * transition strings and may be NULL.  A quality outside 0..31 or a non-finite confidence ->
 * SONAR_ERR_UNSUPPORTED. */
int sonar_chord_progression(sonar_ctx* ctx, const int32_t* root, const int32_t* quality, const int32_t* inversion,
                            const double* confidence, int64_t F, int64_t* num_chords, int32_t* insufficient_data,
                            double* average_confidence, int32_t* most_common_quality, int32_t device_ptrs);

/* ---- path B: normalized cross-correlation (float64) --------------------
 * corr has 2L+1 entries, L = max(0, min(max_lag, na-1, nb-1)); metrics[10] =
 * {peak_corr, peak_lag, peak_index, p_value, snr, sharpness, second_peak,
 *  peak_to_sidelobe, overlap_length, num_lags} (correlation.go:131-200). */
int sonar_ncc(sonar_ctx* ctx, const double* a, int64_t na, const double* b, int64_t nb,
              int32_t max_lag, double* corr, double* metrics, int32_t device_ptrs);

/* ---- cross-correlation in full: CrossCorrelation.Compute (correlation.go:131-200) for every
 * correlation type, method and constructor; sonar_ncc above is the one instance
 * NewCrossCorrelationWithParams(maxLag, NormalizedCrossCorrelation, TimeDomain).
 * corr_type and method are CorrelationType's and CorrelationMethod's values (:12-41).  use_fft is
 * the private field the constructors set: NewCrossCorrelation(maxLag) is {PEARSON, TIME_DOMAIN,
 * use_fft 1}; NewCrossCorrelationWithParams(maxLag, type, method) is use_fft = (method ==
 * FREQUENCY_DOMAIN); NewAutoCorrelation(maxLag) with SetParameters(type, method) keeps use_fft 1.
 * As in Compute: empty inputs are SONAR_ERR_EMPTY "empty signals provided"; with use_fft and more
 * than 1,000 samples in either input the method becomes FREQUENCY_DOMAIN (:139-142); a method that
 * is then none of the three is SONAR_ERR_INVALID "unsupported correlation method"; SLIDING_WINDOW
 * is TIME_DOMAIN (:294-297).  Both inputs are z-scored first (normalize :464-501) under every
 * method.  corr has 2L+1 entries, L = max(0, min(max_lag, na-1, nb-1)).
 * TIME_DOMAIN, per lag: PEARSON pearsonCorrelation (:314-370: overlap means, centred sums, 0 when
 * the overlap is <= 1 sample or the denominator < 1e-10, clamped to [-1, 1]); SPEARMAN, KENDALL and
 * every unknown type are PEARSON (:301-310); NCC as sonar_ncc, bit for bit; ZNCC the NCC of the
 * z-scores after subtractMean (:412-418, 504-523).
 * FREQUENCY_DOMAIN (computeFFT :231-291) does not consult the type: corr[i] is the un-normalised
 * circular sum real(ifft(fft(a) * conj(fft(b))))[lag or N + lag], N = nextPowerOf2(na + nb - 1), with
 * Go's recursive radix-2 transform (:726-774) bit for bit.  The peak is then of the order of the
 * overlap length, and calculatePValue's sqrt(1 - peak^2) is NaN: p_value 0.5.  Limit: na + nb - 1
 * <= 4,194,304 (N <= 2^22), beyond it SONAR_ERR_UNSUPPORTED; TIME_DOMAIN has no limit.  The first
 * call at a given N builds its twiddle table (cached in the context until sonar_trim).
 * metrics[12] = sonar_ncc's ten, then the method that ran (after the switch) and corr_type as given.
 * Host or device pointers (device_ptrs); with device pointers a null corr goes to library scratch. */
enum { SONAR_CORR_PEARSON = 0, SONAR_CORR_SPEARMAN = 1, SONAR_CORR_KENDALL = 2,
       SONAR_CORR_NCC = 3, SONAR_CORR_ZNCC = 4 };
enum { SONAR_CORR_TIME_DOMAIN = 0, SONAR_CORR_FREQUENCY_DOMAIN = 1, SONAR_CORR_SLIDING_WINDOW = 2 };
int sonar_xcorr_params(sonar_ctx* ctx, const double* a, int64_t na, const double* b, int64_t nb,
                       int32_t max_lag, int32_t corr_type, int32_t method, int32_t use_fft,
                       double* corr, double* metrics /*[12]*/, int32_t device_ptrs);
/* AutoCorrelation.Compute (:669-690) = Compute(x, x) of NewCrossCorrelation(max_lag) after
 * SetParameters(corr_type, method): use_fft stays 1, so above 1,000 samples it is always the FFT
 * method.  The one input is transformed once. */
int sonar_autocorr(sonar_ctx* ctx, const double* x, int64_t n, int32_t max_lag, int32_t corr_type,
                   int32_t method, double* corr, double* metrics /*[12]*/, int32_t device_ptrs);

/* ---- path B: DTW (float64, optional Sakoe-Chiba band).  sonar_dtw is the default
 * DTWAlignment (Euclidean, symmetric2); sonar_dtw_params takes NewDTWAlignmentWithParams'
 * step pattern and metric (below).
 * q: nq x dim, r: nr x dim row-major.  path_* capacity >= nq + nr.  cost
 * (nullable) receives costMatrix[1:] = nq x (nr+1) (dtw.go:96).  Path points
 * are in forward order with cost = C[i][j] - C[i-1][j-1] (dtw.go:165-188). */
int sonar_dtw(sonar_ctx* ctx, const double* q, int64_t nq, const double* r, int64_t nr, int32_t dim,
              int32_t band, double* distance, int32_t* path_q, int32_t* path_r, double* path_cost,
              int64_t* path_len, double* cost, int32_t device_ptrs);

/* stats.NewDTWAlignmentWithParams(constraintBand, stepPattern, metric) (dtw.go:45-52).
 * Step patterns, applyStepPattern (dtw.go:137-162): symmetric2 Min(Min(up, left), diag),
 * asymmetric Min(up, left), symmetric1 Min(up+1, Min(left+1, diag)).  "asymmetric" never reads
 * C[0][0], so with finite inputs every cell is +Inf: distance +Inf, a path of nq + nr points up
 * column nr and along row 0 (query index -1), cost NaN where i > 0 and j > 0.
 * Metrics, GetDistanceFunction (distance.go:10-26) in DistanceMetric's iota order
 * (clustering.go:23-28): Euclidean (:29-36), Manhattan (:39-45), Cosine (:48-65; 1.0 when either
 * norm is 0; may be slightly negative), Pearson (:73-107; 1.0 when either square sum is 0).
 * Mahalanobis (:150-153) and every other value are Euclidean, as in Go.  Cosine and Pearson can
 * be NaN for finite inputs (overflow to Inf / Inf). */
#define SONAR_DTW_STEP_SYMMETRIC2 0
#define SONAR_DTW_STEP_ASYMMETRIC 1
#define SONAR_DTW_STEP_SYMMETRIC1 2
#define SONAR_DTW_METRIC_EUCLIDEAN 0
#define SONAR_DTW_METRIC_MANHATTAN 1
#define SONAR_DTW_METRIC_COSINE 2
#define SONAR_DTW_METRIC_PEARSON 3
#define SONAR_DTW_METRIC_MAHALANOBIS 4
/* DTWAlignment.Align (dtw.go:55-103) of a DTWAlignment built with those parameters: sonar_dtw's
 * arguments and outputs plus step_pattern and metric.  An unknown step_pattern is
 * SONAR_ERR_INVALID "failed to fill cost matrix: unknown step pattern: <value>" (dtw.go:76-78,
 * 159-160), after the empty-sequence check.  Symmetric2 with Euclidean runs sonar_dtw's code.
 * (ConstrainedAlign, dtw.go:236-251, is a stub that calls Align: use this entry.) */
int sonar_dtw_params(sonar_ctx* ctx, const double* q, int64_t nq, const double* r, int64_t nr, int32_t dim,
                     int32_t band, int32_t step_pattern, int32_t metric, double* distance, int32_t* path_q,
                     int32_t* path_r, double* path_cost, int64_t* path_len, double* cost, int32_t device_ptrs);
/* DTWAlignment.GetAlignmentQuality (dtw.go:253-286), host only (no context, no GPU): out4 =
 * {path_efficiency, diagonal_ratio, average_cost, normalized_distance}; average_cost is summed in
 * path order; one point gives diagonal_ratio 0/0 = NaN as in Go.  path_len <= 0 (Go: an empty
 * map) is SONAR_ERR_EMPTY. */
int sonar_dtw_quality(const int32_t* path_q, const int32_t* path_r, const double* path_cost, int64_t path_len,
                      int64_t nq, int64_t nr, double distance, double* out4);
/* DTWAlignment.OptimizeStepPattern (dtw.go:288-311): three Align calls in the order symmetric2,
 * asymmetric, symmetric1; *best = the SONAR_DTW_STEP_* with the smallest Distance by strict <,
 * starting from symmetric2.  distances3 (nullable) receives the three distances, NaN for a call
 * that failed (Go skips it).  Returns SONAR_OK even when all three fail (*best = symmetric2), as
 * Go returns "symmetric2", nil. */
int sonar_dtw_optimize_step_pattern(sonar_ctx* ctx, const double* q, int64_t nq, const double* r, int64_t nr,
                                    int32_t dim, int32_t band, int32_t metric, int32_t device_ptrs, int32_t* best,
                                    double* distances3);

/* ---- LPC formants: FormantAnalyzer.AnalyzeMultipleFrames (algorithms/speech/format.go:427-449)
 * over FormantAnalyzer.AnalyzeFormants (:85-124) + LPCAnalyzer.Analyze (lpc.go:44-82).
 * Analysis window W = 2048 if sample_rate >= 16000 else 1024, LPC order 12 + sr/1000,
 * pre-emphasis 0.97, symmetric Hamming (format.go:48-69).  Frames start at 0, hop, ...
 * while start < n - frame_size (frame_size <= 0 -> W, hop <= 0 -> frame_size/2).  Every
 * attempted frame gets a record; status != 0 marks the frames Go skips. ------------ */
typedef struct {
  int32_t status;          /* 0 ok; 1 frame shorter than W; 3 "zero energy signal";
                              4 "prediction error energy became zero" (lpc.go:93-113)   */
  int32_t n_formants;      /* validated formants, <= 4 (ascending frequency)            */
  double frequency[4];
  double bandwidth[4];
  double amplitude[4];
  double confidence[4];
  double vocal_tract_length;   /* cm, 17.5 when no formant qualifies                    */
  double quality;              /* calculateAnalysisQuality                               */
  double gain;                 /* sqrt(residual energy)                                  */
  double residual_energy;
  int32_t stable;              /* checkStability: every |a_i| < 1                        */
  int32_t lpc_order;
} sonar_formant_frame;

int64_t sonar_formant_frame_count(int64_t n, int32_t sample_rate, int32_t frame_size, int32_t hop_size);
/* lpc_coeffs (nullable): frames x (order+1) a[0..p], a[0] = 1; reflection (nullable): frames x order;
 * the rows of a frame with status != 0 are zero */
int sonar_formants(sonar_ctx* ctx, const double* pcm, int64_t n, int32_t sample_rate, int32_t frame_size,
                   int32_t hop_size, sonar_formant_frame* out, double* lpc_coeffs, double* reflection,
                   int32_t device_ptrs);

/* ---- VoiceQualityAnalyzer.AnalyzeVoiceQuality (algorithms/speech/voice_quality.go:56-111),
 * the analysis AnalyzeSpeech runs on the speech extractor's pre-emphasised PCM
 * (speech_analysis.go:77-80) and whose Jitter / Shimmer land in SpeechFeatures
 * (extractors/speech.go:306-309).  Pitch periods come from a YIN scan of 1024-sample frames at
 * hop 256 with a fresh PitchDetector (:114-157); voicing_strength is DetectPitch on the whole
 * signal, which Go only accepts for exactly 1024 samples (else 0).  Errors, as Go:
 * SONAR_ERR_TOO_SHORT "signal too short for voice quality analysis (need at least 1 second)"
 * and "insufficient pitch periods for analysis (found k, need at least 3)". ------------------ */
typedef struct {                     /* speech.VoiceQualityResult (voice_quality.go:21-43) */
  double jitter, shimmer, hnr, noise_measure, f0_stability, amplitude_stability;
  double voicing_strength, overall_quality;
  int64_t num_periods;
  double mean_f0, f0_range, analysis_quality;
} sonar_voice_quality_result;

int sonar_voice_quality(sonar_ctx* ctx, const double* pcm, int64_t n, int32_t sample_rate,
                        sonar_voice_quality_result* out);

/* ---- host mirror of the Go API (C++ above the kernels) ------------------ */
typedef struct sonar_result sonar_result;   /* named float64 arrays + scalars */

typedef struct {              /* fingerprint.FingerprintConfig (fingerprint.go:29-35) */
  int32_t window_size;        /* FingerprintConfig.WindowSize (STFT)                 */
  int32_t hop_size;           /* FingerprintConfig.HopSize                            */
  int32_t feature_window_size;/* FingerprintConfig.FeatureConfig.WindowSize (energy)  */
  int32_t feature_hop_size;   /* FingerprintConfig.FeatureConfig.HopSize              */
  int32_t enable_content_detect;
  int32_t window_type;        /* content settings WindowType (all Hann in the tables) */
  int32_t precision;          /* SONAR_F32 / SONAR_F64                                */
  /* ContentConfig (config.ContentAwareConfig, config/config.go:5-10) and the rest of
   * AudioData.Metadata, used by ContentDetector.DetectContentType when the content type
   * is unknown and enable_content_detect is set (fingerprint.go:155-158) */
  int32_t acoustic_detection;     /* ContentConfig.EnableContentDetection               */
  int32_t default_content_type;   /* ContentConfig.DefaultContentType (SONAR_CT_*)      */
  double auto_detect_threshold;   /* ContentConfig.AutoDetectThreshold                  */
  const char* genre;              /* Metadata.Genre   (NULL = "")                       */
  const char* station;            /* Metadata.Station (NULL = "")                       */
  const char* url;                /* Metadata.URL     (NULL = "")                       */
} sonar_fingerprint_config;

void sonar_fingerprint_config_default(sonar_fingerprint_config* cfg);  /* fingerprint.go:70-98 */

typedef struct {              /* config.FeatureConfig fields the speech extractor reads (config/config.go:13-38) */
  int32_t sample_rate;        /* FeatureConfig.SampleRate (0 under GenerateFingerprint, F1)           */
  int32_t window_size;        /* FeatureConfig.WindowSize: ShortTimeEnergy frames                     */
  int32_t hop_size;           /* FeatureConfig.HopSize                                                */
  int32_t stft_window_size;   /* spectrogram handed to ExtractFeatures (ComputeSTFTWithWindow W)     */
  int32_t stft_hop_size;      /* ... and H                                                            */
  int32_t window_type;
  int32_t enable_mfcc;
  int32_t enable_speech_features;
  int32_t enable_temporal_features;
  int32_t mfcc_coefficients;
  int32_t is_news;
  int32_t precision;          /* SONAR_F64 (parity, default) / SONAR_F32                              */
} sonar_feature_config;

void sonar_feature_config_default(sonar_feature_config* cfg);

/* NewSpeechFeatureExtractor(cfg, is_news) + ExtractFeatures(STFT(pcm, W, H), pcm, sample_rate).
 * Result arrays: "mfcc", "spectral_centroid" ... "spectral_flux", "zero_crossing_rate",
 * "short_time_energy", "energy_variance", "loudness_range", "energy_entropy",
 * "low_energy_ratio", "high_energy_ratio", "pitch_estimate", "pitch_confidence",
 * "voicing_strength", "harmonic_ratio", "inharmonicity_ratio", "tonal_centroid",
 * temporal ("rms_energy", "dynamic_range", "silence_ratio", "peak_amplitude",
 * "average_amplitude", "onset_density", "attack_time", "envelope_shape") and speech
 * ("is_speech", "voicing_probability", "spectral_tilt", "pause_duration") groups when enabled. */
int sonar_extract_speech_features(sonar_ctx* ctx, const double* pcm, int64_t n, int32_t sample_rate,
                                  const sonar_feature_config* cfg, sonar_result** out);

/* NewMusicFeatureExtractor(cfg) + ExtractFeatures(STFT(pcm, W, H), pcm, sample_rate)
 * (fingerprint/extractors/music.go:70-583).  cfg: sample_rate = FeatureConfig.SampleRate (the
 * analyzers' and MFCC's rate), window_size / hop_size = FeatureConfig (ShortTimeEnergy frames,
 * chroma hop), stft_window_size / stft_hop_size / window_type = the spectrogram; sample_rate
 * (the argument) = SpectrogramResult.SampleRate.  Result arrays: "spectral_centroid" ..
 * "spectral_slope", "spectral_flux" (F, [0] = 0), "zero_crossing_rate" (F zeros, never filled in
 * Go), "spectral_contrast" (F x 6), "mfcc" (F x 13 of |X|^4 over 26 mels, F5), "chroma" (F x 12),
 * "rms_energy", "envelope_shape", "peak_amplitude", "average_amplitude", then "dynamic_range",
 * "onset_density", "attack_time", "crest_factor", "silence_ratio", "activity_level",
 * "short_time_energy", "energy_variance", "energy_entropy", "loudness_range",
 * "low_energy_ratio", "high_energy_ratio" and the harmonic block "pitch_estimate",
 * "pitch_confidence", "voicing_strength", "harmonic_ratio", "inharmonicity_ratio",
 * "tonal_centroid" (zero by F7 unless the chroma frame is exactly 1024 samples).
 * The reference panics in extractTemporalFeatures for every signal of >= 1536 samples
 * (music.go:403 passes percentiles 10 and 90 where fractions are expected:
 * "index out of range [10 (L-1)] with length L") and for a signal with no energy frame
 * (music.go:383: "integer divide by zero").  Then the call returns SONAR_ERR_PANIC with that
 * text and *out holds the arrays computed before the panic (the spectral group, "mfcc",
 * "chroma", "rms_energy", and after the division also "envelope_shape" and the amplitudes);
 * the caller frees it.  float64. */
int sonar_extract_music_features(sonar_ctx* ctx, const double* pcm, int64_t n, int32_t sample_rate,
                                 const sonar_feature_config* cfg, sonar_result** out);

/* AudioData{PCM, SampleRate, Metadata.ContentType}.  content_type is the raw
 * metadata string ("music", "news", "talk", ... ; unknown strings -> content
 * detection, F12).  Returns arrays named like ExtractedFeatures fields:
 * "mfcc", "spectral_centroid", ..., "short_time_energy", "pitch_estimate", ... */
int sonar_generate_fingerprint(sonar_ctx* ctx, const double* pcm, int64_t n, int32_t sample_rate,
                               const char* content_type, const sonar_fingerprint_config* cfg,
                               sonar_result** out);

/* AlignmentExtractor.ExtractAlignmentFeatures on the energy (+ optional chroma)
 * features of two fingerprints.  feature_sample_rate / hop / window are the
 * extractor's FeatureConfig; max_lag_seconds as NewAlignmentExtractorWithMaxLag. */
int sonar_align_features(sonar_ctx* ctx,
                         const double* q_energy, int64_t nq_energy, const double* r_energy, int64_t nr_energy,
                         const double* q_chroma, int64_t nq_chroma, const double* r_chroma, int64_t nr_chroma,
                         int64_t q_pcm_len, int64_t r_pcm_len, int32_t sample_rate,
                         int32_t feature_sample_rate, int32_t hop_size, int32_t window_size,
                         double max_lag_seconds, sonar_result** out);

/* One stream pair end to end (the C5 unit): sonar_music_alignment_features of both device-resident
 * float64 PCM streams into ctx buffers (stft_window / hop; energy frames feature_window / hop), then
 * sonar_align_features on those device arrays with feature_sample_rate = sample_rate.  Same result
 * arrays as sonar_align_features; only the feature round trip through the host is gone. */
int sonar_align_pair_device(sonar_ctx* ctx, const double* q_pcm, int64_t nq, const double* r_pcm, int64_t nr,
                            int32_t sample_rate, int32_t stft_window, int32_t hop, int32_t feature_window,
                            double max_lag_seconds, sonar_result** out);

/* ---- many stream pairs (the C5 workload) -----------------------------------------
 * The fixed-size record a caller of ExtractAlignmentFeatures keeps per pair
 * (extractors/alignment.go:139-219: TemporalOffset, OffsetConfidence, AlignmentSimilarity,
 * AlignmentQuality, Method; the NCC candidate's offset and peak lag; the chroma DTW distance). */
typedef struct {
  double temporal_offset;        /* seconds                                       */
  double offset_confidence;
  double alignment_similarity;
  double alignment_quality;
  double method;                 /* SONAR_ALIGN_* of the chosen candidate          */
  double corr_offset_seconds;    /* the energy-NCC candidate (NaN if none)         */
  double dtw_distance;           /* the chroma-DTW candidate (NaN if none)         */
  double peak_lag;               /* NCC peak lag in feature frames (NaN if none)   */
  int32_t status;                /* SONAR_OK or this pair's error code             */
  int32_t flags;                 /* SONAR_PAIR_REDONE_* bits (0: the batched path) */
} sonar_pair_record;

/* sonar_pair_record.flags: the pair's record came from the single-pair path instead of its batch */
#define SONAR_PAIR_REDONE_TIMEOUT 1    /* its batched band pipeline timed out (retry on)  */
#define SONAR_PAIR_REDONE_NONFINITE 2  /* its chroma is not finite (exact math.Min path)  */

/* sonar_align_pair_device over npairs pairs: q_pcm[k] / r_pcm[k] float64 streams of nq[k] / nr[k]
 * samples (device pointers on ctx's device if device_ptrs, else host arrays).  `workers` is the
 * number of pairs in flight (<= 0: 128).  They are split over SONAR_PAIR_STREAMS worker contexts
 * (environment, default 16; each one HIP stream and one host thread) in batches of
 * ceil(workers / streams) pairs, each batch's chroma DTWs in ONE band-kernel launch, so the pairs'
 * latency-bound kernels (the DC-removal scan, the Go-order NCC sums, the DTW band pipeline and
 * walk) overlap on the GPU.  HIP maps a process's streams onto GPU_MAX_HW_QUEUES hardware queues
 * (4 by default, at most 32): set GPU_MAX_HW_QUEUES >= SONAR_PAIR_STREAMS in the environment
 * before the first HIP call of the process, or the streams share queues and serialise.  out[k] is
 * filled for every pair; the return is SONAR_OK or the first error.  A pair whose batched band
 * pipeline timed out is redone once on the single-pair path (exact; counted in
 * sonar_dtw_counters and flagged SONAR_PAIR_REDONE_TIMEOUT in its record); with
 * SONAR_PAIR_RETRY=0 it is an error instead, naming the pair and carrying its diagnostic record in
 * sonar_last_error. */
int sonar_align_pairs(sonar_ctx* ctx, int64_t npairs, const double* const* q_pcm, const int64_t* nq,
                      const double* const* r_pcm, const int64_t* nr, int32_t sample_rate, int32_t stft_window,
                      int32_t hop, int32_t feature_window, double max_lag_seconds, int32_t workers,
                      int32_t device_ptrs, sonar_pair_record* out);

/* ---- one process, several GPUs: a context per device plus an RCCL communicator
 * over them (ncclCommInitAll; collectives run over xGMI). ------------------------------------- */
typedef struct sonar_multi sonar_multi;
int sonar_multi_create(const int32_t* devices, int32_t n_devices, sonar_multi** out);
void sonar_multi_destroy(sonar_multi* m);
const char* sonar_multi_last_error(const sonar_multi* m);
int32_t sonar_multi_size(const sonar_multi* m);
sonar_ctx* sonar_multi_ctx(sonar_multi* m, int32_t rank);   /* the rank's context (do not destroy) */

/* Frame shard g of G over n samples at W/H: frames [f0, f1) = [e(g), e(g+1)) with
 * e(k) = floor(k F / G) rounded down to even (e(G) = F), F = sonar_stft_frames(n, W, H), and the
 * samples they read [s0, s1) = [f0 H, (f1-1) H + W) (empty shard: f0 == f1, s0 == s1).  Even
 * boundaries keep the headline kernel's frame pairs, so the shards reassemble bit-identically to
 * the unsharded call.  Pure arithmetic, the same on every host. */
int sonar_multi_shard(int64_t n, int32_t window_size, int32_t hop_size, int32_t n_shards, int32_t shard,
                      int64_t* f0, int64_t* f1, int64_t* s0, int64_t* s1);

/* sonar_fingerprint with the STFT frames sharded over the devices: device g runs frames [f0, f1)
 * of sonar_multi_shard on its sample slice (host pcm, cfg->device_ptrs must be 0) and writes its
 * rows of every requested output straight into the host arrays.  Frames are independent, so the
 * result equals the single-device call.  Supported flags: SONAR_FP_MFCC, SONAR_FP_MAGNITUDE,
 * SONAR_FP_COMPLEX, SONAR_FP_PHASE and SONAR_FP_SPECTRAL without flux (out->flux must be NULL: frame f0's flux needs frame f0-1); the
 * pre-emphasised outputs (ZCR, energy) read the sample before the slice -> SONAR_ERR_UNSUPPORTED. */
int sonar_fingerprint_multi(sonar_multi* m, const void* pcm, int64_t n, const sonar_fp_cfg* cfg,
                            sonar_fp_out* out);

/* The MFCC timeline assembled on EVERY device over RCCL: device g holds its shard's sample slice
 * pcm_dev[g] (samples [s0, s1) of sonar_multi_shard, cfg->pcm_dtype), computes its frames, and one
 * ncclAllGather (shards padded to the largest) fills mfcc_dev[g] (F x n_mfcc, cfg->out_dtype) on
 * every device -- the device-resident timeline a comparator on any GPU can read.  Synchronous. */
int sonar_fingerprint_multi_gather(sonar_multi* m, const void* const* pcm_dev, int64_t n, const sonar_fp_cfg* cfg,
                                   void* const* mfcc_dev);

/* sonar_align_pairs with the pairs split into contiguous ranges over the devices (host PCM; each
 * device aligns its range as sonar_align_pairs, `workers` pairs in flight); the per-device records are then
 * all-gathered over RCCL and device 0's gathered copy is returned in out[npairs]. */
int sonar_align_pairs_multi(sonar_multi* m, int64_t npairs, const double* const* q_pcm, const int64_t* nq,
                            const double* const* r_pcm, const int64_t* nr, int32_t sample_rate,
                            int32_t stft_window, int32_t hop, int32_t feature_window, double max_lag_seconds,
                            int32_t workers, sonar_pair_record* out);

/* ---- AlignmentAnalyzer.AnalyzeAlignmentConsistency (algorithms/stats/alignment.go:709-800) -----
 * num_trials (< 2 -> 5) alignments of addNoise(query, 0.01) (:737-749: q[i][j] += sin(i*j+i+j)
 * * 0.01 * q[i][j]) against reference with AlignFeatures (:84-106) for `method`, then the offset
 * statistics (:751-800).  The perturbation is deterministic, so every trial aligns the same
 * perturbed query: the alignment runs once and its offset is counted num_trials times (the
 * statistics are those of num_trials equal offsets, as in Go).  query / reference: host
 * row-major nq x dim / nr x dim float64.  method: SONAR_ALIGN_*; max_lag and hop as
 * NewAlignmentAnalyzer (:60-81).  Errors: "no successful alignments" (empty input or an
 * unsupported method, where every Go trial fails). */
enum { SONAR_ALIGN_DTW = 0, SONAR_ALIGN_XCORR = 1, SONAR_ALIGN_PHASE = 2, SONAR_ALIGN_HYBRID = 3 };
typedef struct {                     /* stats.AlignmentStats (alignment.go:700-707) */
  double mean_offset, stddev_offset, median_offset, offset_range, consistency;
  int64_t offset;                    /* the (single) AlignFeatures offset, samples or frames per method */
  int32_t trials;
} sonar_alignment_stats;

int sonar_alignment_consistency(sonar_ctx* ctx, const double* query, int64_t nq, const double* reference, int64_t nr,
                                int32_t dim, int32_t method, int32_t max_lag, int32_t hop, int32_t sample_rate,
                                int32_t num_trials, sonar_alignment_stats* out);

/* ---- AlignmentAnalyzer.AlignFeatures / AlignAudio and AlignmentExtractor.AlignAudioFiles --------
 * The analyzer's own entry (algorithms/stats/alignment.go:84-106) for method SONAR_ALIGN_DTW,
 * SONAR_ALIGN_XCORR or SONAR_ALIGN_HYBRID (alignWithHybrid :308-337: the cross-correlation of the
 * features' first component; when its confidence is <= 0.7 the DTW of the full rows, with Go's
 * result aliasing F8: Confidence = 0.6 c + 0.4 c and Similarity = 0.7 s + 0.3 s of the DTW values,
 * Offset / AlignmentQuality / Stability the DTW's, NoiseLevel the correlation's).  query /
 * reference: row-major nq x dim / nr x dim float64 (device pointers if device_ptrs).  max_lag and
 * hop as NewAlignmentAnalyzer (:60-81).  *out: scalars "method", "offset" (samples for the
 * correlation, frames for the DTW, F9), "offset_seconds", "confidence", "similarity",
 * "alignment_quality", "noise_level", "stability", "query_length", "reference_length",
 * "sample_rate", "dtw_ran"; with the correlation "correlations" (2L+1) and its metrics
 * ("peak_correlation", "peak_lag", ... as sonar_ncc); with the DTW "dtw_distance",
 * "dtw_path_query", "dtw_path_reference", "dtw_path_cost".  Errors as Go: "empty feature sequences
 * provided", "unsupported alignment method: N". */
int sonar_analyzer_align_features(sonar_ctx* ctx, const double* query, int64_t nq, const double* reference,
                                  int64_t nr, int32_t dim, int32_t method, int32_t max_lag, int32_t hop,
                                  int32_t sample_rate, int32_t device_ptrs, sonar_result** out);

/* AlignmentAnalyzer.AlignAudio (:108-126): extractEnergyFeatures (:341-361) of both float64 PCM
 * streams -- numFrames = (len - window) / hop + 1 (truncating), RMS over [i hop, min(i hop + window,
 * len)) -- then sonar_analyzer_align_features with dim 1.  Go panics are SONAR_ERR_PANIC with
 * Go's text (hop 0: "integer divide by zero"; a negative frame count: "makeslice: len out of
 * range"); window <= 0, hop < 0 or an empty stream: SONAR_ERR_UNSUPPORTED (Go divides 0 by 0). */
int sonar_align_audio(sonar_ctx* ctx, const double* q_pcm, int64_t nq, const double* r_pcm, int64_t nr,
                      int32_t method, int32_t max_lag, int32_t hop, int32_t window, int32_t sample_rate,
                      int32_t device_ptrs, sonar_result** out);

/* AlignmentExtractor.AlignAudioFiles (extractors/alignment.go:489-553) of an extractor built by
 * NewAlignmentExtractorWithMaxLag (:99-136) from FeatureConfig{feature_sample_rate, hop, window}:
 * ShortTimeEnergy (algorithms/temporal/energy.go:25-50) of both streams, then the Hybrid
 * AlignFeatures at maxLagFrames = int(max_lag_seconds * feature_sample_rate) / hop.  *out: the
 * sonar_analyzer_align_features keys (BestAlignment) plus the AlignmentFeatures fields
 * "temporal_offset", "offset_confidence", "alignment_similarity", "alignment_quality",
 * "feature_similarity_energy", "query_length_seconds", "reference_length_seconds", "time_stretch"
 * (never set by Go: 0) and "max_lag_frames"; Method is always "energy_correlation".  Errors as Go:
 * "alignment failed: empty feature sequences provided"; hop 0 panics ("integer divide by zero"). */
int sonar_align_audio_files(sonar_ctx* ctx, const double* q_pcm, int64_t nq, const double* r_pcm, int64_t nr,
                            int32_t sample_rate, int32_t feature_sample_rate, int32_t hop, int32_t window,
                            double max_lag_seconds, int32_t device_ptrs, sonar_result** out);

/* AlignmentExtractor.TruncateToAlignmentPCM (extractors/alignment.go:223-297) as sample indices:
 * the aligned segments are pcm1[start1 : start1+length] and pcm2[start2 : start2+length] (the
 * PCM stays where it is, e.g. in HBM).  Errors as Go: "offset too large ...", "no overlapping
 * audio after alignment". */
int sonar_truncate_to_alignment(sonar_ctx* ctx, int64_t n1, int64_t n2, int32_t sample_rate, double temporal_offset,
                                int64_t* start1, int64_t* start2, int64_t* length);

/* The two MusicFeatureExtractor.ExtractFeatures outputs that the alignment extractor consumes
 * (fingerprint/extractors/music.go:178-245): preprocessAudio (DC removal R = 0.995, then
 * pre-emphasis 0.95, :245-259) -> extractEnergyFeatures' ShortTimeEnergy with the extractor's
 * FeatureConfig WindowSize/HopSize (:460-466, temporal/energy.go:25-50) and
 * extractChromaFeatures (:327-376): spectrogram frames F = sonar_stft_frames(n, stft_window,
 * stft_hop), frame length n / F, hop = FeatureConfig.HopSize.  energy has
 * sonar_energy_frames(n, feature_window, feature_hop) entries, chroma F x 12.  float64. */
int sonar_music_alignment_features(sonar_ctx* ctx, const double* pcm, int64_t n, int32_t sample_rate,
                                   int32_t stft_window, int32_t stft_hop, int32_t feature_window,
                                   int32_t feature_hop, double* energy, double* chroma, int32_t device_ptrs);

/* ---- ContentDetector (fingerprint/content_detector.go) -----------------------------
 * DetectFromAudio (:72-101): zero-crossing rate, energy variance, silence ratio, dynamic range
 * and temporal stability over the whole PCM, the spectral centroid / frequency split /
 * harmonic ratio of a direct DFT of the first min(2048, n) samples, then classifyFromFeatures
 * (:153-217).  Go picks among equal best scores in map order (random); here the order is
 * music, news, talk, sports. */
typedef struct {                     /* AcousticFeatures (:104-115) */
  double zero_crossing_rate, spectral_centroid, energy_variance, silence_ratio, harmonic_ratio;
  double low_freq_energy, high_freq_energy, dynamic_range, temporal_stability;
  double classification_confidence;
} sonar_acoustic_features;

/* content_type <- SONAR_CT_* (SONAR_CT_UNKNOWN when no score beats the threshold).
 * sample_rate < 10 -> SONAR_ERR_INVALID (the 100 ms frame loop never ends in Go). */
int sonar_detect_from_audio(sonar_ctx* ctx, const double* pcm, int64_t n, int32_t sample_rate,
                            double auto_detect_threshold, int32_t* content_type,
                            sonar_acoustic_features* features);

/* DetectContentType (:31-69): metadata first (parseContentType of Metadata.ContentType, else
 * inferFromGenre, else inferFromStation on station + URL), then DetectFromAudio when
 * acoustic_detection is set and n > 0, else default_content_type.  has_metadata = 0 is a nil
 * Metadata; NULL strings are "". */
int sonar_detect_content_type(sonar_ctx* ctx, const double* pcm, int64_t n, int32_t sample_rate,
                              int32_t has_metadata, const char* content_type, const char* genre,
                              const char* station, const char* url, int32_t acoustic_detection,
                              int32_t default_content_type, double auto_detect_threshold,
                              int32_t* out_content_type);

/* ---- FingerprintComparator (fingerprint/comparison.go) ------------------------------
 * The comparator's candidate set lives on the device as a gallery of per-fingerprint
 * summary records (MFCC column mean/std, chroma column means, mean/std of the compared
 * sequences, the scalars and weights).  Compare() in the reference rebuilds those
 * statistics from the full feature arrays on every call (comparison.go:344-402,
 * 646-770, 774-842); they depend on one fingerprint only, so they are reduced once per
 * fingerprint when it is added, and every comparison reads two records.  Results are the
 * reference's formulas on the same statistics. */

/* config.ContentType (fingerprint/config/config.go:39-48).  Any other content-type string
 * is given its own code >= SONAR_CT_UNKNOWN by the caller, so ContentTypeMatch (string
 * equality, comparison.go:157) keeps distinct unknown strings apart. */
enum { SONAR_CT_MUSIC = 0, SONAR_CT_NEWS, SONAR_CT_SPORTS, SONAR_CT_TALK, SONAR_CT_MIXED,
       SONAR_CT_UNKNOWN };

/* sonar_fp_features.present: which members of AudioFingerprint.Features are non-nil */
enum {
  SONAR_FEAT_FEATURES = 1u << 0,   /* Features != nil                                    */
  SONAR_FEAT_MFCC = 1u << 1,       /* Features.MFCC != nil                               */
  SONAR_FEAT_SPECTRAL = 1u << 2,   /* Features.SpectralFeatures != nil                   */
  SONAR_FEAT_CHROMA = 1u << 3,     /* Features.ChromaFeatures != nil                     */
  SONAR_FEAT_TEMPORAL = 1u << 4,   /* Features.TemporalFeatures != nil                   */
  SONAR_FEAT_SPEECH = 1u << 5,     /* Features.SpeechFeatures != nil                     */
  SONAR_FEAT_HARMONIC = 1u << 6,   /* Features.HarmonicFeatures != nil                   */
  SONAR_FEAT_WEIGHTS = 1u << 7     /* Metadata["feature_weights"] is a map[string]float64 */
};

/* FeatureDistances keys (comparison.go:284-330), bit i of sonar_similarity.distance_mask */
enum { SONAR_FD_MFCC = 0, SONAR_FD_SPECTRAL, SONAR_FD_CHROMA, SONAR_FD_TEMPORAL, SONAR_FD_SPEECH,
       SONAR_FD_HARMONIC };

/* One AudioFingerprint as the comparator reads it (fingerprint.go:15-26,
 * extractors/features.go).  Matrices are row-major float64; MFCC rows are len(mfcc[0])
 * wide -- a shorter Go row is padded with 0 (the value extractMFCCStatistics uses for a
 * missing coefficient, comparison.go:784-789).  A sequence with n_* = 0 is empty. */
typedef struct {
  int64_t id;                      /* AudioFingerprint.ID, interned (self-skip, comparison.go:218) */
  uint32_t present;                /* SONAR_FEAT_*                                        */
  int32_t content_type;            /* SONAR_CT_* (or a distinct code >= SONAR_CT_UNKNOWN)  */
  double duration_seconds;         /* Duration.Seconds()                                  */
  const double* mfcc; int64_t mfcc_frames; int32_t mfcc_coeffs;
  const double* chroma; int64_t chroma_frames; int32_t chroma_bins;
  const double* spectral_centroid; int64_t n_spectral_centroid;
  const double* spectral_rolloff; int64_t n_spectral_rolloff;
  const double* spectral_flux; int64_t n_spectral_flux;
  double dynamic_range, silence_ratio, onset_density;          /* TemporalFeatures     */
  const double* rms_energy; int64_t n_rms_energy;
  double speech_rate, vocal_tract_length;                      /* SpeechFeatures       */
  const double* voicing_probability; int64_t n_voicing_probability;
  const double* harmonic_ratio; int64_t n_harmonic_ratio;      /* HarmonicFeatures     */
  const double* pitch_estimate; int64_t n_pitch_estimate;
  double feature_weights[6];       /* Metadata weights by SONAR_FD_* (absent key = 0)     */
} sonar_fp_features;

/* config.ComparisonConfig (fingerprint/config/config.go:68-80) */
typedef struct {
  double similarity_threshold;
  int32_t max_candidates;
  int32_t enable_detailed_metrics;
  int32_t enable_content_filter;
  int32_t method;                  /* 0 auto, 1 fast, 2 precise (Compare ignores it, :133-194) */
} sonar_compare_cfg;

/* SimilarityResult (comparison.go:28-39) */
typedef struct {
  double overall_similarity;
  double feature_similarity;
  double confidence;
  double feature_distances[6];     /* by SONAR_FD_*, where distance_mask has the bit      */
  double data_availability, feature_coverage, temporal_alignment;   /* QualityMetrics,   */
  double noise_level, dynamic_range_match, spectral_coherence;      /* when has_quality  */
  uint32_t distance_mask;
  int32_t content_type_match;
  int32_t has_quality;
  int32_t status;                  /* 0 compared, 1 skipped (same ID), 2 calculateFeatureSimilarity
                                      returned an error (nil features / nothing comparable) */
} sonar_similarity;

enum { SONAR_MATCH_EXACT = 0, SONAR_MATCH_VERY_SIMILAR, SONAR_MATCH_SIMILAR,
       SONAR_MATCH_SOMEWHAT_SIMILAR, SONAR_MATCH_WEAK };   /* classifyMatch, comparison.go:1040-1052 */

typedef struct {                   /* Match (comparison.go:52-58) */
  int64_t candidate;               /* position in the candidates list of the call          */
  int32_t rank;                    /* 1-based                                              */
  int32_t match_type;              /* SONAR_MATCH_*                                        */
  sonar_similarity similarity;
} sonar_match;

typedef struct sonar_gallery sonar_gallery;
int sonar_gallery_create(sonar_ctx* ctx, sonar_gallery** out);
void sonar_gallery_destroy(sonar_gallery* g);
int64_t sonar_gallery_size(const sonar_gallery* g);
/* Append `count` fingerprints: their statistics are reduced on the device and only the
 * records stay resident.  keep_sequences keeps SpectralCentroid / SpectralRolloff on the
 * device for EnableDetailedMetrics' spectral coherence (comparison.go:977-1008).
 * device_ptrs: the feature arrays are device pointers.  Index of the first -> *first. */
int sonar_gallery_add(sonar_gallery* g, const sonar_fp_features* fps, int32_t count,
                      int32_t keep_sequences, int32_t device_ptrs, int64_t* first);
/* FingerprintComparator.Compare / BatchCompare (comparison.go:133-194, 1107-1151) for every
 * (query, candidate) pair: out[q * nc + c].  candidates NULL -> the whole gallery
 * (nc = sonar_gallery_size).  A pair with equal IDs gets status 1 (BatchCompare drops it).
 * Detailed metrics need SpectralCentroid / SpectralRolloff of equal length on both sides
 * when both are non-empty (gonum stat.Correlation panics otherwise) -> SONAR_ERR_INVALID.
 * device_ptrs: out is a device pointer. */
int sonar_compare(sonar_gallery* g, const int64_t* queries, int64_t nq, const int64_t* candidates,
                  int64_t nc, const sonar_compare_cfg* cfg, sonar_similarity* out, int32_t device_ptrs);
/* FingerprintComparator.FindBestMatches (comparison.go:197-263) per query: matches with
 * OverallSimilarity >= threshold, descending, at most max_candidates, ranked from 1.
 * out[q * max_candidates + k], n_matches[q].  Equal similarities keep candidate order. */
int sonar_find_best_matches(sonar_gallery* g, const int64_t* queries, int64_t nq,
                            const int64_t* candidates, int64_t nc, const sonar_compare_cfg* cfg,
                            sonar_match* out, int64_t* n_matches);

/* FindBestMatches over candidates split across ranks: lists[r] holds rank r's
 * sonar_find_best_matches output (nq x max_candidates, row q at q * max_candidates) with
 * counts[r * nq + q] valid entries and its candidates numbered from cand_base[r].  out / n_out:
 * the result of ONE call over all ranks' candidates -- similarity descending (the single call's
 * radix order), equal similarities in global candidate order, at most max_candidates, ranked
 * from 1, candidate = cand_base[r] + local position.  Host-only (no device); the rank-local lists
 * can come from other processes (torch.distributed all-gather) or sonar_find_best_matches_multi. */
int sonar_merge_matches(const sonar_match* const* lists, const int64_t* counts, const int64_t* cand_base,
                        int32_t nlists, int64_t nq, int32_t max_candidates, sonar_match* out, int64_t* n_out);

/* FingerprintComparator.FindBestMatches (fingerprint/comparison.go:197-263) over rank-local
 * galleries: galleries[g] lives on rank g's context (sonar_multi_ctx); queries[g] are the query
 * fingerprints' indices in galleries[g] (every rank holds the queries); candidates[g] / nc[g] rank
 * g's candidates (candidates NULL: every gallery whole, nc ignored).  Each rank ranks its own
 * candidates, the per-rank top max_candidates travel through one RCCL all-gather, and
 * sonar_merge_matches gives out[q * max_candidates + k] / n_matches[q] equal to one call over the
 * concatenated candidates (rank g's numbered after those of ranks 0..g-1).  Synchronous. */
int sonar_find_best_matches_multi(sonar_multi* m, sonar_gallery* const* galleries, const int64_t* const* queries,
                                  int64_t nq, const int64_t* const* candidates, const int64_t* nc,
                                  const sonar_compare_cfg* cfg, sonar_match* out, int64_t* n_matches);

/* ---- PitchDetector in full (algorithms/tonal/pitch_detection.go): every method of DetectPitch's
 * switch (:239-260) at any supported window, threshold and frequency range, its post-processing and
 * temporal tracking, ProcessAudioStream and AnalyzePitchStability.  sonar_pitch_yin above stays the
 * constructor-default YIN core; at the defaults the YIN rows here are the same bits. ------------- */
enum {                             /* PitchDetectionMethod (:16-35), Go's values */
  SONAR_PITCH_YIN = 0,
  SONAR_PITCH_ACF = 1,
  SONAR_PITCH_NSDF = 2,
  SONAR_PITCH_HPS = 3,
  SONAR_PITCH_CEPSTRUM = 4,
  SONAR_PITCH_PEAKS = 5,           /* detectPitchPeaks is detectPitchHPS (:687-691) */
  SONAR_PITCH_ZERO_CROSSING = 6,
  SONAR_PITCH_PEAK_PICKING = 7,    /* not in the switch: "unsupported pitch detection method: 7" */
  SONAR_PITCH_YIN_FFT = 8,         /* detectPitchYinFFT is detectPitchYin (:730-733) */
  SONAR_PITCH_MPM = 9,             /* detectPitchMPM is detectPitchNSDF (:736-740) */
  SONAR_PITCH_PRAAT = 10           /* not in the switch */
};
enum {                             /* createWindowFunction's strings (:317-345); Go maps every other string to
                                      Hann, which the bindings do before they fill the field */
  SONAR_PITCH_WIN_HANN = 0,
  SONAR_PITCH_WIN_HAMMING = 1,
  SONAR_PITCH_WIN_BLACKMAN = 2,
  SONAR_PITCH_WIN_RECTANGULAR = 3
};
/* PitchDetectionParams (:84-117) field for field.  The reference never reads cepstral_threshold,
 * min_salience, voicing_threshold, max_harmonics and harmonic_tolerance; hop_size is read only by
 * estimateVibratoRate (:1156) -- the entries here also use it as the frame step of a signal, which in Go
 * is the caller's slicing.  The library ignores the never-read fields as well. */
typedef struct sonar_pitch_params {
  int32_t method;                  /* SONAR_PITCH_* */
  int32_t sample_rate;
  int32_t window_size;
  int32_t hop_size;
  double min_freq, max_freq;
  double yin_threshold;
  double autocorr_threshold;       /* ACF and NSDF peaks; see the un-normalised ACF below */
  double cepstral_threshold;       /* never read */
  double min_confidence;
  double min_salience;             /* never read */
  double voicing_threshold;        /* never read */
  int32_t max_harmonics;           /* never read */
  double harmonic_tolerance;       /* never read */
  int32_t pre_emphasis;            /* 0 / 1: y[i] = x[i] - 0.97 x[i - 1], fresh per frame (:300-314) */
  int32_t window_function;         /* SONAR_PITCH_WIN_*, denominator W - 1 */
  int32_t zero_padding;            /* HPS / PEAKS: the transform has W * zero_padding points */
  int32_t median_filter;
  int32_t temporal_smoothing;      /* 0 / 1 */
  int32_t octave_correction;       /* 0 / 1 */
} sonar_pitch_params;

/* NewPitchDetector(sample_rate) (:159-193): YIN, 1024 / 512, 80-1000 Hz, 0.15, 0.3, 0.3, 0.5, 0.1, 0.45,
 * 10, 0.1, pre-emphasis, Hann, zero padding 2, median 3, smoothing and octave correction on. */
void sonar_pitch_params_default(sonar_pitch_params* p, int32_t sample_rate);

/* n < W ? 0 : (n - W) / H + 1 whole frames of W samples every H: DetectPitch rejects a frame of any
 * other length (:226), so a trailing partial frame does not count.  W < 1 or H < 1 gives 0. */
int64_t sonar_pitch_detect_frames(int64_t n, int32_t window_size, int32_t hop_size);

/* The parameter checks of the entries below, without a device, and the width of a frame's curve:
 * YIN / YIN_FFT the CMNDF, W / 2; NSDF / MPM the NSDF, W / 2; ACF the correlations (AutocorrPeaks,
 * lags -(W - 1) .. W - 1), 2 W - 1; HPS / PEAKS the harmonic product, W * zero_padding / 2; cepstrum the
 * real cepstrum, W; zero crossing none, 0.  Returns the width or a negative SONAR_ERR_*:
 *   PEAK_PICKING, PRAAT and unknown methods -> SONAR_ERR_INVALID "unsupported pitch detection method: N"
 *     (:259), before anything else is looked at;
 *   hop_size < 1 or sample_rate < 1 -> SONAR_ERR_INVALID;
 *   not 0 < min_freq < max_freq, both finite -> SONAR_ERR_INVALID (a documented narrowing: Go would
 *     divide by zero or convert an infinity to int);
 *   HPS / PEAKS with zero_padding < 1 -> SONAR_ERR_PANIC (hps[0] of an empty slice, :580);
 *   cepstrum with int(sample_rate / max_freq) >= W -> SONAR_ERR_PANIC (:650);
 *   window_size not a power of two in [64, 2048], or HPS / PEAKS with zero_padding not 1, 2 or 4 or
 *     W * zero_padding > 4096, or a window_function outside the enum -> SONAR_ERR_UNSUPPORTED (the
 *     largest transform, the ACF's 2 W included, fits one 4096-point LDS tile). */
int64_t sonar_pitch_curve_width(const sonar_pitch_params* p);

/* DetectPitch up to postProcessResult, per frame f of pcm (float64, n samples; host pointers, or
 * device pointers for pcm and every output when device_ptrs is set): preprocessFrame (:282-345), then
 * the method.  Outputs, F = sonar_pitch_detect_frames(n, W, H) entries each unless noted; all but pitch
 * and confidence may be NULL:
 *   pitch, confidence   what detectPitch* returns (Periodicity and Voicing equal confidence)
 *   index               the chosen lag (YIN: minTau, also when its frequency is out of range; ACF, NSDF),
 *                       bin (HPS), quefrency (cepstrum) or the crossing count; -1 when none
 *   n_candidates        len(Candidates), all of them, not only the reported ones
 *   second_confidence   Candidates[1].Confidence for calculateClarity (:840), 0 with fewer than two
 *   cand_index, cand_conf   F x max_candidates (0..8): the best candidates by descending confidence;
 *                       unused slots are -1 and 0
 *   curve               F x sonar_pitch_curve_width(p)
 * Quirks of the reference kept here:
 *  - YIN / YIN_FFT (:349-420): halfN = W / 2, the first tau with cmndf < yin_threshold that is below its
 *    right neighbour, parabolic interpolation, the frequency gate; bit-identical to a sequential float64
 *    evaluation in Go's order (and to sonar_pitch_yin at the defaults).
 *  - NSDF / MPM (:485-550): acf, m1 and m2 are three sums in j order; peaks are strict local maxima above
 *    autocorr_threshold at 1 <= i <= W/2 - 2 with sample_rate / i in range.  Bit-identical.
 *  - ACF (:423-482): AutoCorrelation.Compute on the preprocessed frame exactly as sonar_autocorr defines
 *    it with max_lag 2 W, i.e. use_fft is set and the regime depends on W: W > 1000 is the
 *    frequency-domain regime, z-score, N = 2 W, re(ifft(fft conj(fft))) / N and NOT normalised further, so
 *    autocorr_threshold compares values of the order of W (lag 0 is W); W <= 512 is Pearson per lag in
 *    [-1, 1].  Candidates are lags 1 .. W - 2.  Bit-identical to sonar_autocorr on the same frame.
 *  - Candidate order: Go's sort.Slice is not stable, so the reference leaves the order of equal
 *    confidences unspecified; the library orders them by ascending lag.
 *  - HPS / PEAKS (:553-620): zero-padded to W * zero_padding, |X| of the first half, times the harmonics
 *    2..5 over len / h bins; the scan over [int(min_freq N / sr), int(max_freq N / sr)) clipped to the
 *    length starts from maxIdx = 0, maxVal = hps[0] with a strict >, so when nothing beats bin 0 the pitch
 *    is 0 Hz and a confidence min(maxVal / 1000, 1) is still reported.  The transform is go-dsp's in the
 *    reference: parity at tolerance.
 *  - Cepstrum (:623-684): ln(|X| + 1e-10) of the W-point spectrum, the inverse transform's real part, the
 *    scan from int(sr / max_freq) to min(int(sr / min_freq), W) with a strict >, pitch sr / index,
 *    confidence min(max / 0.1, 1), which may be negative.  Parity at tolerance.
 *  - Zero crossing (:694-727): crossings of the preprocessed frame, pitch crossings sr / (2 W),
 *    confidence 0.3 (which the default min_confidence gate zeroes).
 * Errors: those of sonar_pitch_curve_width; max_candidates outside 0..8, n < 0, NULL pcm with frames
 * due, NULL pitch or confidence -> SONAR_ERR_INVALID.  F == 0 succeeds and writes nothing. */
int sonar_pitch_frames_raw(sonar_ctx* ctx, const double* pcm, int64_t n, const sonar_pitch_params* p,
                           int32_t max_candidates, double* pitch, double* confidence, int32_t* index,
                           int32_t* n_candidates, double* second_confidence, int32_t* cand_index,
                           double* cand_conf, double* curve, int32_t device_ptrs);

/* postProcessResult + updateTemporalTracking (:767-963) over F raw rows in order, from an empty history
 * (a fresh detector, or one after Reset).  Host-only, no context.  Per frame:
 *  - octave correction (octave_correction) of a non-zero pitch against the median of the positive ones
 *    among the last five history entries, once three entries exist: ratios 0.5, 2, 1/3, 3 in that order,
 *    the first within 10 % decides, and the pitch moves to median * ratio (f0_multiple = ratio) only when
 *    that is closer to the median; f0_multiple is 0 otherwise;
 *  - clarity (:830-849), strength and salience (:852-873) are computed BEFORE the min_confidence gate;
 *  - the gate (:783-787) zeroes pitch, confidence and voicing but not periodicity;
 *  - the history holds the last 20 gated, octave-corrected and UNSMOOTHED pitches; stability
 *    (calculateStability :924-963) runs over it;
 *  - smoothing (temporal_smoothing, from the second frame): the median of the positive entries among the
 *    last median_filter ones when at least three exist (median_filter above 20 reads the whole history,
 *    below 1 none), otherwise 0.3 p + 0.7 previous, previous being the last smoothed pitch.
 * Reads octave_correction, temporal_smoothing, median_filter and min_confidence of p.  n_candidates and
 * second_confidence may be NULL (one candidate whenever the raw confidence is not 0).  Every output may
 * be NULL. */
int sonar_pitch_track(const sonar_pitch_params* p, int64_t F, const double* raw_pitch,
                      const double* raw_confidence, const int32_t* n_candidates, const double* second_confidence,
                      double* pitch, double* confidence, double* voicing, double* periodicity, double* clarity,
                      double* strength, double* salience, double* stability, double* f0_multiple);

/* ProcessAudioStream (:1016-1028) over the frames of pcm: sonar_pitch_frames_raw, then
 * sonar_pitch_track, in one call.  With device_ptrs, pcm and the nine outputs are device pointers. */
int sonar_pitch_detect(sonar_ctx* ctx, const double* pcm, int64_t n, const sonar_pitch_params* p, double* pitch,
                       double* confidence, double* voicing, double* periodicity, double* clarity, double* strength,
                       double* salience, double* stability, double* f0_multiple, int64_t* frames,
                       int32_t device_ptrs);

/* AnalyzePitchStability + estimateVibratoRate (:1059-1160) of a pitch sequence.  Host-only.  out7:
 * mean_pitch, pitch_std_dev, coefficient_of_variation, jitter, stability, vibrato_rate,
 * voiced_frames_ratio; *empty = 1 and zeros for the empty map Go returns with fewer than two entries or
 * fewer than two voiced (> 0) ones.  The vibrato rate is 0 below ten voiced frames and reads
 * sample_rate / hop_size. */
int sonar_pitch_stability(const double* pitch, int64_t n, int32_t sample_rate, int32_t hop_size, double* out7,
                          int32_t* empty);

/* ---- HarmonicRatioAnalyzer in full (algorithms/tonal/harmonic_ratio.go): every method of AnalyzeFrame's
 * switch (:228-243), its post-processing and temporal tracking, AnalyzeSequence and the helpers.
 * Everything is float64.  sonar_extract_music_features keeps writing its harmonic_ratio row as zeros
 * (SURVEY.md F7); these entries are the analyzer itself. ------------------------------------------ */
enum {                             /* HarmonicRatioMethod (:17-24), Go's values; every other value is HNR, the
                                      switch's default case (:241) */
  SONAR_HRATIO_HNR = 0,
  SONAR_HRATIO_ACF = 1,
  SONAR_HRATIO_HPS = 2,
  SONAR_HRATIO_COMB = 3,           /* analyzeComb is analyzeHNR (:457-461) */
  SONAR_HRATIO_SPECTRAL = 4,
  SONAR_HRATIO_YIN = 5
};
enum {                             /* NoiseFloorMethod's strings (:633-642); Go maps every other string to
                                      "percentile", which the bindings do before they fill the field, and so
                                      does the library with every other value */
  SONAR_HRATIO_NOISE_MEDIAN = 0,
  SONAR_HRATIO_NOISE_PERCENTILE = 1,
  SONAR_HRATIO_NOISE_MINIMUM = 2
};
enum {                             /* ClassifyHarmonicRatio's categories (:1130-1142) */
  SONAR_HRATIO_VERY_LOW = 0, SONAR_HRATIO_LOW = 1, SONAR_HRATIO_MEDIUM = 2, SONAR_HRATIO_HIGH = 3,
  SONAR_HRATIO_VERY_HIGH = 4
};
#define SONAR_HRATIO_MAX_HARMONICS 64
/* HarmonicRatioParams (:27-57) field for field, and autocorr_max_lag: the argument of the analyzer's
 * NewAutoCorrelation, 2048 in NewHarmonicRatioAnalyzer (:157) and WindowSize in ...WithParams (:171).
 * The reference never reads use_freq_weighting, use_psychoacoustic_mask and adaptive_threshold, and reads
 * hop_size nowhere either: the entries here use it as the frame step of a signal, which in Go is the
 * caller's slicing.  The library ignores the never-read fields as well.  min_peak_height is the height of
 * the analyzer's peak detector, NewSpectralPeaks(sample_rate, min_peak_height, 20.0, 100): 0.001 in
 * NewHarmonicRatioAnalyzer, which hard-codes it (:155), and params.MinPeakHeight in ...WithParams (:169);
 * nothing else reads the field. */
typedef struct sonar_hratio_params {
  int32_t method;                  /* SONAR_HRATIO_* */
  int32_t sample_rate;
  int32_t window_size;
  int32_t hop_size;                /* never read by the reference; the frame step here */
  double min_freq, max_freq;
  int32_t max_harmonics;
  double harmonic_tolerance;
  double min_peak_height;
  int32_t peak_detection_width;
  int32_t spectral_smoothing_len;
  int32_t noise_floor_method;      /* SONAR_HRATIO_NOISE_* */
  double noise_floor_percentile;
  int32_t noise_floor_smoothing_len;
  int32_t use_temporal_smoothing;  /* 0 / 1 */
  int32_t temporal_smoothing_len;
  int32_t use_freq_weighting;      /* never read */
  int32_t use_psychoacoustic_mask; /* never read */
  int32_t adaptive_threshold;      /* never read */
  int32_t autocorr_max_lag;
} sonar_hratio_params;

/* NewHarmonicRatioAnalyzer(sample_rate) (:130-161): HNR, 2048 / 512, 80-8000 Hz, 20 harmonics, tolerance
 * 0.1, height 0.001, width 3, smoothing 5, "percentile" 0.1 smoothed over 10, temporal smoothing on over 5,
 * the three unread switches off, autocorr_max_lag 2048. */
void sonar_hratio_params_default(sonar_hratio_params* p, int32_t sample_rate);

/* The parameter checks of the entries below, without a device.  SONAR_OK or a negative SONAR_ERR_*:
 *   NULL params -> SONAR_ERR_INVALID;
 *   sample_rate < 1 or hop_size < 1 -> SONAR_ERR_INVALID;
 *   min_freq, max_freq, harmonic_tolerance or min_peak_height not finite -> SONAR_ERR_INVALID (a documented
 *     narrowing: Go would convert an infinity or a NaN to int);
 *   noise_floor_method percentile (or unknown) with a NaN noise_floor_percentile -> SONAR_ERR_PANIC "stat:
 *     percentile out of bounds" (common.Percentile's own range test lets a NaN through to gonum, HNR and
 *     Comb included: computeSpectrum estimates the floor under every method);
 *   method HPS with int(min_freq W / sr) < 0 and a scan that starts (int(max_freq W / sr) above it) ->
 *     SONAR_ERR_PANIC "runtime error: index out of range [-N]" (hps[i] :434);
 *   temporal_smoothing_len < 0 -> SONAR_ERR_PANIC "runtime error: slice bounds out of range [a:b]" with
 *     a = 1 + 2 |len|, b = 1 (hrHistory[len - maxHistory:] :996, at the first frame), from
 *     sonar_hratio_track and sonar_hratio only: the per-frame entries never reach that line;
 *   window_size not a power of two in [64, 2048] (the LDS tile of the transform, go-dsp's radix-2 branch),
 *     max_harmonics > 64, autocorr_max_lag < window_size - 1 (fewer than all lags; both constructors give
 *     all of them at a supported window), |min_freq| or |max_freq| times W / sr beyond 2^31 ->
 *     SONAR_ERR_UNSUPPORTED.
 * A frame-size mismatch (:213) cannot occur: the entries slice the frames themselves. */
int sonar_hratio_check(const sonar_hratio_params* p);

/* Everything AnalyzeFrame does after the transform for the methods HNR, COMB (which is HNR), HPS and
 * SPECTRAL, on F rows of K = W / 2 unsmoothed magnitudes |X| (computeSpectrum's hra.magnitude before :286)
 * and, optionally, their phases.  Host pointers, or device pointers for mag, phase and every output when
 * device_ptrs is set.  Every output may be NULL and then costs nothing.  Per frame:
 *   harmonic_ratio (raw, before postProcessResult's smoothing), harmonic_energy, noise_energy,
 *   total_energy, f0, f0_confidence, snr, periodicity, harmonicity, voicing, roughness, num_harmonics;
 *   h_bin, h_freq, h_amp, h_phase: F x max_harmonics, the result's SpectralPeaks (BinIndex, Frequency,
 *   Magnitude, Phase), which HNR also copies to HarmonicFrequencies / Amplitudes / Phases; slots past
 *   num_harmonics are -1 for h_bin and 0 for the rest; h_phase is 0 when phase is NULL;
 *   noise_floor: F x K.
 * Fields a method leaves unset in Go's result are 0: HPS sets harmonic_ratio, f0, the peaks and
 * num_harmonics; SPECTRAL adds the three energies; HNR sets all of them.
 * Quirks of the reference kept here:
 *  - MovingAverage (common/math.go:140-166) is a trailing window: entry i < L averages 0..i, the others
 *    the L entries ending at i, sums in j order; L > K or L <= 0 returns the input.  Smoothing runs only
 *    for a length above 1 (:286, :645).
 *  - The noise floor (:650-705) of bin i looks at [max(0, i - 10), min(K, i + 10)), 10 to 20 values.
 *    common.Percentile is gonum's stat.Quantile(p, stat.Empirical, sorted, nil): the first sorted value
 *    whose count reaches p n (x[0] at p = 0); "median" is that at 0.5, not a mean of two.  gonum is restated
 *    from its published rule, parity unpinned.  A percentile outside [0, 1] gives a floor of zeros
 *    (math.go:39) and an SNR of 60.
 *  - detectFundamentalFrequency (:546-563) walks DetectPeaks' output, sorted by magnitude descending, for
 *    its "lowest significant peak": f0 is the strongest of the 100 strongest peaks at or above min_freq,
 *    else the strongest of all; f0_confidence is that peak's magnitude, not a value in [0, 1].  No peak:
 *    f0 0, no harmonics, harmonic_energy 0 and harmonic_ratio -Inf when there is noise energy.
 *  - The detector runs on the K smoothed magnitudes as sonar_spectral_peaks defines it, with
 *    DetectPeaks(mag, W): equal magnitudes in ascending bin order, also for estimateF0FromPeaks' second
 *    sort.  At a power-of-two W, i sr / W (freqBins :195) and i (sr / W) (the detector) are the same double,
 *    because sr / W is exact.
 *  - findNearestPeak (:596-630) does not use the detector: a strict > scan from maxMag = 0 over
 *    int(f W / sr) +- peak_detection_width (an all-zero stretch leaves the target bin), then a strict local
 *    maximum test at 1 .. K - 2.  Its magnitude is the smoothed one, its phase the unsmoothed spectrum's.
 *    Several harmonics can return the same bin; it is then listed several times.
 *  - The mask (:312-320) is laid around int(peak.Frequency W / sr), which can be one below BinIndex.
 *  - noise_energy > 0 else 60 dB; harmonic_energy 0 with noise gives -Inf.
 *  - HPS (:413-454): harmonics 2 .. min(5, max_harmonics); the scan starts from maxIdx 0, maxVal hps[0]
 *    with a strict >, so when nothing beats bin 0 the f0 is 0 Hz and there are no harmonics.
 *  - SPECTRAL (:463-512): the energies are sums over the peaks in [min_freq, max_freq], in the detector's
 *    order; noise_energy = total_energy - harmonic_energy is exactly 0, and the ratio 60 dB, when every
 *    peak is harmonic (two sums over the same terms in the same order).
 * Errors: those of sonar_hratio_check; methods ACF and YIN (they need the samples), K != W / 2, F < 0, NULL
 * mag with frames due -> SONAR_ERR_INVALID.  F == 0 succeeds and writes nothing. */
int sonar_hratio_from_spectrum(sonar_ctx* ctx, const double* mag /* F x K */, const double* phase /* F x K or NULL */,
                               int64_t F, int32_t K, const sonar_hratio_params* params, double* harmonic_ratio,
                               double* harmonic_energy, double* noise_energy, double* total_energy, double* f0,
                               double* f0_confidence, double* snr, double* periodicity, double* harmonicity,
                               double* voicing, double* roughness, int32_t* num_harmonics,
                               int32_t* h_bin /* F x max_harmonics */, double* h_freq, double* h_amp, double* h_phase,
                               double* noise_floor /* F x K */, int32_t device_ptrs);

/* AnalyzeFrame up to postProcessResult for every method, on the F = sonar_pitch_detect_frames(n, W, H)
 * whole frames of pcm; the outputs are sonar_hratio_from_spectrum's.
 *  - preprocessFrame (:260-270) multiplies by a Hann window with denominator W - 1 (:1004-1013).
 *  - HNR, COMB, HPS, SPECTRAL: the W-point transform, |X| and atan2 of the first W / 2 bins, then the
 *    stage above, one block per frame, nothing but results in device memory.  The transform is go-dsp's in
 *    the reference: parity at tolerance.
 *  - ACF (:385-411): AutoCorrelation.Compute of the windowed frame, the bits of sonar_autocorr on that
 *    frame.  Correlations[0] is lag -(W - 1), not lag 0, so calculatePeriodicityFromACF's "excluding lag
 *    0" (:823) excludes the wrong entry: periodicity and voicing are both max |corr| with lag 0 in it.
 *    harmonic_ratio = 20 log10(max / (1 - max + 1e-10)): at W > 1000 (the un-normalised frequency-domain
 *    regime, lag 0 of the order of W) the logarithm's argument is negative and the ratio is NaN; at
 *    W <= 512 (Pearson, lag 0 = 1) it is 20 log10(1e10) = 200.  Every other output is 0.
 *  - YIN (:515-542): a temporary PitchDetector with only method, rate, window and range set, on the
 *    already windowed frame: its threshold is 0, pre-emphasis off, and the empty window name means Hann,
 *    so the frame is windowed twice, (x w) w; min_confidence is 0 and there is no history.  Sets
 *    harmonic_ratio = 20 log10(confidence + 1e-10), f0, f0_confidence, periodicity and voicing.  The
 *    bits of sonar_pitch_frames_raw on the windowed frames.
 * Errors: those of sonar_hratio_check; n < 0 or NULL pcm with frames due -> SONAR_ERR_INVALID. */
int sonar_hratio_frames(sonar_ctx* ctx, const double* pcm, int64_t n, const sonar_hratio_params* params,
                        double* harmonic_ratio, double* harmonic_energy, double* noise_energy, double* total_energy,
                        double* f0, double* f0_confidence, double* snr, double* periodicity, double* harmonicity,
                        double* voicing, double* roughness, int32_t* num_harmonics, int32_t* h_bin, double* h_freq,
                        double* h_amp, double* h_phase, double* noise_floor, int32_t device_ptrs);

/* postProcessResult + updateTemporalTracking (:926-1002) over F raw rows in order, from an empty history (a
 * fresh analyzer, or one after Reset).  Host-only, no context.  Per frame: from the second frame on (and
 * with use_temporal_smoothing) harmonic_ratio = 0.3 raw + 0.7 previous, previous being the last smoothed
 * value; temporal_stability = max(0, 1 - sqrt(gonum variance) / mean) of the history once it has three
 * entries and a mean > 0, else 0 (gonum's stat.Mean and stat.Variance restated, parity unpinned);
 * temporal_coherence = exp(-mean |difference of neighbours| / 10) once it has two, else 0.  Both are
 * computed BEFORE the frame's own value enters the history, which holds the last 2 temporal_smoothing_len
 * smoothed values (none at 0: stability and coherence stay 0, the smoothing stops too).  raw_f0 is
 * accepted for f0History, which nothing reads; it may be NULL, and so may every output. */
int sonar_hratio_track(const sonar_hratio_params* params, int64_t F, const double* raw_harmonic_ratio,
                       const double* raw_f0, double* harmonic_ratio, double* temporal_stability,
                       double* temporal_coherence);

/* AnalyzeSequence (:1042-1054) over the whole frames of pcm: sonar_hratio_frames, then sonar_hratio_track,
 * in one call.  harmonic_ratio is the smoothed one; *frames receives F.  With device_ptrs, pcm and every
 * output array are device pointers. */
int sonar_hratio(sonar_ctx* ctx, const double* pcm, int64_t n, const sonar_hratio_params* params,
                 double* harmonic_ratio, double* temporal_stability, double* temporal_coherence,
                 double* harmonic_energy, double* noise_energy, double* total_energy, double* f0,
                 double* f0_confidence, double* snr, double* periodicity, double* harmonicity, double* voicing,
                 double* roughness, int32_t* num_harmonics, int32_t* h_bin, double* h_freq, double* h_amp,
                 double* h_phase, double* noise_floor, int64_t* frames, int32_t device_ptrs);

/* GetAverageHarmonicRatio (:1057-1077): the mean of the ratios above -60 (a NaN is not), 0 without any. */
double sonar_hratio_average(const double* harmonic_ratio, int64_t n);
/* ClassifyHarmonicRatio (:1130-1142) as SONAR_HRATIO_VERY_LOW .. VERY_HIGH (a NaN is "Very Low", the else
 * branch), and Go's strings; NULL for a category outside the enum. */
int32_t sonar_hratio_classify(double harmonic_ratio);
const char* sonar_hratio_category_name(int32_t category);
/* EstimateVoicingQuality (:1145-1148): 1 / (1 + exp(-0.1 (ratio - 5))). */
double sonar_hratio_voicing_quality(double harmonic_ratio);

/* ---- InharmonicityAnalyzer (algorithms/tonal/inharmonicity.go): AnalyzeFrame's harmonic search, every
 * method of its switch (:252-267), the physical model, the quality metrics, the temporal
 * tracking, AnalyzeSequence and the helpers.  Everything is float64.  sonar_extract_music_features keeps
 * writing its inharmonicity_ratio row as zeros; these entries are the analyzer itself.
 * DESIGN.md F100-F107 record the reference's quirks. --------------------------------------------------- */
enum {                             /* InharmonicityMethod (:17-24), Go's values; every other value is
                                      SpectralDeviation, the switch's default case (:265) */
  SONAR_INHARM_RAILSBACK = 0,
  SONAR_INHARM_FLETCHER_MUNSON = 1,
  SONAR_INHARM_SPECTRAL_DEVIATION = 2,
  SONAR_INHARM_PARTIAL_TRACKING = 3,   /* calculatePartialTrackingInharmonicity is SpectralDeviation (:548) */
  SONAR_INHARM_BEAT_PATTERN = 4,       /* needs the samples: sonar_inharm_frames and sonar_inharm only */
  SONAR_INHARM_STATISTICAL = 5
};
enum {                             /* InharmonicityModel (:29-34); only STRING changes a result (:847-896) */
  SONAR_INHARM_MODEL_STRING = 0, SONAR_INHARM_MODEL_PIPE = 1, SONAR_INHARM_MODEL_MEMBRANE = 2,
  SONAR_INHARM_MODEL_GENERAL = 3
};
enum {                             /* AnalysisQuality: assessAnalysisQuality's five strings (:1103-1137) and the
                                      early return's (:240); -1 on an INSUFFICIENT row, which has no result */
  SONAR_INHARM_QUALITY_VERY_POOR = 0, SONAR_INHARM_QUALITY_POOR = 1, SONAR_INHARM_QUALITY_FAIR = 2,
  SONAR_INHARM_QUALITY_GOOD = 3, SONAR_INHARM_QUALITY_EXCELLENT = 4, SONAR_INHARM_QUALITY_INVALID_F0 = 5
};
enum {                             /* what AnalyzeFrame returned for the frame */
  SONAR_INHARM_STATUS_OK = 0,
  SONAR_INHARM_STATUS_INVALID_F0 = 1,    /* the nil-error early return of :236-242 */
  SONAR_INHARM_STATUS_INSUFFICIENT = 2   /* the error of :369, "insufficient harmonics found: %d < %d" */
};
enum {                             /* ClassifyInharmonicity (:1272-1286) */
  SONAR_INHARM_VERY_LOW = 0, SONAR_INHARM_LOW = 1, SONAR_INHARM_MODERATE = 2, SONAR_INHARM_HIGH = 3,
  SONAR_INHARM_VERY_HIGH = 4
};
enum {                             /* EstimateInstrumentType (:1289-1313) */
  SONAR_INHARM_INSTRUMENT_PIANO_STRING = 0, SONAR_INHARM_INSTRUMENT_WIND_BRASS = 1,
  SONAR_INHARM_INSTRUMENT_PLUCKED_STRING = 2, SONAR_INHARM_INSTRUMENT_VOCAL_HARMONIC = 3,
  SONAR_INHARM_INSTRUMENT_UNKNOWN = 4
};
#define SONAR_INHARM_MAX_HARMONICS 64
/* InharmonicityParams (:37-72) field for field.  The reference never reads freq_resolution,
 * reference_harmonic, use_log_frequency, string_stiffness and confidence_level; the library ignores them
 * as well. */
typedef struct sonar_inharm_params {
  int32_t method;                  /* SONAR_INHARM_* */
  int32_t model;                   /* SONAR_INHARM_MODEL_* */
  int32_t sample_rate;
  int32_t window_size;
  int32_t max_harmonics;
  int32_t min_harmonics;
  double harmonic_tolerance;
  double min_harmonic_strength;
  double min_freq, max_freq;
  double freq_resolution;          /* never read */
  int32_t reference_harmonic;      /* never read */
  int32_t weight_by_amplitude;     /* 0 / 1 */
  int32_t use_log_frequency;       /* never read */
  double string_tension, string_length;
  double string_stiffness;         /* never read */
  double outlier_threshold;
  double confidence_level;         /* never read */
  int32_t use_robust_estimation;   /* 0 / 1 */
  int32_t use_temporal_tracking;   /* 0 / 1 */
  int32_t temporal_window;
} sonar_inharm_params;

/* NewInharmonicityAnalyzer(sample_rate) (:147-172): SpectralDeviation, the General model, window 4096, 20 / 3
 * harmonics, tolerance 0.05, strength 0.01, 80-2000 Hz, resolution 1, reference harmonic 1, amplitude weights
 * on, log frequency off, tension 1, length 1, stiffness 0.001, outlier threshold 2, confidence level 0.95,
 * robust estimation on, temporal tracking off over a window of 10.  The window of 4096 is the constructor's:
 * the analyzer's own PitchDetector takes frames of 1024 only (F100), so AnalyzeFrame fails at every frame
 * length with these defaults, and sonar_inharm_frames says so in Go's words. */
void sonar_inharm_params_default(sonar_inharm_params* p, int32_t sample_rate);

/* The parameter checks of the entries below, without a device.  SONAR_OK or a negative SONAR_ERR_*:
 *   NULL params -> SONAR_ERR_INVALID;
 *   sample_rate < 1 -> SONAR_ERR_INVALID;
 *   min_freq, max_freq, harmonic_tolerance or min_harmonic_strength not finite -> SONAR_ERR_INVALID (a
 *     documented narrowing: Go would convert an infinity or a NaN to int);
 *   max_harmonics > 64, or a search window max_freq (1 + |harmonic_tolerance|) window_size / sample_rate
 *     beyond 2^31 bins -> SONAR_ERR_UNSUPPORTED.
 * A negative temporal_window with use_temporal_tracking is not refused here: it is SONAR_ERR_PANIC "runtime
 * error: slice bounds out of range [a:1]", a = 1 + |temporal_window| (inharmonicityHistory[len - maxHistory:]
 * :1098, at the first frame that reaches the history), from sonar_inharm_track and sonar_inharm only. */
int sonar_inharm_check(const sonar_inharm_params* p);

/* Everything AnalyzeFrame does after the transform (:236-292, without postProcessResult's tracking), on F
 * rows of K = W / 2 magnitudes |X[0 .. W/2 - 1]| of the unwindowed frame (:206, :321-328) and each frame's
 * f0 and its confidence (the analyzer's PitchDetector gives them; here they are inputs).  W = 2 K replaces
 * params->window_size, K from 4 to 4096: the row is only loaded.  Host pointers, or device pointers for
 * mag, f0, f0_confidence and every output when device_ptrs is set.  Every output may be NULL and then
 * costs nothing.  Per frame:
 *   status: SONAR_INHARM_STATUS_*;
 *   inharmonicity (raw, before postProcessResult's smoothing), std_dev, confidence;
 *   f0_out, f0_confidence_out: the inputs (F0Frequency, F0Confidence);
 *   num_harmonics: len(harmonicData.frequencies); n_deviations: len(HarmonicDeviations), which Statistical's
 *     outlier removal makes shorter than the other arrays;
 *   h_number, h_freq, h_ideal, h_amp, h_deviation: F x max(max_harmonics, 0): HarmonicNumbers,
 *     HarmonicFrequencies, IdealFrequencies, HarmonicAmplitudes, HarmonicDeviations; unused slots are -1 for
 *     h_number and 0 for the rest;
 *   estimated_stiffness, model_fit_quality; harmonic_clarity, spectral_purity, partial_coherence;
 *   r_squared, chi_squared, p_value; quality: SONAR_INHARM_QUALITY_*.
 * Fields a method leaves unset in Go are 0.  An INVALID_F0 row (f0 <= 0, below min_freq or above max_freq,
 * :236) has only the two f0 fields and its quality.  An INSUFFICIENT row has the f0 fields and num_harmonics
 * = the count found; everything else is 0 and quality is -1.  ProcessingTime is always 0 (:1173) and has
 * no output.  ModelParameters holds values of other outputs: "railsback_coefficient" = inharmonicity and
 * "fundamental_frequency" = f0_out (Railsback with >= 3 harmonics only), "string_stiffness" =
 * estimated_stiffness, "string_tension" / "string_length" = the parameters (the String model only).
 * Quirks of the reference kept here:
 *  - findHarmonicPeak (:376-416) scans int(max(0, eb - tb)) .. int(min(K - 1, eb + tb)), eb = f W / sr,
 *    tb = tol f W / sr, with a strict > from maxMag = 0 (an all-zero or empty stretch leaves the start
 *    bin and a magnitude of 0), then demands a strict local maximum at 1 .. K - 2; the frequency is
 *    bin sr / W, so the deviation is quantised to bins.  The loop over h stops at the first h f0 > max_freq.
 *  - Railsback (:467-510, :632-680): 201 values of B from -0.01 by 200 float64 additions of 0.0001 (the last
 *    is 0.00999999999999999); a grid point whose 1 + B n^2 is negative for some harmonic has a NaN error and
 *    is skipped; the first strict minimum wins; fewer than 3 harmonics give an empty result.
 *  - Statistical (:576-610, :735-845): quartiles are gonum's empirical quantile (restated, parity unpinned);
 *    the chi-squared test needs 5 values, and at 6 or 7 its p-value is 0 or NaN (zero degrees of freedom).
 *  - The String model overwrites model_fit_quality, Railsback's R^2 included (:874).
 *  - FletcherMunson's weight above 4 kHz, the clarity, the purity, the String fit and the chi-squared test go
 *    through log10 / exp: parity at a few ulp there, bit for bit elsewhere.
 * Errors: those of sonar_inharm_check; method BEAT_PATTERN (it needs the samples), K outside [4, 4096], F < 0, NULL mag, f0 or f0_confidence with
 * frames due, and (host pointers only) a non-finite f0 -> SONAR_ERR_INVALID: the detector cannot give one on
 * finite PCM, a documented narrowing.  With device pointers such a frame is an INVALID_F0 row.  F == 0
 * succeeds and writes nothing. */
int sonar_inharm_from_spectrum(sonar_ctx* ctx, const double* mag /* F x K */, const double* f0,
                               const double* f0_confidence, int64_t F, int32_t K, const sonar_inharm_params* params,
                               int32_t* status, double* inharmonicity, double* std_dev, double* confidence,
                               double* f0_out, double* f0_confidence_out, int32_t* num_harmonics,
                               int32_t* n_deviations, int32_t* h_number /* F x max_harmonics */, double* h_freq,
                               double* h_ideal, double* h_amp, double* h_deviation, double* estimated_stiffness,
                               double* model_fit_quality, double* harmonic_clarity, double* spectral_purity,
                               double* partial_coherence, double* r_squared, double* chi_squared, double* p_value,
                               int32_t* quality, int32_t device_ptrs);

/* AnalyzeFrame without postProcessResult's tracking on the F = sonar_pitch_detect_frames(n, W, hop_size)
 * whole frames of pcm; the outputs are sonar_inharm_from_spectrum's.
 *  - With a frame due and window_size != 1024: SONAR_ERR_INVALID "audio frame size (W) doesn't match window
 *    size (1024)" (pitch_detection.go:226 under :231; F100).  F == 0 succeeds.
 *  - f0 / f0_confidence are sonar_pitch_detect's pitch / confidence on the same frames with
 *    sonar_pitch_params_default (YIN, 80-1000 Hz, its history carried from frame to frame whatever
 *    use_temporal_tracking says, F101), bit for bit.
 *  - The spectrum is the W-point transform of the raw frame, no window (:321), one block per frame, nothing
 *    but results in device memory.  The transform is go-dsp's in the reference: parity at tolerance.
 *  - BEAT_PATTERN (:552-573) still runs the harmonic search (which can be INSUFFICIENT) and sets
 *    num_harmonics, the String model and the metrics, but no confidence and no harmonic array.  Its
 *    inharmonicity is 0.001 times the coefficient of variation of the lags of FindPeaks(corr, 0.1, 1.0)
 *    (common/math.go:265: strict local maxima >= 0.1; the distance of 1.0 never binds), corr being
 *    NewAutoCorrelation(W).Compute of the raw frame: the bits of sonar_autocorr on it, 2 W - 1 values from lag
 *    -(W - 1), un-normalised at W = 1024.  The lags run over both signs, so their mean is 0 or negative for a
 *    correlation that is symmetric in its bits, and the result is then 0 (mean > 0 else 0, :728); fewer than
 *    two peaks give 0 as well.
 * Errors: those of sonar_inharm_check; n < 0, hop_size < 1 or NULL pcm with frames due -> SONAR_ERR_INVALID. */
int sonar_inharm_frames(sonar_ctx* ctx, const double* pcm, int64_t n, int32_t hop_size,
                        const sonar_inharm_params* params, int32_t* status, double* inharmonicity, double* std_dev,
                        double* confidence, double* f0, double* f0_confidence, int32_t* num_harmonics,
                        int32_t* n_deviations, int32_t* h_number, double* h_freq, double* h_ideal, double* h_amp,
                        double* h_deviation, double* estimated_stiffness, double* model_fit_quality,
                        double* harmonic_clarity, double* spectral_purity, double* partial_coherence,
                        double* r_squared, double* chi_squared, double* p_value, int32_t* quality,
                        int32_t device_ptrs);

/* postProcessResult + updateTemporalTracking (:1007-1101) over F rows in order, from an empty history (a fresh
 * analyzer, or one after Reset).  Host-only, no context.  Frames whose status is not OK pass through
 * (inharmonicity = raw, the other three 0) and do not touch the history: the early return of :236 comes
 * before both.  status NULL means every frame is OK.  With use_temporal_tracking and a non-empty history,
 * inharmonicity = 0.3 raw + 0.7 last, last being the last smoothed value.  temporal_stability = 1 / (1 +
 * sqrt(gonum variance) / |mean|) of the history (mean != 0), inharmonicity_trend = the slope of gonum's
 * stat.LinearRegression over x = 0, 1, ..., f0_stability = 1 / (1 + sqrt(variance) / mean) of the f0 history
 * (mean > 0): each needs three entries and is computed BEFORE the frame's own value enters the history,
 * which keeps its last temporal_window entries (0 empties it every frame).  Without use_temporal_tracking
 * nothing is appended and all three stay 0.  gonum is restated from its published rules, parity unpinned.
 * temporal_window < 0 with tracking: SONAR_ERR_PANIC at the first OK frame (rows before it are written). */
int sonar_inharm_track(const sonar_inharm_params* params, int64_t F, const int32_t* status,
                       const double* raw_inharmonicity, const double* f0, double* inharmonicity,
                       double* temporal_stability, double* inharmonicity_trend, double* f0_stability);

/* AnalyzeSequence (:1181-1193) over the whole frames of pcm: sonar_inharm_frames, then sonar_inharm_track, in
 * one call.  inharmonicity is the smoothed one; *frames receives F.  The first INSUFFICIENT frame makes Go
 * return nil and the error: here SONAR_ERR_INVALID with Go's message "insufficient harmonics found: %d < %d",
 * *error_frame = that frame (-1 otherwise), and the rows before it are written (Go returns none of them); the rows
 * from that frame on hold what sonar_inharm_frames gives, untracked (inharmonicity raw, the three tracking outputs 0).
 * With device_ptrs, pcm and every output array are device pointers. */
int sonar_inharm(sonar_ctx* ctx, const double* pcm, int64_t n, int32_t hop_size, const sonar_inharm_params* params,
                 int32_t* status, double* inharmonicity, double* temporal_stability, double* inharmonicity_trend,
                 double* f0_stability, double* std_dev, double* confidence, double* f0, double* f0_confidence,
                 int32_t* num_harmonics, int32_t* n_deviations, int32_t* h_number, double* h_freq, double* h_ideal,
                 double* h_amp, double* h_deviation, double* estimated_stiffness, double* model_fit_quality,
                 double* harmonic_clarity, double* spectral_purity, double* partial_coherence, double* r_squared,
                 double* chi_squared, double* p_value, int32_t* quality, int64_t* frames, int64_t* error_frame,
                 int32_t device_ptrs);

/* GetAverageInharmonicity (:1196-1216): the mean of the inharmonicities whose confidence is above 0.5 (a NaN
 * is not), 0 without any. */
double sonar_inharm_average(const double* inharmonicity, const double* confidence, int64_t n);
/* ClassifyInharmonicity (:1272-1286) as SONAR_INHARM_VERY_LOW .. VERY_HIGH (a NaN is "Very High", the else
 * branch) and EstimateInstrumentType (:1289-1313) as SONAR_INHARM_INSTRUMENT_*, with Go's strings; NULL for
 * a value outside the enum. */
int32_t sonar_inharm_classify(double inharmonicity);
const char* sonar_inharm_class_name(int32_t cls);
int32_t sonar_inharm_instrument_type(double inharmonicity, double f0);
const char* sonar_inharm_instrument_name(int32_t type);
/* getMethodName / getModelName (:1139-1171) and the AnalysisQuality strings; "Unknown" for a method or model
 * outside the enum, NULL for a quality outside it. */
const char* sonar_inharm_method_name(int32_t method);
const char* sonar_inharm_model_name(int32_t model);
const char* sonar_inharm_quality_name(int32_t quality);

/* result accessors: rows*cols float64 values, row-major; scalars are 1x1 */
int sonar_result_get(const sonar_result* res, const char* name, const double** data, int64_t* rows,
                     int64_t* cols);
int sonar_result_count(const sonar_result* res);
const char* sonar_result_name(const sonar_result* res, int index);
void sonar_result_free(sonar_result* res);

#ifdef __cplusplus
}
#endif
#endif /* SONAR_GPU_H */
