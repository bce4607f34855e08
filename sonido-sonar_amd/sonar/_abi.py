"""ctypes binding of include/sonar_gpu.h (see package docstring)."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))       # sonido-sonar_amd/
_REPO = os.path.dirname(_PKG)
LIB_PATH = os.environ.get("SONAR_LIB") or os.path.join(_PKG, "lib", "libsonar_gpu.so")   # override: A/B builds
HEADER = os.path.join(_REPO, "include", "sonar_gpu.h")

OK, ERR_INVALID, ERR_TOO_SHORT, ERR_EMPTY, ERR_UNSUPPORTED, ERR_DEVICE, ERR_NOMEM = 0, -1, -2, -3, -4, -5, -6
ERR_PANIC = -7          # SONAR_ERR_PANIC: the Go reference panics on this input (message: its runtime error)
FP_MFCC, FP_MAGNITUDE, FP_SPECTRAL, FP_ZCR, FP_ENERGY, FP_COMPLEX, FP_PHASE = 1, 2, 4, 8, 16, 32, 64
FP_GENERIC = 1 << 30   # force the general fused kernel (A/B checks of the f32 MFCC path)
F32, F64 = 0, 1
INGEST_DEVICE_CONVERT, INGEST_HOST_CONVERT = 0, 1   # sonar_ingest_f64le modes
WINDOWS = {"hann": 0, "hamming": 1, "blackman": 2, "blackman_harris": 3, "kaiser": 4,
           "tukey": 5, "rectangular": 6, "bartlett": 7, "welch": 8}
SPECTRAL_NAMES = ["centroid", "rolloff", "bandwidth", "flatness", "crest", "slope", "flux",
                  "low_ratio", "high_ratio"]
# NewDTWAlignmentWithParams' step patterns and metrics (SONAR_DTW_STEP_* / SONAR_DTW_METRIC_*)
DTW_STEPS = {"symmetric2": 0, "asymmetric": 1, "symmetric1": 2}
DTW_STEP_NAMES = ["symmetric2", "asymmetric", "symmetric1"]
DTW_METRICS = {"euclidean": 0, "manhattan": 1, "cosine": 2, "pearson": 3, "mahalanobis": 4}
DTW_QUALITY_KEYS = ["path_efficiency", "diagonal_ratio", "average_cost", "normalized_distance"]
# CorrelationType / CorrelationMethod (SONAR_CORR_*), correlation.go:12-41
CORR_TYPES = {"pearson": 0, "spearman": 1, "kendall": 2, "ncc": 3, "zncc": 4}
CORR_METHODS = {"time": 0, "frequency": 1, "sliding": 2}
# ChromaSimilarityMethod / the frame metrics (SONAR_CHROMA_SIM_* / SONAR_CHROMA_DIST_*)
CHROMA_SIM_METHODS = {"direct": 0, "binary": 1, "smith_waterman": 2, "dtw": 3, "qmax": 4, "oti": 5}
CHROMA_DIST_METRICS = {"euclidean": 0, "manhattan": 1, "cosine": 2, "pearson": 3, "kl": 4, "js": 5, "hellinger": 6}
NCC_KEYS = ["peak_correlation", "peak_lag", "peak_index", "p_value", "snr", "sharpness",
            "second_peak", "peak_to_sidelobe", "overlap_length", "num_lags"]


def _exported_symbols():
    with open(HEADER) as f:
        txt = f.read()
    return sorted(set(re.findall(r"\b(sonar_[a-z0-9_]+)\s*\(", txt)))


EXPORTED_SYMBOLS = _exported_symbols()


class SonarError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"[{code}] {msg}")
        self.code = code
        self.msg = msg


class FpConfig(C.Structure):
    _fields_ = [("window_size", C.c_int32), ("hop_size", C.c_int32), ("window_type", C.c_int32),
                ("sample_rate", C.c_int32), ("n_mfcc", C.c_int32), ("n_filters", C.c_int32),
                ("filterbank", C.c_int32), ("use_lifter", C.c_int32), ("low_freq", C.c_double),
                ("high_freq", C.c_double), ("lifter", C.c_double), ("mfcc_input_power", C.c_int32),
                ("energy_window", C.c_int32), ("energy_hop", C.c_int32), ("preemph_alpha", C.c_double),
                ("flags", C.c_uint32), ("precision", C.c_int32), ("pcm_dtype", C.c_int32),
                ("out_dtype", C.c_int32), ("device_ptrs", C.c_int32)]


class HpcpParams(C.Structure):
    """sonar_hpcp_params (HPCPParams, algorithms/chroma/hpcp.go:11-26)."""
    _fields_ = [(n, C.c_int32) for n in ("size", "harmonics_removal", "normalized", "weight_type", "max_shifted",
                                         "non_linear", "band_preset", "max_harmonics")] + \
               [(n, C.c_double) for n in ("reference_freq", "window_size", "min_freq", "max_freq", "split_freq",
                                          "harmonics_strength")]


HPCP_WEIGHTS = {"none": 0, "cosine": 1, "squared_cosine": 2}


class TempoResult(C.Structure):
    """sonar_tempo_result: EstimateTempo, EstimateTempoAutocorrelation, EstimateTempoRange and
    ClassifyTempoCategory of one signal (tempo_estimation.go)."""
    _fields_ = [(n, C.c_double) for n in ("onset_tempo", "autocorr_tempo", "tempo", "confidence", "difference")] + \
               [("onset_count", C.c_int64), ("best_lag", C.c_int64), ("category", C.c_int32), ("onset_error", C.c_int32)]


# ClassifyTempoCategory's names by SONAR_TEMPO_* code; DetectOnsets' and DetectOnsetsEnergy's grids
TEMPO_CATEGORIES = ["very_slow", "slow", "moderate", "fast", "very_fast"]
ONSET_WINDOW, ONSET_HOP, ONSET_ENERGY_FRAME, ONSET_ENERGY_HOP = 1024, 512, 512, 256


class KeyParams(C.Structure):
    """sonar_key_params: the fields of KeyEstimationParams the reference reads (key_estimation.go:88-113)."""
    _fields_ = [(n, C.c_int32) for n in ("profile", "hpcp_size", "normalize_chroma", "remove_mean", "binary_mode",
                                         "max_candidates")] + [("min_confidence", C.c_double)]


# KeyProfile (SONAR_KEY_PROFILE_*), the transition types (SONAR_KEY_TRANSITION_*) and getKeyName's names
KEY_PROFILES = {"krumhansl": 0, "temperley": 1, "shaath": 2, "edma": 3, "bgate": 4, "diatonic": 5, "tonic_triad": 6}
KEY_TRANSITIONS = ["same_key", "parallel", "relative", "dominant", "subdominant", "distant"]
KEY_NAMES = ["C", "C#", "D", "D#", "E", "F", "F#", "G", "G#", "A", "A#", "B"]
KEY_FRAME_FIELDS = ("key", "mode", "known", "confidence", "strength", "clarity", "ambiguity", "tonality", "scores",
                    "candidates", "processed")


class ChordParams(C.Structure):
    """sonar_chord_params: the fields of ChordDetectionParams the reference reads (chord_detection.go:136-175)."""
    _fields_ = [(n, C.c_int32) for n in ("method", "normalize_templates", "use_inversions", "max_candidates",
                                         "use_bass_detection", "detect_extensions", "max_extension",
                                         "use_temporal_smoothing", "temporal_window", "use_functional_analysis")] + \
               [("min_chord_strength", C.c_double), ("bass_weight", C.c_double)]


# the per-frame outputs of the chord entries, in the order of sonar_chord_out
CHORD_FIELDS = ("root", "quality", "inversion", "n_found", "confidence", "strength", "clarity", "ambiguity",
                "consonance", "tension", "stability", "extensions", "role", "template_scores", "candidates",
                "cand_inversion", "cand_confidence", "cand_strength")
_CHORD_INT_FIELDS = ("root", "quality", "inversion", "n_found", "extensions", "role", "candidates", "cand_inversion")


class ChordOut(C.Structure):
    """sonar_chord_out: one pointer per name of CHORD_FIELDS."""
    _fields_ = [(n, C.c_void_p) for n in CHORD_FIELDS]


# ChordDetectionMethod (SONAR_CHORD_*), ChordQuality's names (GetChordQualityName), the templates' quality
# codes by slot // 12, analyzeFunctionalRole's strings by role code and the inversion suffixes of getChordName
CHORD_METHODS = {"template_matching": 0, "harmonic_analysis": 1, "cqt_based": 2, "statistical": 3, "ml_based": 4,
                 "hybrid": 5}
CHORD_QUALITY_NAMES = ["major", "minor", "diminished", "augmented", "sus2", "sus4", "major7", "minor7", "dominant7",
                       "minor-major7", "augmented7", "diminished7", "half-diminished7", "add9", "major9", "minor9",
                       "dominant9", "major11", "minor11", "dominant11", "major13", "minor13", "dominant13", "power",
                       "unknown"]
CHORD_SLOT_QUALITIES = [0, 1, 2, 3, 4, 5, 6, 7, 8, 23]
CHORD_ROLES = ["", "tonic", "subdominant", "dominant", "leading_tone", "other"]
CHORD_INVERSIONS = ["", "/1st", "/2nd", "/3rd", "/4th"]
CHORD_EXTENSION_ORDER = [10, 11, 2, 5, 9]
CHORD_SLOTS = 120


class FpOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ["mfcc", "magnitude", "centroid", "rolloff", "bandwidth", "flatness",
                                          "crest", "slope", "flux", "low_ratio", "high_ratio", "zcr", "energy",
                                          "complex", "phase"]]


class FingerprintConfig(C.Structure):
    _fields_ = [("window_size", C.c_int32), ("hop_size", C.c_int32), ("feature_window_size", C.c_int32),
                ("feature_hop_size", C.c_int32), ("enable_content_detect", C.c_int32),
                ("window_type", C.c_int32), ("precision", C.c_int32),
                ("acoustic_detection", C.c_int32), ("default_content_type", C.c_int32),
                ("auto_detect_threshold", C.c_double), ("genre", C.c_char_p), ("station", C.c_char_p),
                ("url", C.c_char_p)]


class AcousticFeatures(C.Structure):
    """sonar_acoustic_features (content_detector.go:104-115)."""
    _fields_ = [(n, C.c_double) for n in ("zero_crossing_rate", "spectral_centroid", "energy_variance",
                                          "silence_ratio", "harmonic_ratio", "low_freq_energy", "high_freq_energy",
                                          "dynamic_range", "temporal_stability", "classification_confidence")]


CONTENT_NAMES = ["music", "news", "sports", "talk", "mixed", "unknown"]


class FeatureConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ["sample_rate", "window_size", "hop_size", "stft_window_size",
                                         "stft_hop_size", "window_type", "enable_mfcc", "enable_speech_features",
                                         "enable_temporal_features", "mfcc_coefficients", "is_news", "precision"]]


class FormantFrame(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_formants", C.c_int32), ("frequency", C.c_double * 4),
                ("bandwidth", C.c_double * 4), ("amplitude", C.c_double * 4), ("confidence", C.c_double * 4),
                ("vocal_tract_length", C.c_double), ("quality", C.c_double), ("gain", C.c_double),
                ("residual_energy", C.c_double), ("stable", C.c_int32), ("lpc_order", C.c_int32)]


class VoiceQuality(C.Structure):
    """sonar_voice_quality (speech.VoiceQualityResult, voice_quality.go:21-43)."""
    _fields_ = [(n, C.c_double) for n in ("jitter", "shimmer", "hnr", "noise_measure", "f0_stability",
                                          "amplitude_stability", "voicing_strength", "overall_quality")] + \
               [("num_periods", C.c_int64)] + \
               [(n, C.c_double) for n in ("mean_f0", "f0_range", "analysis_quality")]


class AlignmentStats(C.Structure):
    """sonar_alignment_stats (stats.AlignmentStats, alignment.go:700-707) + the offset and trials."""
    _fields_ = [(n, C.c_double) for n in ("mean_offset", "stddev_offset", "median_offset", "offset_range",
                                          "consistency")] + [("offset", C.c_int64), ("trials", C.c_int32)]


ALIGN_DTW, ALIGN_XCORR, ALIGN_PHASE, ALIGN_HYBRID = 0, 1, 2, 3


class FpFeatures(C.Structure):
    """sonar_fp_features (one AudioFingerprint as FingerprintComparator reads it)."""
    _fields_ = [("id", C.c_int64), ("present", C.c_uint32), ("content_type", C.c_int32),
                ("duration_seconds", C.c_double),
                ("mfcc", C.c_void_p), ("mfcc_frames", C.c_int64), ("mfcc_coeffs", C.c_int32),
                ("chroma", C.c_void_p), ("chroma_frames", C.c_int64), ("chroma_bins", C.c_int32),
                ("spectral_centroid", C.c_void_p), ("n_spectral_centroid", C.c_int64),
                ("spectral_rolloff", C.c_void_p), ("n_spectral_rolloff", C.c_int64),
                ("spectral_flux", C.c_void_p), ("n_spectral_flux", C.c_int64),
                ("dynamic_range", C.c_double), ("silence_ratio", C.c_double), ("onset_density", C.c_double),
                ("rms_energy", C.c_void_p), ("n_rms_energy", C.c_int64),
                ("speech_rate", C.c_double), ("vocal_tract_length", C.c_double),
                ("voicing_probability", C.c_void_p), ("n_voicing_probability", C.c_int64),
                ("harmonic_ratio", C.c_void_p), ("n_harmonic_ratio", C.c_int64),
                ("pitch_estimate", C.c_void_p), ("n_pitch_estimate", C.c_int64),
                ("feature_weights", C.c_double * 6)]


class CompareCfg(C.Structure):
    _fields_ = [("similarity_threshold", C.c_double), ("max_candidates", C.c_int32),
                ("enable_detailed_metrics", C.c_int32), ("enable_content_filter", C.c_int32),
                ("method", C.c_int32)]


class Similarity(C.Structure):
    _fields_ = [("overall_similarity", C.c_double), ("feature_similarity", C.c_double),
                ("confidence", C.c_double), ("feature_distances", C.c_double * 6),
                ("data_availability", C.c_double), ("feature_coverage", C.c_double),
                ("temporal_alignment", C.c_double), ("noise_level", C.c_double),
                ("dynamic_range_match", C.c_double), ("spectral_coherence", C.c_double),
                ("distance_mask", C.c_uint32), ("content_type_match", C.c_int32),
                ("has_quality", C.c_int32), ("status", C.c_int32)]


class Match(C.Structure):
    _fields_ = [("candidate", C.c_int64), ("rank", C.c_int32), ("match_type", C.c_int32),
                ("similarity", Similarity)]


class PairRecord(C.Structure):
    """sonar_pair_record: what ExtractAlignmentFeatures leaves per pair (extractors/alignment.go:139-219)."""
    _fields_ = [(n, C.c_double) for n in ("temporal_offset", "offset_confidence", "alignment_similarity",
                                          "alignment_quality", "method", "corr_offset_seconds", "dtw_distance",
                                          "peak_lag")] + [("status", C.c_int32), ("flags", C.c_int32)]


PAIR_FIELDS = [f for f, _ in PairRecord._fields_[:8]]
PAIR_REDONE_TIMEOUT = 1     # sonar_pair_record.flags (include/sonar_gpu.h)
PAIR_REDONE_NONFINITE = 2

_lib = None
_vp, _d, _i32p, _i64p = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)


def build():
    """Compile libsonar_gpu.so in-tree for gfx950 (hipcc; no GPU needed)."""
    subprocess.run(["make", "-s", "-j8", "-C", _PKG], check=True)


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SonarError(ERR_DEVICE, f"{LIB_PATH} not built: run `make -C sonido-sonar_amd` "
                                     "(there is no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    L.sonar_create.argtypes = [C.c_int, C.POINTER(_vp)]
    L.sonar_destroy.argtypes = [_vp]
    L.sonar_destroy.restype = None
    L.sonar_last_error.argtypes = [_vp]
    L.sonar_last_error.restype = C.c_char_p
    L.sonar_set_stream.argtypes = [_vp, _vp]
    L.sonar_synchronize.argtypes = [_vp]
    L.sonar_last_kernel_ms.argtypes = [_vp, _d]
    L.sonar_enable_kernel_timing.argtypes = [_vp, C.c_int]
    L.sonar_dtw_last_timing.argtypes = [_vp, C.POINTER(C.c_double)]
    if hasattr(L, "sonar_dtw_counters"):      # (absent from A/B builds of earlier rounds)
        L.sonar_dtw_counters.argtypes = [_vp, C.POINTER(C.c_int64), C.c_int32]
    if hasattr(L, "sonar_trim"):
        L.sonar_trim.argtypes = [_vp]
    L.sonar_last_fp_kernel.argtypes = [_vp]
    L.sonar_last_fp_kernel.restype = C.c_char_p
    for f in ("sonar_stft_frames", "sonar_energy_frames"):
        getattr(L, f).argtypes = [C.c_int64, C.c_int32, C.c_int32]
        getattr(L, f).restype = C.c_int64
    L.sonar_pitch_frames.argtypes = [C.c_int64]
    L.sonar_pitch_frames.restype = C.c_int64
    L.sonar_fp_cfg_default.argtypes = [C.POINTER(FpConfig)]
    L.sonar_fp_cfg_default.restype = None
    L.sonar_stft_stream_create.argtypes = [_vp, C.POINTER(FpConfig), C.POINTER(_vp)]
    L.sonar_stft_stream_frames.argtypes = [_vp, C.c_int64]
    L.sonar_stft_stream_frames.restype = C.c_int64
    L.sonar_stft_stream_buffered.argtypes = [_vp]
    L.sonar_stft_stream_buffered.restype = C.c_int64
    L.sonar_stft_stream_push.argtypes = [_vp, _vp, C.c_int64, C.POINTER(FpOut), C.POINTER(C.c_int64)]
    L.sonar_stft_stream_destroy.argtypes = [_vp]
    L.sonar_stft_stream_destroy.restype = None
    L.sonar_fp_kernel_plan.argtypes = [C.POINTER(FpConfig), C.c_int64]
    L.sonar_fp_kernel_plan.restype = C.c_int32
    L.sonar_fingerprint.argtypes = [_vp, _vp, C.c_int64, C.POINTER(FpConfig), C.POINTER(FpOut)]
    L.sonar_fingerprint_batch.argtypes = [_vp, C.POINTER(_vp), C.POINTER(C.c_int64), C.c_int32,
                                          C.POINTER(FpConfig), C.POINTER(FpOut)]
    L.sonar_pitch_yin.argtypes = [_vp, _vp, C.c_int64, C.c_int32, _vp, _vp, _vp, C.c_int32]
    L.sonar_chroma_stft.argtypes = [_vp, _vp, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32]
    L.sonar_chroma_cqt_plan.argtypes = [C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_double, C.c_double, C.c_int64,
                                        C.c_int64, _i64p, _i64p, _i64p, _i64p, _vp, _vp]
    L.sonar_chroma_cqt.argtypes = [_vp, _vp, C.c_int64, C.c_int64, C.c_int32, C.c_double, C.c_double, C.c_int32,
                                   C.c_double, C.c_double, _vp, _vp, C.c_int32]
    L.sonar_chroma_frame_matrix.argtypes = [_vp, _vp, C.c_int64, _vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                            C.c_int32, _vp]
    L.sonar_chroma_similarity.argtypes = [_vp, _vp, C.c_int64, _vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                          C.c_double, C.c_int32, C.c_int32, C.c_int32, _vp, C.POINTER(C.c_int32), _d,
                                          C.POINTER(C.c_int32), _vp, _vp, _vp, _i64p]
    L.sonar_chroma_similarity_plan.argtypes = [C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                               _i64p, _i64p, _i64p, _i64p, _i64p]
    L.sonar_chroma_similarity_last_timing.argtypes = [_vp, C.POINTER(C.c_double)]
    L.sonar_spectral_peaks_width.argtypes = [C.c_int64, C.c_int64]
    L.sonar_spectral_peaks_width.restype = C.c_int64
    L.sonar_spectral_peaks.argtypes = [_vp, _vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double,
                                       C.c_int32, _vp, _vp, _vp, _vp, C.c_int32]
    L.sonar_hpcp_params_default.argtypes = [C.POINTER(HpcpParams)]
    L.sonar_hpcp_params_default.restype = None
    L.sonar_hpcp_from_spectrum.argtypes = [_vp, _vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(HpcpParams),
                                           _vp, _vp, _vp, C.c_int32]
    L.sonar_hpcp_table.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(HpcpParams), _i64p, _vp, _vp, _vp, _vp]
    L.sonar_hpcp_plan.argtypes = [C.c_int64, C.c_int32, C.c_int32, _i64p, _i64p, _i64p]
    L.sonar_hpcp.argtypes = [_vp, _vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(HpcpParams),
                             _vp, _vp, _vp, C.c_int32]
    L.sonar_hps_bins.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, _i32p, _i32p]
    L.sonar_hps_optimal_harmonics.argtypes = [C.c_int32, C.c_double, _i32p]
    L.sonar_hps_from_spectrum.argtypes = [_vp, _vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double,
                                          C.c_double, C.c_int32, _vp, _vp, _vp, _vp, _vp, C.c_int32]
    L.sonar_hps_plan.argtypes = [C.c_int64, C.c_int32, C.c_int32, _i64p, _i64p, _i64p]
    L.sonar_hps.argtypes = [_vp, _vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double,
                            C.c_int32, _vp, _vp, _vp, _vp, _vp, _i64p, C.c_int32]
    L.sonar_spectral_flux.argtypes = [_vp, _vp, C.c_int64, C.c_int32, C.c_int32, _vp, C.c_int32]
    L.sonar_rms_envelope_frames.argtypes = [C.c_int64, C.c_int32, C.c_int32]
    L.sonar_rms_envelope_frames.restype = C.c_int64
    L.sonar_rms_envelope.argtypes = [_vp, _vp, C.c_int64, C.c_int32, C.c_int32, _vp, _i64p, C.c_int32]
    L.sonar_onset_peaks_width.argtypes = [C.c_int64]
    L.sonar_onset_peaks_width.restype = C.c_int64
    L.sonar_onset_min_interval_frames.argtypes = [C.c_double, C.c_int32, C.c_int32, _i32p]
    L.sonar_onset_peaks.argtypes = [_vp, _vp, C.c_int64, C.c_double, C.c_double, C.c_int32, C.c_int32, _vp, _i64p,
                                    C.c_int32]
    L.sonar_onset_adaptive_threshold.argtypes = [_vp, _vp, C.c_int64, _vp, C.c_int32]
    L.sonar_onsets_flux.argtypes = [_vp, _vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, _vp,
                                    _i64p, _vp, _vp, _i64p, C.c_int32]
    L.sonar_onsets_energy.argtypes = [_vp, _vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, _vp,
                                      _i64p, _vp, _i64p, C.c_int32]
    L.sonar_onsets_complex_width.argtypes = [C.c_int64]
    L.sonar_onsets_complex_width.restype = C.c_int64
    L.sonar_onsets_complex.argtypes = [_vp, _vp, C.c_int64, C.c_int32, _vp, _i64p, _d, C.c_int32]
    L.sonar_tempo_from_onsets.argtypes = [_vp, C.c_int64, C.c_int32, _d, _i32p]
    L.sonar_tempo_autocorr_plan.argtypes = [C.c_int64, C.c_int32, _i32p, _i32p, _i64p, _i64p, _i64p, _i64p]
    L.sonar_tempo_autocorrelation.argtypes = [_vp, _vp, C.c_int64, C.c_int32, _vp, _vp, _vp, _i64p, C.c_int32]
    L.sonar_tempo_category.argtypes = [C.c_double]
    L.sonar_tempo_category.restype = C.c_int32
    L.sonar_tempo_category_name.argtypes = [C.c_int32]
    L.sonar_tempo_category_name.restype = C.c_char_p
    L.sonar_tempo.argtypes = [_vp, _vp, C.c_int64, C.c_int32, C.POINTER(TempoResult), C.c_int32]
    L.sonar_key_params_default.argtypes = [C.POINTER(KeyParams)]
    L.sonar_key_params_default.restype = None
    _key = [_vp, _vp, C.c_int64, C.c_int32, C.POINTER(KeyParams)]
    L.sonar_key_frames.argtypes = _key + [_vp] * 11 + [C.c_int32]
    L.sonar_key_sequence.argtypes = _key + [_vp] * 13 + [C.c_int32]
    L.sonar_key_batch.argtypes = _key + [_vp] * 21 + [C.c_int32]
    L.sonar_key_transition.argtypes = [C.c_int32] * 4 + [_i32p, _i32p, _i32p, _d]
    L.sonar_chord_params_default.argtypes = [C.POINTER(ChordParams)]
    L.sonar_chord_params_default.restype = None
    _chord = [_vp, _vp, C.c_int64, C.c_int32, _vp, _vp, C.POINTER(ChordParams), C.POINTER(ChordOut), C.c_int32]
    L.sonar_chord_frames.argtypes = _chord
    L.sonar_chord_sequence.argtypes = _chord
    L.sonar_chord_detect.argtypes = [_vp, _vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _vp, _vp,
                                     C.POINTER(ChordParams), C.POINTER(ChordOut), _vp, _i64p, C.c_int32]
    L.sonar_chord_progression.argtypes = [_vp, _vp, _vp, _vp, _vp, C.c_int64, _vp, _vp, _vp, _vp, C.c_int32]
    L.sonar_ncc.argtypes = [_vp, _vp, C.c_int64, _vp, C.c_int64, C.c_int32, _vp, _vp, C.c_int32]
    L.sonar_xcorr_params.argtypes = [_vp, _vp, C.c_int64, _vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                     _vp, _vp, C.c_int32]
    L.sonar_autocorr.argtypes = [_vp, _vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, C.c_int32]
    L.sonar_pitch_params_default.argtypes = [C.POINTER(PitchParams), C.c_int32]
    L.sonar_pitch_params_default.restype = None
    L.sonar_pitch_detect_frames.argtypes = [C.c_int64, C.c_int32, C.c_int32]
    L.sonar_pitch_detect_frames.restype = C.c_int64
    L.sonar_pitch_curve_width.argtypes = [C.POINTER(PitchParams)]
    L.sonar_pitch_curve_width.restype = C.c_int64
    L.sonar_pitch_frames_raw.argtypes = [_vp, _vp, C.c_int64, C.POINTER(PitchParams), C.c_int32] + [_vp] * 8 + [C.c_int32]
    L.sonar_pitch_track.argtypes = [C.POINTER(PitchParams), C.c_int64] + [_vp] * 13
    L.sonar_pitch_detect.argtypes = [_vp, _vp, C.c_int64, C.POINTER(PitchParams)] + [_vp] * 9 + [_i64p, C.c_int32]
    L.sonar_pitch_stability.argtypes = [_vp, C.c_int64, C.c_int32, C.c_int32, _vp, _i32p]
    L.sonar_hratio_params_default.argtypes = [C.POINTER(HratioParams), C.c_int32]
    L.sonar_hratio_params_default.restype = None
    L.sonar_hratio_check.argtypes = [C.POINTER(HratioParams)]
    L.sonar_hratio_from_spectrum.argtypes = [_vp, _vp, _vp, C.c_int64, C.c_int32, C.POINTER(HratioParams)] + [_vp] * 17 + \
        [C.c_int32]
    L.sonar_hratio_frames.argtypes = [_vp, _vp, C.c_int64, C.POINTER(HratioParams)] + [_vp] * 17 + [C.c_int32]
    L.sonar_hratio_track.argtypes = [C.POINTER(HratioParams), C.c_int64] + [_vp] * 5
    L.sonar_hratio.argtypes = [_vp, _vp, C.c_int64, C.POINTER(HratioParams)] + [_vp] * 19 + [_i64p, C.c_int32]
    L.sonar_hratio_average.argtypes = [_vp, C.c_int64]
    L.sonar_hratio_average.restype = C.c_double
    L.sonar_hratio_classify.argtypes = [C.c_double]
    L.sonar_hratio_classify.restype = C.c_int32
    L.sonar_hratio_category_name.argtypes = [C.c_int32]
    L.sonar_hratio_category_name.restype = C.c_char_p
    L.sonar_hratio_voicing_quality.argtypes = [C.c_double]
    L.sonar_hratio_voicing_quality.restype = C.c_double
    L.sonar_inharm_params_default.argtypes = [C.POINTER(InharmParams), C.c_int32]
    L.sonar_inharm_params_default.restype = None
    L.sonar_inharm_check.argtypes = [C.POINTER(InharmParams)]
    L.sonar_inharm_from_spectrum.argtypes = [_vp, _vp, _vp, _vp, C.c_int64, C.c_int32, C.POINTER(InharmParams)] + \
        [_vp] * 22 + [C.c_int32]
    L.sonar_inharm_frames.argtypes = [_vp, _vp, C.c_int64, C.c_int32, C.POINTER(InharmParams)] + [_vp] * 22 + [C.c_int32]
    L.sonar_inharm_track.argtypes = [C.POINTER(InharmParams), C.c_int64] + [_vp] * 7
    L.sonar_inharm.argtypes = [_vp, _vp, C.c_int64, C.c_int32, C.POINTER(InharmParams)] + [_vp] * 25 + \
        [_i64p, _i64p, C.c_int32]
    L.sonar_inharm_average.argtypes = [_vp, _vp, C.c_int64]
    L.sonar_inharm_average.restype = C.c_double
    L.sonar_inharm_classify.argtypes = [C.c_double]
    L.sonar_inharm_classify.restype = C.c_int32
    L.sonar_inharm_instrument_type.argtypes = [C.c_double, C.c_double]
    L.sonar_inharm_instrument_type.restype = C.c_int32
    for fn in (L.sonar_inharm_class_name, L.sonar_inharm_instrument_name, L.sonar_inharm_method_name,
               L.sonar_inharm_model_name, L.sonar_inharm_quality_name):
        fn.argtypes = [C.c_int32]
        fn.restype = C.c_char_p
    L.sonar_music_alignment_features.argtypes = [_vp, _vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                 C.c_int32, _vp, _vp, C.c_int32]
    L.sonar_dtw.argtypes = [_vp, _vp, C.c_int64, _vp, C.c_int64, C.c_int32, C.c_int32, _d, _vp, _vp, _vp, _i64p,
                            _vp, C.c_int32]
    L.sonar_dtw_params.argtypes = [_vp, _vp, C.c_int64, _vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                   _d, _vp, _vp, _vp, _i64p, _vp, C.c_int32]
    L.sonar_dtw_quality.argtypes = [_vp, _vp, _vp, C.c_int64, C.c_int64, C.c_int64, C.c_double, _d]
    L.sonar_dtw_optimize_step_pattern.argtypes = [_vp, _vp, C.c_int64, _vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                                  C.c_int32, _i32p, _d]
    L.sonar_fingerprint_config_default.argtypes = [C.POINTER(FingerprintConfig)]
    L.sonar_fingerprint_config_default.restype = None
    L.sonar_generate_fingerprint.argtypes = [_vp, _vp, C.c_int64, C.c_int32, C.c_char_p,
                                             C.POINTER(FingerprintConfig), C.POINTER(_vp)]
    L.sonar_feature_config_default.argtypes = [C.POINTER(FeatureConfig)]
    L.sonar_feature_config_default.restype = None
    L.sonar_extract_speech_features.argtypes = [_vp, _vp, C.c_int64, C.c_int32, C.POINTER(FeatureConfig),
                                                C.POINTER(_vp)]
    if hasattr(L, "sonar_extract_music_features"):
        L.sonar_extract_music_features.argtypes = [_vp, _vp, C.c_int64, C.c_int32, C.POINTER(FeatureConfig),
                                                   C.POINTER(_vp)]
    L.sonar_align_features.argtypes = [_vp, _vp, C.c_int64, _vp, C.c_int64, _vp, C.c_int64, _vp, C.c_int64,
                                       C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_double, C.POINTER(_vp)]
    L.sonar_formant_frame_count.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_int32]
    L.sonar_formant_frame_count.restype = C.c_int64
    L.sonar_formants.argtypes = [_vp, _vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_int32]
    L.sonar_align_pair_device.argtypes = [_vp, _vp, C.c_int64, _vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                          C.c_int32, C.c_double, C.POINTER(C.c_void_p)]
    _pairs = [C.c_int64, C.POINTER(C.c_void_p), _i64p, C.POINTER(C.c_void_p), _i64p, C.c_int32, C.c_int32,
              C.c_int32, C.c_int32, C.c_double, C.c_int32]
    L.sonar_align_pairs.argtypes = [_vp] + _pairs + [C.c_int32, C.POINTER(PairRecord)]
    L.sonar_align_pairs_multi.argtypes = [_vp] + _pairs + [C.POINTER(PairRecord)]
    L.sonar_multi_create.argtypes = [_i32p, C.c_int32, C.POINTER(C.c_void_p)]
    L.sonar_multi_destroy.argtypes = [_vp]
    L.sonar_multi_destroy.restype = None
    L.sonar_multi_last_error.argtypes = [_vp]
    L.sonar_multi_last_error.restype = C.c_char_p
    L.sonar_multi_size.argtypes = [_vp]
    L.sonar_multi_ctx.argtypes = [_vp, C.c_int32]
    L.sonar_multi_ctx.restype = _vp
    L.sonar_multi_shard.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _i64p, _i64p, _i64p,
                                    _i64p]
    L.sonar_fingerprint_multi.argtypes = [_vp, _vp, C.c_int64, C.POINTER(FpConfig), C.POINTER(FpOut)]
    L.sonar_fingerprint_multi_gather.argtypes = [_vp, C.POINTER(C.c_void_p), C.c_int64, C.POINTER(FpConfig),
                                                 C.POINTER(C.c_void_p)]
    L.sonar_alignment_consistency.argtypes = [_vp, _vp, C.c_int64, _vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                              C.c_int32, C.c_int32, C.c_int32, C.POINTER(AlignmentStats)]
    L.sonar_analyzer_align_features.argtypes = [_vp, _vp, C.c_int64, _vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                                C.c_int32, C.c_int32, C.c_int32, C.POINTER(_vp)]
    L.sonar_align_audio.argtypes = [_vp, _vp, C.c_int64, _vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                    C.c_int32, C.c_int32, C.POINTER(_vp)]
    L.sonar_align_audio_files.argtypes = [_vp, _vp, C.c_int64, _vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                          C.c_int32, C.c_double, C.c_int32, C.POINTER(_vp)]
    L.sonar_truncate_to_alignment.argtypes = [_vp, C.c_int64, C.c_int64, C.c_int32, C.c_double,
                                              C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.sonar_voice_quality.argtypes = [_vp, _vp, C.c_int64, C.c_int32, C.POINTER(VoiceQuality)]
    L.sonar_fingerprint_f64le.argtypes = [_vp, _vp, C.c_int64, C.c_int32, C.POINTER(FpConfig), C.POINTER(FpOut)]
    L.sonar_ingest_f64le.argtypes = [_vp, _vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _vp, _i64p]
    L.sonar_detect_from_audio.argtypes = [_vp, _vp, C.c_int64, C.c_int32, C.c_double, _i32p,
                                          C.POINTER(AcousticFeatures)]
    L.sonar_detect_content_type.argtypes = [_vp, _vp, C.c_int64, C.c_int32, C.c_int32, C.c_char_p, C.c_char_p,
                                            C.c_char_p, C.c_char_p, C.c_int32, C.c_int32, C.c_double, _i32p]
    L.sonar_gallery_create.argtypes = [_vp, C.POINTER(_vp)]
    L.sonar_gallery_destroy.argtypes = [_vp]
    L.sonar_gallery_destroy.restype = None
    L.sonar_gallery_size.argtypes = [_vp]
    L.sonar_gallery_size.restype = C.c_int64
    L.sonar_gallery_add.argtypes = [_vp, C.POINTER(FpFeatures), C.c_int32, C.c_int32, C.c_int32, _i64p]
    L.sonar_compare.argtypes = [_vp, _i64p, C.c_int64, _i64p, C.c_int64, C.POINTER(CompareCfg), _vp, C.c_int32]
    L.sonar_find_best_matches.argtypes = [_vp, _i64p, C.c_int64, _i64p, C.c_int64, C.POINTER(CompareCfg),
                                          C.POINTER(Match), _i64p]
    L.sonar_merge_matches.argtypes = [C.POINTER(C.c_void_p), _i64p, _i64p, C.c_int32, C.c_int64, C.c_int32,
                                      C.POINTER(Match), _i64p]
    L.sonar_find_best_matches_multi.argtypes = [_vp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int64,
                                                C.POINTER(C.c_void_p), _i64p, C.POINTER(CompareCfg),
                                                C.POINTER(Match), _i64p]
    L.sonar_result_get.argtypes = [_vp, C.c_char_p, C.POINTER(_d), _i64p, _i64p]
    L.sonar_result_count.argtypes = [_vp]
    L.sonar_result_name.argtypes = [_vp, C.c_int]
    L.sonar_result_name.restype = C.c_char_p
    L.sonar_result_free.argtypes = [_vp]
    L.sonar_result_free.restype = None
    _lib = L
    return L


def _formant_dict(recs, F):
    a = np.ctypeslib.as_array(recs)[:F] if F else np.zeros(0, dtype=np.dtype(FormantFrame))
    return {k: np.array(a[k]) for k in ("status", "n_formants", "frequency", "bandwidth", "amplitude", "confidence",
                                        "vocal_tract_length", "quality", "gain", "residual_energy", "stable",
                                        "lpc_order")}


def abi_version():
    return lib().sonar_abi_version()


def dtw_quality(res, nq, nr):
    """DTWAlignment.GetAlignmentQuality of a dtw / dtw_params result (sonar_dtw_quality, host only):
    path_efficiency, diagonal_ratio, average_cost, normalized_distance.  An empty path raises
    (ERR_EMPTY; Go returns an empty map)."""
    pq = np.ascontiguousarray(res["path_q"], dtype=np.int32)
    pr = np.ascontiguousarray(res["path_r"], dtype=np.int32)
    pc = np.ascontiguousarray(res["path_cost"], dtype=np.float64)
    out = (C.c_double * 4)()
    rc = lib().sonar_dtw_quality(_ptr(pq), _ptr(pr), _ptr(pc), len(pq), nq, nr, float(res["distance"]), out)
    if rc != OK:
        raise SonarError(rc, "empty alignment path" if rc == ERR_EMPTY else "invalid argument")
    return dict(zip(DTW_QUALITY_KEYS, out))


def _dtw_step(step, empty=False):
    """SONAR_DTW_STEP_* of a step-pattern name; an int passes through (unknown values reach the
    library, which answers with Go's error and the value).  An unknown name raises Go's error with
    the name, unless a sequence is empty: that error comes first, from the library."""
    if not isinstance(step, str):
        return int(step)
    if step not in DTW_STEPS and not empty:
        raise SonarError(ERR_INVALID, f"failed to fill cost matrix: unknown step pattern: {step}")
    return DTW_STEPS.get(step, -1)


def _corr_enum(v, table):
    """SONAR_CORR_* of a name; an int passes through (unknown values reach the library, as in Go)."""
    return table[v] if isinstance(v, str) else int(v)


def _xcorr_metrics(met):
    """metrics[12] as a dict: NCC_KEYS, then the method that ran and the type (both ints)."""
    d = dict(zip(NCC_KEYS, met[:10].tolist()))
    d["method"], d["type"] = int(met[10]), int(met[11])
    return d


def _dtw_metric(metric):
    if isinstance(metric, str):
        return DTW_METRICS[metric]
    return int(metric)


def stft_frames(n, W, H):
    return int(lib().sonar_stft_frames(n, W, H))


PLAN_NONE, PLAN_PAIR, PLAN_WAVE, PLAN_DFT = 0, 1, 2, 3
PAIR_MAX_FRAMES = 2147483646          # SONAR_PAIR_MAX_FRAMES: mfcc_pair_kernel's 32-bit frame indices


def fp_kernel_plan(cfg, n):
    """sonar_fp_kernel_plan: the transform kernel sonar_fingerprint runs for (cfg, n) (host logic)."""
    return int(lib().sonar_fp_kernel_plan(C.byref(cfg), n))


def energy_frames(n, W, H):
    return int(lib().sonar_energy_frames(n, W, H))


def pitch_frames(n):
    return int(lib().sonar_pitch_frames(n))


_CQT_PLAN_ERRORS = {ERR_PANIC: "the Go reference panics on these parameters (no bins, a negative bin count, or "
                               "hop 0 with samples to frame); sonar_chroma_cqt reports its runtime error text",
                    ERR_UNSUPPORTED: "chroma CQT: parameters the library does not reproduce (include/sonar_gpu.h)"}


def chroma_cqt_plan(sample_rate, min_freq=65.4, max_freq=2093.0, bins_per_octave=12, q_factor=25.0, tuning_freq=440.0,
                    n=0, hop=512):
    """sonar_chroma_cqt_plan (host only): the integer side of NewChromaCQT(...)'s kernel and the frame
    count of ComputeChroma on n samples at hop -> dict of total_bins, fft_size, n_frames, sum_taps,
    kernel_len and chroma_bin (int32 arrays of total_bins entries).  n = 0 gives n_frames = 0."""
    L = lib()
    v = [C.c_int64() for _ in range(4)]
    args = (int(sample_rate), float(min_freq), float(max_freq), int(bins_per_octave), float(q_factor),
            float(tuning_freq), int(n), int(hop))
    rc = L.sonar_chroma_cqt_plan(*args, *[C.byref(x) for x in v], None, None)
    if rc != OK:
        raise SonarError(rc, _CQT_PLAN_ERRORS.get(rc, "sonar_chroma_cqt_plan"))
    K = v[0].value
    klen, cls = np.zeros(K, np.int32), np.zeros(K, np.int32)
    rc = L.sonar_chroma_cqt_plan(*args, *[C.byref(x) for x in v], _ptr(klen), _ptr(cls))
    if rc != OK:
        raise SonarError(rc, _CQT_PLAN_ERRORS.get(rc, "sonar_chroma_cqt_plan"))
    return {"total_bins": K, "fft_size": v[1].value, "n_frames": v[2].value, "sum_taps": v[3].value,
            "kernel_len": klen, "chroma_bin": cls}


def _chroma_enum(table, v):
    return table[v] if isinstance(v, str) else int(v)


def chroma_similarity_plan(method, nq, nr, dim=12, oti_radius=10, dtw_band_radius=50):
    """sonar_chroma_similarity_plan (host only): the integer side of ComputeSimilarity -> dict of
    sample_step and sampled_pairs (findBestTransposition, per shift), oti_cells (per shift),
    dtw_skipped_columns (the columns j >= 1 the band rule leaves 0) and scratch_bytes."""
    v = [C.c_int64() for _ in range(5)]
    rc = lib().sonar_chroma_similarity_plan(_chroma_enum(CHROMA_SIM_METHODS, method), int(nq), int(nr), int(dim),
                                            int(oti_radius), int(dtw_band_radius), *[C.byref(x) for x in v])
    if rc != OK:
        raise SonarError(rc, "sonar_chroma_similarity_plan: negative frame count or dim < 1")
    return dict(zip(("sample_step", "sampled_pairs", "oti_cells", "dtw_skipped_columns", "scratch_bytes"),
                    [x.value for x in v]))


def hpcp_params(**kw):
    """sonar_hpcp_params with NewHPCP's defaults (sonar_hpcp_params_default), fields overridden by
    keyword; weight_type takes Go's string ("none", "cosine", "squared_cosine"; any other string is
    "none", as in Go) or the enum value."""
    p = HpcpParams()
    lib().sonar_hpcp_params_default(C.byref(p))
    for k, v in kw.items():
        if k == "weight_type" and isinstance(v, str):
            v = HPCP_WEIGHTS.get(v, 0)
        setattr(p, k, v)
    return p


_HPCP_ERRORS = {ERR_PANIC: "runtime error: makeslice: len out of range",
                ERR_UNSUPPORTED: "HPCP: parameters the library does not reproduce (include/sonar_gpu.h)",
                ERR_INVALID: "HPCP: invalid argument"}
_HPCP_PLAN_ERRORS = {ERR_EMPTY: "empty signal", ERR_INVALID: "window size and hop size must be positive",
                     ERR_TOO_SHORT: "signal too short for given window size and hop size",
                     ERR_UNSUPPORTED: "window size above the generic STFT path's limit"}


def key_params(**kw):
    """sonar_key_params with NewKeyEstimator's defaults (sonar_key_params_default), fields overridden by
    keyword; profile takes a name of KEY_PROFILES or the enum value."""
    p = KeyParams()
    lib().sonar_key_params_default(C.byref(p))
    for k, v in kw.items():
        if k == "profile" and isinstance(v, str):
            v = KEY_PROFILES[v]
        setattr(p, k, v)
    return p


def key_name(code):
    """getKeyName of a code key * 2 + mode ("C major", ...); -1 is GetGlobalKey's empty name."""
    return "" if code < 0 else KEY_NAMES[(code >> 1) % 12] + (" minor" if code & 1 else " major")


def key_transition(from_key, from_mode, to_key, to_mode):
    """AnalyzeKeyTransition (sonar_key_transition, host only) -> dict of transition_type (a name of
    KEY_TRANSITIONS), type, semitone_distance, fifths_distance, transition_strength."""
    t, sd, fd, st = C.c_int32(), C.c_int32(), C.c_int32(), C.c_double()
    lib().sonar_key_transition(int(from_key), int(from_mode), int(to_key), int(to_mode), C.byref(t), C.byref(sd),
                               C.byref(fd), C.byref(st))
    return {"transition_type": KEY_TRANSITIONS[t.value], "type": t.value, "semitone_distance": sd.value,
            "fifths_distance": fd.value, "transition_strength": st.value}


def _key_frame_arrays(F, p, skip=()):
    """numpy outputs of the per-frame fields (None for the names in skip), in the C argument order."""
    nc, hs = min(max(p.max_candidates, 0), 24), max(p.hpcp_size, 0)
    shapes = {"key": ((F,), np.int32), "mode": ((F,), np.int32), "known": ((F,), np.int32),
              "scores": ((F, 24), np.float64), "candidates": ((F, nc), np.int32), "processed": ((F, hs), np.float64)}
    return {n: None if n in skip else np.zeros(*shapes.get(n, ((F,), np.float64))) for n in KEY_FRAME_FIELDS}


def _key_rows(chroma):
    chroma = _f64(chroma)
    return chroma[None, :] if chroma.ndim == 1 else chroma


def chord_params(**kw):
    """sonar_chord_params with NewChordDetector's defaults (sonar_chord_params_default), fields overridden by
    keyword; method takes a name of CHORD_METHODS or the enum value."""
    p = ChordParams()
    lib().sonar_chord_params_default(C.byref(p))
    for k, v in kw.items():
        if k == "method" and isinstance(v, str):
            v = CHORD_METHODS[v]
        setattr(p, k, v)
    return p


def chord_quality_name(quality):
    """GetChordQualityName of a ChordQuality code."""
    return CHORD_QUALITY_NAMES[quality] if 0 <= quality < len(CHORD_QUALITY_NAMES) else "unknown"


def chord_name(root, quality, inversion=0):
    """getChordName: the root's name, the template's name unless it is "major" ("unknown" for a quality
    without a template), and the inversion's suffix."""
    name = KEY_NAMES[root % 12]
    qn = CHORD_QUALITY_NAMES[quality] if quality in CHORD_SLOT_QUALITIES else "unknown"
    if qn != "major":
        name += qn
    if 0 < inversion < len(CHORD_INVERSIONS):
        name += CHORD_INVERSIONS[inversion]
    return name


def chord_extensions(mask):
    """The raw intervals of an extensions mask, in the order of the reference's map literal."""
    return [i for i in CHORD_EXTENSION_ORDER if mask >> i & 1]


def _chord_arrays(F, p, skip=()):
    """numpy outputs of the chord entries (None for the names in skip) and the sonar_chord_out over them."""
    mc = max(p.max_candidates, 0)
    o = {}
    for n in CHORD_FIELDS:
        shape = (F, CHORD_SLOTS) if n == "template_scores" else (F, mc) if n.startswith("cand") else (F,)
        o[n] = None if n in skip else np.zeros(shape, np.int32 if n in _CHORD_INT_FIELDS else np.float64)
    out = ChordOut(*[o[n].ctypes.data if o[n] is not None and o[n].size else None for n in CHORD_FIELDS])
    return o, out


def _chord_bass(bass_note, bass_confidence):
    bn = None if bass_note is None else np.ascontiguousarray(bass_note, dtype=np.int32)
    bc = None if bass_confidence is None else _f64(bass_confidence)
    return bn, bc


def spectral_peaks_width(K, max_peaks):
    """sonar_spectral_peaks_width: slots per row of spectral_peaks, min(max_peaks, max((K - 1) / 2, 0))."""
    return int(lib().sonar_spectral_peaks_width(int(K), int(max_peaks)))


def hpcp_table(sample_rate, window_size, K, params=None):
    """sonar_hpcp_table (host only): the CSR contribution table of NewHPCPWithParams(sample_rate, params)
    for rows of K bins at window_size -> dict of row_start (int64, K + 1), wrapped_bin (int32), factor,
    window_weight."""
    L = lib()
    p = params if params is not None else hpcp_params()
    n = C.c_int64()
    rc = L.sonar_hpcp_table(int(sample_rate), int(window_size), int(K), C.byref(p), C.byref(n), None, None, None, None)
    if rc != OK:
        raise SonarError(rc, _HPCP_ERRORS.get(rc, "sonar_hpcp_table"))
    rs = np.zeros(int(K) + 1, np.int64)
    wb, fac, ww = np.zeros(n.value, np.int32), np.zeros(n.value), np.zeros(n.value)
    rc = L.sonar_hpcp_table(int(sample_rate), int(window_size), int(K), C.byref(p), C.byref(n), _ptr(rs), _ptr(wb),
                            _ptr(fac), _ptr(ww))
    if rc != OK:
        raise SonarError(rc, _HPCP_ERRORS.get(rc, "sonar_hpcp_table"))
    return {"row_start": rs, "wrapped_bin": wb, "factor": fac, "window_weight": ww}


def hpcp_plan(n, window_size, hop_size):
    """sonar_hpcp_plan (host only): how Context.hpcp splits its frames -> dict of frames, chunk_frames,
    n_chunks."""
    v = [C.c_int64() for _ in range(3)]
    rc = lib().sonar_hpcp_plan(int(n), int(window_size), int(hop_size), *[C.byref(x) for x in v])
    if rc != OK:
        raise SonarError(rc, _HPCP_PLAN_ERRORS.get(rc, "sonar_hpcp_plan"))
    return dict(zip(("frames", "chunk_frames", "n_chunks"), [x.value for x in v]))


_HPS_ERRORS = {ERR_UNSUPPORTED: "harmonic product: parameters the library does not reproduce (include/sonar_gpu.h)",
               ERR_INVALID: "harmonic product: invalid argument"}


def hps_bins(sample_rate, window_size, K, min_f0=80.0, max_f0=2000.0):
    """sonar_hps_bins (host only): findF0Peak's scan range for rows of K bins -> (min_bin, max_bin);
    min_bin > max_bin is an empty range."""
    lo, hi = C.c_int32(), C.c_int32()
    rc = lib().sonar_hps_bins(int(sample_rate), int(window_size), int(K), float(min_f0), float(max_f0), C.byref(lo),
                              C.byref(hi))
    if rc != OK:
        raise SonarError(rc, _HPS_ERRORS.get(rc, "sonar_hps_bins"))
    return lo.value, hi.value


def hps_optimal_harmonics(sample_rate, min_f0):
    """sonar_hps_optimal_harmonics (host only): HarmonicProduct.GetOptimalNumHarmonics."""
    v = C.c_int32()
    rc = lib().sonar_hps_optimal_harmonics(int(sample_rate), float(min_f0), C.byref(v))
    if rc != OK:
        raise SonarError(rc, _HPS_ERRORS.get(rc, "sonar_hps_optimal_harmonics"))
    return v.value


def hps_plan(n, window_size, hop_size):
    """sonar_hps_plan (host only): how Context.hps splits its frames -> dict of frames, chunk_frames,
    n_chunks."""
    v = [C.c_int64() for _ in range(3)]
    rc = lib().sonar_hps_plan(int(n), int(window_size), int(hop_size), *[C.byref(x) for x in v])
    if rc != OK:
        raise SonarError(rc, "window size below 2" if rc == ERR_UNSUPPORTED and 0 < int(window_size) < 2
                         else _HPCP_PLAN_ERRORS.get(rc, "sonar_hps_plan"))
    return dict(zip(("frames", "chunk_frames", "n_chunks"), [x.value for x in v]))


_HPS_OPTIONAL = ("confidence", "strengths", "hps")


# PitchDetectionMethod (SONAR_PITCH_*, pitch_detection.go:16-35), createWindowFunction's strings
# (SONAR_PITCH_WIN_*) and GetPitchDetectionMethodName's names by code
PITCH_METHODS = {"yin": 0, "acf": 1, "nsdf": 2, "hps": 3, "cepstrum": 4, "peaks": 5, "zero_crossing": 6,
                 "peak_picking": 7, "yin_fft": 8, "mpm": 9, "praat": 10}
PITCH_WINDOWS = {"hann": 0, "hamming": 1, "blackman": 2, "rectangular": 3}
PITCH_METHOD_NAMES = ["YIN (Autocorrelation)", "Autocorrelation Function", "Normalized Square Difference Function",
                      "Harmonic Product Spectrum", "Cepstral Analysis", "Spectral Peaks", "Zero Crossing Rate",
                      "Peak Picking", "YIN-FFT Hybrid", "McLeod Pitch Method", "PRAAT Algorithm"]
PITCH_TRACK_FIELDS = ("pitch", "confidence", "voicing", "periodicity", "clarity", "strength", "salience", "stability",
                      "f0_multiple")
PITCH_STABILITY_KEYS = ("mean_pitch", "pitch_std_dev", "coefficient_of_variation", "jitter", "stability",
                        "vibrato_rate", "voiced_frames_ratio")
PITCH_MAX_CANDIDATES = 8


class PitchParams(C.Structure):
    """sonar_pitch_params (PitchDetectionParams, pitch_detection.go:84-117, field for field)."""
    _fields_ = [(n, C.c_int32) for n in ("method", "sample_rate", "window_size", "hop_size")] + \
               [(n, C.c_double) for n in ("min_freq", "max_freq", "yin_threshold", "autocorr_threshold",
                                          "cepstral_threshold", "min_confidence", "min_salience",
                                          "voicing_threshold")] + \
               [("max_harmonics", C.c_int32), ("harmonic_tolerance", C.c_double)] + \
               [(n, C.c_int32) for n in ("pre_emphasis", "window_function", "zero_padding", "median_filter",
                                         "temporal_smoothing", "octave_correction")]


def pitch_params_default(sample_rate, **kw):
    """sonar_pitch_params_default: NewPitchDetector(sample_rate)'s parameters, then the overrides.  method
    and window_function take their names; a window name Go does not know is Hann, as in
    createWindowFunction."""
    p = PitchParams()
    lib().sonar_pitch_params_default(C.byref(p), int(sample_rate))
    for k, v in kw.items():
        if k == "method" and isinstance(v, str):
            v = PITCH_METHODS[v]
        if k == "window_function" and isinstance(v, str):
            v = PITCH_WINDOWS.get(v, 0)
        if not hasattr(p, k):
            raise TypeError(f"unknown pitch parameter {k}")
        setattr(p, k, v)
    return p


def pitch_method_name(method):
    """GetPitchDetectionMethodName (:1163-1190)."""
    return PITCH_METHOD_NAMES[method] if 0 <= method < len(PITCH_METHOD_NAMES) else "Unknown"


def pitch_detect_frames(n, window_size, hop_size):
    """sonar_pitch_detect_frames (host only): the whole frames of n samples."""
    return int(lib().sonar_pitch_detect_frames(int(n), int(window_size), int(hop_size)))


def pitch_curve_width(params):
    """sonar_pitch_curve_width (host only): the parameter checks and the width of a frame's curve;
    raises SonarError with the code of a parameter set the entries refuse."""
    w = int(lib().sonar_pitch_curve_width(C.byref(params)))
    if w < 0:
        raise SonarError(w, "unsupported pitch detection method: %d" % params.method
                         if w == ERR_INVALID and params.method not in (0, 1, 2, 3, 4, 5, 6, 8, 9)
                         else "pitch detection: parameters refused (include/sonar_gpu.h)")
    return w


def pitch_track(params, raw_pitch, raw_confidence, n_candidates=None, second_confidence=None):
    """sonar_pitch_track (host only): postProcessResult + updateTemporalTracking over raw rows in order,
    from an empty history -> dict of PITCH_TRACK_FIELDS."""
    rp, rc_ = _f64(raw_pitch), _f64(raw_confidence)
    F = len(rp)
    nc = None if n_candidates is None else np.ascontiguousarray(n_candidates, dtype=np.int32)
    sc = None if second_confidence is None else _f64(second_confidence)
    out = {k: np.zeros(F) for k in PITCH_TRACK_FIELDS}
    rc = lib().sonar_pitch_track(C.byref(params), F, _ptr(rp), _ptr(rc_), _ptr(nc), _ptr(sc),
                                 *[_ptr(out[k]) for k in PITCH_TRACK_FIELDS])
    if rc != OK:
        raise SonarError(rc, "sonar_pitch_track")
    return out


def pitch_stability(pitch, sample_rate, hop_size=512):
    """sonar_pitch_stability (host only): AnalyzePitchStability -> dict of PITCH_STABILITY_KEYS, or {} for
    the empty map Go returns with fewer than two voiced frames."""
    p = _f64(pitch)
    out, empty = np.zeros(7), C.c_int32()
    rc = lib().sonar_pitch_stability(_ptr(p) if len(p) else None, len(p), int(sample_rate), int(hop_size), _ptr(out),
                                     C.byref(empty))
    if rc != OK:
        raise SonarError(rc, "sonar_pitch_stability")
    return {} if empty.value else dict(zip(PITCH_STABILITY_KEYS, out.tolist()))


# HarmonicRatioMethod (SONAR_HRATIO_*, harmonic_ratio.go:17-24), NoiseFloorMethod's strings
# (SONAR_HRATIO_NOISE_*), getMethodName's names by code and the per-frame outputs in the entries' order
HRATIO_METHODS = {"hnr": 0, "acf": 1, "hps": 2, "comb": 3, "spectral": 4, "yin": 5}
HRATIO_NOISE_METHODS = {"median": 0, "percentile": 1, "minimum": 2}
HRATIO_METHOD_NAMES = ["Harmonic-to-Noise Ratio", "Autocorrelation Function", "Harmonic Product Spectrum",
                       "Comb Filtering", "Spectral Peak Analysis", "YIN-based"]
HRATIO_CATEGORIES = ["Very Low", "Low", "Medium", "High", "Very High"]
HRATIO_FRAME_FIELDS = ("harmonic_ratio", "harmonic_energy", "noise_energy", "total_energy", "f0", "f0_confidence", "snr",
                       "periodicity", "harmonicity", "voicing", "roughness", "num_harmonics", "h_bin", "h_freq", "h_amp",
                       "h_phase", "noise_floor")
HRATIO_FIELDS = ("harmonic_ratio", "temporal_stability", "temporal_coherence") + HRATIO_FRAME_FIELDS[1:]
HRATIO_MAX_HARMONICS = 64


class HratioParams(C.Structure):
    """sonar_hratio_params (HarmonicRatioParams, harmonic_ratio.go:27-57, field for field, and
    autocorr_max_lag)."""
    _fields_ = [(n, C.c_int32) for n in ("method", "sample_rate", "window_size", "hop_size")] + \
               [("min_freq", C.c_double), ("max_freq", C.c_double), ("max_harmonics", C.c_int32),
                ("harmonic_tolerance", C.c_double), ("min_peak_height", C.c_double),
                ("peak_detection_width", C.c_int32), ("spectral_smoothing_len", C.c_int32),
                ("noise_floor_method", C.c_int32), ("noise_floor_percentile", C.c_double)] + \
               [(n, C.c_int32) for n in ("noise_floor_smoothing_len", "use_temporal_smoothing", "temporal_smoothing_len",
                                         "use_freq_weighting", "use_psychoacoustic_mask", "adaptive_threshold",
                                         "autocorr_max_lag")]


def hratio_params_default(sample_rate, **kw):
    """sonar_hratio_params_default: NewHarmonicRatioAnalyzer(sample_rate)'s parameters, then the overrides.
    method and noise_floor_method take their names; a noise floor name Go does not know is "percentile",
    as in estimateNoiseFloor."""
    p = HratioParams()
    lib().sonar_hratio_params_default(C.byref(p), int(sample_rate))
    for k, v in kw.items():
        if k == "method" and isinstance(v, str):
            v = HRATIO_METHODS[v]
        if k == "noise_floor_method" and isinstance(v, str):
            v = HRATIO_NOISE_METHODS.get(v, 1)
        if not hasattr(p, k):
            raise TypeError(f"unknown harmonic ratio parameter {k}")
        setattr(p, k, v)
    return p


def hratio_method_name(method):
    """getMethodName (:1015-1032)."""
    return HRATIO_METHOD_NAMES[method] if 0 <= method < len(HRATIO_METHOD_NAMES) else "Unknown"


def hratio_check(params):
    """sonar_hratio_check (host only): SONAR_OK or the code of a parameter set the entries refuse."""
    return int(lib().sonar_hratio_check(C.byref(params)))


def hratio_track(params, raw_harmonic_ratio, raw_f0=None):
    """sonar_hratio_track (host only): postProcessResult + updateTemporalTracking over raw rows in order,
    from an empty history -> dict of harmonic_ratio, temporal_stability, temporal_coherence."""
    r = _f64(raw_harmonic_ratio)
    f0 = None if raw_f0 is None else _f64(raw_f0)
    F = len(r)
    out = {k: np.zeros(F) for k in HRATIO_FIELDS[:3]}
    rc = lib().sonar_hratio_track(C.byref(params), F, _ptr(r), _ptr(f0), *[_ptr(out[k]) for k in HRATIO_FIELDS[:3]])
    if rc != OK:
        raise SonarError(rc, "runtime error: slice bounds out of range [%d:1]" % (1 - 2 * params.temporal_smoothing_len)
                         if rc == ERR_PANIC else "sonar_hratio_track")
    return out


def hratio_average(harmonic_ratio):
    """sonar_hratio_average (host only): GetAverageHarmonicRatio."""
    r = _f64(harmonic_ratio)
    return float(lib().sonar_hratio_average(_ptr(r) if len(r) else None, len(r)))


def hratio_classify(harmonic_ratio):
    """sonar_hratio_classify (host only): ClassifyHarmonicRatio's string."""
    L = lib()
    return L.sonar_hratio_category_name(L.sonar_hratio_classify(float(harmonic_ratio))).decode()


def hratio_voicing_quality(harmonic_ratio):
    """sonar_hratio_voicing_quality (host only): EstimateVoicingQuality."""
    return float(lib().sonar_hratio_voicing_quality(float(harmonic_ratio)))


def _hratio_arrays(F, K, mh, want):
    """host arrays of the wanted per-frame outputs (None for the others), in HRATIO_FRAME_FIELDS' order"""
    shape = {"num_harmonics": ((F,), np.int32), "h_bin": ((F, mh), np.int32), "h_freq": ((F, mh), np.float64),
             "h_amp": ((F, mh), np.float64), "h_phase": ((F, mh), np.float64), "noise_floor": ((F, K), np.float64)}
    out = {}
    for k in HRATIO_FRAME_FIELDS:
        s, t = shape.get(k, ((F,), np.float64))
        out[k] = np.zeros(s, t) if (want is None or k in want) else None
    return out


# InharmonicityMethod / InharmonicityModel (SONAR_INHARM_*, inharmonicity.go:17-34), the row statuses and the
# per-frame outputs in the entries' order
INHARM_METHODS = {"railsback": 0, "fletcher_munson": 1, "spectral_deviation": 2, "partial_tracking": 3,
                  "beat_pattern": 4, "statistical": 5}
INHARM_MODELS = {"string": 0, "pipe": 1, "membrane": 2, "general": 3}
INHARM_OK, INHARM_INVALID_F0, INHARM_INSUFFICIENT = 0, 1, 2
INHARM_FRAME_FIELDS = ("status", "inharmonicity", "std_dev", "confidence", "f0", "f0_confidence", "num_harmonics",
                       "n_deviations", "h_number", "h_freq", "h_ideal", "h_amp", "h_deviation", "estimated_stiffness",
                       "model_fit_quality", "harmonic_clarity", "spectral_purity", "partial_coherence", "r_squared",
                       "chi_squared", "p_value", "quality")
INHARM_TRACK_FIELDS = ("inharmonicity", "temporal_stability", "inharmonicity_trend", "f0_stability")
INHARM_FIELDS = ("status",) + INHARM_TRACK_FIELDS + INHARM_FRAME_FIELDS[2:]
INHARM_MAX_HARMONICS = 64
_INHARM_INT = ("status", "num_harmonics", "n_deviations", "h_number", "quality")
_INHARM_ROWS = ("h_number", "h_freq", "h_ideal", "h_amp", "h_deviation")


class InharmParams(C.Structure):
    """sonar_inharm_params (InharmonicityParams, inharmonicity.go:37-72, field for field)."""
    _fields_ = [(n, C.c_int32) for n in ("method", "model", "sample_rate", "window_size", "max_harmonics",
                                         "min_harmonics")] + \
               [(n, C.c_double) for n in ("harmonic_tolerance", "min_harmonic_strength", "min_freq", "max_freq",
                                          "freq_resolution")] + \
               [(n, C.c_int32) for n in ("reference_harmonic", "weight_by_amplitude", "use_log_frequency")] + \
               [(n, C.c_double) for n in ("string_tension", "string_length", "string_stiffness", "outlier_threshold",
                                          "confidence_level")] + \
               [(n, C.c_int32) for n in ("use_robust_estimation", "use_temporal_tracking", "temporal_window")]


def inharm_params_default(sample_rate, **kw):
    """sonar_inharm_params_default: NewInharmonicityAnalyzer(sample_rate)'s parameters (window 4096 included),
    then the overrides.  method and model take their names."""
    p = InharmParams()
    lib().sonar_inharm_params_default(C.byref(p), int(sample_rate))
    for k, v in kw.items():
        if k == "method" and isinstance(v, str):
            v = INHARM_METHODS[v]
        if k == "model" and isinstance(v, str):
            v = INHARM_MODELS[v]
        if not hasattr(p, k):
            raise TypeError(f"unknown inharmonicity parameter {k}")
        setattr(p, k, v)
    return p


def inharm_check(params):
    """sonar_inharm_check (host only): SONAR_OK or the code of a parameter set the entries refuse."""
    return int(lib().sonar_inharm_check(C.byref(params)))


def inharm_track(params, raw_inharmonicity, f0, status=None):
    """sonar_inharm_track (host only): postProcessResult + updateTemporalTracking over rows in order, from an
    empty history -> dict of INHARM_TRACK_FIELDS.  Rows whose status is not INHARM_OK pass through."""
    r, f = _f64(raw_inharmonicity), _f64(f0)
    st = None if status is None else np.ascontiguousarray(status, np.int32)
    F = len(r)
    out = {k: np.zeros(F) for k in INHARM_TRACK_FIELDS}
    rc = lib().sonar_inharm_track(C.byref(params), F, _ptr(st), _ptr(r) if F else None, _ptr(f) if F else None,
                                  *[_ptr(out[k]) for k in INHARM_TRACK_FIELDS])
    if rc != OK:
        raise SonarError(rc, "runtime error: slice bounds out of range [%d:1]" % (1 - params.temporal_window)
                         if rc == ERR_PANIC else "sonar_inharm_track")
    return out


def inharm_average(inharmonicity, confidence):
    """sonar_inharm_average (host only): GetAverageInharmonicity."""
    i, c = _f64(inharmonicity), _f64(confidence)
    return float(lib().sonar_inharm_average(_ptr(i) if len(i) else None, _ptr(c) if len(c) else None, min(len(i), len(c))))


def _inharm_name(fn, code):
    s = fn(int(code))
    return None if s is None else s.decode()


def inharm_classify(inharmonicity):
    """sonar_inharm_classify (host only): ClassifyInharmonicity's string."""
    L = lib()
    return _inharm_name(L.sonar_inharm_class_name, L.sonar_inharm_classify(float(inharmonicity)))


def inharm_instrument_type(inharmonicity, f0):
    """sonar_inharm_instrument_type (host only): EstimateInstrumentType's string."""
    L = lib()
    return _inharm_name(L.sonar_inharm_instrument_name, L.sonar_inharm_instrument_type(float(inharmonicity), float(f0)))


def inharm_method_name(method):
    """getMethodName (:1139-1156)."""
    return _inharm_name(lib().sonar_inharm_method_name, method)


def inharm_model_name(model):
    """getModelName (:1158-1171)."""
    return _inharm_name(lib().sonar_inharm_model_name, model)


def inharm_quality_name(quality):
    """AnalysisQuality's string of a SONAR_INHARM_QUALITY_* code; None outside the enum (an INSUFFICIENT row)."""
    return _inharm_name(lib().sonar_inharm_quality_name, quality)


def _inharm_arrays(F, mh, want, fields=INHARM_FRAME_FIELDS):
    """host arrays of the wanted outputs (None for the others)"""
    out = {}
    for k in fields:
        shape = (F, mh) if k in _INHARM_ROWS else (F,)
        out[k] = np.zeros(shape, np.int32 if k in _INHARM_INT else np.float64) if (want is None or k in want) else None
    return out


_ONSET_ERRORS = {ERR_UNSUPPORTED: "onsets: parameters the library does not reproduce (include/sonar_gpu.h)",
                 ERR_INVALID: "onsets: invalid argument"}


def onset_peaks_width(n):
    """sonar_onset_peaks_width (host only): the most peaks findFluxPeaks returns on n values."""
    return int(lib().sonar_onset_peaks_width(int(n)))


def rms_envelope_frames(n, frame_size, hop_size):
    """sonar_rms_envelope_frames (host only): len(Envelope.ComputeRMS(...))."""
    return int(lib().sonar_rms_envelope_frames(int(n), int(frame_size), int(hop_size)))


def onsets_complex_width(n):
    """sonar_onsets_complex_width (host only): the slots Context.onsets_complex needs for n samples."""
    return int(lib().sonar_onsets_complex_width(int(n)))


def onset_min_interval_frames(min_interval, sample_rate, hop_size):
    """sonar_onset_min_interval_frames (host only): findFluxPeaks' minIntervalFrames."""
    v = C.c_int32()
    rc = lib().sonar_onset_min_interval_frames(float(min_interval), int(sample_rate), int(hop_size), C.byref(v))
    if rc != OK:
        raise SonarError(rc, _ONSET_ERRORS.get(rc, "sonar_onset_min_interval_frames"))
    return v.value


def tempo_from_onsets(onsets, sample_rate):
    """sonar_tempo_from_onsets (host only): EstimateTempo's tail over a list of onset samples ->
    (tempo, the 14 votes of findTempoFromIntervals' bins)."""
    a = np.ascontiguousarray(onsets, dtype=np.int64)
    t, counts = C.c_double(), np.zeros(14, np.int32)
    rc = lib().sonar_tempo_from_onsets(_ptr(a) if a.size else None, int(a.size), int(sample_rate), C.byref(t),
                                       counts.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != OK:
        raise SonarError(rc, _ONSET_ERRORS.get(rc, "sonar_tempo_from_onsets"))
    return t.value, counts


def tempo_autocorr_plan(n, sample_rate):
    """sonar_tempo_autocorr_plan (host only): EstimateTempoAutocorrelation's integer side -> dict of
    frame_size, hop_size, envelope_len, n_autocorr, min_lag, max_lag."""
    a, b = C.c_int32(), C.c_int32()
    v = [C.c_int64() for _ in range(4)]
    rc = lib().sonar_tempo_autocorr_plan(int(n), int(sample_rate), C.byref(a), C.byref(b), *[C.byref(x) for x in v])
    if rc != OK:
        raise SonarError(rc, _ONSET_ERRORS.get(rc, "sonar_tempo_autocorr_plan"))
    return dict(frame_size=a.value, hop_size=b.value, envelope_len=v[0].value, n_autocorr=v[1].value,
                min_lag=v[2].value, max_lag=v[3].value)


def tempo_category(tempo):
    """sonar_tempo_category (host only): ClassifyTempoCategory's SONAR_TEMPO_* code."""
    return int(lib().sonar_tempo_category(float(tempo)))


def tempo_category_name(category):
    """sonar_tempo_category_name (host only)."""
    return lib().sonar_tempo_category_name(int(category)).decode()


def multi_shard(n, W, H, n_shards, shard):
    """sonar_multi_shard: (f0, f1, s0, s1) of frame shard `shard` of `n_shards` (pure arithmetic)."""
    v = [C.c_int64() for _ in range(4)]
    rc = lib().sonar_multi_shard(n, W, H, n_shards, shard, *[C.byref(x) for x in v])
    if rc != OK:
        raise SonarError(rc, "sonar_multi_shard")
    return tuple(x.value for x in v)


def _pair_arrays(qs, rs):
    """ctypes pointer/length arrays of two lists of streams (device int pointers or numpy arrays)."""
    keep = []

    def ptr(x):
        if isinstance(x, (int, np.integer)):
            return int(x)
        a = _f64(x)
        keep.append(a)
        return a.ctypes.data
    n = len(qs)
    qp = (C.c_void_p * n)(*[ptr(x) for x in qs])
    rp = (C.c_void_p * n)(*[ptr(x) for x in rs])
    return qp, rp, keep


def records_dict(recs):
    """sonar_pair_record array -> dict of numpy arrays (PAIR_FIELDS + status)."""
    out = {f: np.array([getattr(r, f) for r in recs]) for f in PAIR_FIELDS}
    out["status"] = np.array([r.status for r in recs], dtype=np.int32)
    out["flags"] = np.array([r.flags for r in recs], dtype=np.int32)
    return out


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


class _ResultOwner:
    """Owns a sonar_result handle; freed (sonar_result_free) when no view of it remains."""
    def __init__(self, L, h):
        self._L, self._h = L, h

    def __del__(self):
        if self._h:
            self._L.sonar_result_free(self._h)
            self._h = None


class _ResultView:
    """numpy's array interface over one result array; the array's base keeps the owner alive."""
    def __init__(self, owner, addr, shape):
        self._owner = owner
        self.__array_interface__ = {"shape": shape, "typestr": "<f8", "data": (addr, False), "version": 3}


def _pcm_arg(x, device_ptrs):
    """(pointer, length, owner) of a PCM argument: a host float64 array, or (device pointer, n); the
    caller keeps `owner` alive across the call (a converted copy)."""
    if device_ptrs:
        p, n = x
        return C.c_void_p(int(p)), int(n), None
    a = _f64(x)
    return (_ptr(a) if a.size else None), int(a.size), a


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class Context:
    """One sonar_ctx (one HIP stream) on `device`."""

    def __init__(self, device=0):
        L = lib()
        h = C.c_void_p()
        rc = L.sonar_create(device, C.byref(h))
        if rc != OK:
            raise SonarError(rc, "sonar_create failed (no GPU visible?)")
        self._h = h
        self._L = L

    @classmethod
    def wrap(cls, handle, owner=None):
        """A non-owning Context over an existing sonar_ctx (e.g. sonar_multi_ctx); `owner` is kept
        alive with it.  close() does not destroy the handle."""
        self = cls.__new__(cls)
        self._h = handle if isinstance(handle, C.c_void_p) else C.c_void_p(handle)
        self._L = lib()
        self._borrowed = owner if owner is not None else True
        return self

    def close(self):
        if getattr(self, "_h", None):
            if not getattr(self, "_borrowed", None):
                self._L.sonar_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != OK:
            raise SonarError(rc, self._L.sonar_last_error(self._h).decode())

    # -- stream / timing -------------------------------------------------
    def set_stream(self, stream_handle):
        self._check(self._L.sonar_set_stream(self._h, C.c_void_p(stream_handle or 0) if stream_handle else None))

    def synchronize(self):
        self._check(self._L.sonar_synchronize(self._h))

    def enable_kernel_timing(self, on=True):
        self._check(self._L.sonar_enable_kernel_timing(self._h, int(on)))

    def last_kernel_ms(self):
        v = C.c_double()
        self._check(self._L.sonar_last_kernel_ms(self._h, C.byref(v)))
        return v.value

    def dtw_last_timing(self):
        """(band sweep, walk, path decode) kernel ms of the last dtw call (HIP events)."""
        v = (C.c_double * 3)()
        self._check(self._L.sonar_dtw_last_timing(self._h, v))
        return tuple(v)

    def dtw_counters(self, reset=False):
        """Band-pipeline liveness counters since the last reset (sonar_dtw_counters): edge refresh
        fences, fences followed by new edge values, timed-out DTWs, timed-out waves."""
        v = (C.c_int64 * 4)()
        self._check(self._L.sonar_dtw_counters(self._h, v, int(bool(reset))))
        return {"edge_refresh_fences": v[0], "edge_refresh_hits": v[1], "dtw_timeouts": v[2],
                "waves_timed_out": v[3]}

    def trim(self):
        """Free the device / pinned host buffers this context and its pair workers cache
        (sonar_trim); the next call allocates again."""
        self._check(self._L.sonar_trim(self._h))

    def last_fp_kernel(self):
        """Name of the fused kernel the last fingerprint call launched (diagnostics)."""
        return self._L.sonar_last_fp_kernel(self._h).decode()

    # -- path A ------------------------------------------------------------
    @staticmethod
    def config(**kw):
        cfg = FpConfig()
        lib().sonar_fp_cfg_default(C.byref(cfg))
        for k, v in kw.items():
            if k == "window_type" and isinstance(v, str):
                v = WINDOWS[v]
            setattr(cfg, k, v)
        return cfg

    def fingerprint(self, pcm, cfg: FpConfig):
        """Host-buffer form: returns a dict of numpy arrays for the requested flags."""
        pcm = np.ascontiguousarray(pcm, dtype=np.float64 if cfg.pcm_dtype == F64 else np.float32)
        n = len(pcm)
        cfg.device_ptrs = 0
        res, out = self._fp_outputs(n, cfg)
        self._check(self._L.sonar_fingerprint(self._h, _ptr(pcm) if n else None, n, C.byref(cfg), C.byref(out)))
        return res

    def fingerprint_batch(self, signals, cfg: FpConfig):
        """sonar_fingerprint_batch (SpectralAnalyzer.ComputeSTFTBatch, spectral.go:234-285), host
        buffers: one dict of numpy arrays per signal, as fingerprint() returns."""
        dt = np.float64 if cfg.pcm_dtype == F64 else np.float32
        sigs = [np.ascontiguousarray(x, dtype=dt) for x in signals]
        cfg.device_ptrs = 0
        k = len(sigs)
        ptrs = (_vp * max(k, 1))(*[x.ctypes.data if x.size else None for x in sigs])
        ns = (C.c_int64 * max(k, 1))(*[x.size for x in sigs])
        outs = (FpOut * max(k, 1))()
        res = []
        for i, x in enumerate(sigs):
            r, o = self._fp_outputs(x.size, cfg)
            res.append(r)
            outs[i] = o
        self._check(self._L.sonar_fingerprint_batch(self._h, ptrs, ns, k, C.byref(cfg), outs))
        return res

    def fingerprint_batch_device(self, pcm_ptrs, ns, mfcc_ptrs, cfg: FpConfig):
        """Device-pointer form (async on the ctx stream): MFCC outputs only (mfcc_ptrs[i] -> F_i x n_mfcc)."""
        cfg.device_ptrs = 1
        k = len(pcm_ptrs)
        outs = (FpOut * max(k, 1))()
        for i, m in enumerate(mfcc_ptrs):
            outs[i].mfcc = m
        self._check(self._L.sonar_fingerprint_batch(self._h, (_vp * max(k, 1))(*pcm_ptrs),
                                                    (C.c_int64 * max(k, 1))(*ns), k, C.byref(cfg), outs))

    def fingerprint_f64le(self, data, cfg: FpConfig, mode=INGEST_HOST_CONVERT):
        """sonar_fingerprint_f64le: the decoder's f64le bytes (decoder.go:850-871) straight into path A."""
        buf = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) \
            else np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        cfg.device_ptrs = 0
        res, out = self._fp_outputs(buf.size // 8, cfg)
        self._check(self._L.sonar_fingerprint_f64le(self._h, buf.ctypes.data if buf.size else None, buf.size, mode,
                                                    C.byref(cfg), C.byref(out)))
        return res

    def _fp_outputs(self, n, cfg, frames=None):
        if frames is not None:
            F = frames
        else:
            F = stft_frames(n, cfg.window_size, cfg.hop_size) if n > 0 and cfg.window_size > 0 and cfg.hop_size > 0 else 0
        od = np.float64 if cfg.out_dtype == F64 else np.float32
        out, res = FpOut(), {}
        if F > 0:
            K = cfg.window_size // 2 + 1
            nm = cfg.n_mfcc if cfg.n_mfcc > 0 else 13
            if cfg.flags & FP_MFCC:
                res["mfcc"] = np.zeros((F, nm), od)
                out.mfcc = res["mfcc"].ctypes.data
            if cfg.flags & FP_MAGNITUDE:
                res["magnitude"] = np.zeros((F, K), od)
                out.magnitude = res["magnitude"].ctypes.data
            if cfg.flags & FP_COMPLEX:      # (re, im) interleaved: a complex view of an F x K x 2 array
                res["complex"] = np.zeros((F, K, 2), od)
                out.complex = res["complex"].ctypes.data
            if cfg.flags & FP_PHASE:
                res["phase"] = np.zeros((F, K), od)
                out.phase = res["phase"].ctypes.data
            if cfg.flags & FP_SPECTRAL:
                for nme in SPECTRAL_NAMES:
                    res[nme] = np.zeros(max(F - 1, 0) if nme == "flux" else F, od)
                    setattr(out, nme, res[nme].ctypes.data if res[nme].size else None)
            if cfg.flags & FP_ZCR:
                res["zcr"] = np.zeros(F, od)
                out.zcr = res["zcr"].ctypes.data
            if cfg.flags & FP_ENERGY:
                fe = energy_frames(n, cfg.energy_window, cfg.energy_hop)
                res["energy"] = np.zeros(fe, od)
                out.energy = res["energy"].ctypes.data if fe > 0 else None
        return res, out

    def stft_stream(self, cfg: FpConfig):
        """sonar_stft_stream_create: SpectralAnalyzer.ComputeSTFTStreaming (spectral.go:287-312)."""
        h = C.c_void_p()
        self._check(self._L.sonar_stft_stream_create(self._h, C.byref(cfg), C.byref(h)))
        return StftStream(self, h, cfg)

    def fingerprint_device(self, pcm_ptr, n, cfg: FpConfig, **out_ptrs):
        """Device-pointer form (async on the ctx stream): out_ptrs name -> device address."""
        cfg.device_ptrs = 1
        out = FpOut()
        for k, v in out_ptrs.items():
            setattr(out, k, v)
        self._check(self._L.sonar_fingerprint(self._h, C.c_void_p(pcm_ptr), n, C.byref(cfg), C.byref(out)))

    def pitch_yin(self, pcm, sample_rate):
        pcm = _f64(pcm)
        F = pitch_frames(len(pcm))
        p, c, t = np.zeros(F), np.zeros(F), np.zeros(F, np.int32)
        self._check(self._L.sonar_pitch_yin(self._h, _ptr(pcm), len(pcm), sample_rate, _ptr(p), _ptr(c), _ptr(t), 0))
        return p, c, t

    def pitch_frames_raw(self, pcm, params, max_candidates=PITCH_MAX_CANDIDATES, want_curve=True):
        """DetectPitch up to postProcessResult per whole frame of pcm (sonar_pitch_frames_raw) -> dict of
        pitch, confidence, index, n_candidates, second_confidence, cand_index, cand_conf (F x
        max_candidates) and curve (F x pitch_curve_width(params), when wanted)."""
        pcm = _f64(pcm)
        F = pitch_detect_frames(len(pcm), params.window_size, params.hop_size)
        K = int(max_candidates)
        width = max(int(self._L.sonar_pitch_curve_width(C.byref(params))), 0)
        out = {"pitch": np.zeros(F), "confidence": np.zeros(F), "index": np.zeros(F, np.int32),
               "n_candidates": np.zeros(F, np.int32), "second_confidence": np.zeros(F),
               "cand_index": np.zeros((F, max(K, 0)), np.int32), "cand_conf": np.zeros((F, max(K, 0))),
               "curve": np.zeros((F, width)) if want_curve else None}
        self._check(self._L.sonar_pitch_frames_raw(self._h, _ptr(pcm) if len(pcm) else None, len(pcm), C.byref(params), K,
                                                   *[_ptr(out[k]) for k in ("pitch", "confidence", "index",
                                                                            "n_candidates", "second_confidence",
                                                                            "cand_index", "cand_conf", "curve")], 0))
        return out

    def pitch_frames_raw_device(self, pcm_ptr, n, params, pitch_ptr, confidence_ptr, max_candidates=0, index_ptr=None,
                                n_candidates_ptr=None, second_confidence_ptr=None, cand_index_ptr=None,
                                cand_conf_ptr=None, curve_ptr=None):
        """pitch_frames_raw on device memory (device_ptrs = 1): every array is a device address."""
        self._check(self._L.sonar_pitch_frames_raw(self._h, pcm_ptr, int(n), C.byref(params), int(max_candidates),
                                                   pitch_ptr, confidence_ptr, index_ptr, n_candidates_ptr,
                                                   second_confidence_ptr, cand_index_ptr, cand_conf_ptr, curve_ptr, 1))

    def pitch_detect(self, pcm, params):
        """ProcessAudioStream over the whole frames of pcm (sonar_pitch_detect): the raw pass, then the
        tracker -> dict of PITCH_TRACK_FIELDS."""
        pcm = _f64(pcm)
        F = pitch_detect_frames(len(pcm), params.window_size, params.hop_size)
        out = {k: np.zeros(F) for k in PITCH_TRACK_FIELDS}
        frames = C.c_int64()
        self._check(self._L.sonar_pitch_detect(self._h, _ptr(pcm) if len(pcm) else None, len(pcm), C.byref(params),
                                               *[_ptr(out[k]) for k in PITCH_TRACK_FIELDS], C.byref(frames), 0))
        assert frames.value == F
        return out

    def pitch_detect_device(self, pcm_ptr, n, params, out_ptrs):
        """pitch_detect on device memory (device_ptrs = 1): out_ptrs maps names of PITCH_TRACK_FIELDS to
        device addresses of F doubles (missing: not wanted) -> the frame count."""
        frames = C.c_int64()
        self._check(self._L.sonar_pitch_detect(self._h, pcm_ptr, int(n), C.byref(params),
                                               *[out_ptrs.get(k) for k in PITCH_TRACK_FIELDS], C.byref(frames), 1))
        return frames.value

    def hratio_from_spectrum(self, mag, params, phase=None, want=None):
        """Everything AnalyzeFrame does after the transform (HNR, Comb, HPS, Spectral) on rows of W / 2
        unsmoothed magnitudes (sonar_hratio_from_spectrum) -> dict of HRATIO_FRAME_FIELDS; `want` names the
        outputs to compute (all by default), the others are None."""
        mag = np.atleast_2d(_f64(mag))
        F, K = mag.shape
        ph = None if phase is None else np.atleast_2d(_f64(phase))
        out = _hratio_arrays(F, K, max(params.max_harmonics, 0), want)
        self._check(self._L.sonar_hratio_from_spectrum(self._h, _ptr(mag) if F else None, _ptr(ph), F, K, C.byref(params),
                                                       *[_ptr(out[k]) for k in HRATIO_FRAME_FIELDS], 0))
        return out

    def hratio_frames(self, pcm, params, want=None):
        """AnalyzeFrame up to postProcessResult per whole frame of pcm, every method (sonar_hratio_frames) ->
        dict of HRATIO_FRAME_FIELDS."""
        pcm = _f64(pcm)
        F = pitch_detect_frames(len(pcm), params.window_size, params.hop_size)
        out = _hratio_arrays(F, max(params.window_size // 2, 0), max(params.max_harmonics, 0), want)
        self._check(self._L.sonar_hratio_frames(self._h, _ptr(pcm) if len(pcm) else None, len(pcm), C.byref(params),
                                                *[_ptr(out[k]) for k in HRATIO_FRAME_FIELDS], 0))
        return out

    def hratio(self, pcm, params, want=None):
        """AnalyzeSequence over the whole frames of pcm (sonar_hratio): the per-frame pass, then the tracker
        -> dict of HRATIO_FIELDS."""
        pcm = _f64(pcm)
        F = pitch_detect_frames(len(pcm), params.window_size, params.hop_size)
        fr = _hratio_arrays(F, max(params.window_size // 2, 0), max(params.max_harmonics, 0), want)
        out = {k: (np.zeros(F) if (want is None or k in want) else None) for k in HRATIO_FIELDS[:3]}
        out.update({k: fr[k] for k in HRATIO_FRAME_FIELDS[1:]})
        frames = C.c_int64()
        self._check(self._L.sonar_hratio(self._h, _ptr(pcm) if len(pcm) else None, len(pcm), C.byref(params),
                                         *[_ptr(out[k]) for k in HRATIO_FIELDS], C.byref(frames), 0))
        assert frames.value == F
        return out

    def hratio_device(self, entry, pcm_ptr, n, params, out_ptrs):
        """sonar_hratio_frames ("frames") or sonar_hratio ("sequence") on device memory (device_ptrs = 1):
        out_ptrs maps output names to device addresses (missing: not wanted) -> the frame count."""
        if entry == "frames":
            self._check(self._L.sonar_hratio_frames(self._h, pcm_ptr, int(n), C.byref(params),
                                                    *[out_ptrs.get(k) for k in HRATIO_FRAME_FIELDS], 1))
            return pitch_detect_frames(int(n), params.window_size, params.hop_size)
        frames = C.c_int64()
        self._check(self._L.sonar_hratio(self._h, pcm_ptr, int(n), C.byref(params),
                                         *[out_ptrs.get(k) for k in HRATIO_FIELDS], C.byref(frames), 1))
        return frames.value

    def hratio_from_spectrum_device(self, mag_ptr, phase_ptr, F, K, params, out_ptrs):
        """hratio_from_spectrum on device memory (device_ptrs = 1)."""
        self._check(self._L.sonar_hratio_from_spectrum(self._h, mag_ptr, phase_ptr, int(F), int(K), C.byref(params),
                                                       *[out_ptrs.get(k) for k in HRATIO_FRAME_FIELDS], 1))

    def inharm_from_spectrum(self, mag, f0, f0_confidence, params, want=None):
        """Everything AnalyzeFrame does after the transform, on rows of W / 2 magnitudes of the unwindowed
        frame and each frame's f0 and its confidence (sonar_inharm_from_spectrum) -> dict of
        INHARM_FRAME_FIELDS; `want` names the outputs to compute (all by default), the others are None."""
        mag = np.atleast_2d(_f64(mag))
        F, K = mag.shape
        f0, fc = _f64(f0), _f64(f0_confidence)
        assert len(f0) == F and len(fc) == F
        out = _inharm_arrays(F, max(params.max_harmonics, 0), want)
        self._check(self._L.sonar_inharm_from_spectrum(self._h, _ptr(mag) if F else None, _ptr(f0) if F else None,
                                                       _ptr(fc) if F else None, F, K, C.byref(params),
                                                       *[_ptr(out[k]) for k in INHARM_FRAME_FIELDS], 0))
        return out

    def inharm_frames(self, pcm, hop_size, params, want=None):
        """AnalyzeFrame without the tracking per whole frame of pcm, every method (sonar_inharm_frames) -> dict
        of INHARM_FRAME_FIELDS."""
        pcm = _f64(pcm)
        F = pitch_detect_frames(len(pcm), params.window_size, hop_size)
        out = _inharm_arrays(F, max(params.max_harmonics, 0), want)
        self._check(self._L.sonar_inharm_frames(self._h, _ptr(pcm) if len(pcm) else None, len(pcm), int(hop_size),
                                                C.byref(params), *[_ptr(out[k]) for k in INHARM_FRAME_FIELDS], 0))
        return out

    def inharm(self, pcm, hop_size, params, want=None):
        """AnalyzeSequence over the whole frames of pcm (sonar_inharm): the per-frame pass, then the tracker ->
        dict of INHARM_FIELDS.  Where Go returns nil and an error (the first frame with too few harmonics) this
        raises SonarError with Go's message; its `frame` attribute is that frame and `rows` the dict, whose
        rows before that frame are written."""
        pcm = _f64(pcm)
        F = pitch_detect_frames(len(pcm), params.window_size, hop_size)
        out = _inharm_arrays(F, max(params.max_harmonics, 0), want, INHARM_FIELDS)
        frames, bad = C.c_int64(), C.c_int64(-1)
        try:
            self._check(self._L.sonar_inharm(self._h, _ptr(pcm) if len(pcm) else None, len(pcm), int(hop_size),
                                             C.byref(params), *[_ptr(out[k]) for k in INHARM_FIELDS], C.byref(frames),
                                             C.byref(bad), 0))
        except SonarError as e:
            e.frame, e.rows = bad.value, out
            raise
        assert frames.value == F
        return out

    def inharm_device(self, entry, pcm_ptr, n, hop_size, params, out_ptrs):
        """sonar_inharm_frames ("frames") or sonar_inharm ("sequence") on device memory (device_ptrs = 1):
        out_ptrs maps output names to device addresses (missing: not wanted) -> the frame count."""
        if entry == "frames":
            self._check(self._L.sonar_inharm_frames(self._h, pcm_ptr, int(n), int(hop_size), C.byref(params),
                                                    *[out_ptrs.get(k) for k in INHARM_FRAME_FIELDS], 1))
            return pitch_detect_frames(int(n), params.window_size, hop_size)
        frames, bad = C.c_int64(), C.c_int64(-1)
        self._check(self._L.sonar_inharm(self._h, pcm_ptr, int(n), int(hop_size), C.byref(params),
                                         *[out_ptrs.get(k) for k in INHARM_FIELDS], C.byref(frames), C.byref(bad), 1))
        return frames.value

    def inharm_from_spectrum_device(self, mag_ptr, f0_ptr, f0_confidence_ptr, F, K, params, out_ptrs):
        """inharm_from_spectrum on device memory (device_ptrs = 1)."""
        self._check(self._L.sonar_inharm_from_spectrum(self._h, mag_ptr, f0_ptr, f0_confidence_ptr, int(F), int(K),
                                                       C.byref(params), *[out_ptrs.get(k) for k in INHARM_FRAME_FIELDS], 1))

    def chroma_stft(self, pcm, n_frames, hop, sample_rate, preprocess=True):
        pcm = _f64(pcm)
        out = np.zeros((n_frames, 12))
        self._check(self._L.sonar_chroma_stft(self._h, _ptr(pcm), len(pcm), n_frames, hop, sample_rate,
                                              int(preprocess), _ptr(out), 0))
        return out

    def chroma_cqt(self, pcm, hop, sample_rate, min_freq=65.4, max_freq=2093.0, bins_per_octave=12, q_factor=25.0,
                   tuning_freq=440.0, return_cqt=False):
        """NewChromaCQT(sample_rate, min_freq, max_freq, bins_per_octave, q_factor, tuning_freq)
        .ComputeChroma(pcm, hop) (sonar_chroma_cqt; the defaults are NewChromaCQTDefault's) -> the
        (n_frames, 12) chroma, with return_cqt also the (n_frames, total_bins) CQT magnitudes.  An empty
        signal gives a (0, 12) array (Go returns nil, nil)."""
        pcm = _f64(pcm)
        n = len(pcm)
        params = (int(sample_rate), float(min_freq), float(max_freq), int(bins_per_octave), float(q_factor),
                  float(tuning_freq))
        if n == 0:
            return (np.zeros((0, 12)), np.zeros((0, 0))) if return_cqt else np.zeros((0, 12))
        v = [C.c_int64() for _ in range(4)]
        F = K = 0
        if self._L.sonar_chroma_cqt_plan(*params, n, int(hop), *[C.byref(x) for x in v], None, None) == OK:
            K, F = v[0].value, v[2].value                  # otherwise the call below reports the error
        chroma = np.zeros((F, 12))
        cqt = np.zeros((F, K)) if return_cqt else None
        self._check(self._L.sonar_chroma_cqt(self._h, _ptr(pcm), n, int(hop), *params, _ptr(chroma), _ptr(cqt), 0))
        return (chroma, cqt) if return_cqt else chroma

    @staticmethod
    def _chroma_frames(x):
        x = _f64(x)
        return x.reshape(0, 0) if x.size == 0 else (x[:, None] if x.ndim == 1 else x)

    def chroma_frame_matrix(self, q, r, metric="cosine", shift=0, as_similarity=False):
        """ChromaVectorAnalyzer.Distance (or Similarity) of CircularShift(q[i], shift) and r[j] for every
        pair (sonar_chroma_frame_matrix) -> the (nq, nr) matrix.  metric: a CHROMA_DIST_METRICS name
        or value (unknown values are Euclidean, as in Go)."""
        q, r = self._chroma_frames(q), self._chroma_frames(r)
        nq, nr = q.shape[0], r.shape[0]
        dim = q.shape[1] if nq else (r.shape[1] if nr else 1)
        out = np.zeros((nq, nr))
        self._check(self._L.sonar_chroma_frame_matrix(self._h, _ptr(q) if nq else None, nq, _ptr(r) if nr else None,
                                                      nr, dim, _chroma_enum(CHROMA_DIST_METRICS, metric), int(shift),
                                                      int(bool(as_similarity)), _ptr(out) if out.size else None))
        return out

    def chroma_frame_matrix_device(self, q_ptr, nq, r_ptr, nr, dim, out_ptr, metric="cosine", shift=0,
                                   as_similarity=False):
        """chroma_frame_matrix on device memory: q, r and the nq x nr output are device addresses."""
        self._check(self._L.sonar_chroma_frame_matrix(self._h, q_ptr, int(nq), r_ptr, int(nr), int(dim),
                                                      _chroma_enum(CHROMA_DIST_METRICS, metric), int(shift),
                                                      int(bool(as_similarity)), out_ptr))

    def chroma_similarity(self, q, r, method="direct", metric="cosine", binary_threshold=0.4, oti_radius=10,
                          dtw_band_radius=50, transposition_invariant=False, matrix=True):
        """NewChromaSequenceSimilarityWithParams(...).ComputeSimilarity(q, r) (sonar_chroma_similarity;
        the defaults are NewChromaSequenceSimilarity's) -> dict of matrix ((nq, nr); None when the
        reference's is nil or with matrix=False, which does not materialise it), overall,
        best_transposition, path_q, path_r, path_score (empty unless Smith-Waterman or DTW)."""
        q, r = self._chroma_frames(q), self._chroma_frames(r)
        nq, nr = q.shape[0], r.shape[0]
        dim = q.shape[1] if nq else (r.shape[1] if nr else 1)
        mat = np.zeros((nq, nr)) if matrix else None
        cap = nq + nr + 1
        pq, pr, ps = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap)
        nil, best, overall, plen = C.c_int32(), C.c_int32(), C.c_double(), C.c_int64()
        self._check(self._L.sonar_chroma_similarity(
            self._h, _ptr(q) if nq else None, nq, _ptr(r) if nr else None, nr, dim,
            _chroma_enum(CHROMA_SIM_METHODS, method), _chroma_enum(CHROMA_DIST_METRICS, metric),
            float(binary_threshold), int(oti_radius), int(dtw_band_radius), int(bool(transposition_invariant)),
            _ptr(mat) if mat is not None and mat.size else None, C.byref(nil), C.byref(overall), C.byref(best),
            _ptr(pq), _ptr(pr), _ptr(ps), C.byref(plen)))
        P = plen.value
        return {"matrix": None if nil.value or mat is None else mat, "overall": overall.value,
                "best_transposition": best.value, "path_q": pq[:P], "path_r": pr[:P], "path_score": ps[:P]}

    def chroma_similarity_device(self, q_ptr, nq, r_ptr, nr, dim, method="direct", metric="cosine",
                                 binary_threshold=0.4, oti_radius=10, dtw_band_radius=50,
                                 transposition_invariant=False, matrix_ptr=None, path_q_ptr=None, path_r_ptr=None,
                                 path_score_ptr=None):
        """chroma_similarity on device memory: q, r, the optional nq x nr matrix and the optional path
        arrays (nq + nr entries each) are device addresses -> dict of matrix_is_nil, overall,
        best_transposition, path_len."""
        nil, best, overall, plen = C.c_int32(), C.c_int32(), C.c_double(), C.c_int64()
        self._check(self._L.sonar_chroma_similarity(
            self._h, q_ptr, int(nq), r_ptr, int(nr), int(dim), _chroma_enum(CHROMA_SIM_METHODS, method),
            _chroma_enum(CHROMA_DIST_METRICS, metric), float(binary_threshold), int(oti_radius), int(dtw_band_radius),
            int(bool(transposition_invariant)), matrix_ptr, C.byref(nil), C.byref(overall), C.byref(best),
            path_q_ptr, path_r_ptr, path_score_ptr, C.byref(plen)))
        return {"matrix_is_nil": bool(nil.value), "overall": overall.value, "best_transposition": best.value,
                "path_len": plen.value}

    def chroma_similarity_last_timing(self):
        """(frame matrix, ordered sums, DP fill, traceback) HIP-event ms of the last chroma similarity call."""
        v = (C.c_double * 4)()
        self._check(self._L.sonar_chroma_similarity_last_timing(self._h, v))
        return tuple(v)

    def chroma_cqt_device(self, pcm_ptr, n, hop, sample_rate, chroma_ptr, min_freq=65.4, max_freq=2093.0,
                          bins_per_octave=12, q_factor=25.0, tuning_freq=440.0, cqt_ptr=None):
        """chroma_cqt on device memory (device_ptrs = 1): pcm (n doubles), chroma (n_frames x 12) and the
        optional CQT array (n_frames x total_bins; None: library scratch) are device addresses; the
        sizes are chroma_cqt_plan's."""
        self._check(self._L.sonar_chroma_cqt(self._h, pcm_ptr, int(n), int(hop), int(sample_rate), float(min_freq),
                                             float(max_freq), int(bins_per_octave), float(q_factor),
                                             float(tuning_freq), chroma_ptr, cqt_ptr, 1))

    def spectral_peaks(self, mag, window_size, sample_rate, min_height=0.00001, min_distance_hz=20.0, max_peaks=60):
        """NewSpectralPeaks(sample_rate, min_height, min_distance_hz, max_peaks).DetectPeaks(row,
        window_size) on every row of mag (F x K) (sonar_spectral_peaks; the defaults are
        HPCP.ComputeFromSpectrum's) -> dict of count (F), bin, magnitude, frequency (F x P, sorted by
        magnitude descending then bin ascending, zeros past count)."""
        mag = _f64(mag)
        mag = mag[None, :] if mag.ndim == 1 else mag
        F, K = mag.shape
        P = max(spectral_peaks_width(K, max_peaks), 0)
        count, bins = np.zeros(F, np.int32), np.zeros((F, P), np.int32)
        pm, pf = np.zeros((F, P)), np.zeros((F, P))
        self._check(self._L.sonar_spectral_peaks(self._h, _ptr(mag) if mag.size else None, F, K, int(window_size),
                                                 int(sample_rate), float(min_height), float(min_distance_hz),
                                                 int(max_peaks), _ptr(count) if F else None, _ptr(bins), _ptr(pm),
                                                 _ptr(pf), 0))
        return {"count": count, "bin": bins, "magnitude": pm, "frequency": pf}

    def spectral_peaks_device(self, mag_ptr, F, K, window_size, sample_rate, count_ptr, bin_ptr, magnitude_ptr,
                              frequency_ptr=None, min_height=0.00001, min_distance_hz=20.0, max_peaks=60):
        """spectral_peaks on device memory (device_ptrs = 1): every array is a device address."""
        self._check(self._L.sonar_spectral_peaks(self._h, mag_ptr, int(F), int(K), int(window_size), int(sample_rate),
                                                 float(min_height), float(min_distance_hz), int(max_peaks), count_ptr,
                                                 bin_ptr, magnitude_ptr, frequency_ptr, 1))

    def hpcp_from_spectrum(self, mag, window_size, sample_rate, params=None):
        """NewHPCPWithParams(sample_rate, params).ComputeFromSpectrum(row, window_size) on every row of mag
        (F x K) (sonar_hpcp_from_spectrum; params: hpcp_params(...), default NewHPCP's) -> dict of hpcp
        (F x size), energy, entropy (F)."""
        p = params if params is not None else hpcp_params()
        mag = _f64(mag)
        mag = mag[None, :] if mag.ndim == 1 else mag
        F, K = mag.shape
        out, e, h = np.zeros((F, max(p.size, 0))), np.zeros(F), np.zeros(F)
        self._check(self._L.sonar_hpcp_from_spectrum(self._h, _ptr(mag) if mag.size else None, F, K, int(window_size),
                                                     int(sample_rate), C.byref(p), _ptr(out), _ptr(e), _ptr(h), 0))
        return {"hpcp": out, "energy": e, "entropy": h}

    def hpcp_from_spectrum_device(self, mag_ptr, F, K, window_size, sample_rate, hpcp_ptr, params=None,
                                  energy_ptr=None, entropy_ptr=None):
        """hpcp_from_spectrum on device memory (device_ptrs = 1): mag (F x K), hpcp (F x size) and the
        optional energy and entropy (F) are device addresses; the profile can go to
        chroma_similarity_device as it is."""
        p = params if params is not None else hpcp_params()
        self._check(self._L.sonar_hpcp_from_spectrum(self._h, mag_ptr, int(F), int(K), int(window_size),
                                                     int(sample_rate), C.byref(p), hpcp_ptr, energy_ptr, entropy_ptr, 1))

    def hpcp(self, pcm, sample_rate, window_size=2048, hop_size=512, window_type="hann", params=None):
        """SpectralAnalyzer.ComputeSTFTWithWindow(pcm, window_size, hop_size, window_type) magnitudes ->
        HPCP.ComputeFromSpectrum per frame (sonar_hpcp: float64 PCM, the float64 transform, the rows in
        a bounded device scratch, hpcp_plan's chunks) -> dict of hpcp (frames x size), energy, entropy."""
        p = params if params is not None else hpcp_params()
        pcm = _f64(pcm)
        n = len(pcm)
        wt = WINDOWS[window_type] if isinstance(window_type, str) else int(window_type)
        v = [C.c_int64() for _ in range(3)]
        F = 0
        if self._L.sonar_hpcp_plan(n, int(window_size), int(hop_size), *[C.byref(x) for x in v]) == OK:
            F = v[0].value                                  # otherwise the call below reports the error
        out, e, h = np.zeros((F, max(p.size, 0))), np.zeros(F), np.zeros(F)
        self._check(self._L.sonar_hpcp(self._h, _ptr(pcm) if n else None, n, int(sample_rate), int(window_size),
                                       int(hop_size), wt, C.byref(p), _ptr(out), _ptr(e), _ptr(h), 0))
        return {"hpcp": out, "energy": e, "entropy": h}

    def hpcp_device(self, pcm_ptr, n, sample_rate, hpcp_ptr, window_size=2048, hop_size=512, window_type="hann",
                    params=None, energy_ptr=None, entropy_ptr=None):
        """hpcp on device memory (device_ptrs = 1): pcm (n doubles), hpcp (frames x size) and the optional
        energy and entropy are device addresses; frames is hpcp_plan's."""
        p = params if params is not None else hpcp_params()
        wt = WINDOWS[window_type] if isinstance(window_type, str) else int(window_type)
        self._check(self._L.sonar_hpcp(self._h, pcm_ptr, int(n), int(sample_rate), int(window_size), int(hop_size), wt,
                                       C.byref(p), hpcp_ptr, energy_ptr, entropy_ptr, 1))

    def hps_from_spectrum(self, mag, window_size, sample_rate, num_harmonics=10, min_f0=80.0, max_f0=2000.0,
                          interpolated=False, skip=("hps",)):
        """NewHarmonicProduct(sample_rate, num_harmonics, min_f0, max_f0) on every row of mag (F x K) with
        signalLength window_size (sonar_hps_from_spectrum; the defaults are MusicFeatureExtractor's):
        ComputeHPS (ComputeHPSWithInterpolation when interpolated), findF0Peak, the harmonic strengths
        and the harmonicity -> dict of f0_bin (F, int32), f0, confidence (F), strengths (F x
        num_harmonics) and hps (F x K); a name of confidence, strengths, hps in skip is passed as NULL
        and comes back None."""
        mag = _f64(mag)
        mag = mag[None, :] if mag.ndim == 1 else mag
        F, K = mag.shape
        shapes = {"confidence": (F,), "strengths": (F, max(int(num_harmonics), 0)), "hps": (F, K)}
        o = {"f0_bin": np.zeros(F, np.int32), "f0": np.zeros(F)}
        o.update({k: None if k in skip else np.zeros(shapes[k]) for k in _HPS_OPTIONAL})
        self._check(self._L.sonar_hps_from_spectrum(self._h, _ptr(mag) if mag.size else None, F, K, int(window_size),
                                                    int(sample_rate), int(num_harmonics), float(min_f0), float(max_f0),
                                                    int(bool(interpolated)), _ptr(o["f0_bin"]) if F else None,
                                                    _ptr(o["f0"]) if F else None, *[_ptr(o[k]) for k in _HPS_OPTIONAL], 0))
        return o

    def hps_from_spectrum_device(self, mag_ptr, F, K, window_size, sample_rate, f0_bin_ptr, f0_ptr, num_harmonics=10,
                                 min_f0=80.0, max_f0=2000.0, interpolated=False, confidence_ptr=None,
                                 strengths_ptr=None, hps_ptr=None):
        """hps_from_spectrum on device memory (device_ptrs = 1): mag (F x K), f0_bin (F int32), f0 (F) and
        the optional confidence (F), strengths (F x num_harmonics) and hps (F x K) are device addresses."""
        self._check(self._L.sonar_hps_from_spectrum(self._h, mag_ptr, int(F), int(K), int(window_size), int(sample_rate),
                                                    int(num_harmonics), float(min_f0), float(max_f0),
                                                    int(bool(interpolated)), f0_bin_ptr, f0_ptr, confidence_ptr,
                                                    strengths_ptr, hps_ptr, 1))

    def hps(self, pcm, sample_rate, window_size=2048, hop_size=512, num_harmonics=10, min_f0=80.0, max_f0=2000.0,
            interpolated=False, skip=("magnitude",)):
        """HarmonicProduct.EstimateF0WithConfidence on every frame of window_size samples at hop_size
        (sonar_hps: applyWindow's unnormalised symmetric Hann, the float64 transform, the rows in a
        bounded device scratch, hps_plan's chunks) -> dict of f0_bin, f0, confidence (frames), strengths
        (frames x num_harmonics) and magnitude (frames x K, the rows the estimates were made on); a
        name of confidence, strengths, magnitude in skip is passed as NULL and comes back None."""
        pcm = _f64(pcm)
        n = len(pcm)
        v = [C.c_int64() for _ in range(3)]
        F = 0
        if self._L.sonar_hps_plan(n, int(window_size), int(hop_size), *[C.byref(x) for x in v]) == OK:
            F = v[0].value                                  # otherwise the call below reports the error
        shapes = {"confidence": (F,), "strengths": (F, max(int(num_harmonics), 0)),
                  "magnitude": (F, int(window_size) // 2 + 1)}
        o = {"f0_bin": np.zeros(F, np.int32), "f0": np.zeros(F)}
        o.update({k: None if k in skip else np.zeros(shapes[k]) for k in shapes})
        frames = C.c_int64()
        self._check(self._L.sonar_hps(self._h, _ptr(pcm) if n else None, n, int(sample_rate), int(window_size),
                                      int(hop_size), int(num_harmonics), float(min_f0), float(max_f0),
                                      int(bool(interpolated)), _ptr(o["f0_bin"]), _ptr(o["f0"]),
                                      *[_ptr(o[k]) for k in shapes], C.byref(frames), 0))
        assert frames.value == F
        return o

    def hps_device(self, pcm_ptr, n, sample_rate, f0_bin_ptr, f0_ptr, window_size=2048, hop_size=512, num_harmonics=10,
                   min_f0=80.0, max_f0=2000.0, interpolated=False, confidence_ptr=None, strengths_ptr=None,
                   magnitude_ptr=None):
        """hps on device memory (device_ptrs = 1): pcm (n doubles), f0_bin, f0 and the optional confidence,
        strengths and magnitude are device addresses sized by hps_plan's frames, which is returned."""
        frames = C.c_int64()
        self._check(self._L.sonar_hps(self._h, pcm_ptr, int(n), int(sample_rate), int(window_size), int(hop_size),
                                      int(num_harmonics), float(min_f0), float(max_f0), int(bool(interpolated)),
                                      f0_bin_ptr, f0_ptr, confidence_ptr, strengths_ptr, magnitude_ptr,
                                      C.byref(frames), 1))
        return frames.value

    def spectral_flux(self, mag, all_changes=False):
        """SpectralFlux.Compute (ComputeAllChanges when all_changes) over the rows of mag (F x K)
        (sonar_spectral_flux) -> max(F - 1, 0) values."""
        mag = _f64(mag)
        F, K = mag.shape
        flux = np.zeros(max(F - 1, 0))
        self._check(self._L.sonar_spectral_flux(self._h, _ptr(mag) if mag.size else None, F, K, int(bool(all_changes)),
                                                _ptr(flux) if flux.size else None, 0))
        return flux

    def spectral_flux_device(self, mag_ptr, F, K, flux_ptr, all_changes=False):
        """spectral_flux on device memory (device_ptrs = 1): mag (F x K) and flux (F - 1) are device addresses."""
        self._check(self._L.sonar_spectral_flux(self._h, mag_ptr, int(F), int(K), int(bool(all_changes)), flux_ptr, 1))

    def rms_envelope(self, pcm, frame_size, hop_size):
        """Envelope.ComputeRMS (sonar_rms_envelope) -> the envelope, empty where the reference's is."""
        pcm = _f64(pcm)
        env = np.zeros(rms_envelope_frames(len(pcm), frame_size, hop_size))
        frames = C.c_int64()
        self._check(self._L.sonar_rms_envelope(self._h, _ptr(pcm) if pcm.size else None, len(pcm), int(frame_size),
                                               int(hop_size), _ptr(env) if env.size else None, C.byref(frames), 0))
        assert frames.value == len(env)
        return env

    def rms_envelope_device(self, pcm_ptr, n, frame_size, hop_size, env_ptr):
        """rms_envelope on device memory (device_ptrs = 1) -> the number of values written."""
        frames = C.c_int64()
        self._check(self._L.sonar_rms_envelope(self._h, pcm_ptr, int(n), int(frame_size), int(hop_size), env_ptr,
                                               C.byref(frames), 1))
        return frames.value

    def onset_peaks(self, curve, threshold, min_interval, hop_size, sample_rate, padded=False):
        """findFluxPeaks on any curve (sonar_onset_peaks) -> the kept indices (int64), or with padded the
        whole onset_peaks_width(n) slots and the count."""
        curve = _f64(curve)
        n = len(curve)
        index = np.full(onset_peaks_width(n), -1, np.int64)
        count = C.c_int64(-1)
        self._check(self._L.sonar_onset_peaks(self._h, _ptr(curve) if n else None, n, float(threshold),
                                              float(min_interval), int(hop_size), int(sample_rate),
                                              _ptr(index) if index.size else None, C.byref(count), 0))
        return (index, count.value) if padded else index[:count.value]

    def onset_peaks_device(self, curve_ptr, n, threshold, min_interval, hop_size, sample_rate, index_ptr):
        """onset_peaks on device memory (device_ptrs = 1): curve (n) and index (onset_peaks_width(n) int64)
        are device addresses -> the count."""
        count = C.c_int64(-1)
        self._check(self._L.sonar_onset_peaks(self._h, curve_ptr, int(n), float(threshold), float(min_interval),
                                              int(hop_size), int(sample_rate), index_ptr, C.byref(count), 1))
        return count.value

    def onset_adaptive_threshold(self, curve):
        """OnsetDetection.AdaptiveThreshold (sonar_onset_adaptive_threshold)."""
        curve = _f64(curve)
        v = np.full(1, -1.0)
        self._check(self._L.sonar_onset_adaptive_threshold(self._h, _ptr(curve) if curve.size else None, len(curve),
                                                           _ptr(v), 0))
        return float(v[0])

    def onset_adaptive_threshold_device(self, curve_ptr, n, value_ptr):
        """onset_adaptive_threshold on device memory (device_ptrs = 1): curve (n) and value (a double)."""
        self._check(self._L.sonar_onset_adaptive_threshold(self._h, curve_ptr, int(n), value_ptr, 1))

    def onsets_flux(self, pcm, sample_rate, threshold, min_interval, window_size=0, hop_size=0, skip=("magnitude",)):
        """OnsetDetection.DetectOnsets (sonar_onsets_flux; window_size / hop_size 0 are the reference's 1024 /
        512) -> dict of onsets (samples, int64), flux (frames - 1), magnitude (frames x K, the unwindowed
        STFT rows the flux was taken on) and frames; a name of flux, magnitude in skip is passed as NULL
        and comes back None."""
        pcm = _f64(pcm)
        n = len(pcm)
        W, H = int(window_size) or ONSET_WINDOW, int(hop_size) or ONSET_HOP
        F = max(stft_frames(n, W, H), 0) if n > 0 and W > 0 and H > 0 else 0   # Go's truncating count
        onsets = np.full(onset_peaks_width(F - 1), -1, np.int64)
        o = {"flux": None if "flux" in skip else np.zeros(max(F - 1, 0)),
             "magnitude": None if "magnitude" in skip else np.zeros((F, W // 2 + 1))}
        count, frames = C.c_int64(), C.c_int64()
        self._check(self._L.sonar_onsets_flux(self._h, _ptr(pcm) if n else None, n, int(sample_rate), int(window_size),
                                              int(hop_size), float(threshold), float(min_interval),
                                              _ptr(onsets) if onsets.size else None, C.byref(count),
                                              _ptr(o["flux"]) if F > 1 else None, _ptr(o["magnitude"]) if F else None,
                                              C.byref(frames), 0))
        assert frames.value == F and not onsets[count.value:].any()
        o.update(onsets=onsets[:count.value], frames=F)
        return o

    def onsets_flux_device(self, pcm_ptr, n, sample_rate, threshold, min_interval, onsets_ptr, window_size=0,
                           hop_size=0, flux_ptr=None, magnitude_ptr=None):
        """onsets_flux on device memory (device_ptrs = 1) -> (count, frames)."""
        count, frames = C.c_int64(), C.c_int64()
        self._check(self._L.sonar_onsets_flux(self._h, pcm_ptr, int(n), int(sample_rate), int(window_size),
                                              int(hop_size), float(threshold), float(min_interval), onsets_ptr,
                                              C.byref(count), flux_ptr, magnitude_ptr, C.byref(frames), 1))
        return count.value, frames.value

    def onsets_energy(self, pcm, sample_rate, threshold, min_interval, frame_size=0, hop_size=0):
        """OnsetDetection.DetectOnsetsEnergy (sonar_onsets_energy; frame_size / hop_size 0 are the
        reference's 512 / 256) -> dict of onsets (samples, int64) and curve (the energyDiff)."""
        pcm = _f64(pcm)
        n = len(pcm)
        fs, hs = int(frame_size) or ONSET_ENERGY_FRAME, int(hop_size) or ONSET_ENERGY_HOP
        nc = max(rms_envelope_frames(n, fs, hs) - 1, 0)
        onsets, curve = np.full(onset_peaks_width(nc), -1, np.int64), np.zeros(nc)
        count, ncurve = C.c_int64(), C.c_int64()
        self._check(self._L.sonar_onsets_energy(self._h, _ptr(pcm) if n else None, n, int(sample_rate), int(frame_size),
                                                int(hop_size), float(threshold), float(min_interval),
                                                _ptr(onsets) if onsets.size else None, C.byref(count),
                                                _ptr(curve) if nc else None, C.byref(ncurve), 0))
        assert ncurve.value == nc and not onsets[count.value:].any()
        return {"onsets": onsets[:count.value], "curve": curve}

    def onsets_energy_device(self, pcm_ptr, n, sample_rate, threshold, min_interval, onsets_ptr, frame_size=0,
                             hop_size=0, curve_ptr=None):
        """onsets_energy on device memory (device_ptrs = 1) -> (count, the curve's length)."""
        count, ncurve = C.c_int64(), C.c_int64()
        self._check(self._L.sonar_onsets_energy(self._h, pcm_ptr, int(n), int(sample_rate), int(frame_size),
                                                int(hop_size), float(threshold), float(min_interval), onsets_ptr,
                                                C.byref(count), curve_ptr, C.byref(ncurve), 1))
        return count.value, ncurve.value

    def onsets_complex(self, pcm, sample_rate):
        """OnsetDetection.DetectOnsetsComplex and ComputeOnsetDensity (sonar_onsets_complex) -> dict of
        onsets (samples, int64) and density (onsets per second)."""
        pcm = _f64(pcm)
        n = len(pcm)
        onsets = np.full(onsets_complex_width(n), -1, np.int64)
        count, density = C.c_int64(), C.c_double()
        self._check(self._L.sonar_onsets_complex(self._h, _ptr(pcm) if n else None, n, int(sample_rate),
                                                 _ptr(onsets) if onsets.size else None, C.byref(count),
                                                 C.byref(density), 0))
        assert not onsets[count.value:].any()
        return {"onsets": onsets[:count.value], "density": density.value}

    def onsets_complex_device(self, pcm_ptr, n, sample_rate, onsets_ptr):
        """onsets_complex on device memory (device_ptrs = 1): onsets has onsets_complex_width(n) int64 slots
        -> (count, density)."""
        count, density = C.c_int64(), C.c_double()
        self._check(self._L.sonar_onsets_complex(self._h, pcm_ptr, int(n), int(sample_rate), onsets_ptr, C.byref(count),
                                                 C.byref(density), 1))
        return count.value, density.value

    def tempo_autocorrelation(self, pcm, sample_rate, full=False):
        """TempoEstimation.EstimateTempoAutocorrelation (sonar_tempo_autocorrelation) -> dict of tempo,
        best_lag and autocorr: None, or with full the whole curve (tempo_autocorr_plan's n_autocorr
        values) where the narrow form computes only the lags the peak search reads."""
        pcm = _f64(pcm)
        n = len(pcm)
        nac = tempo_autocorr_plan(n, sample_rate)["n_autocorr"]
        ac = np.zeros(nac) if full else None
        tempo, lag, got = np.full(1, -1.0), np.full(1, -1, np.int64), C.c_int64()
        self._check(self._L.sonar_tempo_autocorrelation(self._h, _ptr(pcm) if n else None, n, int(sample_rate),
                                                        _ptr(tempo), _ptr(lag), _ptr(ac) if full and nac else None,
                                                        C.byref(got), 0))
        assert got.value == nac
        return {"tempo": float(tempo[0]), "best_lag": int(lag[0]), "autocorr": ac}

    def tempo_autocorrelation_device(self, pcm_ptr, n, sample_rate, tempo_ptr, best_lag_ptr=None, autocorr_ptr=None):
        """tempo_autocorrelation on device memory (device_ptrs = 1): tempo (a double), best_lag (an int64)
        and autocorr are device addresses -> n_autocorr."""
        got = C.c_int64()
        self._check(self._L.sonar_tempo_autocorrelation(self._h, pcm_ptr, int(n), int(sample_rate), tempo_ptr,
                                                        best_lag_ptr, autocorr_ptr, C.byref(got), 1))
        return got.value

    def tempo(self, pcm, sample_rate, device_n=None):
        """TempoEstimation.EstimateTempo, EstimateTempoAutocorrelation, EstimateTempoRange and
        ClassifyTempoCategory (sonar_tempo) -> dict of the fields of sonar_tempo_result plus
        category_name.  With device_n, pcm is a device address of that many doubles."""
        r = TempoResult()
        if device_n is None:
            pcm = _f64(pcm)
            self._check(self._L.sonar_tempo(self._h, _ptr(pcm) if pcm.size else None, len(pcm), int(sample_rate),
                                            C.byref(r), 0))
        else:
            self._check(self._L.sonar_tempo(self._h, pcm, int(device_n), int(sample_rate), C.byref(r), 1))
        out = {n: getattr(r, n) for n, _ in r._fields_}
        out["category_name"] = tempo_category_name(r.category)
        return out

    def key_frames(self, chroma, params=None, skip=()):
        """KeyEstimator.EstimateKey on every row of chroma (F x dim) (sonar_key_frames; params:
        key_params(...), default NewKeyEstimator's) -> dict of key, mode, known, confidence, strength,
        clarity, ambiguity, tonality (F), scores (F x 24), candidates (F x min(max_candidates, 24) codes
        key * 2 + mode) and processed (F x hpcp_size); a name in skip is passed as NULL and comes back None."""
        p = params if params is not None else key_params()
        chroma = _key_rows(chroma)
        F, dim = chroma.shape
        o = _key_frame_arrays(F, p, skip)
        self._check(self._L.sonar_key_frames(self._h, _ptr(chroma) if chroma.size else None, F, dim, C.byref(p),
                                             *[_ptr(o[n]) for n in KEY_FRAME_FIELDS], 0))
        return o

    def key_frames_device(self, chroma_ptr, F, dim, params=None, **ptrs):
        """key_frames on device memory (device_ptrs = 1): chroma (F x dim) and every output given by
        keyword (the names of KEY_FRAME_FIELDS) are device addresses."""
        p = params if params is not None else key_params()
        self._check(self._L.sonar_key_frames(self._h, chroma_ptr, int(F), int(dim), C.byref(p),
                                             *[ptrs.get(n) for n in KEY_FRAME_FIELDS], 1))

    _KEY_SEQ_FIELDS = KEY_FRAME_FIELDS[:9] + ("processed", "stability", "modulations", "n_modulations")

    def key_sequence(self, chroma, params=None, skip=()):
        """KeyEstimator.EstimateKeySequence of chroma (F x dim) (sonar_key_sequence) -> dict of the average
        row's key, mode, known, confidence, strength, clarity, ambiguity, tonality, scores (24), processed
        (hpcp_size), and stability and modulations (the positions); a name in skip is passed as NULL."""
        p = params if params is not None else key_params()
        chroma = _key_rows(chroma)
        F, dim = chroma.shape
        o = _key_frame_arrays(1, p, skip)
        del o["candidates"]
        o["stability"] = None if "stability" in skip else np.zeros(1)
        o["modulations"] = None if "modulations" in skip else np.zeros(max(F - 20, 0), np.int32)
        o["n_modulations"] = None if "n_modulations" in skip else np.zeros(1, np.int64)
        self._check(self._L.sonar_key_sequence(self._h, _ptr(chroma) if chroma.size else None, F, dim, C.byref(p),
                                               *[_ptr(o[n]) for n in self._KEY_SEQ_FIELDS], 0))
        r = {n: (None if v is None else v.reshape(v.shape[1:]) if n in ("scores", "processed") else
                 v if n == "modulations" else v[0]) for n, v in o.items()}
        if r["modulations"] is not None and r["n_modulations"] is not None:
            r["modulations"] = r["modulations"][:int(r["n_modulations"])]
        return r

    def key_sequence_device(self, chroma_ptr, F, dim, params=None, **ptrs):
        """key_sequence on device memory (device_ptrs = 1): chroma and every output given by keyword (key,
        ..., scores, processed, stability, modulations, n_modulations; the single values too) are device
        addresses; modulations holds max(F - 20, 0) int32, n_modulations one int64."""
        p = params if params is not None else key_params()
        self._check(self._L.sonar_key_sequence(self._h, chroma_ptr, int(F), int(dim), C.byref(p),
                                               *[ptrs.get(n) for n in self._KEY_SEQ_FIELDS], 1))

    _KEY_BATCH_FIELDS = KEY_FRAME_FIELDS + ("global_code", "global_confidence", "global_strength", "votes", "t_frame",
                                            "t_from", "t_to", "t_confidence", "t_type", "n_transitions")

    def key_batch(self, chroma, params=None, skip=()):
        """KeyEstimationBatch on chroma (F x dim) (sonar_key_batch): ProcessBatch's per-frame outputs as
        key_frames', GetGlobalKey's global_code (-1: no vote), global_confidence, global_strength and
        votes (24, by code), and GetKeyProgression's records t_frame, t_from, t_to (codes), t_confidence,
        t_type (an index of KEY_TRANSITIONS), cut to n_transitions; a name in skip is passed as NULL."""
        p = params if params is not None else key_params()
        chroma = _key_rows(chroma)
        F, dim = chroma.shape
        o = _key_frame_arrays(F, p, skip)
        cap = max(F - 1, 0)
        extra = {"global_code": ((1,), np.int32), "global_confidence": ((1,), np.float64),
                 "global_strength": ((1,), np.float64), "votes": ((24,), np.float64), "t_frame": ((cap,), np.int32),
                 "t_from": ((cap,), np.int32), "t_to": ((cap,), np.int32), "t_confidence": ((cap,), np.float64),
                 "t_type": ((cap,), np.int32), "n_transitions": ((1,), np.int64)}
        for n, (shape, dt) in extra.items():
            o[n] = None if n in skip else np.zeros(shape, dt)
        self._check(self._L.sonar_key_batch(self._h, _ptr(chroma) if chroma.size else None, F, dim, C.byref(p),
                                            *[_ptr(o[n]) for n in self._KEY_BATCH_FIELDS], 0))
        for n in ("global_code", "global_confidence", "global_strength", "n_transitions"):
            if o[n] is not None:
                o[n] = o[n][0]
        if o["n_transitions"] is not None:
            for n in ("t_frame", "t_from", "t_to", "t_confidence", "t_type"):
                if o[n] is not None:
                    o[n] = o[n][:int(o["n_transitions"])]
        return o

    def key_batch_device(self, chroma_ptr, F, dim, params=None, **ptrs):
        """key_batch on device memory (device_ptrs = 1): chroma and every output given by keyword (the names
        key_batch returns) are device addresses; the t_ arrays hold max(F - 1, 0) entries."""
        p = params if params is not None else key_params()
        self._check(self._L.sonar_key_batch(self._h, chroma_ptr, int(F), int(dim), C.byref(p),
                                            *[ptrs.get(n) for n in self._KEY_BATCH_FIELDS], 1))

    def _chord_rows(self, fn, chroma, params, bass_note, bass_confidence, skip):
        p = params if params is not None else chord_params()
        chroma = _key_rows(chroma)
        F, dim = chroma.shape
        bn, bc = _chord_bass(bass_note, bass_confidence)
        o, out = _chord_arrays(F, p, skip)
        self._check(fn(self._h, _ptr(chroma) if chroma.size else None, F, dim, _ptr(bn), _ptr(bc), C.byref(p),
                       C.byref(out), 0))
        return o

    def chord_frames(self, chroma, params=None, bass_note=None, bass_confidence=None, skip=()):
        """ChordDetector.DetectChord from templateMatching on, every row of chroma (F x dim) through a fresh
        detector (sonar_chord_frames; params: chord_params(...), default NewChordDetector's; bass_note /
        bass_confidence: what detectBassNote returned per row, default 0 and 0.0) -> dict of the names of
        CHORD_FIELDS: F entries each, template_scores F x 120, the candidate arrays F x max_candidates
        (slots t * 12 + root, -1 beyond the kept ones); a name in skip is passed as NULL and comes back None."""
        return self._chord_rows(self._L.sonar_chord_frames, chroma, params, bass_note, bass_confidence, skip)

    def chord_sequence(self, chroma, params=None, bass_note=None, bass_confidence=None, skip=()):
        """chord_frames with one detector fed the rows in order (sonar_chord_sequence): the temporal
        smoothing and the stability history apply."""
        return self._chord_rows(self._L.sonar_chord_sequence, chroma, params, bass_note, bass_confidence, skip)

    def chord_rows_device(self, chroma_ptr, F, dim, params=None, sequence=True, bass_note_ptr=None,
                          bass_confidence_ptr=None, **ptrs):
        """chord_sequence (or chord_frames with sequence=False) on device memory (device_ptrs = 1): chroma,
        the bass arrays and every output given by keyword (the names of CHORD_FIELDS) are device addresses."""
        p = params if params is not None else chord_params()
        out = ChordOut(*[ptrs.get(n) for n in CHORD_FIELDS])
        fn = self._L.sonar_chord_sequence if sequence else self._L.sonar_chord_frames
        self._check(fn(self._h, chroma_ptr, int(F), int(dim), bass_note_ptr, bass_confidence_ptr, C.byref(p),
                       C.byref(out), 1))

    def chord_detect(self, pcm, sample_rate, frame_len, hop, params=None, bass_note=None, bass_confidence=None,
                     skip=()):
        """ChordDetector.DetectChord on every frame of frame_len samples at hop, one detector in order
        (sonar_chord_detect) -> chord_sequence's dict plus hpcp (frames x 12), the profiles the detector saw."""
        p = params if params is not None else chord_params()
        pcm = _f64(pcm)
        n = len(pcm)
        F = (n - frame_len) // hop + 1 if frame_len > 0 and hop > 0 and n >= frame_len else 0
        bn, bc = _chord_bass(bass_note, bass_confidence)
        o, out = _chord_arrays(F, p, skip)
        o["hpcp"] = None if "hpcp" in skip else np.zeros((F, 12))
        frames = C.c_int64()
        self._check(self._L.sonar_chord_detect(self._h, _ptr(pcm) if n else None, n, int(sample_rate), int(frame_len),
                                               int(hop), _ptr(bn), _ptr(bc), C.byref(p), C.byref(out),
                                               _ptr(o["hpcp"]) if F else None, C.byref(frames), 0))
        assert frames.value == F
        return o

    def chord_progression(self, quality, confidence, root=None, inversion=None):
        """ChordProgressionAnalyzer.AnalyzeProgression over per-frame results (sonar_chord_progression) ->
        dict of num_chords and insufficient_data, and with two chords or more average_confidence,
        most_common_quality (the code) and most_common_quality_name."""
        q = np.ascontiguousarray(quality, dtype=np.int32)
        cf = _f64(confidence)
        r = None if root is None else np.ascontiguousarray(root, dtype=np.int32)
        iv = None if inversion is None else np.ascontiguousarray(inversion, dtype=np.int32)
        num, ins, avg, most = C.c_int64(), C.c_int32(), C.c_double(), C.c_int32()
        self._check(self._L.sonar_chord_progression(self._h, _ptr(r), _ptr(q) if q.size else None, _ptr(iv),
                                                    _ptr(cf) if cf.size else None, len(q), C.byref(num), C.byref(ins),
                                                    C.byref(avg), C.byref(most), 0))
        o = {"num_chords": num.value, "insufficient_data": ins.value}
        if not ins.value:
            o.update(average_confidence=avg.value, most_common_quality=most.value,
                     most_common_quality_name=chord_quality_name(most.value))
        return o

    def chord_progression_device(self, quality_ptr, confidence_ptr, F, num_chords_ptr=None,
                                 insufficient_data_ptr=None, average_confidence_ptr=None,
                                 most_common_quality_ptr=None):
        """chord_progression on device memory (device_ptrs = 1): every array and single value is a device address."""
        self._check(self._L.sonar_chord_progression(self._h, None, quality_ptr, None, confidence_ptr, int(F),
                                                    num_chords_ptr, insufficient_data_ptr, average_confidence_ptr,
                                                    most_common_quality_ptr, 1))

    def music_alignment_features(self, pcm, sample_rate, stft_window=1024, stft_hop=256, feature_window=1024,
                                 feature_hop=256):
        """MusicFeatureExtractor's ShortTimeEnergy + ChromaFeatures (host arrays) -> (energy, chroma)."""
        pcm = _f64(pcm)
        n = len(pcm)
        F = stft_frames(n, stft_window, stft_hop) if n > 0 else 0
        energy = np.zeros(max(energy_frames(n, feature_window, feature_hop), 0))
        chroma = np.zeros((max(F, 0), 12))
        self._check(self._L.sonar_music_alignment_features(
            self._h, _ptr(pcm) if n else None, n, sample_rate, stft_window, stft_hop, feature_window, feature_hop,
            _ptr(energy) if len(energy) else None, _ptr(chroma) if len(chroma) else None, 0))
        return energy, chroma

    def music_alignment_features_device(self, pcm_ptr, n, sample_rate, energy_ptr, chroma_ptr, stft_window=1024,
                                        stft_hop=256, feature_window=1024, feature_hop=256):
        """Device-pointer form (float64 buffers, async on the ctx stream)."""
        self._check(self._L.sonar_music_alignment_features(
            self._h, C.c_void_p(pcm_ptr), n, sample_rate, stft_window, stft_hop, feature_window, feature_hop,
            C.c_void_p(energy_ptr), C.c_void_p(chroma_ptr), 1))

    def align_pair_device(self, q_ptr, nq, r_ptr, nr, sample_rate=44100, stft_window=1024, hop=256,
                          feature_window=1024, max_lag_seconds=60.0):
        """sonar_align_pair_device: music features + ExtractAlignmentFeatures of one pair of
        device-resident float64 streams; returns the align_features result dict."""
        h = C.c_void_p()
        self._check(self._L.sonar_align_pair_device(self._h, C.c_void_p(q_ptr), nq, C.c_void_p(r_ptr), nr, sample_rate,
                                                    stft_window, hop, feature_window, max_lag_seconds, C.byref(h)))
        return self._result(h)

    def align_pairs(self, qs, rs, nq=None, nr=None, sample_rate=44100, stft_window=1024, hop=256,
                    feature_window=1024, max_lag_seconds=20.0, workers=128, device_ptrs=False):
        """sonar_align_pairs: records of many pairs (workers = pairs in flight).  qs / rs: lists of host arrays, or of device
        pointers (ints) with device_ptrs=True and the lengths in nq / nr."""
        n = len(qs)
        qp, rp, keep = _pair_arrays(qs, rs)
        nqa = (C.c_int64 * n)(*(nq if nq is not None else [len(x) for x in qs]))
        nra = (C.c_int64 * n)(*(nr if nr is not None else [len(x) for x in rs]))
        recs = (PairRecord * max(n, 1))()
        self._check(self._L.sonar_align_pairs(self._h, n, qp, nqa, rp, nra, sample_rate, stft_window, hop,
                                              feature_window, max_lag_seconds, workers, int(bool(device_ptrs)),
                                              recs))
        del keep
        return records_dict(recs[:n])

    # -- path B ------------------------------------------------------------
    def ncc(self, a, b, max_lag):
        a, b = _f64(a), _f64(b)
        L = max(0, min(max_lag, len(a) - 1, len(b) - 1)) if len(a) and len(b) else 0
        corr = np.zeros(2 * L + 1)
        met = np.zeros(10)
        self._check(self._L.sonar_ncc(self._h, _ptr(a) if len(a) else None, len(a), _ptr(b) if len(b) else None,
                                      len(b), max_lag, _ptr(corr), _ptr(met), 0))
        return corr, dict(zip(NCC_KEYS, met.tolist()))

    def formants(self, pcm, sample_rate, frame_size=0, hop_size=0, want_lpc=False):
        """FormantAnalyzer.AnalyzeMultipleFrames; every attempted frame, `status` != 0 where Go skips."""
        pcm = _f64(pcm)
        L = lib()
        F = int(L.sonar_formant_frame_count(len(pcm), sample_rate, frame_size, hop_size))
        recs = (FormantFrame * max(F, 1))()
        p = 12 + sample_rate // 1000
        co = np.zeros((F, p + 1)) if want_lpc else None
        rf = np.zeros((F, p)) if want_lpc else None
        self._check(L.sonar_formants(self._h, _ptr(pcm), len(pcm), sample_rate, frame_size, hop_size, recs,
                                     _ptr(co) if want_lpc else None, _ptr(rf) if want_lpc else None, 0))
        out = _formant_dict(recs, F)
        if want_lpc:
            out["lpc_coeffs"], out["reflection"] = co, rf
        return out

    def alignment_consistency(self, query, reference, sample_rate, method=ALIGN_XCORR, max_lag=100, hop=256,
                              num_trials=5):
        """AlignmentAnalyzer.AnalyzeAlignmentConsistency -> dict of AlignmentStats (+ offset, trials)."""
        q, r = _f64(query), _f64(reference)
        if q.ndim == 1:
            q = q[:, None]
        if r.ndim == 1:
            r = r[:, None]
        st = AlignmentStats()
        self._check(self._L.sonar_alignment_consistency(
            self._h, _ptr(q) if q.size else None, len(q), _ptr(r) if r.size else None, len(r),
            q.shape[1] if q.size else 1, method, max_lag, hop, sample_rate, num_trials, C.byref(st)))
        return {k: getattr(st, k) for k, _ in AlignmentStats._fields_}

    def analyzer_align_features(self, query, reference, sample_rate, method=ALIGN_HYBRID, max_lag=100, hop=256):
        """AlignmentAnalyzer.AlignFeatures (stats/alignment.go:84-106) for DTW / CrossCorrelation /
        Hybrid -> the AlignmentResult fields (+ "correlations", NCC metrics, "dtw_path_*")."""
        q, r = _f64(query), _f64(reference)
        if q.ndim == 1:
            q = q[:, None]
        if r.ndim == 1:
            r = r[:, None]
        h = C.c_void_p()
        self._check(self._L.sonar_analyzer_align_features(
            self._h, _ptr(q) if q.size else None, len(q) if q.size else 0, _ptr(r) if r.size else None,
            len(r) if r.size else 0, q.shape[1] if q.size else 1, method, max_lag, hop, sample_rate, 0, C.byref(h)))
        return self._result(h)

    def align_audio(self, q_pcm, r_pcm, sample_rate, method=ALIGN_HYBRID, max_lag=100, hop=256, window=1024,
                    device_ptrs=False):
        """AlignmentAnalyzer.AlignAudio (stats/alignment.go:108-126): RMS energy frames of both signals
        (extractEnergyFeatures :341-361), then AlignFeatures.  q_pcm / r_pcm: float64 arrays, or device
        pointers (ints) with lengths as (ptr, n) tuples when device_ptrs."""
        (qp, nq, qa), (rp, nr, ra) = _pcm_arg(q_pcm, device_ptrs), _pcm_arg(r_pcm, device_ptrs)
        h = C.c_void_p()
        self._check(self._L.sonar_align_audio(self._h, qp, nq, rp, nr, method, max_lag, hop, window, sample_rate,
                                              int(device_ptrs), C.byref(h)))
        del qa, ra
        return self._result(h)

    def align_audio_files(self, q_pcm, r_pcm, sample_rate, feature_sample_rate=None, hop=256, window=1024,
                          max_lag_seconds=60.0, device_ptrs=False):
        """AlignmentExtractor.AlignAudioFiles (extractors/alignment.go:489-553): ShortTimeEnergy of
        both PCM streams, then the extractor's Hybrid AlignFeatures."""
        (qp, nq, qa), (rp, nr, ra) = _pcm_arg(q_pcm, device_ptrs), _pcm_arg(r_pcm, device_ptrs)
        fsr = sample_rate if feature_sample_rate is None else feature_sample_rate
        h = C.c_void_p()
        self._check(self._L.sonar_align_audio_files(self._h, qp, nq, rp, nr, sample_rate, fsr, hop, window,
                                                    float(max_lag_seconds), int(device_ptrs), C.byref(h)))
        del qa, ra
        return self._result(h)

    def truncate_to_alignment(self, n1, n2, sample_rate, temporal_offset):
        """AlignmentExtractor.TruncateToAlignmentPCM -> (start1, start2, length)."""
        a, b, n = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self._L.sonar_truncate_to_alignment(self._h, n1, n2, sample_rate, temporal_offset, C.byref(a),
                                                        C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    def ingest_f64le(self, data, d_out=None, out_dtype=F32, mode=INGEST_DEVICE_CONVERT, host_threads=0):
        """Decoder.bytesToFloat64 (decoder.go:850-871) into device memory: `data` is the ffmpeg f64le
        byte stream (bytes / bytearray / uint8 or float64 array), `d_out` a device pointer of
        n * (4 if out_dtype == F32 else 8) bytes (None: only count).  Returns the sample count."""
        buf = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) \
            else np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        n = C.c_int64()
        self._check(self._L.sonar_ingest_f64le(self._h, buf.ctypes.data if buf.size else None, buf.size, out_dtype,
                                               mode, host_threads, d_out, C.byref(n)))
        return n.value

    def voice_quality(self, signal, sample_rate):
        """VoiceQualityAnalyzer.AnalyzeVoiceQuality -> dict of VoiceQualityResult fields."""
        x = _f64(signal)
        q = VoiceQuality()
        self._check(self._L.sonar_voice_quality(self._h, _ptr(x) if len(x) else None, len(x), sample_rate,
                                                C.byref(q)))
        return {k: getattr(q, k) for k, _ in VoiceQuality._fields_}

    def xcorr_params(self, a, b, max_lag, corr_type="pearson", method="time", use_fft=None):
        """CrossCorrelation.Compute (sonar_xcorr_params) -> (correlations, lags, metrics dict).
        corr_type: "pearson" | "spearman" | "kendall" | "ncc" | "zncc"; method: "time" | "frequency"
        | "sliding"; or the SONAR_CORR_* values.  use_fft None is NewCrossCorrelationWithParams'
        rule (method == frequency); xcorr() is NewCrossCorrelation, autocorr() NewAutoCorrelation."""
        a, b = _f64(a), _f64(b)
        t, m = _corr_enum(corr_type, CORR_TYPES), _corr_enum(method, CORR_METHODS)
        if use_fft is None:
            use_fft = m == CORR_METHODS["frequency"]
        L = max(0, min(max_lag, len(a) - 1, len(b) - 1)) if len(a) and len(b) else 0
        corr, met = np.zeros(2 * L + 1), np.zeros(12)
        self._check(self._L.sonar_xcorr_params(self._h, _ptr(a) if len(a) else None, len(a),
                                               _ptr(b) if len(b) else None, len(b), max_lag, t, m, int(bool(use_fft)),
                                               _ptr(corr), _ptr(met), 0))
        return corr, np.arange(-L, L + 1), _xcorr_metrics(met)

    def xcorr(self, a, b, max_lag):
        """stats.NewCrossCorrelation(max_lag).Compute(a, b): Pearson in the time domain up to 1,000
        samples, the FFT method's un-normalised sums above."""
        return self.xcorr_params(a, b, max_lag, "pearson", "time", use_fft=True)

    def autocorr(self, x, max_lag, corr_type="pearson", method="time"):
        """NewAutoCorrelation(max_lag) [+ SetParameters(corr_type, method)].Compute(x)
        (sonar_autocorr) -> (correlations, lags, metrics dict)."""
        x = _f64(x)
        L = max(0, min(max_lag, len(x) - 1)) if len(x) else 0
        corr, met = np.zeros(2 * L + 1), np.zeros(12)
        self._check(self._L.sonar_autocorr(self._h, _ptr(x) if len(x) else None, len(x), max_lag,
                                           _corr_enum(corr_type, CORR_TYPES), _corr_enum(method, CORR_METHODS),
                                           _ptr(corr), _ptr(met), 0))
        return corr, np.arange(-L, L + 1), _xcorr_metrics(met)

    def xcorr_params_device(self, a_ptr, na, b_ptr, nb, max_lag, corr_type="pearson", method="time", use_fft=None,
                            corr_ptr=None):
        """xcorr_params on device memory (device_ptrs = 1): a, b and the optional correlation array
        (2L + 1 doubles; None: library scratch) are device addresses -> metrics dict."""
        t, m = _corr_enum(corr_type, CORR_TYPES), _corr_enum(method, CORR_METHODS)
        if use_fft is None:
            use_fft = m == CORR_METHODS["frequency"]
        met = np.zeros(12)
        self._check(self._L.sonar_xcorr_params(self._h, a_ptr, na, b_ptr, nb, max_lag, t, m, int(bool(use_fft)),
                                               corr_ptr, _ptr(met), 1))
        return _xcorr_metrics(met)

    def autocorr_device(self, x_ptr, n, max_lag, corr_type="pearson", method="time", corr_ptr=None):
        """autocorr on device memory (device_ptrs = 1) -> metrics dict."""
        met = np.zeros(12)
        self._check(self._L.sonar_autocorr(self._h, x_ptr, n, max_lag, _corr_enum(corr_type, CORR_TYPES),
                                           _corr_enum(method, CORR_METHODS), corr_ptr, _ptr(met), 1))
        return _xcorr_metrics(met)

    def dtw(self, q, r, band=-1, want_cost=False):
        q, r = _f64(q), _f64(r)
        if q.ndim == 1:
            q = q[:, None]
        if r.ndim == 1:
            r = r[:, None]
        nq, d = q.shape if q.size else (0, 1)
        nr = r.shape[0] if r.size else 0
        cap = nq + nr + 1
        pq, pr, pc = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap)
        plen, dist = C.c_int64(), C.c_double()
        cost = np.zeros((nq, nr + 1)) if want_cost else None
        self._check(self._L.sonar_dtw(self._h, _ptr(q) if nq else None, nq, _ptr(r) if nr else None, nr, d, band,
                                      C.byref(dist), _ptr(pq), _ptr(pr), _ptr(pc), C.byref(plen),
                                      _ptr(cost) if want_cost else None, 0))
        P = plen.value
        return {"distance": dist.value, "path_q": pq[:P], "path_r": pr[:P], "path_cost": pc[:P], "cost": cost}

    def dtw_params(self, q, r, band=-1, step="symmetric2", metric="euclidean", want_cost=False):
        """NewDTWAlignmentWithParams(band, step, metric).Align (sonar_dtw_params): the dict of dtw.
        step: "symmetric2" | "asymmetric" | "symmetric1"; metric: "euclidean" | "manhattan" |
        "cosine" | "pearson" | "mahalanobis" (= Euclidean, as in Go), or the SONAR_DTW_* values."""
        q, r = _f64(q), _f64(r)
        if q.ndim == 1:
            q = q[:, None]
        if r.ndim == 1:
            r = r[:, None]
        nq, d = q.shape if q.size else (0, 1)
        nr = r.shape[0] if r.size else 0
        cap = nq + nr + 1
        pq, pr, pc = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap)
        plen, dist = C.c_int64(), C.c_double()
        cost = np.zeros((nq, nr + 1)) if want_cost else None
        self._check(self._L.sonar_dtw_params(self._h, _ptr(q) if nq else None, nq, _ptr(r) if nr else None, nr, d,
                                             band, _dtw_step(step, not (nq and nr)), _dtw_metric(metric),
                                             C.byref(dist), _ptr(pq),
                                             _ptr(pr), _ptr(pc), C.byref(plen), _ptr(cost) if want_cost else None, 0))
        P = plen.value
        return {"distance": dist.value, "path_q": pq[:P], "path_r": pr[:P], "path_cost": pc[:P], "cost": cost}

    def dtw_params_device(self, q_ptr, nq, r_ptr, nr, dim, path_q_ptr, path_r_ptr, path_cost_ptr, band=-1,
                          step="symmetric2", metric="euclidean", cost_ptr=None):
        """dtw_params on device memory (device_ptrs = 1): q, r, the path arrays (capacity nq + nr)
        and the optional nq x (nr + 1) cost matrix are device addresses -> (distance, path length)."""
        plen, dist = C.c_int64(), C.c_double()
        self._check(self._L.sonar_dtw_params(self._h, q_ptr, nq, r_ptr, nr, dim, band,
                                             _dtw_step(step, not (nq > 0 and nr > 0 and q_ptr and r_ptr)),
                                             _dtw_metric(metric), C.byref(dist), path_q_ptr, path_r_ptr,
                                             path_cost_ptr, C.byref(plen), cost_ptr, 1))
        return dist.value, plen.value

    def dtw_optimize_step_pattern(self, q, r, band=-1, metric="euclidean"):
        """DTWAlignment.OptimizeStepPattern (sonar_dtw_optimize_step_pattern) -> (best pattern's
        name, {pattern: distance}; NaN for a pattern whose Align failed)."""
        q, r = _f64(q), _f64(r)
        if q.ndim == 1:
            q = q[:, None]
        if r.ndim == 1:
            r = r[:, None]
        nq, d = q.shape if q.size else (0, 1)
        nr = r.shape[0] if r.size else 0
        best, d3 = C.c_int32(), (C.c_double * 3)()
        self._check(self._L.sonar_dtw_optimize_step_pattern(self._h, _ptr(q) if nq else None, nq,
                                                            _ptr(r) if nr else None, nr, d, band, _dtw_metric(metric),
                                                            0, C.byref(best), d3))
        return DTW_STEP_NAMES[best.value], dict(zip(DTW_STEP_NAMES, d3))

    def dtw_optimize_step_pattern_device(self, q_ptr, nq, r_ptr, nr, dim, band=-1, metric="euclidean"):
        """dtw_optimize_step_pattern on device memory (device_ptrs = 1): q and r are device addresses."""
        best, d3 = C.c_int32(), (C.c_double * 3)()
        self._check(self._L.sonar_dtw_optimize_step_pattern(self._h, q_ptr, nq, r_ptr, nr, dim, band,
                                                            _dtw_metric(metric), 1, C.byref(best), d3))
        return DTW_STEP_NAMES[best.value], dict(zip(DTW_STEP_NAMES, d3))

    # -- Go API mirror -----------------------------------------------------
    def _result(self, h):
        """The result's arrays as numpy views of its memory (no copy; large arrays live in pinned
        host memory the device copied into); the handle is freed when the last view goes."""
        L = self._L
        owner = _ResultOwner(L, h)
        out = {}
        for i in range(L.sonar_result_count(h)):
            name = L.sonar_result_name(h, i).decode()
            data, rows, cols = _d(), C.c_int64(), C.c_int64()
            L.sonar_result_get(h, name.encode(), C.byref(data), C.byref(rows), C.byref(cols))
            n = rows.value * cols.value
            shape = (rows.value, cols.value) if cols.value > 1 else (n,)
            addr = C.cast(data, C.c_void_p).value
            out[name] = np.asarray(_ResultView(owner, addr, shape)) if n else np.zeros(0)
        return out

    @staticmethod
    def fingerprint_config(**kw):
        cfg = FingerprintConfig()
        lib().sonar_fingerprint_config_default(C.byref(cfg))
        for k, v in kw.items():
            setattr(cfg, k, v)
        return cfg

    def generate_fingerprint(self, pcm, sample_rate, content_type, cfg: FingerprintConfig = None):
        pcm = _f64(pcm)
        cfg = cfg or self.fingerprint_config()
        h = C.c_void_p()
        self._check(self._L.sonar_generate_fingerprint(self._h, _ptr(pcm) if len(pcm) else None, len(pcm),
                                                       sample_rate, content_type.encode(), C.byref(cfg),
                                                       C.byref(h)))
        return self._result(h)

    def detect_from_audio(self, pcm, sample_rate, auto_detect_threshold=2.0):
        """ContentDetector.DetectFromAudio -> (content type name, AcousticFeatures dict)."""
        pcm = _f64(pcm)
        ct = C.c_int32()
        f = AcousticFeatures()
        self._check(self._L.sonar_detect_from_audio(self._h, _ptr(pcm) if len(pcm) else None, len(pcm), sample_rate,
                                                    auto_detect_threshold, C.byref(ct), C.byref(f)))
        return CONTENT_NAMES[ct.value], {k: getattr(f, k) for k, _ in AcousticFeatures._fields_}

    def detect_content_type(self, pcm, sample_rate, metadata=None, acoustic_detection=True,
                            default_content_type="unknown", auto_detect_threshold=2.0):
        """ContentDetector.DetectContentType; metadata = dict(content_type, genre, station, url) or None."""
        pcm = _f64(pcm)
        ct = C.c_int32()
        md = metadata or {}
        enc = lambda k: md.get(k, "").encode() if md.get(k) else None  # noqa: E731
        self._check(self._L.sonar_detect_content_type(
            self._h, _ptr(pcm) if len(pcm) else None, len(pcm), sample_rate, int(metadata is not None),
            enc("content_type"), enc("genre"), enc("station"), enc("url"), int(acoustic_detection),
            CONTENT_NAMES.index(default_content_type), auto_detect_threshold, C.byref(ct)))
        return CONTENT_NAMES[ct.value]

    @staticmethod
    def feature_config(**kw):
        cfg = FeatureConfig()
        lib().sonar_feature_config_default(C.byref(cfg))
        for k, v in kw.items():
            setattr(cfg, k, v)
        return cfg

    def extract_speech_features(self, pcm, sample_rate, cfg: FeatureConfig = None):
        pcm = _f64(pcm)
        cfg = cfg or self.feature_config()
        h = C.c_void_p()
        self._check(self._L.sonar_extract_speech_features(self._h, _ptr(pcm) if len(pcm) else None, len(pcm),
                                                          sample_rate, C.byref(cfg), C.byref(h)))
        return self._result(h)

    def extract_music_features(self, pcm, sample_rate, cfg: FeatureConfig = None):
        """sonar_extract_music_features: MusicFeatureExtractor.ExtractFeatures as a dict of arrays.
        Where the Go reference panics (SONAR_ERR_PANIC) this raises SonarError whose .partial holds
        the arrays computed before the panic."""
        pcm = _f64(pcm)
        cfg = cfg or self.feature_config()
        h = C.c_void_p()
        rc = self._L.sonar_extract_music_features(self._h, _ptr(pcm) if len(pcm) else None, len(pcm), sample_rate,
                                                  C.byref(cfg), C.byref(h))
        partial = self._result(h) if h.value else None
        if rc != OK:
            err = SonarError(rc, self._L.sonar_last_error(self._h).decode())
            err.partial = partial
            raise err
        return partial

    def align_features(self, q_energy, r_energy, q_chroma=None, r_chroma=None, q_pcm_len=0, r_pcm_len=0,
                       sample_rate=44100, feature_sample_rate=44100, hop_size=256, window_size=1024,
                       max_lag_seconds=60.0):
        qe, re_ = _f64(q_energy), _f64(r_energy)
        qc = _f64(q_chroma) if q_chroma is not None else np.zeros((0, 12))
        rc = _f64(r_chroma) if r_chroma is not None else np.zeros((0, 12))
        h = C.c_void_p()
        self._check(self._L.sonar_align_features(
            self._h, _ptr(qe) if len(qe) else None, len(qe), _ptr(re_) if len(re_) else None, len(re_),
            _ptr(qc) if len(qc) else None, len(qc), _ptr(rc) if len(rc) else None, len(rc),
            q_pcm_len, r_pcm_len, sample_rate, feature_sample_rate, hop_size, window_size, max_lag_seconds,
            C.byref(h)))
        return self._result(h)


class StftStream:
    """STFTStreamer (fingerprint/analyzers/spectral.go:314-366) over sonar_stft_stream_*: push(chunk)
    is ProcessChunk and returns the emitted frames as a dict of arrays (the cfg's outputs, rows =
    frames; empty arrays when no frame is complete).  Host buffers (cfg.device_ptrs = 0) unless
    push_device is used."""

    def __init__(self, ctx, h, cfg):
        self._ctx, self._h, self.cfg = ctx, h, cfg

    def frames(self, n):
        return int(self._ctx._L.sonar_stft_stream_frames(self._h, n))

    @property
    def buffered(self):
        return int(self._ctx._L.sonar_stft_stream_buffered(self._h))

    def push(self, chunk):
        cfg = self.cfg
        x = np.ascontiguousarray(chunk, dtype=np.float64 if cfg.pcm_dtype == F64 else np.float32)
        n = len(x)
        F = self.frames(n)
        res, out = self._ctx._fp_outputs(n, cfg, frames=max(F, 0))
        got = C.c_int64()
        self._ctx._check(self._ctx._L.sonar_stft_stream_push(self._h, _ptr(x) if n else None, n, C.byref(out),
                                                             C.byref(got)))
        assert got.value == max(F, 0), (got.value, F)
        return res

    def push_device(self, ptr, n, **out_ptrs):
        """Device chunk and outputs (cfg.device_ptrs must be 1): async on the ctx stream; returns the
        number of frames written."""
        out = FpOut()
        for k, v in out_ptrs.items():
            setattr(out, k, v)
        got = C.c_int64()
        self._ctx._check(self._ctx._L.sonar_stft_stream_push(self._h, C.c_void_p(ptr), n, C.byref(out), C.byref(got)))
        return got.value

    def close(self):
        if getattr(self, "_h", None):
            self._ctx._L.sonar_stft_stream_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Multi:
    """sonar_multi: one context per device + an RCCL communicator over them (one process)."""

    def __init__(self, devices):
        L = lib()
        devs = (C.c_int32 * len(devices))(*devices)
        h = C.c_void_p()
        rc = L.sonar_multi_create(devs, len(devices), C.byref(h))
        if rc != OK:
            raise SonarError(rc, "sonar_multi_create failed (GPUs / RCCL)")
        self._h, self._L, self.devices = h, L, list(devices)

    def close(self):
        if getattr(self, "_h", None):
            self._L.sonar_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != OK:
            raise SonarError(rc, self._L.sonar_multi_last_error(self._h).decode())

    def size(self):
        return int(self._L.sonar_multi_size(self._h))

    def ctx(self, rank):
        """Rank `rank`'s context (sonar_multi_ctx) as a non-owning Context."""
        return Context.wrap(self._L.sonar_multi_ctx(self._h, rank), owner=self)

    def find_best_matches(self, galleries, queries, candidates, cfg):
        """sonar_find_best_matches_multi: galleries[g] on rank g (sonar.compare.Gallery built on
        Context wrappers of sonar_multi_ctx), queries[g] the queries' indices in galleries[g],
        candidates[g] rank g's candidates (None: the whole gallery).  Returns per query the merged
        Match list (candidates numbered globally, rank g's after ranks 0..g-1)."""
        G = len(galleries)
        nq = len(queries[0])
        qs = [np.ascontiguousarray(q, dtype=np.int64) for q in queries]
        cs = None if candidates is None else [np.ascontiguousarray(c, dtype=np.int64) for c in candidates]
        nc = np.array([len(g) if cs is None else len(cs[i]) for i, g in enumerate(galleries)], dtype=np.int64)
        gp = (C.c_void_p * G)(*[g._h.value for g in galleries])
        qp = (C.c_void_p * G)(*[q.ctypes.data for q in qs])
        cp = None if cs is None else (C.c_void_p * G)(*[c.ctypes.data if len(c) else None for c in cs])
        K = max(0, cfg.max_candidates)
        out = (Match * max(1, nq * K))()
        nm = np.zeros(max(1, nq), dtype=np.int64)
        self._check(self._L.sonar_find_best_matches_multi(self._h, gp, qp, nq, cp, nc.ctypes.data_as(_i64p),
                                                          C.byref(cfg), out, nm.ctypes.data_as(_i64p)))
        return [[out[i * K + k] for k in range(int(nm[i]))] for i in range(nq)]

    def fingerprint(self, pcm, cfg: FpConfig):
        """sonar_fingerprint_multi (host PCM, host outputs): MFCC / magnitude / descriptors."""
        F = stft_frames(len(pcm), cfg.window_size, cfg.hop_size)
        if F <= 0:
            raise SonarError(-2, "signal too short for given window size and hop size")
        pdt = np.float32 if cfg.pcm_dtype == F32 else np.float64
        odt = np.float32 if cfg.out_dtype == F32 else np.float64
        x = np.ascontiguousarray(pcm, dtype=pdt)
        res, o = {}, FpOut()
        if cfg.flags & FP_MFCC:
            res["mfcc"] = np.zeros((F, cfg.n_mfcc if cfg.n_mfcc > 0 else 13), odt)
            o.mfcc = res["mfcc"].ctypes.data
        if cfg.flags & FP_MAGNITUDE:
            res["magnitude"] = np.zeros((F, cfg.window_size // 2 + 1), odt)
            o.magnitude = res["magnitude"].ctypes.data
        if cfg.flags & FP_COMPLEX:
            res["complex"] = np.zeros((F, cfg.window_size // 2 + 1, 2), odt)
            o.complex = res["complex"].ctypes.data
        if cfg.flags & FP_PHASE:
            res["phase"] = np.zeros((F, cfg.window_size // 2 + 1), odt)
            o.phase = res["phase"].ctypes.data
        if cfg.flags & FP_SPECTRAL:
            for k in ("centroid", "rolloff", "bandwidth", "flatness", "crest", "slope", "low_ratio", "high_ratio"):
                res[k] = np.zeros(F, odt)
                setattr(o, k, res[k].ctypes.data)
        self._check(self._L.sonar_fingerprint_multi(self._h, x.ctypes.data, len(x), C.byref(cfg), C.byref(o)))
        return res

    def fingerprint_gather(self, pcm_ptrs, n, cfg: FpConfig, mfcc_ptrs):
        """sonar_fingerprint_multi_gather: device slices in, the MFCC timeline on every device."""
        G = len(pcm_ptrs)
        pp = (C.c_void_p * G)(*pcm_ptrs)
        mp = (C.c_void_p * G)(*mfcc_ptrs)
        self._check(self._L.sonar_fingerprint_multi_gather(self._h, pp, n, C.byref(cfg), mp))

    def align_pairs(self, qs, rs, sample_rate=44100, stft_window=1024, hop=256, feature_window=1024,
                    max_lag_seconds=20.0, workers=128):
        """sonar_align_pairs_multi: host streams, pair ranges per device, records all-gathered over RCCL."""
        n = len(qs)
        qp, rp, keep = _pair_arrays(qs, rs)
        nqa = (C.c_int64 * n)(*[len(x) for x in qs])
        nra = (C.c_int64 * n)(*[len(x) for x in rs])
        recs = (PairRecord * max(n, 1))()
        self._check(self._L.sonar_align_pairs_multi(self._h, n, qp, nqa, rp, nra, sample_rate, stft_window, hop,
                                                    feature_window, max_lag_seconds, workers, recs))
        del keep
        return records_dict(recs[:n])
