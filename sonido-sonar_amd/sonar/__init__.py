"""sonar -- Python view of the MI355X sonido-sonar hot path.

Thin ctypes binding over the C ABI in include/sonar_gpu.h (library
sonido-sonar_amd/lib/libsonar_gpu.so).  Names and argument meaning follow the
Go reference (RyanBlaney/sonido-sonar) so that tests read like the reference's
API:  ``Context.fingerprint`` ~ ComputeSTFTWithWindow + MFCC.ComputeFrames,
``Context.ncc`` ~ CrossCorrelation.Compute, ``Context.xcorr_params`` / ``xcorr`` / ``autocorr`` ~ the
same for every type, method and constructor, ``Context.dtw`` ~ DTWAlignment.Align,
``Context.dtw_params`` ~ NewDTWAlignmentWithParams(...).Align, ``dtw_quality`` ~ GetAlignmentQuality,
``Context.chroma_cqt`` ~ NewChromaCQT(...).ComputeChroma (``chroma_cqt_plan``: its sizes, host only),
``Context.chroma_similarity`` ~ ChromaSequenceSimilarity.ComputeSimilarity (``chroma_frame_matrix``: its
frame distances / similarities, ``chroma_similarity_plan``: its integer side, host only),
``Context.spectral_peaks`` ~ SpectralPeaks.DetectPeaks per spectrum row, ``Context.hpcp_from_spectrum`` ~
HPCP.ComputeFromSpectrum per row and ``Context.hpcp`` ~ the same over the STFT magnitudes of a signal
(``hpcp_params``: NewHPCP's defaults, ``hpcp_table``: the per-bin contribution table, ``hpcp_plan``: the
frame count and chunks, host only),
``Context.key_frames`` ~ KeyEstimator.EstimateKey per chroma row (also ProcessBatch and EstimateKeyFromHPCP),
``Context.key_sequence`` ~ EstimateKeySequence and ``Context.key_batch`` ~ KeyEstimationBatch's ProcessBatch,
GetGlobalKey and GetKeyProgression (``key_params``: NewKeyEstimator's defaults, ``key_transition``:
AnalyzeKeyTransition, host only, ``key_name``: getKeyName of a code),
``Context.generate_fingerprint`` ~ FingerprintGenerator.GenerateFingerprint,
``Context.align_features`` ~ AlignmentExtractor.ExtractAlignmentFeatures.

There is no CPU fallback: if the shared library is missing or no GPU is
visible, calls raise.
"""
from ._abi import (  # noqa: F401
    LIB_PATH,
    SonarError,
    Context,
    Multi,
    FpConfig,
    PairRecord,
    PAIR_FIELDS,
    PAIR_REDONE_NONFINITE,
    PAIR_REDONE_TIMEOUT,
    multi_shard,
    WINDOWS,
    abi_version,
    dtw_quality,
    DTW_STEPS,
    DTW_METRICS,
    CORR_TYPES,
    CORR_METHODS,
    build,
    lib,
    stft_frames,
    energy_frames,
    pitch_frames,
    fp_kernel_plan,
    chroma_cqt_plan,
    chroma_similarity_plan,
    HpcpParams,
    HPCP_WEIGHTS,
    hpcp_params,
    hpcp_table,
    hpcp_plan,
    spectral_peaks_width,
    KeyParams,
    KEY_PROFILES,
    KEY_TRANSITIONS,
    KEY_NAMES,
    KEY_FRAME_FIELDS,
    key_params,
    key_name,
    key_transition,
    CHROMA_SIM_METHODS,
    CHROMA_DIST_METRICS,
    PLAN_NONE,
    PLAN_PAIR,
    PLAN_WAVE,
    PLAN_DFT,
    PAIR_MAX_FRAMES,
    FP_MFCC,
    FP_MAGNITUDE,
    FP_SPECTRAL,
    FP_ZCR,
    FP_ENERGY,
    FP_COMPLEX,
    FP_PHASE,
    FP_GENERIC,
    F32,
    F64,
    INGEST_DEVICE_CONVERT,
    INGEST_HOST_CONVERT,
    ERR_INVALID,
    ERR_EMPTY,
    ERR_TOO_SHORT,
    ERR_UNSUPPORTED,
    ERR_PANIC,
    EXPORTED_SYMBOLS,
)
