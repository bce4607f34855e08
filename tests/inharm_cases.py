"""The cases the inharmonicity tests share (tests/test_inharm_cpu.py, tests/test_gpu_inharm.py): the spectrum rows
and their f0, the signals, the parameter pairs (checker, library) and the cached reference of every case.

Spectrum rows.  K = 32 (W = 64, 16 kHz, bins of 250 Hz) is where the search window is a bin or two wide and clamps
at both ends of the row; K = 512 (W = 1024, 44.1 kHz) is the analyzer's own shape, with up to 20 harmonics under
max_freq.  Each row has stretched partials n f0 sqrt(1 + B n^2) as three-bin peaks over a low noise floor.  One
reference of 130 frames serves every F: a frame's row depends on nothing else.  The f0 of frames 1, 2 and 3
(where F reaches them) are 0, below min_freq and above max_freq; frame 4's is negative.

Signals.  W = 1024 only (the analyzer's detector takes nothing else).  `tone` is a stretched-partial tone whose
f0 lies inside 80-1000 Hz, `sine` a single partial (too few harmonics), `noise` and `silence` give an f0 of 0
(invalid), `step` changes its f0 halfway (the tracker's histories move)."""
import functools

import numpy as np

import inharm_ref as R

METHODS = {"railsback": R.RAILSBACK, "fletcher_munson": R.FLETCHER_MUNSON, "spectral_deviation": R.SPECTRAL_DEVIATION,
           "partial_tracking": R.PARTIAL_TRACKING, "beat_pattern": R.BEAT_PATTERN, "statistical": R.STATISTICAL}
MODELS = {"string": R.MODEL_STRING, "pipe": R.MODEL_PIPE, "membrane": R.MODEL_MEMBRANE, "general": R.MODEL_GENERAL}
SPECTRUM_METHODS = ("railsback", "fletcher_munson", "spectral_deviation", "partial_tracking", "statistical")
SPECTRUM_K = {32: 16000, 512: 44100}                        # K -> sample rate
# at K = 32 a bin is 250 Hz: the defaults (5 %, 2 kHz) keep nearly nothing, so those cases search wider and higher
SPECTRUM_EXTRA = {32: (("harmonic_tolerance", 0.25), ("max_freq", 7500.0)), 512: ()}
SPECTRUM_F = (1, 5, 65, 66, 130)
F_MAX = 130
# bit for bit | through log10 / exp (hratio_cases.ULP16, scaled as there: relative, or absolute near 0)
EXACT_KEYS = ("status", "num_harmonics", "n_deviations", "h_number", "h_freq", "h_ideal", "h_amp", "f0", "f0_confidence",
              "h_deviation", "inharmonicity", "std_dev", "confidence", "estimated_stiffness", "partial_coherence",
              "r_squared", "quality")
LOG_KEYS = ("model_fit_quality", "harmonic_clarity", "spectral_purity", "chi_squared", "p_value")
PCM_HOPS = (512, 1024)
PCM_F = (1, 5, 66)


def ref_params(sr, method, model="general", **kw):
    return R.Params(sr, method=METHODS[method], model=MODELS[model], **kw)


def lib_params(sonar, sr, method, model="general", **kw):
    kw = {k: (int(v) if isinstance(v, bool) else v) for k, v in kw.items()}
    return sonar.inharm_params_default(sr, method=method, model=model, **kw)


@functools.lru_cache(maxsize=None)
def spectrum_rows(K):
    """(mag F_MAX x K, f0, f0_confidence) of the spectrum cases"""
    sr, W = SPECTRUM_K[K], 2 * K
    rng = np.random.default_rng(1000 + K)
    mag = 0.004 * np.abs(rng.standard_normal((F_MAX, K)))
    lo, hi = (300.0, 1100.0) if K == 32 else (85.0, 420.0)
    f0 = rng.uniform(lo, hi, F_MAX)
    conf = rng.uniform(0.3, 1.0, F_MAX)
    for f in range(F_MAX):
        B = rng.choice([0.0, 1e-4, 8e-4, 3e-3, -2e-3])
        amp = rng.uniform(0.5, 30.0)
        for n in range(1, 41):
            if 1.0 + B * n * n <= 0:
                break
            b = int(round(n * f0[f] * np.sqrt(1.0 + B * n * n) * W / sr + rng.uniform(-0.4, 0.4)))
            if not 1 <= b < K - 1:
                break
            a = amp * rng.uniform(0.3, 1.0) / n ** rng.uniform(0.3, 1.5)
            if rng.random() < 0.1:
                a = 0.0                                     # a missing partial
            mag[f, b] += a
            mag[f, b - 1] += 0.45 * a
            mag[f, b + 1] += 0.35 * a
    f0[1], f0[2], f0[3], f0[4] = 0.0, 60.0, 9000.0, -200.0
    for a in (mag, f0, conf):
        a.setflags(write=False)
    return mag, f0, conf


@functools.lru_cache(maxsize=None)
def spectrum_ref(K, method, model, extra=()):
    """the checker's rows of the F_MAX frames under SPECTRUM_EXTRA[K] and then `extra` (pairs)"""
    mag, f0, conf = spectrum_rows(K)
    kw = dict(SPECTRUM_EXTRA[K] + tuple(extra))
    return R.from_spectrum(mag, f0, conf, ref_params(SPECTRUM_K[K], method, model, window_size=2 * K, **kw))


def _n_samples(F, hop, W=1024):
    return (F - 1) * hop + W


@functools.lru_cache(maxsize=None)
def signal(kind, sr, F, hop):
    """one of the PCM inputs, exactly F whole frames of 1024 every hop"""
    n = _n_samples(F, hop)
    t = np.arange(n, dtype=np.float64) / sr
    rng = np.random.default_rng(7 + F + hop)
    if kind == "silence":
        x = np.zeros(n)
    elif kind == "noise":
        x = 0.3 * rng.standard_normal(n)
    elif kind == "sine":
        x = 0.8 * np.sin(2 * np.pi * 330.0 * t)
    else:
        f0 = np.full(n, 220.0 if sr == 16000 else 300.0)
        if kind == "step":
            f0[n // 2:] *= 1.5
        B = 4e-4
        ph = 2 * np.pi * np.cumsum(f0) / sr
        x = 0.002 * rng.standard_normal(n)
        for k in range(1, 9):
            x = x + (0.8 ** k) * np.sin(k * np.sqrt(1.0 + B * k * k) * ph)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def pcm_ref(kind, sr, F, hop, method, model="general", fft="numpy", extra=()):
    p = ref_params(sr, method, model, window_size=1024, **dict(extra))
    return R.frames(signal(kind, sr, F, hop), hop, p, fft)


def same_bits(a, b):
    """bit for bit, a NaN equal to a NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)
