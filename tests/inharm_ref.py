"""The checker of sonar_inharm_from_spectrum / sonar_inharm_frames / sonar_inharm_track / sonar_inharm: a float64
restatement of the reference's InharmonicityAnalyzer for every method of AnalyzeFrame's switch (test
infrastructure, never the product).

  NewInharmonicityAnalyzer, AnalyzeFrame, analyzeHarmonicStructure, findHarmonicPeak, calculate{SpectralDeviation,
  Railsback,FletcherMunson,PartialTracking,BeatPattern,Statistical}Inharmonicity, calculateConfidence,
  fitRailsbackCurve, calculateRSquared, calculateFletcherMunsonWeight, analyzePeriodicityVariation, removeOutliers,
  calculateStatisticalConfidence, performGoodnessOfFitTest, applyStringModel, calculateStringModelFit,
  calculateQualityMetrics, postProcessResult, updateTemporalTracking, assessAnalysisQuality, AnalyzeSequence,
  GetAverageInharmonicity, ClassifyInharmonicity, EstimateInstrumentType
                                                          (algorithms/tonal/inharmonicity.go:147-1313)
  common.Mean, Variance, Percentile, LinRegression, FindPeaks   (algorithms/common/math.go)

Staged like hratio_ref.py: the f0 of every frame is pitch_ref.detect's tracked pitch at NewPitchDetector's
parameters; the spectrum of a frame is the unwindowed transform (`fft` picks numpy's or
xcorr_params_ref.go_fft, two independent float64 orderings); everything after it runs on |X| rows.  Every sum
is a Python loop in Go's order.  math.Min / math.Max follow Go's NaN rules (go_min, go_max) and int() of a NaN
or of a value out of range is the minimum int64, as amd64 gives it (go_int).  gonum is not in the tree:
stat.Mean is a sequential sum, stat.Variance the compensated two-pass form, stat.Quantile(p, Empirical) the
first sorted value whose count reaches p n (hratio_ref's), stat.LinearRegression's slope the compensated
covariance over the variance of x.

frames() also returns `decided` per frame: false where the harmonic search (which harmonics are kept, and at
which bins) differs between the two transforms, so that a bin comparison there hangs on the transform's
rounding."""
import math
from dataclasses import dataclass

import numpy as np

import hratio_ref as HR
import pitch_ref as PR
import xcorr_params_ref as X

RAILSBACK, FLETCHER_MUNSON, SPECTRAL_DEVIATION, PARTIAL_TRACKING, BEAT_PATTERN, STATISTICAL = range(6)
MODEL_STRING, MODEL_PIPE, MODEL_MEMBRANE, MODEL_GENERAL = range(4)
OK, INVALID_F0, INSUFFICIENT = range(3)
METHOD_NAMES = ["Railsback Curve", "Fletcher-Munson Weighted", "Spectral Deviation", "Partial Tracking",
                "Beat Pattern Analysis", "Statistical Analysis"]
MODEL_NAMES = ["String Instrument", "Pipe/Wind Instrument", "Membrane/Percussion", "General"]
QUALITY_NAMES = ["Very Poor", "Poor", "Fair", "Good", "Excellent", "Poor - Invalid F0"]
CLASS_NAMES = ["Very Low", "Low", "Moderate", "High", "Very High"]
INSTRUMENT_NAMES = ["Piano/String", "Wind/Brass", "Plucked String", "Vocal/Harmonic", "Unknown"]
INT_KEYS = ("status", "num_harmonics", "n_deviations", "h_number", "quality")
ROW_KEYS = ("h_number", "h_freq", "h_ideal", "h_amp", "h_deviation")
SCALAR_KEYS = ("status", "inharmonicity", "std_dev", "confidence", "f0", "f0_confidence", "num_harmonics", "n_deviations",
               "estimated_stiffness", "model_fit_quality", "harmonic_clarity", "spectral_purity", "partial_coherence",
               "r_squared", "chi_squared", "p_value", "quality")
MIN_INT64 = -2 ** 63
DETECTOR_WINDOW = 1024                                      # NewPitchDetector's WindowSize (pitch_detection.go:163)


@dataclass
class Params:
    """InharmonicityParams with NewInharmonicityAnalyzer's values (:147-172), the never-read ones left out"""
    sample_rate: int
    method: int = SPECTRAL_DEVIATION
    model: int = MODEL_GENERAL
    window_size: int = 4096
    max_harmonics: int = 20
    min_harmonics: int = 3
    harmonic_tolerance: float = 0.05
    min_harmonic_strength: float = 0.01
    min_freq: float = 80.0
    max_freq: float = 2000.0
    weight_by_amplitude: bool = True
    string_tension: float = 1.0
    string_length: float = 1.0
    outlier_threshold: float = 2.0
    use_robust_estimation: bool = True
    use_temporal_tracking: bool = False
    temporal_window: int = 10


class InsufficientHarmonics(ValueError):
    """analyzeHarmonicStructure's error (:369)"""

    def __init__(self, found, need):
        super().__init__("insufficient harmonics found: %d < %d" % (found, need))
        self.found = found


# ------------------------------------------------------------------ Go's arithmetic ----
def go_max(x, y):
    """math.Max: +Inf wins, then a NaN propagates, then +0 > -0"""
    if x == math.inf or y == math.inf:
        return math.inf
    if x != x or y != y:
        return math.nan
    if x == 0 and y == 0:
        return y if math.copysign(1.0, x) < 0 else x
    return x if x > y else y


def go_min(x, y):
    """math.Min: -Inf wins, then a NaN propagates, then -0 < +0"""
    if x == -math.inf or y == -math.inf:
        return -math.inf
    if x != x or y != y:
        return math.nan
    if x == 0 and y == 0:
        return x if math.copysign(1.0, x) < 0 else y
    return x if x < y else y


def go_int(x):
    """int(float64) on amd64: CVTTSD2SQ gives the minimum int64 for a NaN or a value out of range"""
    if x != x or not -9223372036854775808.0 <= x < 9223372036854775808.0:
        return MIN_INT64
    return int(x)


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _sqrt(x):
    return math.nan if (x != x or x < 0) else math.sqrt(x)


def _exp(x):
    if x != x:
        return math.nan
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


_log10 = HR._log10


def mean(x):
    """common.Mean (math.go:14-19)"""
    if len(x) == 0:
        return 0.0
    s = 0.0
    for v in x:
        s += v
    return _div(s, float(len(x)))


def variance(x):
    """common.Variance (math.go:22-27)"""
    return 0.0 if len(x) < 2 else HR.gonum_variance([float(v) for v in x])


def linear_regression_slope(x, y):
    """stat.LinearRegression(x, y, nil, false)'s beta: covarianceMeans / variance of x, around stat.Mean's means"""
    n = len(x)
    xu, yu = mean(x), mean(y)
    ss = xc = yc = 0.0
    for a, b in zip(x, y):
        xd, yd = a - xu, b - yu
        ss += xd * yd
        xc += xd
        yc += yd
    cov = (ss - xc * yc / float(n)) / float(n - 1)
    return _div(cov, variance(x))


def grid():
    """for b := -0.01; b <= 0.01; b += 0.0001 (:640)"""
    out, b = [], -0.01
    while b <= 0.01:
        out.append(b)
        b += 0.0001
    return out


GRID = grid()


def stretched(n, f0, B):
    """n * f0 * math.Sqrt(1 + B*n*n)"""
    return n * f0 * _sqrt(1.0 + B * n * n)


# ------------------------------------------------------------------ the harmonic search ----
def find_harmonic_peak(mag, expected, p, W):
    """findHarmonicPeak (:376-416) -> (frequency, magnitude, bin) or None"""
    K = len(mag)
    sr = float(p.sample_rate)
    eb = expected * float(W) / sr
    tb = p.harmonic_tolerance * expected * float(W) / sr
    start = go_int(go_max(0.0, eb - tb))
    end = go_int(go_min(float(K - 1), eb + tb))
    mx, mb = 0.0, start
    for i in range(start, end + 1):
        if mag[i] > mx:
            mx, mb = float(mag[i]), i
    if 0 < mb < K - 1 and mag[mb] > mag[mb - 1] and mag[mb] > mag[mb + 1]:
        return float(mb) * sr / float(W), mx, mb
    return None


def harmonic_structure(mag, f0, p, W):
    """analyzeHarmonicStructure (:341-365) without its error -> dict of lists (numbers, freqs, ideals, amps,
    deviations, bins)"""
    d = {k: [] for k in ("numbers", "freqs", "ideals", "amps", "deviations", "bins")}
    for h in range(1, p.max_harmonics + 1):
        ideal = f0 * float(h)
        if ideal > p.max_freq:
            break
        pk = find_harmonic_peak(mag, ideal, p, W)
        if pk is not None and pk[1] > p.min_harmonic_strength:
            dev = (pk[0] - ideal) / ideal
            if abs(dev) < p.harmonic_tolerance:
                d["numbers"].append(h); d["freqs"].append(pk[0]); d["ideals"].append(ideal)
                d["amps"].append(pk[1]); d["deviations"].append(dev); d["bins"].append(pk[2])
    return d


# ------------------------------------------------------------------ the methods ----
def _empty():
    return {"inharmonicity": 0.0, "std_dev": 0.0, "confidence": 0.0, "deviations": None, "r_squared": 0.0,
            "model_fit_quality": 0.0, "chi_squared": 0.0, "p_value": 0.0}


def _confidence(d, p):
    """calculateConfidence (:620-630)"""
    return go_min(1.0, _div(float(len(d["freqs"])), float(p.max_harmonics)) * mean(d["amps"]))


def spectral_deviation(d, p):
    """calculateSpectralDeviationInharmonicity (:419-464)"""
    r = _empty()
    if len(d["deviations"]) == 0:
        return r
    num = den = 0.0
    for i, dev in enumerate(d["deviations"]):
        n = float(d["numbers"][i])
        w = d["amps"][i] if p.weight_by_amplitude else 1.0
        num += w * (dev - 0.0) * n * n
        den += w * n * n * n * n
    r["inharmonicity"] = num / den if den > 0 else 0.0
    r["std_dev"] = _sqrt(variance(d["deviations"]))
    r["confidence"] = _confidence(d, p)
    r["deviations"] = list(d["deviations"])
    return r


def fit_railsback(d, f0):
    """fitRailsbackCurve (:632-657)"""
    g = np.array(GRID)
    err = np.zeros(len(g))                                  # every grid value's sum at once, the harmonics in order
    with np.errstate(invalid="ignore"):
        for i, f in enumerate(d["freqs"]):
            n = float(d["numbers"][i])
            diff = f - n * f0 * np.sqrt(1.0 + g * n * n)
            err = err + diff * diff
    best, min_err = 0.0, math.inf
    for b, e in zip(GRID, err.tolist()):
        if e < min_err:
            min_err, best = e, b
    return best


def railsback(d, f0):
    """calculateRailsbackInharmonicity (:467-510), calculateRSquared (:659-680)"""
    r = _empty()
    if len(d["freqs"]) < 3:
        return r
    B = fit_railsback(d, f0)
    mean_obs = mean(d["freqs"])
    ss_res = ss_tot = 0.0
    for i, obs in enumerate(d["freqs"]):
        pred = stretched(float(d["numbers"][i]), f0, B)
        ss_res += (obs - pred) * (obs - pred)
        ss_tot += (obs - mean_obs) * (obs - mean_obs)
    r2 = 1.0 - _div(ss_res, ss_tot) if ss_tot > 0 else 0.0
    devs = []
    for i, f in enumerate(d["freqs"]):
        ex = stretched(float(d["numbers"][i]), f0, B)
        devs.append(_div(f - ex, ex))
    r.update(inharmonicity=B, std_dev=_sqrt(variance(devs)), confidence=go_max(0.0, r2), deviations=devs, r_squared=r2,
             model_fit_quality=r2)
    return r


def fm_weight(freq):
    """calculateFletcherMunsonWeight (:682-704)"""
    if freq < 20 or freq > 20000:
        return 0.0
    w = 1.0
    if freq < 1000:
        w = 0.5 + 0.5 * (freq / 1000)
    elif freq > 4000:
        w = 1.0 - 0.3 * _log10(freq / 4000)
    return go_max(0.1, w)


def fletcher_munson(d, p):
    """calculateFletcherMunsonInharmonicity (:513-542)"""
    r = _empty()
    wd = [dev * fm_weight(d["freqs"][i]) for i, dev in enumerate(d["deviations"])]
    r.update(inharmonicity=mean(wd), std_dev=_sqrt(variance(wd)), confidence=_confidence(d, p), deviations=wd)
    return r


def remove_outliers(data, thr):
    """removeOutliers (:735-762)"""
    if len(data) < 3:
        return list(data)
    q1, q3 = HR.percentile(data, 0.25), HR.percentile(data, 0.75)
    iqr = q3 - q1
    lo, hi = q1 - thr * iqr, q3 + thr * iqr
    return [v for v in data if lo <= v <= hi]


def statistical_confidence(data):
    """calculateStatisticalConfidence (:764-791)"""
    if len(data) < 2:
        return 0.0
    se = _sqrt(_div(variance(data), float(len(data))))
    moe = 2.0 * se
    m = mean(data)
    if m != 0:
        return go_min(1.0, _div(1.0, 1.0 + _div(moe, abs(m))))
    return 0.5


def goodness_of_fit(data):
    """performGoodnessOfFitTest (:793-845) -> (chi squared, p value)"""
    n = len(data)
    if n < 5:
        return 0.0, 1.0
    m, sd = mean(data), _sqrt(variance(data))
    nb = go_int(go_min(10.0, float(n) / 2))
    lo, hi = m - 3 * sd, m + 3 * sd
    bw = _div(hi - lo, float(nb))
    observed = [0] * nb
    for v in data:
        b = go_int(_div(v - lo, bw))
        if 0 <= b < nb:
            observed[b] += 1
    chi = 0.0
    for i in range(nb):
        center = lo + (float(i) + 0.5) * bw
        z = _div(center - m, sd)
        density = _div(_exp(-0.5 * z * z), sd * math.sqrt(2 * math.pi))
        expected = density * bw * float(n)
        if expected > 0:
            diff = float(observed[i]) - expected
            chi += _div(diff * diff, expected)
    dof = float(nb - 3)
    pv = 1.0 - _div(chi, dof * 2.0)
    return chi, go_max(0.0, go_min(1.0, pv))


def statistical(d, p):
    """calculateStatisticalInharmonicity (:576-610)"""
    r = _empty()
    if len(d["deviations"]) == 0:
        return r
    devs = list(d["deviations"])
    if p.use_robust_estimation:
        devs = remove_outliers(devs, p.outlier_threshold)
    chi, pv = goodness_of_fit(devs)
    r.update(inharmonicity=mean(devs), std_dev=_sqrt(variance(devs)), confidence=statistical_confidence(devs),
             deviations=devs, chi_squared=chi, p_value=pv)
    return r


def find_peaks(data, min_height):
    """common.FindPeaks(data, min_height, 1.0) (math.go:265-302): |i - j| < 1.0 holds for no two indices"""
    return [i for i in range(1, len(data) - 1) if data[i] > data[i - 1] and data[i] > data[i + 1] and data[i] >= min_height]


def beat_value(corr, lags):
    """analyzePeriodicityVariation (:706-733) times 0.001 (:567)"""
    v = 0.0
    if len(corr) >= 10:
        peaks = find_peaks(corr, 0.1)
        if len(peaks) >= 2:
            pos = [float(lags[i]) for i in peaks]
            m = mean(pos)
            if m > 0:
                v = _sqrt(variance(pos)) / m
    return v * 0.001


def beat_of_frame(frame):
    """calculateBeatPatternInharmonicity's value for one raw frame: NewAutoCorrelation(W).Compute"""
    r = X.autocorr(frame, len(frame))
    return beat_value(r["corr"], r["lags"])


def string_fit(d, B):
    """calculateStringModelFit (:898-919)"""
    if len(d["freqs"]) == 0:
        return 0.0
    f0 = d["ideals"][0] / float(d["numbers"][0])
    total = 0.0
    for i, f in enumerate(d["freqs"]):
        total += abs(f - stretched(float(d["numbers"][i]), f0, B))
    return _exp(_div(-_div(total, float(len(d["freqs"]))), f0))


def quality_metrics(d):
    """calculateQualityMetrics (:921-1005) -> clarity, purity, coherence"""
    clarity = purity = coherence = 0.0
    amps = d["amps"]
    if len(amps) > 0:
        mx = 0.0
        for a in amps:
            if a > mx:
                mx = a
        mn = mx
        for a in amps:
            if a < mn and a > 0:
                mn = a
        if mn > 0:
            clarity = go_min(1.0, (20 * _log10(mx / mn)) / 60.0)
    if len(d["deviations"]) > 0:
        s = 0.0
        for dev in d["deviations"]:
            s += abs(dev)
        s /= float(len(d["deviations"]))
        purity = _exp(-s * 20)
    f = d["freqs"]
    if len(f) >= 2:
        sp = [f[i] - f[i - 1] for i in range(1, len(f))]
        m = mean(sp)
        if m > 0:
            coherence = 1.0 / (1.0 + _sqrt(variance(sp)) / m)
    return clarity, purity, coherence


def assess(n, p, f0c, conf, fit):
    """assessAnalysisQuality (:1103-1137) -> SONAR_INHARM_QUALITY_*"""
    score = 0.0
    score += _div(float(n), float(p.max_harmonics)) * 0.3
    score += f0c * 0.3
    score += conf * 0.2
    if fit > 0:
        score += fit * 0.2
    else:
        score += 0.1
    return 4 if score >= 0.8 else 3 if score >= 0.6 else 2 if score >= 0.4 else 1 if score >= 0.2 else 0


def _blank(f0, f0c):
    r = {k: 0 if k in INT_KEYS else 0.0 for k in SCALAR_KEYS}
    r.update(f0=float(f0), f0_confidence=float(f0c), harmonics=None, deviations=None, quality=-1)
    return r


def analyze_spectrum(mag, f0, f0c, p, W=None, beat=None):
    """AnalyzeFrame after the transform (:236-292) without postProcessResult's tracking -> the row.  `beat` is the
    BeatPattern value of the frame (it needs the samples)."""
    W = 2 * len(mag) if W is None else W
    method = p.method if p.method in (RAILSBACK, FLETCHER_MUNSON, BEAT_PATTERN, STATISTICAL) else SPECTRAL_DEVIATION
    r = _blank(f0, f0c)
    if f0 <= 0 or f0 < p.min_freq or f0 > p.max_freq:
        r.update(status=INVALID_F0, quality=5)
        return r
    d = harmonic_structure(mag, f0, p, W)
    n = len(d["freqs"])
    r["num_harmonics"] = n
    r["bins"] = d["bins"]
    if n < p.min_harmonics:
        r["status"] = INSUFFICIENT
        return r
    if method == RAILSBACK:
        m = railsback(d, f0)
    elif method == FLETCHER_MUNSON:
        m = fletcher_munson(d, p)
    elif method == STATISTICAL:
        m = statistical(d, p)
    elif method == BEAT_PATTERN:
        m = _empty()
        m["inharmonicity"] = float(beat)
    else:
        m = spectral_deviation(d, p)
    r.update({k: m[k] for k in ("inharmonicity", "std_dev", "confidence", "r_squared", "model_fit_quality", "chi_squared",
                                "p_value")})
    if m["deviations"] is not None:
        r["harmonics"], r["deviations"], r["n_deviations"] = d, m["deviations"], len(m["deviations"])
    if p.model == MODEL_STRING:                                        # applyStringModel :860-884
        B = r["inharmonicity"]
        r["estimated_stiffness"] = B * p.string_tension * p.string_length * p.string_length
        r["model_fit_quality"] = string_fit(d, B)
    r["harmonic_clarity"], r["spectral_purity"], r["partial_coherence"] = quality_metrics(d)
    r["quality"] = assess(n, p, float(f0c), r["confidence"], r["model_fit_quality"])
    return r


def _pack(rows, p):
    F, mh = len(rows), max(p.max_harmonics, 0)
    out = {k: np.array([r[k] for r in rows], dtype=np.int32 if k in INT_KEYS else np.float64).reshape(F)
           for k in SCALAR_KEYS}
    out["h_number"] = np.full((F, mh), -1, np.int32)
    for k in ROW_KEYS[1:]:
        out[k] = np.zeros((F, mh))
    for f, r in enumerate(rows):
        d = r["harmonics"]
        if d is None:
            continue
        n = len(d["freqs"])
        out["h_number"][f, :n] = d["numbers"]
        out["h_freq"][f, :n], out["h_ideal"][f, :n], out["h_amp"][f, :n] = d["freqs"], d["ideals"], d["amps"]
        out["h_deviation"][f, :len(r["deviations"])] = r["deviations"]
    return out


def from_spectrum(mag, f0, f0c, p):
    """the arrays of sonar_inharm_from_spectrum"""
    mag = np.atleast_2d(np.asarray(mag, dtype=np.float64))
    return _pack([analyze_spectrum(mag[f], float(f0[f]), float(f0c[f]), p) for f in range(len(mag))], p)


def spectrum(x, fft="numpy"):
    """|X[0 .. W/2 - 1]| of the raw frame (:321-328)"""
    K = len(x) // 2
    re, im = PR._fft(x, fft)
    re, im = re[:K], im[:K]
    return np.sqrt(re * re + im * im)


def detector_f0(pcm, sample_rate, hop):
    """detectFundamentalFrequency (:308-316) over the frames: the default detector's tracked pitch and confidence"""
    r = PR.detect(pcm, PR.Params(sample_rate, hop_size=hop))
    return r["pitch"], r["confidence"]


def frames(pcm, hop, p, fft="numpy"):
    """the arrays of sonar_inharm_frames, plus `magnitude` (the |X| rows of `fft`), `magnitude_other` (of the other
    transform) and `decided`"""
    pcm = np.ascontiguousarray(pcm, dtype=np.float64)
    W = p.window_size
    F = PR.detect_frames(len(pcm), W, hop)
    if F == 0:
        return _pack([], p)
    if W != DETECTOR_WINDOW:
        raise ValueError("audio frame size (%d) doesn't match window size (%d)" % (W, DETECTOR_WINDOW))
    f0, f0c = detector_f0(pcm, p.sample_rate, hop)
    other = "go" if fft == "numpy" else "numpy"
    rows, mags, others, decided = [], [], [], []
    for f in range(F):
        x = pcm[f * hop:f * hop + W]
        m, m2 = spectrum(x, fft), spectrum(x, other)
        beat = beat_of_frame(x) if p.method == BEAT_PATTERN else None
        r = analyze_spectrum(m, float(f0[f]), float(f0c[f]), p, W, beat)
        ok = True
        if r["status"] != INVALID_F0:
            d2 = harmonic_structure(m2, float(f0[f]), p, W)
            d1 = harmonic_structure(m, float(f0[f]), p, W)
            ok = d1["numbers"] == d2["numbers"] and d1["bins"] == d2["bins"]
        rows.append(r); mags.append(m); others.append(m2); decided.append(ok)
    out = _pack(rows, p)
    out["magnitude"], out["magnitude_other"] = np.array(mags), np.array(others)
    out["decided"] = np.array(decided, dtype=bool)
    return out


# ------------------------------------------------------------------ tracking ----
class Tracker:
    """postProcessResult + updateTemporalTracking (:1007-1101) of one analyzer"""

    def __init__(self, p):
        self.p, self.history, self.f0_history = p, [], []

    def step(self, raw, f0):
        p, h, fh = self.p, self.history, self.f0_history
        inh = raw
        if p.use_temporal_tracking and len(h) > 0:
            inh = 0.3 * raw + (1.0 - 0.3) * h[-1]
        stability = trend = f0_stability = 0.0
        if len(h) >= 3:
            m = mean(h)
            if m != 0:
                stability = 1.0 / (1.0 + _div(_sqrt(variance(h)), abs(m)))
            trend = linear_regression_slope([float(i) for i in range(len(h))], h)
        if len(fh) >= 3:
            m = mean(fh)
            if m > 0:
                f0_stability = 1.0 / (1.0 + _sqrt(variance(fh)) / m)
        if p.use_temporal_tracking:
            h.append(inh)
            fh.append(f0)
            keep = p.temporal_window
            if len(h) > keep:
                if keep < 0:
                    raise IndexError("runtime error: slice bounds out of range [%d:%d]" % (len(h) - keep, len(h)))
                del h[:len(h) - keep]
                del fh[:len(fh) - keep]
        return inh, stability, trend, f0_stability


def track(p, raw, f0, status=None):
    """sonar_inharm_track: the rows in order through a fresh Tracker; rows whose status is not OK pass through"""
    t = Tracker(p)
    rows = []
    for f in range(len(raw)):
        if status is None or status[f] == OK:
            rows.append(t.step(float(raw[f]), float(f0[f])))
        else:
            rows.append((float(raw[f]), 0.0, 0.0, 0.0))
    return {k: np.array([r[i] for r in rows], dtype=np.float64)
            for i, k in enumerate(("inharmonicity", "temporal_stability", "inharmonicity_trend", "f0_stability"))}


def sequence(pcm, hop, p, fft="numpy"):
    """AnalyzeSequence over the whole frames of pcm; InsufficientHarmonics where Go returns nil and the error"""
    out = frames(pcm, hop, p, fft)
    for f, s in enumerate(out["status"]):
        if s == INSUFFICIENT:
            e = InsufficientHarmonics(int(out["num_harmonics"][f]), p.min_harmonics)
            e.frame = f
            raise e
    out.update(track(p, out["inharmonicity"], out["f0"], out["status"]))
    return out


def average(inh, conf):
    """GetAverageInharmonicity (:1196-1216)"""
    s, n = 0.0, 0
    for v, c in zip(inh, conf):
        if c > 0.5:
            s += v
            n += 1
    return s / float(n) if n else 0.0


def classify(v):
    """ClassifyInharmonicity (:1272-1286)"""
    a = abs(v)
    return "Very Low" if a < 0.0001 else "Low" if a < 0.001 else "Moderate" if a < 0.005 else "High" if a < 0.01 \
        else "Very High"


def instrument_type(v, f0):
    """EstimateInstrumentType (:1289-1313)"""
    a = abs(v)
    if a > 0.002 and f0 < 500:
        return "Piano/String"
    if a < 0.0005:
        return "Wind/Brass"
    if 0.0005 < a < 0.002:
        return "Plucked String"
    if a < 0.001 and 100 < f0 < 800:
        return "Vocal/Harmonic"
    return "Unknown"
