"""The checker of sonar_hratio_from_spectrum / sonar_hratio_frames / sonar_hratio_track / sonar_hratio: a float64
restatement of the reference's HarmonicRatioAnalyzer for every method of AnalyzeFrame's switch (test
infrastructure, never the product).

  NewHarmonicRatioAnalyzer, AnalyzeFrame, preprocessFrame, computeSpectrum, analyzeHNR, analyzeACF, analyzeHPS,
  analyzeComb, analyzeSpectral, analyzeYin, detectFundamentalFrequency, findHarmonicPeaks, findNearestPeak,
  estimateNoiseFloor, compute{Percentile,Median,Minimum}NoiseFloor, calculatePeriodicity, calculateHarmonicity,
  calculateVoicing, calculateRoughness, calculateSNR, calculatePeriodicityFromACF, estimateF0FromPeaks,
  evaluateF0Candidate, findClosestPeak, isHarmonic, postProcessResult, applyTemporalSmoothing,
  calculateTemporalStability, calculateTemporalCoherence, updateTemporalTracking, createWindowFunction,
  AnalyzeSequence, GetAverageHarmonicRatio, ClassifyHarmonicRatio, EstimateVoicingQuality
                                                          (algorithms/tonal/harmonic_ratio.go:130-1148)
  common.MovingAverage, common.Percentile                (algorithms/common/math.go:38-50, 140-166)

Staged like pitch_ref.py: the spectrum of a frame (`fft` picks numpy's transform or xcorr_params_ref.go_fft, two
independent float64 orderings), then everything after it on |X| rows.  Every sum is a Python loop in Go's
order; int() is Go's truncation (_go_int).  The peak detector is hpcp_ref's restatement of DetectPeaks, the
autocorrelation xcorr_params_ref.autocorr, the temporary detector's YIN pitch_ref's.  gonum is not in the tree:
stat.Quantile(p, Empirical, sorted, nil) is restated from its published rule (the first sorted value whose
count reaches p n), stat.Mean as a sequential sum and stat.Variance as the compensated two-pass form.

Per frame the checker also returns `margin`: the smallest gap of any comparison of magnitudes (or of values
built from them) that decides a discrete outcome, relative to the row's largest smoothed magnitude (or to
the larger of two scores / products).  Those are: the strict-neighbour and min_height tests of the kept peaks;
the f0 pick against the runner-up; of each findNearestPeak the scan's winner against the window's next
value and the neighbour tests of the winner; the order of the five strongest peaks and the best score against
the next in estimateF0FromPeaks; the HPS argmax against the runner-up.  Mask membership, the range tests and
isHarmonic follow from bins and from f0 alone, so the margins above cover them.  A frame whose margin is not
above 1000 x a test's tolerance is undecided there."""
import math
from dataclasses import dataclass

import numpy as np

import hpcp_ref as HP
import pitch_ref as PR
import xcorr_params_ref as X

HNR, ACF, HPS, COMB, SPECTRAL, YIN = range(6)
METHOD_NAMES = ["Harmonic-to-Noise Ratio", "Autocorrelation Function", "Harmonic Product Spectrum", "Comb Filtering",
                "Spectral Peak Analysis", "YIN-based"]
SCALARS = ("harmonic_ratio", "harmonic_energy", "noise_energy", "total_energy", "f0", "f0_confidence", "snr",
           "periodicity", "harmonicity", "voicing", "roughness")
PEAK_DISTANCE_HZ, PEAK_MAX = 20.0, 100                     # NewSpectralPeaks(sr, height, 20.0, 100) :155, :169


@dataclass
class Params:
    """HarmonicRatioParams with NewHarmonicRatioAnalyzer's values (:130-152)"""
    sample_rate: int
    method: int = HNR
    window_size: int = 2048
    hop_size: int = 512
    min_freq: float = 80.0
    max_freq: float = 8000.0
    max_harmonics: int = 20
    harmonic_tolerance: float = 0.1
    min_peak_height: float = 0.001
    peak_detection_width: int = 3
    spectral_smoothing_len: int = 5
    noise_floor_method: str = "percentile"
    noise_floor_percentile: float = 0.1
    noise_floor_smoothing_len: int = 10
    use_temporal_smoothing: bool = True
    temporal_smoothing_len: int = 5
    autocorr_max_lag: int = 2048


def _go_int(q):
    return int(q)                                           # finite and within int32 in every supported call


def _log10(x):
    if x != x or x < 0:
        return math.nan
    return -math.inf if x == 0 else math.inf if x == math.inf else math.log10(x)


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def window(W):
    """createWindowFunction (:1004-1013)"""
    return np.array([0.5 * (1.0 - math.cos(2.0 * math.pi * float(i) / float(W - 1))) for i in range(W)])


def moving_average(data, L):
    """common.MovingAverage (math.go:140-166): a trailing window; the input itself when L <= 0 or L > len"""
    data = [float(v) for v in data]
    n = len(data)
    if n == 0 or L <= 0 or L > n:
        return np.array(data, dtype=np.float64)
    out = [0.0] * n
    for i in range(n):
        s = 0.0
        for j in range(0 if i < L else i - L + 1, i + 1):
            s += data[j]
        out[i] = s / float(i + 1 if i < L else L)
    return np.array(out, dtype=np.float64)


def quantile(sorted_vals, p):
    """gonum stat.Quantile(p, stat.Empirical, x, nil): the first x[i] whose count i + 1 reaches p * len(x)"""
    if not 0 <= p <= 1:
        raise ValueError("stat: percentile out of bounds")
    fidx = p * float(len(sorted_vals))
    for i, v in enumerate(sorted_vals):
        if float(i + 1) >= fidx:
            return v
    raise AssertionError("impossible")


def percentile(data, p):
    """common.Percentile (math.go:38-50)"""
    if len(data) == 0 or p < 0 or p > 1:
        return 0.0
    return quantile(sorted(float(v) for v in data), p)


def noise_floor(mag, p):
    """estimateNoiseFloor (:632-705): the three local estimates over [i - 10, i + 10), then the smoothing"""
    K = len(mag)
    out = np.zeros(K)
    for i in range(K):
        w = mag[max(0, i - 10):min(K, i + 10)]
        if p.noise_floor_method == "median":
            out[i] = percentile(w, 0.5)
        elif p.noise_floor_method == "minimum":
            mn = w[0]
            for v in w:
                if v < mn:
                    mn = v
            out[i] = mn
        else:                                               # "percentile" and every other string
            out[i] = percentile(w, p.noise_floor_percentile)
    if p.noise_floor_smoothing_len > 1:
        out = moving_average(out, p.noise_floor_smoothing_len)
    return out


def spectrum(x, fft="numpy"):
    """computeSpectrum's magnitude and phase (:275-283) of a windowed frame: the first W / 2 bins"""
    K = len(x) // 2
    re, im = PR._fft(x, fft)
    re, im = re[:K], im[:K]
    return np.sqrt(re * re + im * im), np.arctan2(im, re)


def _is_harmonic(freq, f0, p):
    if f0 <= 0:
        return False
    expected = f0 * float(round_half_away(freq / f0))
    return abs(freq - expected) < p.harmonic_tolerance * expected


def round_half_away(x):
    """math.Round"""
    a = abs(x)
    r = math.floor(a)
    if a - r >= 0.5:                                        # exact: a and floor(a) are within a factor of two
        r += 1.0
    return math.copysign(r, x)


class _Frame:
    """hra.magnitude, hra.phase, hra.freqBins and the margin of one frame"""

    def __init__(self, raw, phase, p):
        self.p = p
        self.K = len(raw)
        self.W, self.sr = p.window_size, p.sample_rate
        self.phase = phase
        self.mag = moving_average(raw, p.spectral_smoothing_len) if p.spectral_smoothing_len > 1 else np.array(raw, dtype=np.float64)
        self.freq = [float(i) * float(self.sr) / float(self.W) for i in range(self.K)]       # :195
        self.scale = float(np.max(self.mag)) if self.K and np.max(self.mag) > 0 else 1.0
        self.margin = math.inf

    def gap(self, a, b, scale=None):
        s = self.scale if scale is None else scale
        g = abs(float(a) - float(b)) / s if s > 0 else math.inf
        self.margin = min(self.margin, g)

    def peaks(self):
        """DetectPeaks(hra.magnitude, W) -> [(bin, magnitude, frequency)], magnitude descending, ties by bin"""
        pk = HP.detect_peaks_last_kept(self.mag, self.W, self.sr, self.p.min_peak_height, PEAK_DISTANCE_HZ, PEAK_MAX)
        for b, m, _ in pk:
            self.gap(m, self.mag[b - 1]), self.gap(m, self.mag[b + 1]), self.gap(m, self.p.min_peak_height)
        return pk

    def nearest_peak(self, target):
        """findNearestPeak (:596-630) -> (bin, frequency, magnitude, phase) or None"""
        m, K, w = self.mag, self.K, self.p.peak_detection_width
        tb = _go_int(target * float(self.W) / float(self.sr))
        if tb >= K:
            return None
        mx, mb = 0.0, tb
        lo, hi = max(0, tb - w), min(K, tb + w + 1)
        for i in range(lo, hi):
            if m[i] > mx:
                mx, mb = m[i], i
        others = [m[i] for i in range(lo, hi) if i != mb]
        if others and lo <= mb < hi:
            self.gap(m[mb], max(others))
        if 0 < mb < K - 1:
            self.gap(m[mb], m[mb - 1]), self.gap(m[mb], m[mb + 1])
            if m[mb] > m[mb - 1] and m[mb] > m[mb + 1]:
                return mb, self.freq[mb], float(m[mb]), float(self.phase[mb]) if self.phase is not None else 0.0
        return None

    def harmonic_peaks(self, f0):
        """findHarmonicPeaks (:565-594)"""
        p = self.p
        if f0 <= 0:
            return []
        out = []
        for h in range(1, _go_int(min(float(p.max_harmonics), p.max_freq / f0)) + 1):
            expected = f0 * float(h)
            if expected > p.max_freq:
                break
            pk = self.nearest_peak(expected)
            if pk is not None and abs(pk[1] - expected) < p.harmonic_tolerance * expected:
                out.append(pk)
        return out


def _ratio_db(h, n):
    return 10.0 * _log10(_div(h, n)) if n > 0 else 60.0


def analyze_hnr(fr, floor):
    """analyzeHNR (:297-382)"""
    p, K = fr.p, fr.K
    pk = fr.peaks()
    f0, conf = 0.0, 0.0                                     # detectFundamentalFrequency :546-563
    if pk:
        eligible = [q for q in pk if q[2] >= p.min_freq] or pk      # the walk's first hit, else peaks[0]
        f0, conf = eligible[0][2], eligible[0][1]
        if len(eligible) > 1:
            fr.gap(eligible[0][1], eligible[1][1])
    hp = fr.harmonic_peaks(f0)
    mask = [False] * K
    for _, f, _, _ in hp:
        b = _go_int(f * float(fr.W) / float(fr.sr))
        for i in range(max(0, b - p.peak_detection_width), min(K, b + p.peak_detection_width + 1)):
            mask[i] = True
    he = ne = te = 0.0
    for i in range(K):
        if p.min_freq <= fr.freq[i] <= p.max_freq:
            e = float(fr.mag[i]) * float(fr.mag[i])
            te += e
            if mask[i]:
                he += e
            else:
                ne += e
    ratio = _ratio_db(he, ne)
    periodicity = 0.0                                       # calculatePeriodicity :707-732
    if f0 > 0:
        hs = ts = 0.0
        for i in range(K):
            if p.min_freq <= fr.freq[i] <= p.max_freq:
                ts += float(fr.mag[i])
                if _is_harmonic(fr.freq[i], f0, p):
                    hs += float(fr.mag[i])
        periodicity = hs / ts if ts > 0 else 0.0
    harmonicity = 0.0                                       # calculateHarmonicity :734-757
    if hp and f0 > 0:
        dev = 0.0
        for _, f, _, _ in hp:
            expected = f0 * float(round_half_away(f / f0))
            dev += abs(f - expected) / expected
        harmonicity = math.exp(-(dev / float(len(hp))) * 10.0)
    voicing = 1.0 / (1.0 + math.exp(-0.1 * (ratio - 10.0)))
    rough = 0.0                                             # calculateRoughness :765-791
    for i in range(len(hp)):
        for j in range(i + 1, len(hp)):
            d = abs(hp[i][1] - hp[j][1])
            if d > 0:
                rough += (hp[i][2] * hp[j][2]) / (d + 1.0)
    se = fe = 0.0                                           # calculateSNR :793-814
    for i in range(K):
        if p.min_freq <= fr.freq[i] <= p.max_freq:
            se += float(fr.mag[i]) * float(fr.mag[i])
            fe += float(floor[i]) * float(floor[i])
    snr = 10.0 * _log10(_div(se, fe)) if fe > 0 else 60.0
    return dict(harmonic_ratio=ratio, harmonic_energy=he, noise_energy=ne, total_energy=te, f0=f0, f0_confidence=conf,
                snr=snr, periodicity=periodicity, harmonicity=harmonicity, voicing=voicing, roughness=rough, peaks=hp,
                noise_floor=np.array(floor, dtype=np.float64))


def analyze_hps(fr):
    """analyzeHPS (:413-454)"""
    p, K = fr.p, fr.K
    hps = [float(v) for v in fr.mag]
    for h in range(2, min(5, p.max_harmonics) + 1):
        for i in range(K // h):
            hps[i] *= float(fr.mag[i * h])
    idx, val = 0, hps[0]
    lo = _go_int(p.min_freq * float(fr.W) / float(fr.sr))
    hi = _go_int(p.max_freq * float(fr.W) / float(fr.sr))
    for i in range(lo, min(hi, K)):
        if hps[i] > val:
            val, idx = hps[i], i
    rest = sorted([hps[0]] + [hps[i] for i in range(lo, min(hi, K)) if i != 0], reverse=True)
    if len(rest) > 1:
        fr.gap(rest[0], rest[1], max(abs(rest[0]), abs(rest[1])))
    f0 = fr.freq[idx]
    hp = fr.harmonic_peaks(f0)
    # what a relative error of the magnitudes (in units of the row's peak) moves the winning product by, relatively
    rel = sum(fr.scale / float(fr.mag[idx * h]) if fr.mag[idx * h] > 0 else math.inf
              for h in range(1, min(5, p.max_harmonics) + 1) if h == 1 or idx < K // h)
    return dict(harmonic_ratio=20.0 * _log10(val + 1e-10), f0=f0, peaks=hp, hps_rel=rel)


def analyze_spectral(fr):
    """analyzeSpectral (:463-512)"""
    p = fr.p
    valid = [q for q in fr.peaks() if p.min_freq <= q[2] <= p.max_freq]
    for a, b in zip(valid[:5], valid[1:6]):                 # the order of the candidates
        fr.gap(a[1], b[1])
    f0, best, scores = 0.0, 0.0, []                         # estimateF0FromPeaks :832-863
    for _, _, cand in valid[:5]:
        score = 0.0                                         # evaluateF0Candidate :865-892
        h = 1
        while h <= _go_int(p.max_freq / cand) and h <= p.max_harmonics:
            expected = cand * float(h)
            closest, md = valid[0], abs(valid[0][2] - expected)   # findClosestPeak :894-911
            for q in valid[1:]:
                d = abs(q[2] - expected)
                if d < md:
                    md, closest = d, q
            tolr = p.harmonic_tolerance * expected
            if md < tolr:
                score += (1.0 - md / tolr) * closest[1]
            h += 1
        scores.append(score)
        if score > best:
            best, f0 = score, cand
    top = sorted(scores + [0.0], reverse=True)
    if len(top) > 1:
        fr.gap(top[0], top[1], max(abs(top[0]), abs(top[1])))
    hp = fr.harmonic_peaks(f0)
    he = te = 0.0
    for _, m, f in valid:
        e = m * m
        te += e
        if _is_harmonic(f, f0, p):
            he += e
    ne = te - he
    return dict(harmonic_ratio=_ratio_db(he, ne), harmonic_energy=he, noise_energy=ne, total_energy=te, f0=f0, peaks=hp)


def analyze_spectrum(raw, phase, p):
    """everything AnalyzeFrame does after the transform for HNR, Comb, HPS and Spectral -> dict with `margin`"""
    fr = _Frame(raw, phase, p)
    if p.method == HPS:
        r = analyze_hps(fr)
    elif p.method == SPECTRAL:
        r = analyze_spectral(fr)
    elif p.method in (ACF, YIN):
        raise ValueError("the ACF and YIN methods need the samples")
    else:
        r = analyze_hnr(fr, noise_floor(fr.mag, p))
    r["margin"] = fr.margin
    r["scale"] = fr.scale
    r["magnitude"] = fr.mag
    return r


def analyze_acf(x, p):
    """analyzeACF (:385-411) on the windowed frame"""
    with np.errstate(all="ignore"):
        corr = X.autocorr(x, p.autocorr_max_lag)["corr"]
    mx = 0.0
    for c in corr:
        if abs(c) > mx:
            mx = abs(c)
    mx1 = 0.0
    for c in corr[1:]:
        if abs(c) > mx1:
            mx1 = abs(c)
    return dict(harmonic_ratio=20.0 * _log10(_div(mx, 1.0 - mx + 1e-10)), periodicity=mx1, voicing=mx, margin=math.inf)


def analyze_yin(x, p):
    """analyzeYin (:515-542): a temporary detector with only method, rate, window and range set, on the windowed
    frame, and its postProcessResult on an empty history (min_confidence 0: a negative confidence is gated)"""
    tp = PR.Params(p.sample_rate, method=PR.YIN, window_size=p.window_size, min_freq=p.min_freq, max_freq=p.max_freq,
                   yin_threshold=0.0, autocorr_threshold=0.0, min_confidence=0.0, pre_emphasis=False, window_function="",
                   zero_padding=0, median_filter=0, temporal_smoothing=False, octave_correction=False)
    raw = PR.detect_frame(x, tp)
    row = PR.Tracker(tp).step(raw["pitch"], raw["confidence"], raw["n_candidates"], 0.0)
    return dict(harmonic_ratio=20.0 * _log10(row["confidence"] + 1e-10), f0=row["pitch"], f0_confidence=row["confidence"],
                periodicity=row["periodicity"], voicing=row["voicing"], margin=math.inf)


def analyze_frame(frame, p, win=None, fft="numpy"):
    """AnalyzeFrame up to postProcessResult on one frame of window_size samples"""
    if len(frame) != p.window_size:
        raise ValueError("audio frame size (%d) doesn't match window size (%d)" % (len(frame), p.window_size))
    x = np.array(frame, dtype=np.float64) * (window(len(frame)) if win is None else win)
    if p.method == ACF:
        return analyze_acf(x, p)
    if p.method == YIN:
        return analyze_yin(x, p)
    raw, phase = spectrum(x, fft)
    r = analyze_spectrum(raw, phase, p)
    r["raw_magnitude"] = raw
    return r


def _pack(rows, p, K):
    """the arrays of the entries from per-frame dicts; what a method leaves unset is 0"""
    F, mh = len(rows), max(p.max_harmonics, 0)
    out = {k: np.array([r.get(k, 0.0) for r in rows], dtype=np.float64) for k in SCALARS}
    out["num_harmonics"] = np.array([len(r.get("peaks", ())) for r in rows], dtype=np.int32)
    out["h_bin"] = np.full((F, mh), -1, dtype=np.int32)
    for k in ("h_freq", "h_amp", "h_phase"):
        out[k] = np.zeros((F, mh))
    out["noise_floor"] = np.zeros((F, K))
    for f, r in enumerate(rows):
        for s, (b, fq, m, ph) in enumerate(r.get("peaks", ())):
            out["h_bin"][f, s], out["h_freq"][f, s], out["h_amp"][f, s], out["h_phase"][f, s] = b, fq, m, ph
        if "noise_floor" in r:
            out["noise_floor"][f] = r["noise_floor"]
    out["margin"] = np.array([r["margin"] for r in rows], dtype=np.float64)
    out["scale"] = np.array([r.get("scale", 1.0) for r in rows], dtype=np.float64)
    out["hps_rel"] = np.array([r.get("hps_rel", 0.0) for r in rows], dtype=np.float64)
    return out


def from_spectrum(mag, phase, p):
    """the arrays of sonar_hratio_from_spectrum, plus `margin` and `scale` per frame"""
    mag = np.atleast_2d(np.asarray(mag, dtype=np.float64))
    rows = [analyze_spectrum(mag[f], None if phase is None else phase[f], p) for f in range(len(mag))]
    return _pack(rows, p, mag.shape[1])


def frames(pcm, p, fft="numpy"):
    """the arrays of sonar_hratio_frames, plus `margin`, `scale` and, for the spectral methods, the raw |X| rows
    (`raw_magnitude`) and their phases (`raw_phase`)"""
    pcm = np.ascontiguousarray(pcm, dtype=np.float64)
    W, H = p.window_size, p.hop_size
    F = PR.detect_frames(len(pcm), W, H)
    win = window(W)
    rows = [analyze_frame(pcm[f * H:f * H + W], p, win, fft) for f in range(F)]
    out = _pack(rows, p, W // 2)
    if p.method not in (ACF, YIN):
        out["raw_magnitude"] = np.array([r["raw_magnitude"] for r in rows], dtype=np.float64).reshape(F, W // 2)
    return out


# ------------------------------------------------------------------ tracking ----
def gonum_variance(x):
    """stat.Variance(x, nil): the compensated two-pass form, n - 1"""
    n = len(x)
    s = 0.0
    for v in x:
        s += v
    mean = s / float(n)
    ss = comp = 0.0
    for v in x:
        d = v - mean
        ss += d * d
        comp += d
    return (ss - comp * comp / float(n)) / float(n - 1)


class Tracker:
    """postProcessResult + updateTemporalTracking (:926-1002) of one analyzer"""

    def __init__(self, p):
        self.p, self.history, self.previous = p, [], 0.0

    def step(self, raw):
        p, h = self.p, self.history
        ratio = raw
        if p.use_temporal_smoothing and len(h) > 0:
            ratio = 0.3 * raw + (1.0 - 0.3) * self.previous
        stability = coherence = 0.0
        if len(h) >= 3:
            s = 0.0
            for v in h:
                s += v
            mean = s / float(len(h))
            if mean > 0:
                q = 1.0 - math.sqrt(gonum_variance(h)) / mean
                stability = q if q != q else max(0.0, q)
        if len(h) >= 2:
            total = 0.0
            for i in range(1, len(h)):
                total += abs(h[i] - h[i - 1])
            coherence = math.exp(-(total / float(len(h) - 1)) / 10.0)
        h.append(ratio)
        keep = p.temporal_smoothing_len * 2
        if len(h) > keep:
            if keep < 0:
                raise IndexError("runtime error: slice bounds out of range [%d:%d]" % (len(h) - keep, len(h)))
            del h[:len(h) - keep]
        self.previous = ratio
        return ratio, stability, coherence


def track(p, raw_ratio):
    """sonar_hratio_track: the rows in order through a fresh Tracker -> dict of arrays"""
    t = Tracker(p)
    rows = [t.step(float(r)) for r in raw_ratio]
    return {k: np.array([r[i] for r in rows], dtype=np.float64)
            for i, k in enumerate(("harmonic_ratio", "temporal_stability", "temporal_coherence"))}


def sequence(pcm, p, fft="numpy"):
    """AnalyzeSequence over the whole frames of pcm"""
    out = frames(pcm, p, fft)
    out.update(track(p, out["harmonic_ratio"]))
    return out


def average(ratios):
    """GetAverageHarmonicRatio (:1057-1077)"""
    s, n = 0.0, 0
    for r in ratios:
        if r > -60.0:
            s += r
            n += 1
    return s / float(n) if n else 0.0


def classify(r):
    """ClassifyHarmonicRatio (:1130-1142)"""
    return "Very High" if r >= 20.0 else "High" if r >= 10.0 else "Medium" if r >= 5.0 else "Low" if r >= 0.0 else "Very Low"


def voicing_quality(r):
    """EstimateVoicingQuality (:1145-1148)"""
    return 1.0 / (1.0 + math.exp(-0.1 * (r - 5.0)))
