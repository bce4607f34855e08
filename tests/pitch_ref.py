"""The checker of sonar_pitch_frames_raw / sonar_pitch_track / sonar_pitch_detect / sonar_pitch_stability: a
float64 restatement of the reference's PitchDetector for every method of DetectPitch's switch (test
infrastructure, never the product).

  NewPitchDetector, DetectPitch, preprocessFrame, applyPreEmphasis, createWindowFunction, detectPitchYin,
  detectPitchACF, detectPitchNSDF, detectPitchHPS, detectPitchCepstrum, detectPitchPeaks,
  detectPitchZeroCrossing, detectPitchYinFFT, detectPitchMPM, parabolicInterpolation, postProcessResult,
  applyOctaveCorrection, calculateClarity, calculateStrength, calculateSalience, updateTemporalTracking,
  applyTemporalSmoothing, calculateStability, getRecentPitches, calculateMedian, ProcessAudioStream,
  AnalyzePitchStability, estimateVibratoRate        (algorithms/tonal/pitch_detection.go:159-1160)

Sums are np.add.accumulate from 0.0 (strictly sequential, Go's index order); elementwise numpy *, +, -, / are
unfused and correctly rounded.  The ACF is xcorr_params_ref.autocorr (AutoCorrelation.Compute).  The HPS
and the cepstrum go through go-dsp's FFT in the reference, whose source is not in the tree: `fft` picks
numpy's transform (the default) or xcorr_params_ref.go_fft, two independent float64 orderings whose
difference is the measured tolerance of the GPU tests.

Go's sort.Slice is not stable, so candidates of equal confidence have no defined order in the
reference; here (and in the library) they are ordered by ascending lag, and `ties` reports whether a
frame had any."""
import math
from dataclasses import dataclass

import numpy as np

import xcorr_params_ref as X

YIN, ACF, NSDF, HPS, CEPSTRUM, PEAKS, ZERO_CROSSING, PEAK_PICKING, YIN_FFT, MPM, PRAAT = range(11)
WINDOWS = {"hann": 0, "hamming": 1, "blackman": 2, "rectangular": 3}
TRACK_FIELDS = ("pitch", "confidence", "voicing", "periodicity", "clarity", "strength", "salience", "stability",
                "f0_multiple")
STABILITY_KEYS = ("mean_pitch", "pitch_std_dev", "coefficient_of_variation", "jitter", "stability", "vibrato_rate",
                  "voiced_frames_ratio")


@dataclass
class Params:
    """PitchDetectionParams with NewPitchDetector's values (:159-181)"""
    sample_rate: int
    method: int = YIN
    window_size: int = 1024
    hop_size: int = 512
    min_freq: float = 80.0
    max_freq: float = 1000.0
    yin_threshold: float = 0.15
    autocorr_threshold: float = 0.3
    min_confidence: float = 0.5
    pre_emphasis: bool = True
    window_function: str = "hann"
    zero_padding: int = 2
    median_filter: int = 3
    temporal_smoothing: bool = True
    octave_correction: bool = True


def make_signal(F, W, H, seed, sample_rate=16000):
    """The signal of the pitch tests: exactly F whole frames ((F - 1) H + W samples); every stretch of H
    samples has its own f0 from 90-900 Hz, six partials of amplitude 0.7^h, plus 0.05 of noise."""
    rng = np.random.default_rng(seed)
    n = (F - 1) * H + W
    i = np.arange(n, dtype=np.float64)
    f0 = rng.uniform(90.0, 900.0, n // H + 1)[(np.arange(n) // H)]
    x = 0.05 * rng.standard_normal(n)
    for h in range(1, 7):
        x += 0.7 ** h * np.sin(2.0 * np.pi * h * f0 * i / sample_rate)
    return x


def _rowsum(M):
    """per row: s := 0.0; for _, v := range row { s += v }"""
    M = np.atleast_2d(M)
    return np.add.accumulate(np.concatenate((np.zeros((M.shape[0], 1)), M), axis=1), axis=1)[:, -1]


def window(kind, W):
    """createWindowFunction (:317-345); every unknown name is Hann"""
    d = float(W - 1)
    w = np.zeros(W)
    for i in range(W):
        x = float(i)
        if kind == "hamming":
            w[i] = 0.54 - 0.46 * math.cos(2.0 * math.pi * x / d)
        elif kind == "blackman":
            w[i] = 0.42 - 0.5 * math.cos(2.0 * math.pi * x / d) + 0.08 * math.cos(4.0 * math.pi * x / d)
        elif kind == "rectangular":
            w[i] = 1.0
        else:
            w[i] = 0.5 * (1.0 - math.cos(2.0 * math.pi * x / d))
    return w


def preprocess(frame, p, win=None):
    """preprocessFrame (:282-314): a fresh pre-emphasis of the frame, then the window"""
    x = np.array(frame, dtype=np.float64)
    if p.pre_emphasis and len(x):
        y = x.copy()
        y[1:] = x[1:] - 0.97 * x[:-1]
        x = y
    return x * (window(p.window_function, len(x)) if win is None else win)


def _lag_matrix(x):
    h = len(x) // 2
    return np.lib.stride_tricks.sliding_window_view(x, h)[:h]     # [tau, j] = x[j + tau]


def _single(pitch, conf, index, n, curve):
    return {"pitch": pitch, "confidence": conf, "index": index, "n_candidates": n,
            "candidates": [(index, conf)] if n else [], "curve": curve, "ties": False}


def yin(x, p):
    """detectPitchYin (:349-420)"""
    h = len(x) // 2
    with np.errstate(all="ignore"):
        d = x[None, :h] - _lag_matrix(x)
        diff = _rowsum(d * d)
        cm = np.ones(h)
        run = np.add.accumulate(np.concatenate(([0.0], diff[1:])))[1:]
        cm[1:] = diff[1:] / (run / np.arange(1, h, dtype=np.float64))
        hit = np.nonzero((cm[1:h - 1] < p.yin_threshold) & (cm[1:h - 1] < cm[2:h]))[0]
        if len(hit) == 0:
            return _single(0.0, 0.0, -1, 0, cm)
        t = int(hit[0]) + 1
        period = float(t)
        if 0 < t < h - 1:                                         # parabolicInterpolation :743-764
            y1, y2, y3 = cm[t - 1], cm[t], cm[t + 1]
            a = (y1 - 2 * y2 + y3) / 2
            b = (y3 - y1) / 2
            if a != 0:
                period = float(t) + float(-b / (2 * a))
        f = float(np.float64(p.sample_rate) / np.float64(period))
        if p.min_freq <= f <= p.max_freq:
            return _single(f, float(1.0 - cm[t]), t, 1, cm)
        return _single(0.0, 0.0, t, 0, cm)


def _peaks(cv, lo, hi, lag0, p):
    """strict local maxima above the threshold at lo <= i <= hi whose frequency is in range, by
    descending confidence (ties: ascending lag) -> (list of (lag, conf), ties)"""
    i = np.arange(lo, hi + 1)
    with np.errstate(all="ignore"):
        ok = (cv[i] > cv[i - 1]) & (cv[i] > cv[i + 1]) & (cv[i] > p.autocorr_threshold)
        f = np.float64(p.sample_rate) / (i - lag0).astype(np.float64)
    ok &= (f >= p.min_freq) & (f <= p.max_freq)
    idx = i[ok]
    cand = sorted(((int(k - lag0), float(cv[k])) for k in idx), key=lambda c: (-c[1], c[0]))
    confs = [c[1] for c in cand]
    return cand, len(set(confs)) != len(confs)


def _multi(cand, ties, curve, p):
    if not cand:
        return {"pitch": 0.0, "confidence": 0.0, "index": -1, "n_candidates": 0, "candidates": [], "curve": curve,
                "ties": False}
    lag, conf = cand[0]
    return {"pitch": float(np.float64(p.sample_rate) / np.float64(lag)), "confidence": conf, "index": lag,
            "n_candidates": len(cand), "candidates": cand, "curve": curve, "ties": ties}


def nsdf(x, p):
    """detectPitchNSDF (:485-550)"""
    h = len(x) // 2
    with np.errstate(all="ignore"):
        x2 = _lag_matrix(x)
        acf = _rowsum(x[None, :h] * x2)
        m1 = _rowsum(x[:h] * x[:h])[0]
        m2 = _rowsum(x2 * x2)
        den = m1 + m2
        cv = np.where(den > 0, 2.0 * acf / den, 0.0)
    cand, ties = _peaks(cv, 1, h - 2, 0, p)
    return _multi(cand, ties, cv, p)


def acf(x, p):
    """detectPitchACF (:423-482) over NewAutoCorrelation(2 W).Compute (useFFT: the regime follows W)"""
    W = len(x)
    with np.errstate(all="ignore"):
        cv = X.autocorr(x, 2 * W)["corr"]
    L = W - 1
    cand, ties = _peaks(cv, L + 1, 2 * W - 3, L, p)
    return _multi(cand, ties, cv, p)


def _fft(re, fft):
    if fft == "go":
        return X.go_fft(np.array(re, dtype=np.float64), np.zeros(len(re)))
    s = np.fft.fft(re)
    return s.real.copy(), s.imag.copy()


def _go_int(q):
    return int(q)                                                   # finite, >= 0 in every supported call


def hps(x, p, fft="numpy"):
    """detectPitchHPS (:553-620)"""
    W = len(x)
    N = W * p.zero_padding
    padded = np.zeros(N)
    padded[:W] = x
    with np.errstate(all="ignore"):
        re, im = _fft(padded, fft)
        n = N // 2
        mag = np.sqrt(re[:n] * re[:n] + im[:n] * im[:n])
        cv = mag.copy()
        for h in range(2, 6):
            k = n // h
            cv[:k] = cv[:k] * mag[::h][:k]
    lo = _go_int(p.min_freq * float(N) / float(p.sample_rate))
    hi = _go_int(p.max_freq * float(N) / float(p.sample_rate))
    idx, val = 0, cv[0]
    for i in range(lo, min(hi, n)):
        if cv[i] > val:
            val, idx = cv[i], i
    f = float(idx) * float(p.sample_rate) / float(N)
    conf = min(float(val) / 1000.0, 1.0) if val > 0 else 0.0
    return _single(f, conf, idx, 1, cv)


def cepstrum(x, p, fft="numpy"):
    """detectPitchCepstrum (:623-684)"""
    W = len(x)
    with np.errstate(all="ignore"):
        re, im = _fft(x, fft)
        lm = np.log(np.hypot(re, im) + 1e-10)
        cr, _ = _fft(lm, fft)                                       # ifft of a real input: re(fft) / W
        cv = cr / float(W)
    lo = _go_int(float(p.sample_rate) / p.max_freq)
    hi = _go_int(float(p.sample_rate) / p.min_freq)
    idx, val = lo, cv[lo]
    for i in range(lo, min(hi, W)):
        if cv[i] > val:
            val, idx = cv[i], i
    with np.errstate(all="ignore"):
        f = float(np.float64(p.sample_rate) / np.float64(idx))
        q = float(np.float64(val) / np.float64(0.1))
    conf = q if q != q else min(q, 1.0)                             # math.Min: NaN stays
    return _single(f, conf, idx, 1, cv)


def zero_crossing(x, p):
    """detectPitchZeroCrossing (:694-727)"""
    a, b = x[1:], x[:-1]
    n = int(np.count_nonzero(((a > 0) & (b <= 0)) | ((a <= 0) & (b > 0))))
    f = float(n) * float(p.sample_rate) / (2.0 * float(len(x)))
    return _single(f, 0.3, n, 1, np.zeros(0))


_DISPATCH = {YIN: yin, YIN_FFT: yin, ACF: acf, NSDF: nsdf, MPM: nsdf, ZERO_CROSSING: zero_crossing}


def detect_frame(frame, p, win=None, fft="numpy"):
    """DetectPitch up to postProcessResult on one frame of window_size samples"""
    if len(frame) != p.window_size:
        raise ValueError("audio frame size (%d) doesn't match window size (%d)" % (len(frame), p.window_size))
    x = preprocess(frame, p, win)
    if p.method in (HPS, PEAKS):
        return hps(x, p, fft)
    if p.method == CEPSTRUM:
        return cepstrum(x, p, fft)
    if p.method not in _DISPATCH:
        raise ValueError("unsupported pitch detection method: %d" % p.method)
    return _DISPATCH[p.method](x, p)


def detect_frames(n, W, H):
    return 0 if n < W else (n - W) // H + 1


def frames_raw(pcm, p, max_candidates=8, fft="numpy"):
    """the arrays of sonar_pitch_frames_raw, plus `ties` per frame"""
    pcm = np.ascontiguousarray(pcm, dtype=np.float64)
    W, H, K = p.window_size, p.hop_size, max_candidates
    F = detect_frames(len(pcm), W, H)
    win = window(p.window_function, W)
    rows = [detect_frame(pcm[f * H:f * H + W], p, win, fft) for f in range(F)]
    out = {"pitch": np.array([r["pitch"] for r in rows], dtype=np.float64),
           "confidence": np.array([r["confidence"] for r in rows], dtype=np.float64),
           "index": np.array([r["index"] for r in rows], dtype=np.int32),
           "n_candidates": np.array([r["n_candidates"] for r in rows], dtype=np.int32),
           "second_confidence": np.array([r["candidates"][1][1] if len(r["candidates"]) > 1 else 0.0 for r in rows],
                                         dtype=np.float64),
           "cand_index": np.full((F, K), -1, dtype=np.int32), "cand_conf": np.zeros((F, K)),
           "ties": np.array([r["ties"] for r in rows], dtype=bool)}
    for f, r in enumerate(rows):
        for k, (i, c) in enumerate(r["candidates"][:K]):
            out["cand_index"][f, k], out["cand_conf"][f, k] = i, c
    width = len(rows[0]["curve"]) if rows else 0
    out["curve"] = np.array([r["curve"] for r in rows], dtype=np.float64).reshape(F, width)
    return out


# ------------------------------------------------------------------ tracking ----
def _median(values):
    """calculateMedian (:978-1007): of the positive values"""
    s = sorted(v for v in values if v > 0)
    if not s:
        return 0.0
    n = len(s)
    return (s[n // 2 - 1] + s[n // 2]) / 2.0 if n % 2 == 0 else s[n // 2]


class Tracker:
    """postProcessResult + updateTemporalTracking (:767-963) of one detector"""

    def __init__(self, p):
        self.p = p
        self.history = []
        self.previous = 0.0

    def _recent(self, count):
        if count <= 0 or not self.history:
            return []
        return self.history[max(len(self.history) - count, 0):]

    def step(self, raw_pitch, raw_conf, n_candidates, second_conf):
        p = self.p
        pitch, conf, voicing, periodicity, f0m = raw_pitch, raw_conf, raw_conf, raw_conf, 0.0
        if p.octave_correction and pitch != 0.0 and self.history:          # applyOctaveCorrection
            recent = self._recent(5)
            if len(recent) >= 3:
                med = _median(recent)
                for ratio in (0.5, 2.0, 1.0 / 3.0, 3.0):
                    ex = med * ratio
                    with np.errstate(all="ignore"):
                        near = float(np.float64(abs(pitch - ex)) / np.float64(ex)) < 0.1
                    if near:
                        if abs(pitch - med) > abs(ex - med):
                            pitch, f0m = ex, ratio
                        break
        clarity = 0.0                                                      # calculateClarity
        if n_candidates == 1:
            clarity = raw_conf
        elif n_candidates > 1 and raw_conf > 0:
            clarity = (raw_conf - second_conf) / raw_conf
        strength = (periodicity + voicing) / 2.0
        base = conf                                                        # calculateSalience
        if 200 <= pitch <= 800:
            base *= 1.2
        if pitch < 100 or pitch > 1000:
            base *= 0.8
        salience = base if base != base else min(base, 1.0)
        if conf < p.min_confidence:
            pitch, conf, voicing = 0.0, 0.0, 0.0
        self.history.append(pitch)                                         # updateTemporalTracking
        if len(self.history) > 20:
            self.history = self.history[-20:]
        if p.temporal_smoothing and len(self.history) > 1:
            recent = self._recent(p.median_filter) if p.median_filter > 0 else []
            if len(recent) >= 3:
                pitch = _median(recent)
            else:
                pitch = 0.3 * pitch + (1 - 0.3) * self.previous
        stability = self._stability()
        self.previous = pitch
        return dict(zip(TRACK_FIELDS, (pitch, conf, voicing, periodicity, clarity, strength, salience, stability, f0m)))

    def _stability(self):
        if len(self.history) < 3:
            return 0.0
        v = [x for x in self.history if x > 0]
        if len(v) < 2:
            return 0.0
        mean = 0.0
        for x in v:
            mean += x
        mean /= float(len(v))
        var = 0.0
        for x in v:
            var += (x - mean) * (x - mean)
        var /= float(len(v) - 1)
        if mean > 0:
            r = 1.0 - math.sqrt(var) / mean
            return r if r != r else max(0.0, r)
        return 0.0


def track(p, raw_pitch, raw_conf, n_candidates, second_conf):
    """sonar_pitch_track: the rows in order through a fresh Tracker -> dict of arrays"""
    t = Tracker(p)
    rows = [t.step(float(a), float(b), int(c), float(d)) for a, b, c, d in zip(raw_pitch, raw_conf, n_candidates,
                                                                             second_conf)]
    return {k: np.array([r[k] for r in rows], dtype=np.float64) for k in TRACK_FIELDS}


def detect(pcm, p, fft="numpy"):
    """ProcessAudioStream over the whole frames of pcm"""
    r = frames_raw(pcm, p, 2, fft)
    return track(p, r["pitch"], r["confidence"], r["n_candidates"], r["second_confidence"])


def stability(seq, sample_rate, hop_size):
    """AnalyzePitchStability + estimateVibratoRate (:1059-1160) -> dict, {} for Go's empty map"""
    if len(seq) < 2:
        return {}
    v = [float(x) for x in seq if x > 0]
    if len(v) < 2:
        return {}
    mean = 0.0
    for x in v:
        mean += x
    mean /= float(len(v))
    var = 0.0
    for x in v:
        var += (x - mean) * (x - mean)
    var /= float(len(v) - 1)
    sd = math.sqrt(var)
    jitter = 0.0
    for i in range(1, len(v)):
        jitter += abs(v[i] - v[i - 1])
    jitter /= float(len(v) - 1)
    vib = 0.0
    if len(v) >= 10:
        n = float(len(v))
        sx = n * (n - 1) / 2
        sx2 = (n - 1) * n * (2 * n - 1) / 6
        sy = sxy = 0.0
        for i, x in enumerate(v):
            sy += x
            sxy += float(i) * x
        slope = (n * sxy - sx * sy) / (n * sx2 - sx * sx)
        icpt = (sy - slope * sx) / n
        det = [x - (icpt + slope * float(i)) for i, x in enumerate(v)]
        cross = sum(1 for i in range(1, len(det)) if (det[i] > 0 and det[i - 1] <= 0) or (det[i] <= 0 and det[i - 1] > 0))
        vib = float(cross) / (2.0 * n / (float(sample_rate) / float(hop_size)))
    return dict(zip(STABILITY_KEYS, (mean, sd, sd / mean, jitter, 1.0 / (1.0 + sd / mean), vib,
                                     float(len(v)) / float(len(seq)))))
