"""Plain-Python restatement of the scalar host tails of three extractors, and of the music extractor's plan:

  music    MusicFeatureExtractor.ExtractFeatures (fingerprint/extractors/music.go): Go's int(float64), the
           spectral contrast's band edges, gonum's variance, crest factors, energy entropy with the loudness
           range, and the two places where Go panics with the arguments its runtime message names;
  content  ContentDetector.extractAcousticFeatures and classifyFromFeatures (fingerprint/content_detector.go);
  voice    VoiceQualityAnalyzer.AnalyzeVoiceQuality (algorithms/speech/voice_quality.go): the period walk
           behind the PitchDetector's temporal tracking (pitch_detection.go:767-921) and the scalar formulas.

Written from their behaviour, with sequential float loops: Python's float is an IEEE double, its + - * / and
math.sqrt round once, and math.log10 / math.log2 / math.pow are the C library's, so every value here has the
bits the library's tail computes.  Arrays are lists of floats.  test_extractor_tail_cpu.py pins this file to
answers worked out by hand."""
import math

from speech_tail_ref import go_div

MIN_INT64 = -(1 << 63)
CT_MUSIC, CT_NEWS, CT_SPORTS, CT_TALK, CT_MIXED, CT_UNKNOWN = range(6)   # SONAR_CT_*


def go_max(x, y):
    """math.Max: +Inf wins, then NaN propagates."""
    if x == math.inf or y == math.inf:
        return math.inf
    if math.isnan(x) or math.isnan(y):
        return math.nan
    return x if x > y else y


def go_min(x, y):
    if x == -math.inf or y == -math.inf:
        return -math.inf
    if math.isnan(x) or math.isnan(y):
        return math.nan
    return x if x < y else y


def c_round(r):
    """round() of C: halves away from zero (r >= 0 here)."""
    fl = math.floor(r)
    return fl + 1.0 if r - fl >= 0.5 else float(fl)


# ---- music ------------------------------------------------------------------------------------------

def go_int(x):
    """Go's int(float64) on amd64: NaN and anything outside int64 give the smallest int64."""
    if math.isnan(x) or not (-9.2233720368547758e18 <= x < 9.2233720368547758e18):
        return MIN_INT64
    return int(x)


def contrast_edges(sample_rate, K, nb):
    """SpectralContrast.initializeBands: nb log-spaced bands from 200 Hz to Nyquist as nb + 1 strictly rising bins."""
    nyquist = float(sample_rate) / 2.0
    minf = 200.0
    maxf = nyquist
    if maxf <= minf:
        maxf = minf * 2
    lmin, lmax = math.log10(minf), math.log10(maxf)
    step = (lmax - lmin) / float(nb)
    e = []
    for i in range(nb + 1):
        f = math.pow(10.0, lmin + float(i) * step)
        b = go_int(go_div(f * float(K - 1), nyquist))
        if b >= K:
            b = K - 1
        if b < 0:
            b = 0
        e.append(b)
    for i in range(1, nb + 1):
        if e[i] <= e[i - 1]:
            e[i] = e[i - 1] + 1
    return e


def gonum_variance(x):
    """stat.Variance(x, nil): two passes, the second compensated, over n - 1; 0 below two values."""
    n = len(x)
    if n < 2:
        return 0.0
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


def crest_factors(peaks, energy):
    return [p / e if e > 0 else 0.0 for p, e in zip(peaks, energy)]


def energy_entropy(energy):
    """(-e log2 e per frame, 20 log10(largest / smallest positive energy) or 0 without a positive one)."""
    ent = []
    mx, mn = 0.0, math.inf
    for e in energy:
        ent.append(-e * math.log2(e) if e > 0 else 0.0)
        if e > mx:
            mx = e
        if e < mn and e > 0:
            mn = e
    return ent, (20 * math.log10(mx / mn) if mn != math.inf and mn > 0 else 0.0)


def chroma_slice_panics(F, hop, n):
    """The first chroma frame whose slice [f hop : ...] starts past the n samples, or None (hop > 0)."""
    return n // hop + 1 if (F - 1) * hop > n else None


def percentile_panics(n):
    """(index, L): sorted[int(10 (L - 1))] of the L RMS frames 1024 / 512; index is None where Go does not panic."""
    L = (n - 1024) // 512 + 1 if n >= 1024 else 0
    return (go_int(10.0 * float(L - 1)) if L >= 2 else None), L


def music_plan(n, F, W, rate, window, hop):
    """The formulas of sonar_extract_music_features, as they stood inline before MusicPlan."""
    K = W // 2 + 1
    edges = contrast_edges(rate, K, 6)
    maxband = 1
    for b in range(6):
        maxband = max(maxband, min(edges[b + 1], K) - edges[b])
    L = (n - 1024) // 512 + 1 if n >= 1024 else 0
    plan = dict(F=F, K=K, chroma_bad=-1, Fe=0, fse=0, Fenv=0, harmonic_live=0, L=L,
                pct_index=go_int(10.0 * float(L - 1)) if L >= 2 else 0, edges=edges, maxband=maxband)
    if hop <= 0:
        return plan
    if (F - 1) * hop > n:
        plan["chroma_bad"] = n // hop + 1
        return plan
    Fe = 0 if (n < window or window <= 0) else (n - window) // hop + 1
    fse = n // Fe if Fe > 0 else 0
    plan.update(Fe=Fe, fse=fse, Fenv=(n - fse) // hop + 1 if (Fe > 0 and fse > 0 and n >= fse) else 0,
                harmonic_live=int((n // F if F > 0 else 0) == 1024 and n < 1536))
    return plan


# ---- content ----------------------------------------------------------------------------------------

def content_features(crossings, mx, mn, spec, esum, tsum, n, sr):
    """spec: |DFT| of the first min(2048, n) samples; esum: sums of squares of frames 1024 / 512; tsum: of
    frames of sr / 10 samples; crossings, mx, mn: sign changes and the extrema of |x| over the signal."""
    K, fe, ft = len(spec), len(esum), len(tsum)
    f = dict.fromkeys(("zero_crossing_rate", "spectral_centroid", "energy_variance", "silence_ratio", "harmonic_ratio",
                       "low_freq_energy", "high_freq_energy", "dynamic_range", "temporal_stability",
                       "classification_confidence"), 0.0)
    f["zero_crossing_rate"] = 0.0 if n <= 1 else float(crossings) / float(n - 1)
    ws = ms = 0.0
    for i in range(K):
        fr = float(i) * float(sr) / float(K * 2)
        ws += fr * spec[i]
        ms += spec[i]
    f["spectral_centroid"] = 0.0 if ms == 0 else ws / ms
    if n >= 2048 and fe > 1:
        mean = 0.0
        for e in esum:
            mean += e / 1024.0
        mean /= float(fe)
        var = 0.0
        for e in esum:
            d = e / 1024.0 - mean
            var += d * d
        f["energy_variance"] = var / float(fe)
    if fe > 0:
        silent = 0
        for e in esum:
            if math.sqrt(e / 1024.0) < 0.01:
                silent += 1
        f["silence_ratio"] = float(silent) / float(fe)
    f["dynamic_range"] = 0.0 if (mn == 0 or math.isinf(mn)) else 20.0 * math.log10(mx / mn)
    split = K // 4
    lo = hi = 0.0
    for i in range(min(split, K)):
        lo += spec[i] * spec[i]
    for i in range(split, K):
        hi += spec[i] * spec[i]
    tot = lo + hi
    if tot != 0:
        f["low_freq_energy"], f["high_freq_energy"] = lo / tot, hi / tot
    if K >= 10:
        peaks = [i for i in range(2, K - 2)
                 if spec[i] > spec[i - 1] and spec[i] > spec[i + 1] and spec[i] > spec[i - 2] and spec[i] > spec[i + 2]]
        if len(peaks) >= 2:
            harm = 0
            for q in peaks[1:]:
                r = float(q) / float(peaks[0])
                if abs(r - c_round(r)) < 0.1:
                    harm += 1
            f["harmonic_ratio"] = float(harm) / float(len(peaks) - 1)
    ts = sr // 10
    if n >= 3 * ts and ft > 1:
        mean = 0.0
        for t in tsum:
            mean += t
        mean /= float(ft)
        if mean != 0:
            var = 0.0
            for t in tsum:
                d = t - mean
                var += d * d
            var /= float(ft)
            f["temporal_stability"] = go_max(0.0, 1.0 - math.sqrt(var) / mean)
    return f


def classify_content(f, thr):
    """(type, confidence): the first score strictly above thr and above those before it, in the order music,
    news, talk, sports; the confidence is that score, or thr, over 6."""
    music = speech = sports = 0.0
    if f["zero_crossing_rate"] < 0.1:
        music += 2.0
    if f["harmonic_ratio"] > 0.3:
        music += 2.0
    if f["temporal_stability"] > 0.5:
        music += 1.0
    if f["dynamic_range"] > 20:
        music += 1.0
    if 0.05 < f["zero_crossing_rate"] < 0.3:
        speech += 2.0
    if 800 < f["spectral_centroid"] < 3000:
        speech += 2.0
    if f["harmonic_ratio"] < 0.2:
        speech += 1.0
    if 0.1 < f["silence_ratio"] < 0.4:
        speech += 1.0
    if f["energy_variance"] > 0.3:
        sports += 2.0
    if f["dynamic_range"] > 30:
        sports += 1.5
    if f["temporal_stability"] < 0.4:
        sports += 1.0
    best, bs = CT_UNKNOWN, thr
    for t, s in ((CT_MUSIC, music), (CT_NEWS, speech), (CT_TALK, speech * 0.9), (CT_SPORTS, sports)):
        if s > bs:
            bs, best = s, t
    return best, bs / 6.0


# ---- voice ------------------------------------------------------------------------------------------

def _median_positive(v):
    pos = sorted(x for x in v if x > 0)
    m = len(pos)
    if m == 0:
        return 0.0
    return (pos[m // 2 - 1] + pos[m // 2]) / 2.0 if m % 2 == 0 else pos[m // 2]


class YinTracker:
    """PitchDetector's post-processing of one raw YIN frame after another: octave correction against the
    median of the last five pitches, the confidence floor 0.5, a history of 20, smoothing over the last three."""

    def __init__(self):
        self.hist, self.prev = [], 0.0

    def step(self, pitch, conf):
        p, c, v = pitch, conf, conf
        if p != 0.0 and self.hist:
            last = self.hist[-5:]
            if len(last) >= 3:
                med = _median_positive(last)
                for r in (0.5, 2.0, 1.0 / 3.0, 3.0):
                    ex = med * r
                    if go_div(abs(p - ex), ex) < 0.1:
                        if abs(p - med) > abs(ex - med):
                            p = ex
                        break
        if c < 0.5:
            p = c = v = 0.0
        self.hist = (self.hist + [p])[-20:]
        if len(self.hist) > 1:
            if len(self.hist) >= 3:
                p = _median_positive(self.hist[-3:])
            else:
                p = 0.3 * p + (1 - 0.3) * self.prev
        self.prev = p
        return p, c, v


def period_walk(raw_pitch, raw_conf, Fv, n, sr):
    """(starts, lengths, f0, voicing): frames 1024 / 256; a frame with voicing and confidence above 0.5 and a
    pitch in [50, 500] gives a period of int(sr / pitch) samples from max(frame start, last end), kept when it
    ends before the signal does.  voicing: one more step on frame 0 when the signal is exactly 1024 samples."""
    tr = YinTracker()
    st, ln, f0 = [], [], []
    last_end = 0
    for i in range(Fv):
        p, c, v = tr.step(raw_pitch[i], raw_conf[i])
        if v > 0.5 and c > 0.5 and 50.0 <= p <= 500.0:
            length = int(float(sr) / p)
            s0 = max(i * 256, last_end)
            if s0 + length < n:
                st.append(s0)
                ln.append(length)
                f0.append(p)
                last_end = s0 + length
    voicing = tr.step(raw_pitch[0], raw_conf[0])[2] if n == 1024 else 0.0
    return st, ln, f0, voicing


def voice_quality_from(ln, amp, f0, ac, head, n, sr, vstr):
    """ln, amp, f0: the periods' lengths, RMS amplitudes and pitches (at least 3); ac: the 2048-lag
    autocorrelation of the middle frame, or None below 2048 samples; head: the first min(n, 1024) samples."""
    k = len(ln)
    avg = js = 0.0
    for v in ln:
        avg += float(v)
    avg /= float(k)
    for i in range(1, k):
        js += abs(float(ln[i]) - float(ln[i - 1]))
    jitter = 0.0 if avg == 0 else (js / float(k - 1)) / avg * 100.0
    aavg = ss = 0.0
    for v in amp:
        aavg += v
    aavg /= float(k)
    for i in range(1, k):
        ss += abs(amp[i] - amp[i - 1])
    shimmer = 0.0 if aavg == 0 else (ss / float(k - 1)) / aavg * 100.0
    mf = 0.0
    for v in f0:
        mf += v
    mf /= float(k)
    hnr = 0.0
    if ac is not None:
        el = int(float(sr) / mf)
        if el < 2048:
            r = el // 4
            mc = 0.0
            for i in range(max(1, el - r), min(2047, el + r) + 1):
                if ac[i] > mc:
                    mc = ac[i]
            if 0 < mc < ac[0]:
                hnr = 10.0 * math.log10(mc / (ac[0] - mc))
    var = 0.0
    for v in f0:
        d = v - mf
        var += d * d
    var /= float(k)
    f0s = 0.0 if mf == 0 else go_max(0.0, 1.0 - math.sqrt(var) / mf)
    av = 0.0
    for v in amp:
        d = v - aavg
        av += d * d
    av /= float(k)
    ams = 0.0 if aavg == 0 else go_max(0.0, 1.0 - math.sqrt(av) / aavg)
    nm = 0.0
    if n >= 1024:
        hf = te = 0.0
        for i in range(1, 1024):
            d = head[i] - head[i - 1]
            hf += d * d
            te += head[i] * head[i]
        nm = 0.0 if te == 0 else hf / te
    return dict(jitter=jitter, shimmer=shimmer, hnr=hnr, noise_measure=nm, f0_stability=f0s,
                amplitude_stability=ams, voicing_strength=vstr,
                overall_quality=(go_max(0.0, 1.0 - jitter / 5.0) + go_max(0.0, 1.0 - shimmer / 10.0) +
                                 go_min(1.0, go_max(0.0, hnr / 20.0)) + f0s) / 4.0,
                num_periods=float(k), mean_f0=mf, f0_range=max(f0) - min(f0),
                analysis_quality=(go_min(1.0, float(k) / 10.0) + f0s + go_min(1.0, go_max(0.0, hnr / 15.0))) / 3.0)
