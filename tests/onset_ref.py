"""Plain-Python checker of the reference's onset and tempo functions: SpectralFlux (spectral_flux.go),
Envelope.ComputeRMS (envelope.go), OnsetDetection (onset_detection.go) and TempoEstimation
(tempo_estimation.go).  Written from their behaviour, with sequential float loops: Python's float is an
IEEE double, its + - * / and math.sqrt round once, so every value here has the bits Go computes.

Curves are lists of floats, index lists are lists of ints.  The STFT is not restated here: the flux
detector takes the magnitude rows (detect_onsets_from_rows), as the GPU tests hold the rows themselves
to numpy's transform.  test_onset_cpu.py pins this file to known answers."""
import math

WINDOW, HOP, ENERGY_FRAME, ENERGY_HOP = 1024, 512, 512, 256
FLUX_THRESHOLD, ENERGY_THRESHOLD, MIN_INTERVAL = 0.3, 0.1, 0.05
TEMPO_RANGE = [60.0, 70.0, 80.0, 90.0, 100.0, 110.0, 120.0, 130.0, 140.0, 150.0, 160.0, 170.0, 180.0, 200.0]
CATEGORIES = ["very_slow", "slow", "moderate", "fast", "very_fast"]


def go_int(x):
    """int(x) of a float64 where Go defines it (truncation toward zero)."""
    assert not math.isnan(x) and abs(x) < 2.0 ** 63
    return int(x)


def spectral_flux(rows, all_changes=False):
    """Compute / ComputeAllChanges: F rows -> F - 1 values."""
    out = []
    for t in range(1, len(rows)):
        s = 0.0
        cur, prev = rows[t], rows[t - 1]
        for f in range(len(cur)):
            d = float(cur[f]) - float(prev[f])
            if all_changes or d > 0:
                s += d * d
        out.append(math.sqrt(s))
    return out


def rms_envelope(x, frame, hop):
    n = len(x)
    if n < frame or frame <= 0 or hop <= 0:
        return []
    out = []
    for i in range((n - frame) // hop + 1):
        s = 0.0
        for j in range(i * hop, i * hop + frame):
            v = float(x[j])
            s += v * v
        out.append(math.sqrt(s / float(frame)))
    return out


def min_interval_frames(min_interval, sample_rate, hop):
    return go_int(min_interval * float(sample_rate) / float(hop))


def find_flux_peaks(v, threshold, min_interval, hop, sample_rate):
    if len(v) < 3:
        return []
    return find_peaks_frames(v, threshold, min_interval_frames(min_interval, sample_rate, hop))


def find_peaks_frames(v, threshold, mif):
    """findFluxPeaks with minIntervalFrames given."""
    if len(v) < 3:
        return []
    peaks, last = [], -mif
    for i in range(1, len(v) - 1):
        if v[i] > v[i - 1] and v[i] > v[i + 1] and v[i] >= threshold and i - last >= mif:
            peaks.append(i)
            last = i
    return peaks


def detect_onsets_from_rows(rows, sample_rate, threshold, min_interval, hop=HOP):
    """DetectOnsets after the STFT: the flux of the magnitude rows, its peaks, index * hop."""
    flux = spectral_flux(rows)
    if not flux:
        return []
    return [i * hop for i in find_flux_peaks(flux, threshold, min_interval, hop, sample_rate)]


def energy_diff(env):
    out = []
    for i in range(len(env) - 1):
        d = env[i + 1] - env[i]
        out.append(d if d > 0 else 0.0)
    return out


def detect_onsets_energy(x, sample_rate, threshold, min_interval, frame=ENERGY_FRAME, hop=ENERGY_HOP):
    """-> (onset samples, the energyDiff curve)"""
    if len(x) == 0:
        return [], []
    env = rms_envelope(x, frame, hop)
    if not env:
        return [], []
    curve = energy_diff(env)
    return [i * hop for i in find_flux_peaks(curve, threshold, min_interval, hop, sample_rate)], curve


def combine_onsets(a, b, tolerance):
    """combineOnsets as written: every value against every kept one."""
    kept = []
    for v in sorted(list(a) + list(b)):
        if not any(abs(v - e) <= tolerance for e in kept):
            kept.append(v)
    return kept


def complex_tolerance(sample_rate):
    return go_int(MIN_INTERVAL * float(sample_rate))


def onset_density(count, n, sample_rate):
    duration = float(n) / float(sample_rate)
    return 0.0 if duration == 0 else float(count) / duration


def adaptive_threshold(v):
    if len(v) == 0:
        return 0.0
    mean = 0.0
    for x in v:
        mean += float(x)
    mean /= float(len(v))
    var = 0.0
    for x in v:
        d = float(x) - mean
        var += d * d
    var /= float(len(v))
    return mean + 2.0 * math.sqrt(var)


def tempo_votes(intervals):
    counts = [0] * len(TEMPO_RANGE)
    for iv in intervals:
        if iv > 0.2 and iv < 2.0:
            tempo = 60.0 / iv
            best, best_diff = 0, abs(tempo - TEMPO_RANGE[0])
            for k, ref in enumerate(TEMPO_RANGE):
                d = abs(tempo - ref)
                if d < best_diff:
                    best, best_diff = k, d
            if best_diff < 10.0:
                counts[best] += 1
    return counts


def find_tempo_from_intervals(intervals):
    if len(intervals) == 0:
        return 0.0
    counts = tempo_votes(intervals)
    best, top = 120.0, 0
    for k, c in enumerate(counts):
        if c > top:
            top, best = c, TEMPO_RANGE[k]
    return best


def tempo_from_onsets(onsets, sample_rate):
    """EstimateTempo after the onset detection -> (tempo, the 14 votes)."""
    if len(onsets) < 2:
        return 0.0, [0] * len(TEMPO_RANGE)
    iv = [float(onsets[i + 1] - onsets[i]) / float(sample_rate) for i in range(len(onsets) - 1)]
    return find_tempo_from_intervals(iv), tempo_votes(iv)


def autocorrelation(e, max_lag):
    """calculateAutocorrelation, its in-place normalisation loop included."""
    max_lag = min(max_lag, len(e))
    ac = [0.0] * max_lag
    for lag in range(max_lag):
        s, count = 0.0, 0
        for i in range(len(e) - lag):
            s += e[i] * e[i + lag]
            count += 1
        if count > 0:
            ac[lag] = s / float(count)
    if len(ac) > 0 and ac[0] > 0:
        for i in range(len(ac)):
            ac[i] = ac[i] / ac[0]                            # ac[0] is 1.0 (or NaN) from the first step on
    return ac


def autocorr_frame_hop(sample_rate):
    frame = go_int(0.1 * float(sample_rate))
    return frame, frame // 4


def lag_range(n_ac, hop, sample_rate):
    tpf = float(hop) / float(sample_rate)
    lo, hi = go_int((60.0 / 180.0) / tpf), go_int(1.0 / tpf)
    return max(lo, 1), min(hi, n_ac - 1), tpf


def find_tempo_from_autocorrelation(ac, hop, sample_rate):
    """-> (tempo, best lag)"""
    if len(ac) < 10:
        return 0.0, 0
    lo, hi, tpf = lag_range(len(ac), hop, sample_rate)
    top, best = 0.0, 0
    for lag in range(lo, hi + 1):
        if 0 < lag < len(ac) - 1:
            if ac[lag] > ac[lag - 1] and ac[lag] > ac[lag + 1] and ac[lag] > top:
                top, best = ac[lag], lag
    if best == 0:
        return 120.0, 0
    return 60.0 / (float(best) * tpf), best


def tempo_autocorrelation_from_envelope(env, hop, sample_rate):
    """EstimateTempoAutocorrelation after ComputeRMS -> (tempo, best lag, the curve or [])."""
    if len(env) < 10:
        return 0.0, 0, []
    ac = autocorrelation(env, len(env) // 2)
    tempo, lag = find_tempo_from_autocorrelation(ac, hop, sample_rate)
    return tempo, lag, ac


def tempo_autocorrelation(x, sample_rate):
    if len(x) == 0:
        return 0.0, 0, []
    frame, hop = autocorr_frame_hop(sample_rate)
    return tempo_autocorrelation_from_envelope(rms_envelope(x, frame, hop), hop, sample_rate)


def tempo_range(onset_tempo, autocorr_tempo):
    """EstimateTempoRange after the two estimates -> (average, confidence, difference)."""
    avg = (onset_tempo + autocorr_tempo) / 2.0
    diff = abs(onset_tempo - autocorr_tempo)
    conf = 1.0 - diff / 50.0
    return avg, (conf if conf > 0.0 else 0.0) if not math.isnan(conf) else math.nan, diff


def classify(tempo):
    return 0 if tempo < 60 else 1 if tempo < 90 else 2 if tempo < 120 else 3 if tempo < 150 else 4


def estimate_tempo_range(x, sample_rate, complex_onsets):
    """EstimateTempoRange of a signal given DetectOnsetsComplex's result, or None where the STFT returned
    its error (len(x) < 1024): the error is dropped and the onset tempo is 0."""
    onset_tempo = 0.0 if complex_onsets is None or len(x) == 0 else tempo_from_onsets(complex_onsets, sample_rate)[0]
    ac_tempo, lag, _ = tempo_autocorrelation(x, sample_rate)
    avg, conf, diff = tempo_range(onset_tempo, ac_tempo)
    return dict(onset_tempo=onset_tempo, autocorr_tempo=ac_tempo, tempo=avg, confidence=conf, difference=diff,
                best_lag=lag, category=classify(avg))
