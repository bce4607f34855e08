"""Plain-Python checker of the speech extractor's sequential host tail: the percentile-10 energy threshold,
calculateSilenceRatio, extractPauseDurations, detectOnsets with calculateAdaptiveThreshold,
calculateAttackTimes and estimateSpeechRate (fingerprint/extractors/speech.go), and detectSpeech with
checkPeriodicity (algorithms/speech/speech_analysis.go).  Written from their behaviour, with sequential
float loops: Python's float is an IEEE double, its + - * / and math.sqrt round once, so every value here
has the bits Go computes.

Energies and signals are lists of floats.  A division by a zero sample rate follows IEEE as Go's does
(go_div): x / 0 is +-Inf, 0 / 0 is NaN.  test_speech_tail_cpu.py pins this file to known answers."""
import math


def go_div(a, b):
    """a / b of two float64 as Go evaluates it."""
    if b != 0.0:
        return a / b
    if a == 0.0 or math.isnan(a):
        return math.nan
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def percentile10_threshold(energies):
    """The element at index len / 10 of the energies in ascending order (Go bubble-sorts a copy)."""
    return sorted(energies)[len(energies) // 10]


def silence_ratio(energies):
    if not energies:
        return 0.0
    thr = percentile10_threshold(energies)
    silent = 0
    for e in energies:
        if e <= thr:
            silent += 1
    return float(silent) / float(len(energies))


def pause_durations(energies, hop, rate):
    """Runs of frames at or below the threshold, in seconds; only those longer than 0.1 s count, a run
    that reaches the end included."""
    if not energies:
        return []
    thr = percentile10_threshold(energies)
    frame_s = go_div(float(hop), float(rate))
    out, in_pause, start = [], False, 0
    for i, e in enumerate(energies):
        if e <= thr:
            if not in_pause:
                in_pause, start = True, i
        elif in_pause:
            d = float(i - start) * frame_s
            if d > 0.1:
                out.append(d)
            in_pause = False
    if in_pause:
        d = float(len(energies) - start) * frame_s
        if d > 0.1:
            out.append(d)
    return out


def adaptive_threshold(values):
    """mean + 2 * population standard deviation."""
    if not values:
        return 0.0
    s = 0.0
    for v in values:
        s += v
    mean = s / float(len(values))
    var = 0.0
    for v in values:
        d = v - mean
        var += d * d
    return mean + 2 * math.sqrt(var / float(len(values)))


def detect_onsets(energies):
    """Strict local maxima of the first difference above its adaptive threshold; the index is the
    difference's (the rise from frame i to i + 1)."""
    if len(energies) < 3:
        return []
    der = [energies[i + 1] - energies[i] for i in range(len(energies) - 1)]
    thr = adaptive_threshold(der)
    out = []
    for i in range(1, len(der) - 1):
        if der[i] > der[i - 1] and der[i] > der[i + 1] and der[i] > thr:
            out.append(i)
    return out


def attack_times(onsets, energies, hop, rate):
    """Per onset: back from it, at most 9 frames and not below frame 0, to the first frame under a tenth
    of the onset frame's energy; that distance in seconds, at most 0.1 (a NaN stays)."""
    frame_s = go_div(float(hop), float(rate))
    out = []
    for on in onsets:
        peak = energies[on]
        start = on
        j = on - 1
        while j >= 0 and j > on - 10:
            if energies[j] < 0.1 * peak:
                start = j
                break
            j -= 1
        t = float(on - start) * frame_s
        if t > 0.1:
            t = 0.1
        out.append(t)
    return out


def onset_density(onsets, n, sample_rate):
    return go_div(float(len(onsets)), go_div(float(n), float(sample_rate)))


def speech_rate(energies, n, rate, is_speech):
    if not is_speech:
        return 0.0
    dur = go_div(float(n), float(rate))
    speech_time = dur * (1.0 - silence_ratio(energies))
    if speech_time > 0:
        return go_div(4.0 * speech_time, dur)
    return 3.0


def zero_crossings(signal):
    c = 0
    for i in range(1, len(signal)):
        if (signal[i - 1] >= 0 and signal[i] < 0) or (signal[i - 1] < 0 and signal[i] >= 0):
            c += 1
    return c


def sum_squares(signal):
    s = 0.0
    for v in signal:
        s += v * v
    return s


def check_periodicity(signal):
    if len(signal) < 1024:
        return False
    fr = signal[:1024]
    best = 0.0
    for lag in range(20, 400):                    # lag < 400 and lag < 1024 / 2
        corr = 0.0
        for i in range(1024 - lag):
            corr += fr[i] * fr[i + lag]
        corr /= float(1024 - lag)
        if corr > best:
            best = corr
    energy = sum_squares(fr) / 1024.0
    if energy > 0:
        best /= energy
    return best > 0.1


def detect_speech_from_sums(n, rate, crossings, sum_sq, head):
    """detectSpeech given the whole signal's zero-crossing count and sum of squares and its first
    min(n, 1024) samples (what the library's kernels hand its host tail)."""
    if n < int(rate / 4):                         # Go: rate / 4 on ints, truncating toward zero
        return False
    z = 0.0 if n <= 1 else float(crossings) / float(n - 1)
    if z < 0.01 or z > 0.3:
        return False
    if n == 0 or math.sqrt(sum_sq / float(n)) < 0.001:
        return False
    return check_periodicity(head)


def detect_speech(signal, rate):
    return detect_speech_from_sums(len(signal), rate, zero_crossings(signal), sum_squares(signal), signal[:1024])


def gated_tone():
    """The tests' voiced signal, 2 s at 16 kHz (numpy array): 0.5 sin(phase), 200 Hz for t < 1 s and 130 Hz
    after (the phase is the running sum of 2 pi f / sr), times a gate of period 0.5 s: 0.35 s on with 30 ms
    linear ramps at both ends, then 0.15 s of exact zeros.  No noise, so YIN is confident and detectSpeech
    says yes."""
    import numpy as np
    sr, n = 16000, 32000
    f = np.where(np.arange(n) / sr < 1.0, 200.0, 130.0)
    x = 0.5 * np.sin(np.cumsum(2.0 * np.pi * f / sr))
    tp = np.arange(n) % 8000
    gate = np.where(tp < 5600, np.minimum(1.0, np.minimum(tp / 480.0, (5600 - tp) / 480.0)), 0.0)
    return x * gate
