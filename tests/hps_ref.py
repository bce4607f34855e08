"""Python checker of HarmonicProduct (algorithms/harmonic/harmonic_product.go): this project's own
restatement of the reference's statements, one by one, with the reference's line numbers.  Python
floats are IEEE doubles (a product that overflows is Inf and 0.0 * Inf is NaN, without an exception),
every product and every sum below is a Python loop in the reference's order, and nothing on the path
calls libm, so what this computes is what Go computes, bit for bit.  The one thing that is not pinned
is which NaN an invalid operation makes (0.0 * Inf): its sign and payload belong to the processor, not
to Go, and the tests compare a NaN with a NaN as equal.

An analyzer is a dict of sample_rate, num_harmonics, min_f0, max_f0 (NewHarmonicProduct :20-29)."""
import math

import numpy as np

INT32_LIMIT = 2147483648.0


def analyzer(sample_rate, num_harmonics=10, min_f0=80.0, max_f0=2000.0):
    """NewHarmonicProduct; the defaults are MusicFeatureExtractor's (extractors/music.go:100)."""
    return dict(sample_rate=sample_rate, num_harmonics=num_harmonics, min_f0=min_f0, max_f0=max_f0)


def downsample_spectrum(spectrum, factor):
    """downsampleSpectrum (:94-124)."""
    if factor <= 1:                                         # :95-100
        return list(spectrum)
    downsampled_len = len(spectrum) // factor               # :103
    if downsampled_len == 0:                                # :104-106
        return []
    downsampled = [0.0] * len(spectrum)                     # :108-113
    for i in range(downsampled_len):                        # :116-121
        source_idx = i * factor
        if source_idx < len(spectrum):
            downsampled[i] = spectrum[source_idx]
    return downsampled


def compute_hps(hp, magnitude_spectrum):
    """ComputeHPS (:32-58) -> list of floats."""
    mag = [float(v) for v in magnitude_spectrum]
    if len(mag) == 0:                                       # :33-35
        return []
    power_spec = [m * m for m in mag]                       # :38-41
    hps = list(power_spec)                                  # :44-45
    for harmonic in range(2, hp["num_harmonics"] + 1):      # :48
        downsampled = downsample_spectrum(power_spec, harmonic)   # :49
        for i in range(min(len(hps), len(downsampled))):    # :52-54
            hps[i] = hps[i] * downsampled[i]
    return hps


def interpolate_spectrum(spectrum, index):
    """interpolateSpectrum (:194-209)."""
    if index < 0 or index >= float(len(spectrum) - 1):      # :195-197
        return 0.0
    left_bin = int(index)                                   # :199
    right_bin = left_bin + 1
    frac = index - float(left_bin)                          # :201
    if right_bin >= len(spectrum):                          # :203-205, never taken below len - 1
        return spectrum[left_bin]
    return spectrum[left_bin] + frac * (spectrum[right_bin] - spectrum[left_bin])   # :208, three roundings


def compute_hps_interpolated(hp, magnitude_spectrum):
    """ComputeHPSWithInterpolation (:163-191)."""
    mag = [float(v) for v in magnitude_spectrum]
    if len(mag) == 0:                                       # :164-166
        return []
    power_spec = [m * m for m in mag]                       # :169-172
    hps = list(power_spec)                                  # :175-176
    for harmonic in range(2, hp["num_harmonics"] + 1):      # :179
        for b in range(len(hps)):                           # :181
            harmonic_bin = float(b) / float(harmonic)       # :182
            hps[b] = hps[b] * interpolate_spectrum(power_spec, harmonic_bin)   # :185-186
    return hps


def go_int(x):
    """int(x) where it is defined and fits an int32; the library does not reproduce the rest."""
    if not 0.0 <= x < INT32_LIMIT:
        raise ValueError("a conversion Go leaves to the implementation")
    return int(x)


def scan_bins(hp, K, signal_length):
    """findF0Peak's range (:128-139) -> (min_bin, max_bin)."""
    freq_resolution = float(hp["sample_rate"]) / float(signal_length)   # :128
    min_bin = go_int(hp["min_f0"] / freq_resolution)        # :131
    max_bin = go_int(hp["max_f0"] / freq_resolution)        # :132
    if min_bin < 1:                                         # :134-136
        min_bin = 1
    if max_bin >= K:                                        # :137-139
        max_bin = K - 1
    return min_bin, max_bin


def find_f0_peak(hp, hps, signal_length):
    """findF0Peak (:127-160)."""
    min_bin, max_bin = scan_bins(hp, len(hps), signal_length)
    best_bin, best_value = 0, 0.0                           # :141-142
    for b in range(min_bin, max_bin + 1):                   # :145-150
        if hps[b] > best_value:
            best_value = hps[b]
            best_bin = b
    if 0 < best_bin < len(hps) - 1:                         # :153-157
        if hps[best_bin] > hps[best_bin - 1] and hps[best_bin] > hps[best_bin + 1]:
            return best_bin
    return best_bin                                         # :159


def compute_harmonic_strength(hp, magnitude_spectrum, f0_freq, signal_length):
    """ComputeHarmonicStrength (:224-247)."""
    mag = [float(v) for v in magnitude_spectrum]
    if len(mag) == 0 or f0_freq <= 0:                       # :225-227
        return []
    freq_resolution = float(hp["sample_rate"]) / float(signal_length)   # :229
    if hp["num_harmonics"] < 0:
        raise IndexError("runtime error: makeslice: len out of range")  # :230
    strengths = [0.0] * hp["num_harmonics"]
    for harmonic in range(1, hp["num_harmonics"] + 1):      # :232
        harmonic_freq = f0_freq * float(harmonic)           # :233
        harmonic_bin = harmonic_freq / freq_resolution      # :234
        if harmonic_bin >= float(len(mag)):                 # :236-239
            strengths[harmonic - 1] = 0.0
            continue
        strengths[harmonic - 1] = interpolate_spectrum(mag, harmonic_bin)   # :242-243
    return strengths


def compute_harmonicity(hp, magnitude_spectrum, f0_freq, signal_length):
    """ComputeHarmonicity (:250-273)."""
    strengths = compute_harmonic_strength(hp, magnitude_spectrum, f0_freq, signal_length)   # :251
    if len(strengths) == 0:                                 # :253-255
        return 0.0
    harmonic_energy = 0.0
    for s in strengths:                                     # :258-261
        harmonic_energy += s * s
    total_energy = 0.0
    for m in magnitude_spectrum:                            # :263-266
        m = float(m)
        total_energy += m * m
    if total_energy == 0:                                   # :268-270
        return 0.0
    return harmonic_energy / total_energy                   # :272


def estimate_row(hp, magnitude_spectrum, signal_length, interpolated=False):
    """What EstimateF0WithConfidence (:276-298) does after its transform, on one row of magnitudes,
    plus the strengths -> dict of f0_bin, f0, confidence, strengths (num_harmonics values, zeros when
    f0 == 0) and hps."""
    mag = [float(v) for v in magnitude_spectrum]
    hps = compute_hps_interpolated(hp, mag) if interpolated else compute_hps(hp, mag)   # :79
    f0_bin = find_f0_peak(hp, hps, signal_length) if len(hps) else 0                   # :82 (an empty range: 0)
    freq_resolution = float(hp["sample_rate"]) / float(signal_length)                   # :89
    f0 = 0.0 if f0_bin == 0 else float(f0_bin) * freq_resolution                        # :84-90
    nh = max(hp["num_harmonics"], 0)
    if f0 == 0:                                             # :279-281
        return dict(f0_bin=0, f0=0.0, confidence=0.0, strengths=[0.0] * nh, hps=hps)
    strengths = compute_harmonic_strength(hp, mag, f0, signal_length)
    return dict(f0_bin=f0_bin, f0=f0, confidence=compute_harmonicity(hp, mag, f0, signal_length),   # :295
                strengths=strengths if strengths else [0.0] * nh, hps=hps)


def estimate_rows(hp, rows, signal_length, interpolated=False):
    """estimate_row per row -> dict of arrays shaped as the library's outputs."""
    rows = np.asarray(rows, dtype=np.float64)
    rows = rows[None, :] if rows.ndim == 1 else rows
    res = [estimate_row(hp, r, signal_length, interpolated) for r in rows]
    F, K, nh = rows.shape[0], rows.shape[1], max(hp["num_harmonics"], 0)
    return dict(f0_bin=np.array([r["f0_bin"] for r in res], np.int32).reshape(F),
                f0=np.array([r["f0"] for r in res], np.float64).reshape(F),
                confidence=np.array([r["confidence"] for r in res], np.float64).reshape(F),
                strengths=np.array([r["strengths"] for r in res], np.float64).reshape(F, nh),
                hps=np.array([r["hps"] for r in res], np.float64).reshape(F, K))


def apply_window(signal):
    """applyWindow (:212-221): symmetric Hann, not normalised."""
    n = len(signal)
    return [s * (0.5 * (1.0 - math.cos(2.0 * math.pi * float(i) / float(n - 1)))) for i, s in enumerate(signal)]


def optimal_num_harmonics(hp):
    """GetOptimalNumHarmonics (:301-314)."""
    nyquist = float(hp["sample_rate"]) / 2.0                # :303
    max_harmonics = go_int(nyquist / hp["min_f0"])          # :304
    if max_harmonics > 7:                                   # :307-313
        return 5
    if max_harmonics > 3:
        return max_harmonics - 1
    return 2
