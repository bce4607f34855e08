"""Python checker of SpectralPeaks.DetectPeaks (algorithms/harmonic/spectral_peaks.go:36-100) and
HPCP.ComputeFromSpectrum / ComputeFromSpectralPeaks (algorithms/chroma/hpcp.go:147-221): this
project's own restatement of the reference's formulas in numpy / math, statement by statement, with
the reference's line numbers.  Python floats are IEEE doubles and every sum below is a Python loop
in the reference's order, so what differs from Go is libm (log, cos, log2) alone.

Parameters are dicts with the fields of sonar_hpcp_params (DEFAULT is NewHPCP's, hpcp.go:54-75);
weight_type is 0 none, 1 cosine, 2 squared_cosine (any other value is none, Go's default case).

One rule is this project's, not Go's: sort.Slice (:90-92) leaves the order of equal magnitudes
open, here they come in ascending bin order."""
import math

import numpy as np

DEFAULT = dict(size=12, reference_freq=440.0, harmonics_removal=0, normalized=1, weight_type=1, window_size=1.0,
               max_shifted=0, non_linear=0, band_preset=1, min_freq=40.0, max_freq=5000.0, split_freq=500.0,
               harmonics_strength=1.0, max_harmonics=0)
# ComputeFromSpectrum's detector (:211-216)
PEAK_MIN_HEIGHT, PEAK_MIN_DISTANCE_HZ, PEAK_MAX = 0.00001, 20.0, 60
INV_LN2 = 1.4426950408889634      # Go's constant 1 / Ln2


def params(**kw):
    p = dict(DEFAULT)
    p.update(kw)
    return p


def go_log2(x):
    """math.Log2 (log10.go): Frexp, exact for powers of two, else exp + Log(frac) * (1 / Ln2)."""
    frac, exp = math.frexp(x)
    if frac == 0.5:
        return float(exp - 1)
    return float(exp) + math.log(frac) * INV_LN2


def min_distance_bins(min_distance_hz, sample_rate, window_size):
    return max(int(min_distance_hz / (float(sample_rate) / float(window_size))), 1)     # :41-43


def _sorted_cut(peaks, max_peaks):
    peaks = sorted(peaks, key=lambda p: (-p[1], p[0]))      # :90-92, ties by bin (this project's rule)
    if len(peaks) > max_peaks:                              # :95-97
        if max_peaks < 0:
            raise IndexError(f"runtime error: slice bounds out of range [:{max_peaks}]")
        peaks = peaks[:max_peaks]
    return peaks


def detect_peaks(mag, window_size, sample_rate, min_height=PEAK_MIN_HEIGHT, min_distance_hz=PEAK_MIN_DISTANCE_HZ,
                 max_peaks=PEAK_MAX):
    """The literal loop -> list of (bin, magnitude, frequency)."""
    mag = [float(v) for v in mag]
    if len(mag) == 0:                                       # :37-39
        return []
    freq_res = float(sample_rate) / float(window_size)      # :41
    dist = min_distance_bins(min_distance_hz, sample_rate, window_size)
    peaks = []
    for i in range(1, len(mag) - 1):                        # :48
        if mag[i] > mag[i - 1] and mag[i] > mag[i + 1] and mag[i] >= min_height:   # :50-52
            valid = True
            for existing in peaks:                          # :56
                if abs(i - existing[0]) < dist:             # :57-58
                    if mag[i] > existing[1]:                # :60
                        peaks = [p for p in peaks if p[0] != existing[0]]   # :62-67
                    else:
                        valid = False                       # :69
                    break                                   # :71
            if valid:
                peaks.append((i, mag[i], float(i) * freq_res))   # :76-84
    return _sorted_cut(peaks, max_peaks)


def candidates(mag, min_height):
    """Bins of the strict local maxima >= min_height, ascending (numpy; NaN compares false as in Go)."""
    mag = np.asarray(mag, dtype=np.float64)
    if len(mag) < 3:
        return np.zeros(0, np.int64)
    with np.errstate(invalid="ignore"):
        c = (mag[1:-1] > mag[:-2]) & (mag[1:-1] > mag[2:]) & (mag[1:-1] >= min_height)
    return np.nonzero(c)[0] + 1


def detect_peaks_last_kept(mag, window_size, sample_rate, min_height=PEAK_MIN_HEIGHT,
                           min_distance_hz=PEAK_MIN_DISTANCE_HZ, max_peaks=PEAK_MAX):
    """The same function in the form the kernel runs: candidates, then, from 3 bins
    on, each candidate against the last kept peak only."""
    mag = np.asarray(mag, dtype=np.float64)
    if len(mag) == 0:
        return []
    freq_res = float(sample_rate) / float(window_size)
    dist = min_distance_bins(min_distance_hz, sample_rate, window_size)
    cand = candidates(mag, min_height)
    if dist >= 3:
        kept = []
        for i in cand.tolist():
            if kept and i - kept[-1] < dist:
                if mag[i] > mag[kept[-1]]:
                    kept[-1] = i
            else:
                kept.append(i)
        cand = kept
    else:
        cand = cand.tolist()
    return _sorted_cut([(i, float(mag[i]), float(i) * freq_res) for i in cand], max_peaks)


def frequency_to_pitch_class(p, freq):                      # :224-236
    midi = 69 + 12 * go_log2(freq / p["reference_freq"])
    pc = math.fmod(midi, 12)
    if pc < 0:
        pc += 12
    return pc * float(p["size"]) / 12.0


def window_weight(p, distance, window_bins):                # :284-300
    if window_bins == 0:
        return 1.0
    if p["weight_type"] == 1:
        return max(0.0, math.cos(math.pi * distance / window_bins))
    if p["weight_type"] == 2:
        c = max(0.0, math.cos(math.pi * distance / window_bins))
        return c * c
    return 1.0


def contribution(p, pc):
    """addPeakContribution's bins (:254-281) -> list of (wrapped_bin, window_weight, margin); margin is
    the least distance of the decisions taken for this bin (floor, ceil, <=) from their boundaries."""
    size = p["size"]
    window_bins = p["window_size"] * float(size) / 12.0     # :256
    lo, hi = pc - window_bins / 2, pc + window_bins / 2
    start, end = int(math.floor(lo)), int(math.ceil(hi))    # :258-259
    edge = min(abs(lo - round(lo)), abs(hi - round(hi)))    # floor(lo) and ceil(hi) change at whole numbers
    out = []
    for b in range(start, end + 1):                         # :261
        wrapped = b
        while wrapped < 0:                                  # :263-267
            wrapped += size
        wrapped %= size
        distance = abs(float(b) - pc)                       # :270
        fold = abs(distance - float(size) / 2)
        if distance > float(size) / 2:                      # :271-273
            distance = float(size) - distance
        if distance <= window_bins / 2:                     # :276
            out.append((wrapped, window_weight(p, distance, window_bins), min(edge, fold, window_bins / 2 - distance)))
        else:
            out.append((None, 0.0, min(edge, fold, distance - window_bins / 2)))
    return out


def peak_rows(p, freq):
    """What one peak at `freq` adds, in program order -> list of (wrapped_bin, factor, window_weight,
    margin), or [] when the peak is skipped (:156); rejected bins are left out."""
    if p["size"] == 0 or freq < p["min_freq"] or freq > p["max_freq"]:
        return []
    rows = []
    factor = 2.0 if (p["band_preset"] and freq < p["split_freq"]) else 1.0   # :239-251
    for wb, ww, margin in contribution(p, frequency_to_pitch_class(p, freq)):
        rows.append((wb, factor, ww, margin))
    if p["max_harmonics"] > 0 and not p["harmonics_removal"]:           # :175
        for h in range(2, p["max_harmonics"] + 1):                      # :304
            hf = freq * float(h)
            if hf > p["max_freq"]:                                      # :308-310
                break
            for wb, ww, margin in contribution(p, frequency_to_pitch_class(p, hf)):
                rows.append((wb, p["harmonics_strength"] / float(h), ww, margin))   # :142, :316
    return rows


def post(h, p):
    """NonLinear, Normalized, MaxShifted, Energy, Entropy (:181-201) -> (hpcp, energy, entropy)."""
    h = list(h)
    n = len(h)
    if p["non_linear"]:                                     # :330-336
        h = [math.log(1 + v) if v > 0 else v for v in h]
    if p["normalized"] and n:                               # common.EnergyNormalize (math.go:116-137)
        e = 0.0
        for v in h:
            e += v * v
        if not e < 1e-10:
            nrm = math.sqrt(e)
            h = [v / nrm for v in h]
    if p["max_shifted"]:                                    # :339-373
        best, shift = 0.0, 0
        for s in range(n):
            corr = 0.0
            for i in range(n):
                corr += h[i] * h[(i + s) % n]
            if corr > best:
                best, shift = corr, s
        h = [h[(i + shift) % n] for i in range(n)]
    e = 0.0
    for v in h:                                             # :376-382
        e += v * v
    total = 0.0
    for v in h:                                             # :387-390
        total += v
    ent = 0.0
    if total != 0:
        for v in h:
            if v > 0:
                prob = v / total
                ent -= prob * math.log2(prob)
    return np.array(h, dtype=np.float64), math.sqrt(e), ent


def hpcp_from_peaks(peaks, p):
    """ComputeFromSpectralPeaks (:147-202) over (bin, magnitude, frequency) peaks, fully in Python."""
    h = [0.0] * p["size"]
    for _, m, f in peaks:
        for wb, factor, ww, _ in peak_rows(p, f):
            if wb is not None:
                h[wb] += (m * factor) * ww                  # weight *= 2 / Magnitude * harmonicWeights[h]; weight * windowWeight
    return post(h, p)


def hpcp_from_spectrum(mag, window_size, sample_rate, p):
    """ComputeFromSpectrum (:205-221)."""
    return hpcp_from_peaks(detect_peaks(mag, window_size, sample_rate), p)


def table(sample_rate, window_size, K, p):
    """The library's contribution table (sonar_hpcp_table) from the checker's formulas -> dict of
    row_start (K + 1), wrapped_bin, factor, window_weight, margin (per entry) and min_margin (over
    every decision of the used bins, rejected bins included)."""
    freq_res = float(sample_rate) / float(window_size)
    row_start, wb, fac, ww, mg = [0], [], [], [], []
    min_margin = math.inf
    for i in range(K):
        if 1 <= i <= K - 2:
            for b, factor, w, margin in peak_rows(p, float(i) * freq_res):
                min_margin = min(min_margin, margin)
                if b is not None:
                    wb.append(b), fac.append(factor), ww.append(w), mg.append(margin)
        row_start.append(len(wb))
    return {"row_start": np.array(row_start, np.int64), "wrapped_bin": np.array(wb, np.int32),
            "factor": np.array(fac, np.float64), "window_weight": np.array(ww, np.float64),
            "margin": np.array(mg, np.float64), "min_margin": min_margin}


def hpcp_with_table(mag, tab, window_size, sample_rate, p, fast=True):
    """The data-dependent part only: the peaks of one row, then the table's entries in order."""
    detect = detect_peaks_last_kept if fast else detect_peaks
    h = [0.0] * p["size"]
    rs, wb, fac, ww = tab["row_start"], tab["wrapped_bin"], tab["factor"], tab["window_weight"]
    for b, m, _ in detect(mag, window_size, sample_rate):
        for e in range(int(rs[b]), int(rs[b + 1])):
            h[int(wb[e])] += (m * float(fac[e])) * float(ww[e])
    return post(h, p)
