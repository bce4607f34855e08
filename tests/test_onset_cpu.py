"""Known answers for the onset and tempo checker (tests/onset_ref.py), worked out by hand on tiny arrays,
so the checker is pinned independently of the GPU, and the host-only library entries
(sonar_tempo_from_onsets, the width and plan helpers, the category names, the struct layout) against it.
No GPU.  The DESIGN.md findings F70-F79 are pinned here."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import onset_ref as R
import sonar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- SpectralFlux ---------------------------------------------------------------------------------

def test_flux_known_answers():
    assert R.spectral_flux([[0, 0], [3, 4]]) == [5.0]
    assert R.spectral_flux([[3, 4], [0, 0]]) == [0.0]                  # only increases count
    assert R.spectral_flux([[3, 4], [0, 0]], all_changes=True) == [5.0]
    assert R.spectral_flux([]) == [] and R.spectral_flux([[1, 2]]) == []
    assert R.spectral_flux([[1.0, 2.0], [math.nan, 5.0]]) == [3.0]     # F70: a NaN difference adds nothing
    assert math.isnan(R.spectral_flux([[1.0, 2.0], [math.nan, 5.0]], True)[0])
    assert R.spectral_flux([[], []]) == [0.0]


# ---- ComputeRMS -----------------------------------------------------------------------------------

def test_rms_known_answers():
    assert R.rms_envelope([3.0, 4.0, 3.0, 4.0], 2, 2) == [math.sqrt(12.5), math.sqrt(12.5)]
    assert R.rms_envelope([1.0, 1.0, 1.0], 2, 1) == [1.0, 1.0]
    assert R.rms_envelope([1.0, 2.0, 3.0], 2, 2) == [math.sqrt(2.5)]   # (3 - 2) / 2 + 1 = 1 frame
    assert R.rms_envelope([1.0], 2, 1) == [] and R.rms_envelope([1.0, 2.0], 0, 1) == [] and R.rms_envelope([1.0], 1, 0) == []
    assert sonar.rms_envelope_frames(3, 2, 2) == 1 and sonar.rms_envelope_frames(1, 2, 1) == 0
    assert sonar.rms_envelope_frames(5, 0, 1) == 0 and sonar.rms_envelope_frames(5, 1, 0) == 0
    assert sonar.rms_envelope_frames(26_460_000, 4410, 1102) == (26_460_000 - 4410) // 1102 + 1


# ---- findFluxPeaks --------------------------------------------------------------------------------

def test_a_plateau_is_no_peak_and_the_threshold_is_inclusive():
    assert R.find_peaks_frames([0, 2, 2, 0], 0.0, 0) == []
    assert R.find_peaks_frames([0, 2, 0], 2.0, 0) == [1]               # a value equal to the threshold
    assert R.find_peaks_frames([0, 2, 0], 2.0000001, 0) == []
    assert R.find_peaks_frames([0, 2], 0.0, 0) == [] and R.find_peaks_frames([5, 1, 5], 0.0, 0) == []
    assert R.find_peaks_frames([0, math.nan, 0, 3, 0], 0.0, 0) == [3]  # a NaN is above nothing and nothing is above it
    assert R.find_peaks_frames([0, 2, 0], math.nan, 0) == []
    assert R.find_peaks_frames([0, math.inf, 0], math.inf, 0) == [1]


def test_min_interval_greedy():
    v = [0, 5, 0, 4, 0, 3, 0, 6, 0, 1, 0]                              # candidates at 1, 3, 5, 7, 9
    assert R.find_peaks_frames(v, 0.0, 0) == [1, 3, 5, 7, 9]
    assert R.find_peaks_frames(v, 0.0, 2) == [1, 3, 5, 7, 9]           # F72: maxima are 2 apart, the rule acts from 3 on
    assert R.find_peaks_frames(v, 0.0, 3) == [1, 5, 9]                 # greedy: the first wins, not the highest
    assert R.find_peaks_frames(v, 0.0, 4) == [1, 5, 9]
    assert R.find_peaks_frames(v, 0.0, 5) == [1, 7]
    assert R.find_peaks_frames(v, 0.0, len(v) + 1) == [1]              # last starts at -minIntervalFrames
    assert R.find_peaks_frames(v, 0.0, -7) == [1, 3, 5, 7, 9]          # a negative interval never rejects
    assert R.find_flux_peaks(v, 0.0, -0.5, 512, 44100) == [1, 3, 5, 7, 9]
    assert R.min_interval_frames(0.05, 44100, 512) == 4 and R.min_interval_frames(0.05, 44100, 256) == 8
    assert R.min_interval_frames(-0.05, 44100, 512) == -4              # truncation toward zero
    for mi, sr, hop in [(0.05, 44100, 512), (0.05, 44100, 256), (-0.05, 44100, 512), (0.05, 8000, 512), (2.999, 1, 1)]:
        assert sonar.onset_min_interval_frames(mi, sr, hop) == R.min_interval_frames(mi, sr, hop)
    for mi in (math.nan, 1e300, -1e300, math.inf):
        with pytest.raises(sonar.SonarError) as e:
            sonar.onset_min_interval_frames(mi, 44100, 512)
        assert e.value.code == sonar.ERR_UNSUPPORTED
    assert [sonar.onset_peaks_width(n) for n in range(7)] == [0, 0, 0, 1, 1, 2, 2]


def test_onset_sample_is_the_flux_index_times_the_hop():
    rows = [[0.0], [0.0], [0.0], [9.0], [9.0], [9.0]]                  # the rise is between rows 2 and 3
    assert R.spectral_flux(rows) == [0.0, 0.0, 9.0, 0.0, 0.0]
    assert R.detect_onsets_from_rows(rows, 44100, 0.3, 0.05) == [2 * 512]   # F73: i * hop, not (i + 1) * hop
    assert R.detect_onsets_from_rows(rows[:1], 44100, 0.3, 0.05) == []


def test_energy_detector():
    assert R.energy_diff([1.0, 3.0, 2.0, math.nan, 5.0]) == [2.0, 0.0, 0.0, 0.0]   # F74: a NaN difference gives 0
    x = [0.0] * 1024 + [1.0] * 512 + [0.0] * 1024
    onsets, curve = R.detect_onsets_energy(x, 44100, 0.1, 0.05)
    # envelope 0, 0, 0, sqrt(0.5), 1, sqrt(0.5), 0, ...: the largest rise is difference 2, reported as 2 * hop
    assert len(curve) == (len(x) - 512) // 256 and curve[:4] == [0.0, 0.0, math.sqrt(0.5), 1.0 - math.sqrt(0.5)]
    assert onsets == [2 * 256]
    assert R.detect_onsets_energy(x[:511], 44100, 0.1, 0.05) == ([], [])
    assert R.detect_onsets_energy([], 44100, 0.1, 0.05) == ([], [])


# ---- combineOnsets, density, AdaptiveThreshold -------------------------------------------------------

def test_combine_tolerance_on_both_sides():
    assert R.combine_onsets([0, 1000], [400, 1401], 400) == [0, 1000, 1401]   # 400 away is a duplicate, 401 is not
    assert R.combine_onsets([1000], [0], 400) == [0, 1000]
    assert R.combine_onsets([], [], 400) == [] and R.combine_onsets([5, 5], [5], 0) == [5]
    # F75: the chain compares with the last kept value: 0, 300, 600 keeps 0 and 600 although 300 lies near both
    assert R.combine_onsets([0, 600], [300], 400) == [0, 600]
    assert R.complex_tolerance(8000) == 400 and R.complex_tolerance(44100) == 2205
    assert R.onset_density(4, 88200, 44100) == 2.0 and R.onset_density(0, 0, 44100) == 0.0


def test_adaptive_threshold_known_answers():
    assert R.adaptive_threshold([]) == 0.0
    assert R.adaptive_threshold([2.0]) == 2.0
    assert R.adaptive_threshold([1.0, 3.0]) == 4.0                     # mean 2, population deviation 1
    assert R.adaptive_threshold([2.0, 4.0, 4.0, 4.0, 5.0, 5.0, 7.0, 9.0]) == 9.0   # mean 5, deviation 2


# ---- the interval histogram ---------------------------------------------------------------------------

def test_tempo_votes_known_answers():
    assert R.find_tempo_from_intervals([]) == 0.0
    assert R.find_tempo_from_intervals([0.5, 0.5, 1.0]) == 120.0
    assert R.tempo_votes([0.2, 2.0]) == [0] * 14                       # F77: the ends of (0.2, 2.0) do not vote
    assert R.tempo_votes([0.3, 1.0]) == [1] + [0] * 12 + [1]          # 200 and 60 bpm, the outermost bins
    assert R.tempo_votes([60.0 / 190.0]) == [0] * 14                   # 10 away from 180 and from 200: not < 10
    assert R.tempo_votes([60.0 / 189.0])[12] == 1
    assert R.tempo_votes([60.0 / 65.0])[0] == 1                        # equally near 60 and 70: the first bin (strict <)
    assert R.find_tempo_from_intervals([1.0, 0.5]) == 60.0             # a tie goes to the lower bin
    assert R.find_tempo_from_intervals([0.1, 3.0]) == 120.0            # the default when nothing voted
    assert R.tempo_from_onsets([100], 8000) == (0.0, [0] * 14) and R.tempo_from_onsets([], 8000)[0] == 0.0


def test_host_tempo_from_onsets_matches_the_checker():
    rng = np.random.default_rng(0)
    lists = [[], [7], [0, 4000], [0, 1600, 17600], [0, 8000, 12000], [0, 8000 * 60 // 190]]
    lists += [np.cumsum(rng.integers(500, 20000, 40)).tolist() for _ in range(20)]
    for sr in (8000, 44100):
        for on in lists:
            t, counts = sonar.tempo_from_onsets(on, sr)
            wt, wc = R.tempo_from_onsets(on, sr)
            assert t == wt and counts.tolist() == wc, (sr, on)
    with pytest.raises(sonar.SonarError) as e:
        sonar.tempo_from_onsets([0, 10], 0)
    assert e.value.code == sonar.ERR_UNSUPPORTED


# ---- the autocorrelation --------------------------------------------------------------------------------

def test_autocorrelation_normalises_only_lag_zero():
    e = [1.0, 2.0, 3.0, 4.0]
    ac = R.autocorrelation(e, 2)
    assert ac == [1.0, 20.0 / 3.0]                                     # F76: (1+4+9+16)/4 -> 1.0; (2+6+12)/3 stays raw
    assert R.autocorrelation([0.0, 0.0, 0.0], 2) == [0.0, 0.0]          # ac[0] is not > 0: nothing is divided
    assert R.autocorrelation(e, 9) == R.autocorrelation(e, 4) and len(R.autocorrelation(e, 9)) == 4
    inf = R.autocorrelation([math.inf, 1.0], 2)
    assert math.isnan(inf[0]) and math.isnan(inf[1])                   # Inf / Inf, then everything over that


def test_autocorrelation_search():
    assert R.autocorr_frame_hop(44100) == (4410, 1102) and R.autocorr_frame_hop(8000) == (800, 200)
    assert R.autocorr_frame_hop(48000) == (4800, 1200) and R.autocorr_frame_hop(39) == (3, 0)
    assert R.lag_range(198, 200, 8000)[:2] == (13, 40) and R.lag_range(25, 200, 8000)[:2] == (13, 24)
    assert R.lag_range(30000, 1102, 44100)[:2] == (13, 40)             # lags 12..41 are all the search reads
    assert R.find_tempo_from_autocorrelation([1.0] * 9, 200, 8000) == (0.0, 0)
    flat = [1.0] + [0.25] * 49
    assert R.find_tempo_from_autocorrelation(flat, 200, 8000) == (120.0, 0)   # no strict maximum
    peak = list(flat)
    peak[20] = 0.5
    peak[30] = 0.5
    assert R.find_tempo_from_autocorrelation(peak, 200, 8000) == (60.0 / (20.0 * (200.0 / 8000.0)), 20)   # the first of equals
    edge = list(flat)
    edge[49] = 9.0                                                     # the last lag is never a peak
    assert R.find_tempo_from_autocorrelation(edge[:41] + [9.0], 200, 8000) == (120.0, 0)
    low = list(flat)
    low[12] = 9.0                                                      # below the range
    assert R.find_tempo_from_autocorrelation(low, 200, 8000) == (120.0, 0)
    assert R.tempo_autocorrelation_from_envelope([1.0] * 9, 200, 8000) == (0.0, 0, [])
    assert R.tempo_autocorrelation_from_envelope([1.0] * 19, 200, 8000)[0] == 0.0
    assert R.tempo_autocorrelation([], 8000) == (0.0, 0, [])
    for n, sr in [(0, 8000), (2599, 8000), (2600, 8000), (4599, 8000), (4600, 8000), (80000, 8000), (441000, 44100),
                  (100, 39), (100, 40), (5000, 79)]:
        p = sonar.tempo_autocorr_plan(n, sr)
        frame, hop = R.autocorr_frame_hop(sr)
        L = len(R.rms_envelope([0.0] * n, frame, hop)) if n <= 5000 else (n - frame) // hop + 1
        assert (p["frame_size"], p["hop_size"], p["envelope_len"]) == (frame, hop, L)
        assert p["n_autocorr"] == (L // 2 if L >= 10 else 0)
        if p["n_autocorr"] >= 10:
            assert (p["min_lag"], p["max_lag"]) == R.lag_range(L // 2, hop, sr)[:2]


# ---- EstimateTempoRange and the categories -----------------------------------------------------------------

def test_categories_at_their_cut_points():
    cuts = [(59.999, 0), (60.0, 1), (89.999, 1), (90.0, 2), (119.999, 2), (120.0, 3), (149.999, 3), (150.0, 4), (1e9, 4),
            (0.0, 0), (-5.0, 0), (math.nan, 4)]
    for tempo, want in cuts:
        assert R.classify(tempo) == want == sonar.tempo_category(tempo), tempo
    assert [sonar.tempo_category_name(k) for k in range(5)] == R.CATEGORIES == sonar.TEMPO_CATEGORIES
    assert sonar.tempo_category_name(5) == "" and sonar.tempo_category_name(-1) == ""


def test_tempo_range():
    assert R.tempo_range(120.0, 100.0) == (110.0, 0.6, 20.0)
    assert R.tempo_range(0.0, 120.0) == (60.0, 0.0, 120.0)             # the confidence stops at 0
    assert R.tempo_range(0.0, 0.0) == (0.0, 1.0, 0.0)
    # F78: EstimateTempo's error is dropped; a signal too short for the STFT has onset tempo 0 and no error
    short = R.estimate_tempo_range([0.1] * 500, 8000, None)
    assert short["onset_tempo"] == 0.0 and short["autocorr_tempo"] == 0.0 and short["confidence"] == 1.0
    assert short["category"] == 0


# ---- widths and the struct ------------------------------------------------------------------------------------

def test_complex_width():
    for n in (0, 511, 512, 1023, 1024, 1535, 1536, 44100, 441000):
        F = max((n - 1024) // 512 + 1, 0) if n >= 1024 else 0
        Fe = (n - 512) // 256 + 1 if n >= 512 else 0
        assert sonar.onsets_complex_width(n) == sonar.onset_peaks_width(F - 1) + sonar.onset_peaks_width(Fe - 1)


def test_tempo_result_layout(tmp_path):
    """The ctypes mirror against the header as a C99 compiler lays it out (-pedantic -Werror)."""
    fields = [n for n, _ in sonar.TempoResult._fields_]
    src = tmp_path / "tempo_layout.c"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "sonar_gpu.h"', 'int main(void) {',
             '  printf("struct %zu\\n", sizeof(sonar_tempo_result));']
    lines += [f'  printf("{f} %zu\\n", offsetof(sonar_tempo_result, {f}));' for f in fields]
    lines += ['  printf("grid %d %d %d %d\\n", SONAR_ONSET_WINDOW, SONAR_ONSET_HOP, SONAR_ONSET_ENERGY_FRAME, '
              'SONAR_ONSET_ENERGY_HOP);',
              '  printf("enum %d %d\\n", SONAR_TEMPO_VERY_SLOW, SONAR_TEMPO_VERY_FAST);', '  return 0;', '}']
    src.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "tempo_layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-O1",
                    "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = dict(line.split(None, 1) for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["struct"]) == ctypes.sizeof(sonar.TempoResult) == 64
    for f in fields:
        assert int(out[f]) == getattr(sonar.TempoResult, f).offset, f
    assert out["grid"].split() == [str(v) for v in (R.WINDOW, R.HOP, R.ENERGY_FRAME, R.ENERGY_HOP)]
    assert out["enum"].split() == ["0", "4"]
