"""The parts of the inharmonicity analyzer that need no GPU: known answers for the Python checker
(tests/inharm_ref.py) worked out by hand, the library's tracker, checks and host helpers against the checker
bit for bit (through ctypes, and host_dsp.cpp again as the stand-alone program tests/c_abi/inharm_track_check.cpp
under a sanitizer), the layout of sonar_inharm_params, and what the shared inputs of tests/inharm_cases.py are
for.  The DESIGN.md findings F100-F107 are pinned here and in test_gpu_inharm.py (each test names its finding)."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import inharm_cases as IC
import inharm_ref as R
import sonar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 16000


# ------------------------------------------------- the checker, by hand ----
def _three_harmonics():
    """W 64 at 16 kHz: bins of 250 Hz.  f0 = 490 Hz: the windows int(1.96 -+ 0.098) = 1..2, int(3.92 -+ 0.196) = 3..4
    and int(5.88 -+ 0.294) = 5..6 hold the peaks at bins 2, 4 and 6 (500, 1000, 1500 Hz, amplitudes 4, 2, 1)."""
    mag = np.zeros(32)
    mag[2], mag[4], mag[6] = 4.0, 2.0, 1.0
    return mag, R.Params(SR, window_size=64, max_freq=1600.0)


def test_f102_three_harmonic_row_by_hand():
    mag, p = _three_harmonics()
    r = R.analyze_spectrum(mag, 490.0, 0.9, p)
    d = [(500.0 - 490.0) / 490.0, (1000.0 - 980.0) / 980.0, (1500.0 - 1470.0) / 1470.0]
    assert r["status"] == R.OK and r["num_harmonics"] == 3 and r["bins"] == [2, 4, 6]
    assert r["harmonics"]["freqs"] == [500.0, 1000.0, 1500.0] and r["harmonics"]["ideals"] == [490.0, 980.0, 1470.0]
    assert r["deviations"] == d and r["n_deviations"] == 3
    num = 4.0 * d[0] * 1 * 1 + 2.0 * d[1] * 2 * 2 + 1.0 * d[2] * 3 * 3          # sum w dev n^2, in harmonic order
    den = 4.0 + 2.0 * 16 + 1.0 * 81                                              # sum w n^4 = 117
    assert r["inharmonicity"] == num / den and r["inharmonicity"] == pytest.approx(21.0 / 49.0 / 117.0, rel=1e-14)
    assert r["std_dev"] == pytest.approx(0.0, abs=1e-17)                         # the three deviations are 1 / 49
    assert r["confidence"] == (3.0 / 20.0) * (7.0 / 3.0) == 0.35000000000000003  # (count / MaxHarmonics) mean(amp)
    assert r["harmonic_clarity"] == pytest.approx(20.0 * math.log10(4.0) / 60.0, rel=1e-15)
    assert r["spectral_purity"] == pytest.approx(math.exp(-20.0 / 49.0), rel=1e-15)
    assert r["partial_coherence"] == 1.0                                         # spacings 500, 500: no variation
    # 0.3 (3 / 20) + 0.3 (0.9) + 0.2 (0.35) + 0.1 (no model fit) = 0.485: Fair
    assert r["quality"] == 2 and R.QUALITY_NAMES[2] == "Fair"
    assert r["model_fit_quality"] == 0.0 and r["estimated_stiffness"] == 0.0 and r["r_squared"] == 0.0
    q = R.analyze_spectrum(mag, 490.0, 0.9, R.Params(SR, window_size=64, max_freq=1600.0, weight_by_amplitude=False))
    assert q["inharmonicity"] == (d[0] + d[1] * 4 + d[2] * 9) / (1.0 + 16 + 81)
    s = R.analyze_spectrum(mag, 490.0, 0.9, R.Params(SR, window_size=64, max_freq=1600.0, model=R.MODEL_STRING,
                                                     string_tension=2.0, string_length=3.0))
    assert s["estimated_stiffness"] == r["inharmonicity"] * 2.0 * 3.0 * 3.0
    B = r["inharmonicity"]
    err = sum(abs(f - n * 490.0 * math.sqrt(1 + B * n * n)) for n, f in ((1, 500.0), (2, 1000.0), (3, 1500.0))) / 3
    assert s["model_fit_quality"] == pytest.approx(math.exp(-err / 490.0), rel=1e-14) and s["model_fit_quality"] > 0.9
    # partial tracking and every unknown method are SpectralDeviation (:548, :265)
    for m in (R.PARTIAL_TRACKING, 17, -1):
        t = R.analyze_spectrum(mag, 490.0, 0.9, R.Params(SR, window_size=64, max_freq=1600.0, method=m))
        assert t["inharmonicity"] == r["inharmonicity"] and t["deviations"] == d


def test_f102_search_window_strict_scan_and_local_maximum():
    """a strict > from maxMag = 0: an all-zero stretch leaves the start bin with magnitude 0; the winner must
    be a strict local maximum at 1 .. K - 2; the loop over h stops at the first h f0 > max_freq"""
    mag, p = _three_harmonics()
    assert R.find_harmonic_peak(mag, 490.0, p, 64) == (500.0, 4.0, 2)
    assert R.find_harmonic_peak(np.zeros(32), 490.0, p, 64) is None              # maxBin 1: 0 > 0 fails
    flat = np.zeros(32)
    flat[2] = flat[3] = 1.0
    assert R.find_harmonic_peak(flat, 490.0, p, 64) is None                      # not above its right neighbour
    edge = np.zeros(32)
    edge[31] = 1.0
    wide = R.Params(SR, window_size=64, harmonic_tolerance=40.0, max_freq=8000.0)
    assert R.find_harmonic_peak(edge, 7000.0, wide, 64) is None                  # the scan clamps to K - 1: no peak there
    assert R.find_harmonic_peak(mag, 7000.0, wide, 64) == (500.0, 4.0, 2)        # ... and to 0 at the other end
    assert R.harmonic_structure(mag, 490.0, R.Params(SR, window_size=64, max_freq=979.0), 64)["numbers"] == [1]
    assert R.harmonic_structure(mag, 490.0, R.Params(SR, window_size=64, max_freq=1600.0, max_harmonics=2), 64)["numbers"] \
        == [1, 2]
    strong = R.Params(SR, window_size=64, max_freq=1600.0, min_harmonic_strength=2.0)     # Magnitude > strength, strict
    assert R.harmonic_structure(mag, 490.0, strong, 64)["numbers"] == [1]


def test_f101_invalid_f0_row_and_f103_insufficient_row():
    mag, p = _three_harmonics()
    for f0 in (0.0, -3.0, 79.9, 1600.1):
        r = R.analyze_spectrum(mag, f0, 0.7, p)
        assert r["status"] == R.INVALID_F0 and r["quality"] == 5 and r["f0"] == f0 and r["f0_confidence"] == 0.7
        assert r["num_harmonics"] == 0 and r["inharmonicity"] == 0.0 and r["harmonics"] is None
    assert R.QUALITY_NAMES[5] == "Poor - Invalid F0"
    r = R.analyze_spectrum(mag, 490.0, 0.7, R.Params(SR, window_size=64, max_freq=1600.0, min_harmonics=4))
    assert r["status"] == R.INSUFFICIENT and r["num_harmonics"] == 3 and r["quality"] == -1 and r["harmonics"] is None
    assert str(R.InsufficientHarmonics(3, 4)) == "insufficient harmonics found: 3 < 4"
    out = R.from_spectrum([mag, mag], [490.0, 0.0], [0.7, 0.2], R.Params(SR, window_size=64, max_freq=1600.0, min_harmonics=4))
    assert out["status"].tolist() == [R.INSUFFICIENT, R.INVALID_F0] and out["num_harmonics"].tolist() == [3, 0]
    assert (out["h_number"] == -1).all() and not out["h_freq"].any() and out["quality"].tolist() == [-1, 5]


def test_f104_railsback_grid():
    """201 values from -0.01 by float64 additions; the last is short of 0.01; index 100 is not 0"""
    g = R.grid()
    assert len(g) == 201 and g[0] == -0.01 and g[-1] == 0.00999999999999999 and g[-1] + 0.0001 > 0.01
    assert g[100] != 0.0 and abs(g[100]) < 1e-17
    b = -0.01
    for k in range(200):
        b += 0.0001
        assert g[k + 1] == b


def test_f104_nan_grid_points_are_skipped():
    """for n >= 11 the early grid points give 1 + B n^2 < 0: the first 18 at n = 11, the first 76 at n = 20; their
    error is NaN and `error < minError` skips them"""
    g = R.grid()
    assert [k for k, b in enumerate(g) if 1 + b * 11 * 11 < 0] == list(range(18))
    assert [k for k, b in enumerate(g) if 1 + b * 20 * 20 < 0] == list(range(76))
    # harmonics 1, 2 and 20 exactly on the B = g[80] curve: the fit returns g[80], never a skipped point
    f0, B = 100.0, g[80]
    d = {"numbers": [1, 2, 20], "freqs": [n * f0 * math.sqrt(1 + B * n * n) for n in (1, 2, 20)]}
    assert R.fit_railsback(d, f0) == B
    # every point NaN (an observed NaN): bestB stays 0.0
    assert R.fit_railsback({"numbers": [1, 2, 3], "freqs": [100.0, math.nan, 300.0]}, f0) == 0.0
    # fewer than three harmonics: the empty result, no arrays
    mag, p = _three_harmonics()
    r = R.analyze_spectrum(mag, 490.0, 0.9, R.Params(SR, window_size=64, max_freq=1000.0, min_harmonics=2, method=R.RAILSBACK))
    assert r["status"] == R.OK and r["num_harmonics"] == 2 and r["harmonics"] is None and r["inharmonicity"] == 0.0
    r = R.analyze_spectrum(mag, 490.0, 0.9, R.Params(SR, window_size=64, max_freq=1600.0, method=R.RAILSBACK))
    assert r["inharmonicity"] in g and r["model_fit_quality"] == r["r_squared"] and r["confidence"] == max(0.0, r["r_squared"])


def test_f105_chi_squared_cases():
    """fewer than 5 values: (0, 1).  5: two bins, -1 degree of freedom, p = min(1, 1 + chi / 2) = 1.  6 and 7: three
    bins, 0 degrees: chi / 0 is +Inf (p = 0) or NaN for chi = 0 (math.Min(1, NaN) is NaN).  10: five bins, 2 degrees."""
    assert R.goodness_of_fit([1.0, 2.0, 3.0, 4.0]) == (0.0, 1.0)
    chi, p = R.goodness_of_fit([1.0, 2.0, 3.0, 4.0, 5.0])
    assert chi > 0 and p == 1.0
    chi, p = R.goodness_of_fit([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    assert chi > 0 and p == 0.0
    chi, p = R.goodness_of_fit([2.0] * 6)                    # zero variance: int(NaN) bins nothing, expected is NaN
    assert chi == 0.0 and math.isnan(p)
    chi, p = R.goodness_of_fit([2.0] * 10)
    assert chi == 0.0 and p == 1.0
    x = [float(v) for v in range(10)]
    chi, p = R.goodness_of_fit(x)
    assert chi > 0 and p == max(0.0, min(1.0, 1.0 - chi / 4.0))
    assert R.go_int(math.nan) == R.go_int(math.inf) == R.go_int(-1e300) == -2 ** 63 and R.go_int(-2.9) == -2
    assert math.isnan(R.go_min(1.0, math.nan)) and math.isnan(R.go_max(0.0, math.nan))
    assert R.go_min(-math.inf, math.nan) == -math.inf and R.go_max(math.nan, math.inf) == math.inf


def test_f105_outlier_removal_shortens_the_deviations():
    """quartiles by gonum's empirical quantile: of [0, 1, 2, 3, 100] q1 = 1 (count 2 >= 1.25), q3 = 3 (count 4 >=
    3.75); 100 > 3 + 2 * 2 goes.  Below three values nothing is removed; a threshold of 0 keeps [q1, q3]."""
    assert R.remove_outliers([0.0, 1.0, 2.0, 3.0, 100.0], 2.0) == [0.0, 1.0, 2.0, 3.0]
    assert R.remove_outliers([100.0, 0.0], 2.0) == [100.0, 0.0]
    assert R.remove_outliers([0.0, 1.0, 2.0, 3.0, 100.0], 0.0) == [1.0, 2.0, 3.0]
    assert R.remove_outliers([0.0, 1.0, 2.0], math.nan) == []
    r = IC.spectrum_ref(512, "statistical", "general")
    short = (r["n_deviations"] < r["num_harmonics"]) & (r["status"] == R.OK)
    f = int(np.flatnonzero(short)[0])
    n, m = int(r["num_harmonics"][f]), int(r["n_deviations"][f])
    assert r["h_freq"][f, n - 1] != 0 and not r["h_deviation"][f, m:].any() and r["h_deviation"][f, :m].all()


def test_f106_beat_pattern_by_hand():
    """eleven correlations, lags -5 .. 5: strict maxima >= 0.1 at lags 2 and 4: mean 3, variance 2"""
    lags = list(range(-5, 6))
    corr = [0.0] * 11
    corr[7], corr[9] = 0.5, 0.3
    assert R.find_peaks(corr, 0.1) == [7, 9]
    assert R.beat_value(corr, lags) == math.sqrt(2.0) / 3.0 * 0.001
    corr[3], corr[1] = 0.5, 0.3                              # symmetric: the lags' mean is 0, not > 0
    assert R.beat_value(corr, lags) == 0.0
    assert R.beat_value([0.0, 0.5, 0.0] + [0.0] * 8, lags) == 0.0     # one peak
    assert R.beat_value([0.0, 0.5, 0.0, 0.3, 0.0], [-2, -1, 0, 1, 2]) == 0.0   # fewer than 10 correlations
    assert R.find_peaks([0.0, 0.09, 0.0, 0.1, 0.0, 0.2, 0.2, 0.0], 0.1) == [3]  # below the height; a plateau is none


def test_f107_tracker_by_hand():
    p = R.Params(SR, use_temporal_tracking=True, temporal_window=10)
    t = R.track(p, [1.0, 2.0, 3.0, 4.0], [100.0, 100.0, 100.0, 100.0])
    # 0.3 cur + 0.7 last smoothed
    h1 = 0.3 * 2.0 + (1.0 - 0.3) * 1.0
    h2 = 0.3 * 3.0 + (1.0 - 0.3) * h1
    assert t["inharmonicity"].tolist() == [1.0, h1, h2, 0.3 * 4.0 + (1.0 - 0.3) * h2] and h1 == pytest.approx(1.3)
    assert not t["temporal_stability"][:3].any() and t["temporal_stability"][3] > 0      # three entries BEFORE the frame
    h = t["inharmonicity"][:3]
    assert t["inharmonicity_trend"][3] == pytest.approx(np.polyfit([0, 1, 2], h, 1)[0], rel=1e-12)
    assert t["f0_stability"].tolist() == [0.0, 0.0, 0.0, 1.0]
    off = R.track(R.Params(SR), [1.0, 2.0, 3.0, 4.0, 5.0], [100.0] * 5)
    assert off["inharmonicity"].tolist() == [1.0, 2.0, 3.0, 4.0, 5.0] and not off["temporal_stability"].any()
    zero = R.track(R.Params(SR, use_temporal_tracking=True, temporal_window=0), [1.0, 2.0, 3.0, 4.0, 5.0], [100.0] * 5)
    assert zero["inharmonicity"].tolist() == [1.0, 2.0, 3.0, 4.0, 5.0] and not zero["f0_stability"].any()
    with pytest.raises(IndexError) as e:
        R.track(R.Params(SR, use_temporal_tracking=True, temporal_window=-3), [1.0], [100.0])
    assert str(e.value) == "runtime error: slice bounds out of range [4:1]"
    # rows that are not OK never reach the histories
    st = [R.OK, R.INVALID_F0, R.OK, R.OK, R.INVALID_F0, R.OK]
    a = R.track(p, [1.0, 9.0, 2.0, 3.0, 9.0, 4.0], [100.0, 0.0, 100.0, 100.0, 0.0, 100.0], st)
    assert a["inharmonicity"][[0, 2, 3, 5]].tolist() == t["inharmonicity"].tolist() and a["inharmonicity"][1] == 9.0
    assert a["temporal_stability"][5] == t["temporal_stability"][3] and a["temporal_stability"][4] == 0.0


def test_f100_only_window_1024_analyses_anything():
    x = np.zeros(8192)
    for W in (4096, 512):
        with pytest.raises(ValueError) as e:
            R.frames(x, 512, R.Params(SR, window_size=W))
        assert str(e.value) == "audio frame size (%d) doesn't match window size (1024)" % W
    assert R.frames(x[:1000], 512, R.Params(SR, window_size=1024))["status"].shape == (0,)
    assert R.frames(x[:4000], 512, R.Params(SR))["status"].shape == (0,)          # n < W: no frame is due


# ------------------------------------------------- the library's host side ----
TRACK_CASES = [dict(), dict(use_temporal_tracking=True), dict(use_temporal_tracking=True, temporal_window=1),
               dict(use_temporal_tracking=True, temporal_window=0), dict(use_temporal_tracking=True, temporal_window=3)]


def _track_rows():
    rng = np.random.default_rng(11)
    raw = np.concatenate((rng.uniform(-0.01, 0.01, 40), [0.0, 0.0, 0.0, 0.0, math.inf, math.nan, 1e-3], rng.uniform(0, 0.005, 10)))
    f0 = np.concatenate((rng.uniform(80.0, 1000.0, 44), [0.0, 0.0, 0.0], rng.uniform(80.0, 1000.0, 10)))
    st = rng.choice([R.OK, R.OK, R.OK, R.INVALID_F0], len(raw)).astype(np.int32)
    return raw, f0, st


@pytest.mark.parametrize("kw", TRACK_CASES, ids=lambda v: str(v))
def test_f107_library_tracker_equals_checker(kw):
    raw, f0, st = _track_rows()
    p = sonar.inharm_params_default(SR, **{k: int(v) for k, v in kw.items()})
    for status in (None, st):
        ref = R.track(R.Params(SR, **kw), raw, f0, status)
        got = sonar.inharm_track(p, raw, f0, status)
        for k in ref:
            assert np.array_equal(got[k], ref[k], equal_nan=True), k
    assert sonar.inharm_track(p, [], [])["inharmonicity"].shape == (0,)


def test_f107_negative_window_is_a_panic_at_the_first_tracked_frame():
    p = sonar.inharm_params_default(SR, use_temporal_tracking=1, temporal_window=-2)
    with pytest.raises(sonar.SonarError) as e:
        sonar.inharm_track(p, [1.0, 2.0], [100.0, 100.0])
    assert e.value.code == sonar.ERR_PANIC and e.value.msg == "runtime error: slice bounds out of range [3:1]"
    got = sonar.inharm_track(p, [1.0, 2.0], [0.0, 0.0], [R.INVALID_F0, R.INSUFFICIENT])     # no frame reaches :1098
    assert got["inharmonicity"].tolist() == [1.0, 2.0]
    off = sonar.inharm_params_default(SR, temporal_window=-2)                              # tracking off: never reached
    assert sonar.inharm_track(off, [1.0, 2.0], [100.0, 100.0])["inharmonicity"].tolist() == [1.0, 2.0]
    assert sonar.inharm_check(p) == 0                        # the per-frame entries never reach it


@pytest.fixture(scope="module")
def track_check(tmp_path_factory):
    """host_dsp.cpp's tracker and regression as a program of their own, under AddressSanitizer and UBSan"""
    exe = str(tmp_path_factory.mktemp("inharm") / "inharm_track_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "c_abi", "inharm_track_check.cpp"),
                    os.path.join(ROOT, "sonido-sonar_amd", "csrc", "host_dsp.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("kw", TRACK_CASES[1:], ids=lambda v: str(v))
def test_f107_host_tracker_under_sanitizers(track_check, kw):
    raw, f0, _ = _track_rows()
    text = "T 1 %d %d\n" % (kw.get("temporal_window", 10), len(raw))
    text += "".join("%s %s\n" % (float(a).hex(), float(b).hex()) for a, b in zip(raw, f0))
    out = subprocess.run([track_check], input=text, check=True, capture_output=True, text=True)
    assert out.stderr == ""
    vals = np.array([[float.fromhex(t) for t in line.split()] for line in out.stdout.splitlines()]).reshape(len(raw), 4)
    ref = R.track(R.Params(SR, **kw), raw, f0)
    for i, k in enumerate(("inharmonicity", "temporal_stability", "inharmonicity_trend", "f0_stability")):
        assert np.array_equal(vals[:, i], ref[k], equal_nan=True), k


def test_f107_host_regression_under_sanitizers(track_check):
    rng = np.random.default_rng(3)
    for n in (2, 3, 10):
        x, y = [float(i) for i in range(n)], rng.uniform(-1, 1, n).tolist()
        text = "R %d\n" % n + "".join("%s %s\n" % (a.hex(), b.hex()) for a, b in zip(x, y))
        out = subprocess.run([track_check], input=text, check=True, capture_output=True, text=True)
        assert out.stderr == "" and float.fromhex(out.stdout.split()[0]) == R.linear_regression_slope(x, y)
    assert R.linear_regression_slope([0.0, 1.0, 2.0], [1.0, 3.0, 5.0]) == 2.0


def test_host_one_liners_and_every_string():
    vals = [0.0, 0.00009, 0.0001, -0.0005, 0.001, 0.004, -0.005, 0.0099, 0.01, 0.5, math.nan, math.inf]
    for v in vals:
        assert sonar.inharm_classify(v) == R.classify(v), v
        for f0 in (50.0, 100.0, 300.0, 499.0, 500.0, 800.0, 2000.0, math.nan):
            assert sonar.inharm_instrument_type(v, f0) == R.instrument_type(v, f0), (v, f0)
    assert sonar.inharm_classify(math.nan) == "Very High" and sonar.inharm_classify(-0.0003) == "Low"
    assert sonar.inharm_instrument_type(0.003, 200.0) == "Piano/String" and sonar.inharm_instrument_type(0.0001, 200.0) == "Wind/Brass"
    assert sonar.inharm_instrument_type(0.001, 600.0) == "Plucked String" and sonar.inharm_instrument_type(0.003, 600.0) == "Unknown"
    assert sonar.inharm_instrument_type(0.0005, 300.0) == "Vocal/Harmonic"       # neither < nor > 0.0005
    L = sonar.lib()
    for fn, names in ((L.sonar_inharm_class_name, R.CLASS_NAMES), (L.sonar_inharm_instrument_name, R.INSTRUMENT_NAMES),
                      (L.sonar_inharm_quality_name, R.QUALITY_NAMES)):
        assert [fn(i).decode() for i in range(len(names))] == names and fn(-1) is None and fn(len(names)) is None
    assert [sonar.inharm_method_name(i) for i in range(6)] == R.METHOD_NAMES and sonar.inharm_method_name(6) == "Unknown"
    assert [sonar.inharm_model_name(i) for i in range(4)] == R.MODEL_NAMES and sonar.inharm_model_name(-1) == "Unknown"
    inh, conf = [0.001, 0.002, 0.5, 0.004], [0.9, 0.51, 0.5, math.nan]           # only confidence > 0.5 counts
    assert sonar.inharm_average(inh, conf) == R.average(inh, conf) == (0.001 + 0.002) / 2.0
    assert sonar.inharm_average([1.0], [0.5]) == 0.0 and sonar.inharm_average([], []) == 0.0


def test_defaults_are_the_constructors():
    """NewInharmonicityAnalyzer (:147-172), window 4096 included"""
    p, r = sonar.inharm_params_default(44100), R.Params(44100)
    for name in ("sample_rate", "method", "model", "window_size", "max_harmonics", "min_harmonics", "harmonic_tolerance",
                 "min_harmonic_strength", "min_freq", "max_freq", "weight_by_amplitude", "string_tension", "string_length",
                 "outlier_threshold", "use_robust_estimation", "use_temporal_tracking", "temporal_window"):
        assert getattr(p, name) == getattr(r, name), name
    assert (p.method, p.model, p.window_size, p.max_harmonics, p.min_harmonics) == (2, 3, 4096, 20, 3)
    assert (p.harmonic_tolerance, p.min_harmonic_strength, p.min_freq, p.max_freq) == (0.05, 0.01, 80.0, 2000.0)
    assert (p.freq_resolution, p.reference_harmonic, p.use_log_frequency, p.string_stiffness, p.confidence_level) == \
        (1.0, 1, 0, 0.001, 0.95)
    assert (p.outlier_threshold, p.use_robust_estimation, p.use_temporal_tracking, p.temporal_window) == (2.0, 1, 0, 10)
    assert sonar.INHARM_METHODS == IC.METHODS and sonar.INHARM_MODELS == IC.MODELS
    assert (sonar.INHARM_OK, sonar.INHARM_INVALID_F0, sonar.INHARM_INSUFFICIENT) == (R.OK, R.INVALID_F0, R.INSUFFICIENT)


CHECKS = [(dict(), 0), (dict(method=99), 0), (dict(method="beat_pattern"), 0), (dict(max_harmonics=64), 0),
          (dict(max_harmonics=-3), 0), (dict(min_harmonics=-1), 0), (dict(harmonic_tolerance=-0.5), 0),
          (dict(outlier_threshold=math.nan), 0), (dict(use_temporal_tracking=1, temporal_window=-1), 0),
          (dict(sample_rate=0), sonar.ERR_INVALID), (dict(max_freq=math.inf), sonar.ERR_INVALID),
          (dict(min_freq=math.nan), sonar.ERR_INVALID), (dict(harmonic_tolerance=math.nan), sonar.ERR_INVALID),
          (dict(min_harmonic_strength=-math.inf), sonar.ERR_INVALID), (dict(max_harmonics=65), sonar.ERR_UNSUPPORTED),
          (dict(max_freq=1e300), sonar.ERR_UNSUPPORTED), (dict(harmonic_tolerance=1e12), sonar.ERR_UNSUPPORTED)]


@pytest.mark.parametrize("kw,code", CHECKS, ids=lambda v: str(v))
def test_parameter_checks_without_a_device(kw, code):
    p = sonar.inharm_params_default(kw.get("sample_rate", SR), **{k: v for k, v in kw.items() if k != "sample_rate"})
    assert sonar.inharm_check(p) == code
    assert sonar.lib().sonar_inharm_check(None) == sonar.ERR_INVALID


def test_inharm_params_layout(tmp_path):
    """The ctypes mirror against the header as a C99 compiler lays it out (-pedantic -Werror)."""
    exe = str(tmp_path / "inharm_layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-O1",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_abi", "inharm_layout.c"),
                    "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert out[0].split() == ["size", "sonar_inharm_params", str(ctypes.sizeof(sonar.InharmParams))]
    offs = {line.split()[1]: int(line.split()[2]) for line in out if line.startswith("offset")}
    assert offs == {n: getattr(sonar.InharmParams, n).offset for n, _ in sonar.InharmParams._fields_}
    assert out[-1].split() == ["enum", "railsback", "0", "statistical", "5", "general", "3", "invalid_f0", "5", "insufficient",
                               "2", "very_high", "4", "unknown", "4", "max", "64"]
    assert sonar.INHARM_MAX_HARMONICS == 64


def test_abi_version_and_symbols():
    assert sonar.abi_version() == 4
    lib = ctypes.CDLL(sonar.LIB_PATH)
    for n in ("sonar_inharm_params_default", "sonar_inharm_check", "sonar_inharm_from_spectrum", "sonar_inharm_frames",
              "sonar_inharm_track", "sonar_inharm", "sonar_inharm_average", "sonar_inharm_classify",
              "sonar_inharm_class_name", "sonar_inharm_instrument_type", "sonar_inharm_instrument_name",
              "sonar_inharm_method_name", "sonar_inharm_model_name", "sonar_inharm_quality_name"):
        assert n in sonar.EXPORTED_SYMBOLS and hasattr(lib, n)


# ------------------------------------- the GPU cases, as the checker sees them ----
def test_inputs_meet_their_conditions():
    """what each shared input is for, held here so that a change of the generators cannot empty a GPU case"""
    for K in IC.SPECTRUM_K:
        mag, f0, conf = IC.spectrum_rows(K)
        assert mag.shape == (IC.F_MAX, K) and f0[1] == 0.0 and 0 < f0[2] < 80.0 and f0[3] > 7500.0 and f0[4] < 0
        r = IC.spectrum_ref(K, "statistical", "general")
        assert r["status"][:5].tolist() == [R.OK, R.INVALID_F0, R.INVALID_F0, R.INVALID_F0, R.INVALID_F0]
        ok = r["status"] == R.OK
        assert np.count_nonzero(ok) > 100 and (np.count_nonzero(r["status"] == R.INSUFFICIENT) >= 1 or K == 32)
        n, m = r["num_harmonics"][ok], r["n_deviations"][ok]
        assert (m < n).any() and (n >= 11).any()             # an outlier goes; the NaN grid points are reached
        assert set(np.unique(m)) >= {3, 4, 5, 6, 7, 10}      # no test, two bins, zero degrees of freedom, five bins
        assert np.isnan(r["p_value"][ok]).any() or K == 32
        assert (r["p_value"][ok] == 0).any() and (r["p_value"][ok] == 1).any() and (r["chi_squared"] > 0).any()
        q = IC.spectrum_ref(K, "railsback", "general")
        assert len(np.unique(q["inharmonicity"][ok])) > 10 and (q["quality"][ok] >= 2).all()
    for sr in (16000, 44100):
        tone = IC.pcm_ref("tone", sr, 5, 512, "spectral_deviation")
        assert (tone["status"] == R.OK).all() and (tone["num_harmonics"] >= 3).all() and (tone["f0"] > 80).all()
        assert (IC.pcm_ref("sine", sr, 5, 512, "spectral_deviation")["status"] == R.INSUFFICIENT).all()
        for kind in ("noise", "silence"):
            r = IC.pcm_ref(kind, sr, 5, 512, "spectral_deviation")
            assert (r["status"] == R.INVALID_F0).all() and not r["f0"].any()
        step = IC.pcm_ref("step", sr, 66, 512, "spectral_deviation", extra=(("min_harmonics", 1),))
        assert (step["status"] == R.OK).sum() >= 60 and len(np.unique(np.round(step["f0"][step["status"] == R.OK]))) >= 2
    assert (IC.pcm_ref("step", 44100, 66, 512, "spectral_deviation")["status"] == R.INSUFFICIENT).any()


PCM_CPU_CASES = [(kind, sr, F, hop) for kind in ("tone", "step") for sr in (16000, 44100) for hop in IC.PCM_HOPS
                 for F in IC.PCM_F]


@pytest.mark.parametrize("kind,sr,F,hop", PCM_CPU_CASES)
def test_pcm_cases_have_no_undecided_frame(kind, sr, F, hop):
    """the harmonic search keeps the same harmonics at the same bins under numpy's transform and under go_fft, on
    every frame of every PCM case: the GPU test's cap of 10 % undecided frames is never what passes a case"""
    a = IC.pcm_ref(kind, sr, F, hop, "spectral_deviation", fft="numpy")
    assert a["decided"].all() and len(a["decided"]) == F
    b = IC.pcm_ref(kind, sr, F, hop, "spectral_deviation", fft="go")
    for k in ("status", "num_harmonics", "h_number", "h_freq", "h_ideal", "h_deviation", "f0"):
        assert np.array_equal(a[k], b[k]), k
    peak = a["magnitude"].max(axis=1, keepdims=True)
    assert 0 < np.max(np.abs(a["magnitude"] - a["magnitude_other"]) / np.maximum(peak, 1e-300)) < 1e-12
