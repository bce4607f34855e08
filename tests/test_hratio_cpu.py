"""The parts of the harmonic-ratio analyzer that need no GPU: known answers for the Python checker
(tests/hratio_ref.py) worked out by hand, the library's tracker and host helpers against the checker, the
layout of sonar_hratio_params, the argument checks that need no device, and, for every case of
tests/test_gpu_hratio.py, the share of frames the checker itself leaves undecided.  The DESIGN.md findings
F86-F99 are pinned here and in test_gpu_hratio.py (each test names its finding)."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import hratio_cases as HC
import hratio_ref as R
import sonar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = HC.SR


# ------------------------------------------------- the checker, by hand ----
def test_f88_moving_average_is_a_trailing_window():
    """entry i < L averages 0..i, the others the L entries ending at i; L > K and L <= 0 return the input"""
    d = [1.0, 2.0, 6.0, 3.0, 8.0]
    assert R.moving_average(d, 3).tolist() == [1.0, 1.5, 3.0, 11.0 / 3.0, 17.0 / 3.0]
    assert R.moving_average(d, 5).tolist() == [1.0, 1.5, 3.0, 3.0, 4.0]
    for L in (6, 0, -2):
        assert R.moving_average(d, L).tolist() == d
    assert R.moving_average(d, 1).tolist() == d
    # sums in j order: 1e16 + 1 + 1 is 1e16 from the left, not 1e16 + 2
    assert R.moving_average([1e16, 1.0, 1.0], 3)[2] == 1e16 / 3.0


def test_f89_quantile_rule_and_out_of_range_percentile():
    """the first sorted value whose count reaches p n; x[0] at p = 0; the median of ten is the fifth, no mean"""
    x = [float(v) for v in range(10, 20)]
    assert R.quantile(x, 0.0) == 10.0 and R.quantile(x, 0.1) == 10.0 and R.quantile(x, 0.11) == 11.0
    assert R.quantile(x, 0.5) == 14.0 and R.quantile(x, 1.0) == 19.0
    assert R.percentile([3.0, 1.0, 2.0], 0.5) == 2.0 and R.percentile([3.0, 1.0, 2.0, 0.0], 0.5) == 1.0
    assert R.percentile(x, -0.1) == 0.0 and R.percentile(x, 1.5) == 0.0 and R.percentile([], 0.5) == 0.0
    with pytest.raises(ValueError):
        R.percentile(x, math.nan)                          # past common.Percentile's test, gonum panics


def test_f89_noise_floor_windows_and_snr_60():
    """[max(0, i - 10), min(K, i + 10)): ten values at bin 0, twenty inside, eleven at bin K - 1"""
    K = 32
    mag = np.arange(1.0, K + 1.0)
    p = R.Params(SR, window_size=64, noise_floor_method="minimum", noise_floor_smoothing_len=1)
    assert R.noise_floor(mag, p).tolist() == [float(max(0, i - 10) + 1) for i in range(K)]
    p.noise_floor_method = "median"                        # bin 0: ten values 1..10 -> 5; bin 20: 11..30 -> 20
    nf = R.noise_floor(mag, p)
    assert nf[0] == 5.0 and nf[20] == 20.0 and nf[K - 1] == 27.0     # 22..32: the count 6 reaches 5.5
    p.noise_floor_method, p.noise_floor_percentile = "something else", 0.1     # Go's default case: percentile
    nf = R.noise_floor(mag, p)
    assert nf[0] == 1.0 and nf[20] == 12.0                 # counts 1 >= 1.0 and 2 >= 2.0
    p.noise_floor_percentile = 1.5                         # a floor of zeros, an SNR of 60
    r = R.analyze_spectrum(mag, None, R.Params(SR, window_size=64, noise_floor_percentile=1.5))
    assert not r["noise_floor"].any() and r["snr"] == 60.0


def _stack(W, k0, amps):
    n = np.arange(W, dtype=np.float64)
    return sum(a * np.sin(2.0 * np.pi * (h + 1) * k0 * n / W) for h, a in enumerate(amps))


def test_bin_centred_sine_stack_by_hand():
    """W 256 at 16 kHz: bins of 62.5 Hz.  Fifteen partials at bins 8 h (500 h Hz), the first the strongest, no
    smoothing.  f0 is the strongest peak at or above 80 Hz: 500 Hz; maxHarmonic = min(20, 8000 / 500) = 16; the
    targets int(500 h 256 / 16000) = 8 h hold a strict maximum for h <= 15, and h = 16 is bin 128 >= K: nil."""
    W = 256
    amps = [1.0 / (1.0 + 0.1 * h) for h in range(15)]
    p = R.Params(SR, window_size=W, hop_size=W, spectral_smoothing_len=1)
    r = R.frames(_stack(W, 8, amps), p)
    assert r["f0"][0] == 500.0 and r["num_harmonics"][0] == 15
    assert r["h_bin"][0, :15].tolist() == [8 * h for h in range(1, 16)] and (r["h_bin"][0, 15:] == -1).all()
    assert r["h_freq"][0, :15].tolist() == [500.0 * h for h in range(1, 16)] and not r["h_freq"][0, 15:].any()
    # a Hann-windowed sine of amplitude a peaks at a W / 4 (the window's denominator W - 1 moves it by < 2 %)
    assert np.allclose(r["h_amp"][0, :15], np.array(amps) * W / 4, rtol=2e-2)
    assert r["f0_confidence"][0] == r["h_amp"][0, 0]       # F86: the peak's magnitude, not a value in [0, 1]
    assert r["f0_confidence"][0] > 60.0
    assert r["harmonicity"][0] == 1.0 and r["harmonic_energy"][0] > 0.99 * r["total_energy"][0]
    for m in (R.HPS, R.SPECTRAL):
        q = R.frames(_stack(W, 8, amps), R.Params(SR, method=m, window_size=W, hop_size=W, spectral_smoothing_len=1))
        assert q["f0"][0] == 500.0 and q["num_harmonics"][0] == 15, m
        assert not q["snr"].any() and not q["voicing"].any() and not q["noise_floor"].any()   # unset in Go's result


def test_f86_f0_is_the_strongest_peak_not_the_lowest():
    """two peaks above min_freq, the upper one stronger: "lowest significant peak" returns the upper one; and
    with every peak below min_freq, the strongest of all"""
    K = 128
    mag = np.zeros(K)
    mag[8], mag[24] = 1.0, 2.0
    p = R.Params(SR, window_size=256, spectral_smoothing_len=1)
    r = R.analyze_spectrum(mag, None, p)
    assert r["f0"] == 24 * 62.5 and r["f0_confidence"] == 2.0
    p.min_freq = 4000.0
    r = R.analyze_spectrum(mag, None, p)
    assert r["f0"] == 24 * 62.5 and r["f0_confidence"] == 2.0


def test_f90_nearest_peak_scan_and_repeated_bins():
    """the scan is a strict > from 0 over the target +- width and then needs a strict local maximum; two
    harmonics whose windows hold the same maximum list it twice when both are within tolerance"""
    K = 128
    mag = np.zeros(K)
    mag[40], mag[41], mag[42] = 1.0, 3.0, 1.0              # one peak at bin 41: 2562.5 Hz
    p = R.Params(SR, window_size=256, spectral_smoothing_len=1, harmonic_tolerance=0.6, max_harmonics=2)
    fr = R._Frame(mag, None, p)
    assert fr.nearest_peak(38 * 62.5)[0] == 41 and fr.nearest_peak(45 * 62.5) is None   # 41 + 3 < 45: all zeros
    hp = fr.harmonic_peaks(22 * 62.5)                      # targets 22 (no: zeros) and 44 (41 in reach)
    assert [q[0] for q in hp] == [41]
    hp = fr.harmonic_peaks(41 * 62.5 / 1.05)               # h = 1 -> bin 39, h = 2 -> bin 78: only the first
    assert [q[0] for q in hp] == [41]
    mag[43], mag[44] = 0.5, 0.25
    fr = R._Frame(mag, None, R.Params(SR, window_size=256, spectral_smoothing_len=1, harmonic_tolerance=0.6,
                                      max_harmonics=2, peak_detection_width=30))
    assert [q[0] for q in fr.harmonic_peaks(30 * 62.5)] == [41, 41]    # targets 30 and 60 both reach bin 41
    flat = np.ones(K)                                      # a plateau: the first bin wins the scan, no strict maximum
    assert R._Frame(flat, None, p).nearest_peak(50 * 62.5) is None


def test_f92_negative_infinity_and_60_db():
    """no peak: harmonic energy 0 with noise energy -> -Inf; no energy in range at all -> 60"""
    K = 128
    p = R.Params(SR, window_size=256, spectral_smoothing_len=1)
    r = R.analyze_spectrum(np.linspace(1.0, 2.0, K), None, p)          # monotone: no local maximum
    assert r["f0"] == 0.0 and r["harmonic_energy"] == 0.0 and r["harmonic_ratio"] == -math.inf
    assert r["voicing"] == 0.0 and r["periodicity"] == 0.0 and len(r["peaks"]) == 0
    r = R.analyze_spectrum(np.zeros(K), None, p)
    assert r["harmonic_ratio"] == 60.0 and r["snr"] == 60.0


def test_f93_hps_scan_starts_at_bin_0():
    """nothing in [minBin, maxBin) beats hps[0]: f0 0 Hz, no harmonics, the ratio from hps[0]"""
    K = 128
    mag = np.full(K, 0.5)
    mag[0] = 4.0
    r = R.analyze_spectrum(mag, None, R.Params(SR, method=R.HPS, window_size=256, spectral_smoothing_len=1))
    assert r["f0"] == 0.0 and len(r["peaks"]) == 0 and r["harmonic_ratio"] == 20.0 * math.log10(4.0 ** 5 + 1e-10)
    r = R.analyze_spectrum(mag, None, R.Params(SR, method=R.HPS, window_size=256, spectral_smoothing_len=1,
                                               max_harmonics=2))       # harmonics 2 .. min(5, 2)
    assert r["harmonic_ratio"] == 20.0 * math.log10(4.0 ** 2 + 1e-10)


@pytest.mark.parametrize("W,want", [(256, 200.0), (2048, math.nan)])
def test_f94_acf_200_db_and_nan(W, want):
    """Correlations[0] is lag -(W - 1), so lag 0 stays in: Pearson's 1 gives 20 log10(1 / 1e-10) = 200; the
    un-normalised frequency-domain lag 0 is about W, 1 - W is negative, the logarithm NaN"""
    x = HC.signal(W, W, 1)
    r = R.analyze_frame(x, HC.ref_params("acf", W, W))
    assert r["periodicity"] == r["voicing"]
    if W == 256:
        assert r["voicing"] == 1.0 and r["harmonic_ratio"] == want
    else:
        assert r["voicing"] > 0.5 * W and math.isnan(r["harmonic_ratio"])


def test_f95_yin_threshold_0_never_finds_a_pitch():
    """the temporary detector's threshold is 0 and the CMNDF is never negative: no tau, confidence 0, -200 dB"""
    r = R.analyze_frame(HC.signal(256, 256, 1), HC.ref_params("yin", 256, 256))
    assert r["f0"] == 0.0 and r["f0_confidence"] == 0.0 and r["harmonic_ratio"] == 20.0 * math.log10(1e-10)


def test_f96_bin_frequencies_agree_at_a_power_of_two():
    """i sr / W (freqBins) and i (sr / W) (the detector) are the same double because sr / W is exact there; at
    another W they differ somewhere"""
    for sr in (16000, 44100, 22050):
        for W in (64, 256, 2048):
            assert all(float(i) * float(sr) / float(W) == float(i) * (float(sr) / float(W)) for i in range(W // 2))
    assert any(float(i) * 44100.0 / 1000.0 != float(i) * (44100.0 / 1000.0) for i in range(500))


def test_f97_tracker_by_hand():
    """raw 10, 20, 30, 40, 50 with smoothing: 10, 13, 18.1, 24.67, 32.269.  Both measures are taken before the
    frame's own value enters the history: frame 2 sees [10, 13] (coherence exp(-3 / 10), no stability yet), frame
    3 sees [10, 13, 18.1]: mean 13.7, variance (3.7^2 + 0.7^2 + 4.4^2) / 2 = 16.77."""
    t = R.track(R.Params(SR), [10.0, 20.0, 30.0, 40.0, 50.0])
    assert np.allclose(t["harmonic_ratio"], [10.0, 13.0, 18.1, 24.67, 32.269], rtol=1e-14)
    assert t["temporal_coherence"][0] == 0.0 and t["temporal_coherence"][1] == 0.0
    assert abs(t["temporal_coherence"][2] - math.exp(-0.3)) < 1e-15
    assert abs(t["temporal_coherence"][3] - math.exp(-0.405)) < 1e-15
    assert not t["temporal_stability"][:3].any()
    assert abs(t["temporal_stability"][3] - (1.0 - math.sqrt(16.77) / 13.7)) < 1e-14
    off = R.track(R.Params(SR, use_temporal_smoothing=False), [10.0, 20.0, 30.0])
    assert off["harmonic_ratio"].tolist() == [10.0, 20.0, 30.0]
    # a history of 2 x 1 entries; none at length 0: nothing is smoothed and both measures stay 0
    short = R.track(R.Params(SR, temporal_smoothing_len=1), [10.0, 20.0, 30.0, 40.0])
    assert not short["temporal_stability"].any() and abs(short["temporal_coherence"][3] - math.exp(-0.51)) < 1e-15    # [13, 18.1]
    none = R.track(R.Params(SR, temporal_smoothing_len=0), [10.0, 20.0, 30.0])
    assert none["harmonic_ratio"].tolist() == [10.0, 20.0, 30.0] and not none["temporal_coherence"].any()
    neg = R.track(R.Params(SR), [-10.0, -20.0, -30.0, -40.0])          # mean <= 0: stability 0
    assert not neg["temporal_stability"].any()
    with pytest.raises(IndexError, match=r"slice bounds out of range \[3:1\]"):
        R.track(R.Params(SR, temporal_smoothing_len=-1), [1.0])


# ------------------------------------------------- the library's host side ----
@pytest.mark.parametrize("kw", [dict(), dict(use_temporal_smoothing=False), dict(temporal_smoothing_len=1),
                                dict(temporal_smoothing_len=0), dict(temporal_smoothing_len=9)])
def test_f97_library_tracker_equals_checker(kw):
    rng = np.random.default_rng(5)
    raw = np.concatenate((rng.uniform(-30.0, 40.0, 60), [math.inf, -math.inf, math.nan, 60.0, 60.0, -200.0], rng.uniform(0, 30, 10)))
    ref = R.track(R.Params(SR, **kw), raw)
    got = sonar.hratio_track(sonar.hratio_params_default(SR, **{k: int(v) for k, v in kw.items()}), raw, np.zeros(len(raw)))
    for k in ref:
        assert np.array_equal(got[k], ref[k], equal_nan=True), k
    assert sonar.hratio_track(sonar.hratio_params_default(SR), [])["harmonic_ratio"].shape == (0,)


def test_f97_negative_history_length_is_a_panic():
    with pytest.raises(sonar.SonarError) as e:
        sonar.hratio_track(sonar.hratio_params_default(SR, temporal_smoothing_len=-2), [1.0, 2.0])
    assert e.value.code == sonar.ERR_PANIC and e.value.msg == "runtime error: slice bounds out of range [5:1]"


def test_host_one_liners():
    vals = [30.0, 20.0, 19.999, 10.0, 5.0, 4.9, 0.0, -0.1, -60.0, -61.0, math.nan, math.inf, -math.inf]
    for v in vals:
        assert sonar.hratio_classify(v) == R.classify(v), v
        q = sonar.hratio_voicing_quality(v)
        assert q == R.voicing_quality(v) or (math.isnan(q) and math.isnan(v)), v
    assert sonar.hratio_classify(20.0) == "Very High" and sonar.hratio_classify(math.nan) == "Very Low"
    assert sonar.hratio_voicing_quality(5.0) == 0.5
    assert sonar.hratio_average(vals[:10]) == R.average(vals[:10]) == sum(vals[:8]) / 8.0     # -60 and below are out
    assert sonar.hratio_average([-60.0, -70.0, math.nan]) == 0.0 and sonar.hratio_average([]) == 0.0
    L = sonar.lib()
    assert [L.sonar_hratio_category_name(i) for i in (-1, 5)] == [None, None]
    assert [L.sonar_hratio_category_name(i).decode() for i in range(5)] == sonar.HRATIO_CATEGORIES
    assert [sonar.hratio_method_name(i) for i in range(6)] == R.METHOD_NAMES and sonar.hratio_method_name(6) == "Unknown"


def test_defaults_are_the_constructors():
    p, r = sonar.hratio_params_default(44100), R.Params(44100)
    for name in ("sample_rate", "method", "window_size", "hop_size", "min_freq", "max_freq", "max_harmonics",
                 "harmonic_tolerance", "min_peak_height", "peak_detection_width", "spectral_smoothing_len",
                 "noise_floor_percentile", "noise_floor_smoothing_len", "use_temporal_smoothing",
                 "temporal_smoothing_len", "autocorr_max_lag"):
        assert getattr(p, name) == getattr(r, name), name
    assert p.noise_floor_method == sonar.HRATIO_NOISE_METHODS[r.noise_floor_method]
    assert (p.use_freq_weighting, p.use_psychoacoustic_mask, p.adaptive_threshold) == (0, 0, 0)
    assert sonar.hratio_params_default(SR, noise_floor_method="no such name").noise_floor_method == 1
    assert sonar.HRATIO_METHODS == HC.METHODS


CHECKS = [(dict(), 0), (dict(method=99), 0), (dict(noise_floor_method=7), 0),
          (dict(window_size=64, autocorr_max_lag=63), 0), (dict(max_harmonics=64), 0),
          (dict(max_harmonics=-3), 0), (dict(noise_floor_percentile=1.5), 0),
          (dict(temporal_smoothing_len=-1), 0),     # the per-frame entries never reach :996
          (dict(sample_rate=0), sonar.ERR_INVALID), (dict(hop_size=0), sonar.ERR_INVALID),
          (dict(max_freq=math.inf), sonar.ERR_INVALID), (dict(min_freq=math.nan), sonar.ERR_INVALID),
          (dict(harmonic_tolerance=math.nan), sonar.ERR_INVALID), (dict(min_peak_height=-math.inf), sonar.ERR_INVALID),
          (dict(noise_floor_percentile=math.nan), sonar.ERR_PANIC),
          (dict(noise_floor_percentile=math.nan, noise_floor_method="median"), 0),
          (dict(method="hps", min_freq=-100.0), sonar.ERR_PANIC), (dict(method="hnr", min_freq=-100.0), 0),
          (dict(method="hps", min_freq=-100.0, max_freq=-200.0), 0),    # the scan never starts
          (dict(window_size=1000), sonar.ERR_UNSUPPORTED), (dict(window_size=32), sonar.ERR_UNSUPPORTED),
          (dict(window_size=4096, autocorr_max_lag=4096), sonar.ERR_UNSUPPORTED),
          (dict(max_harmonics=65), sonar.ERR_UNSUPPORTED), (dict(autocorr_max_lag=2046), sonar.ERR_UNSUPPORTED),
          (dict(max_freq=1e300), sonar.ERR_UNSUPPORTED)]


@pytest.mark.parametrize("kw,code", CHECKS, ids=lambda v: str(v))
def test_parameter_checks_without_a_device(kw, code):
    p = sonar.hratio_params_default(kw.get("sample_rate", SR), **{k: v for k, v in kw.items() if k != "sample_rate"})
    assert sonar.hratio_check(p) == code
    assert sonar.lib().sonar_hratio_check(None) == sonar.ERR_INVALID


def test_hratio_params_layout(tmp_path):
    """The ctypes mirror against the header as a C99 compiler lays it out (-pedantic -Werror)."""
    exe = str(tmp_path / "hratio_layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-O1",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_abi", "hratio_layout.c"),
                    "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert out[0].split() == ["size", "sonar_hratio_params", str(ctypes.sizeof(sonar.HratioParams))]
    offs = {line.split()[1]: int(line.split()[2]) for line in out if line.startswith("offset")}
    assert offs == {n: getattr(sonar.HratioParams, n).offset for n, _ in sonar.HratioParams._fields_}
    assert out[-1].split() == ["enum", "hnr", "0", "yin", "5", "minimum", "2", "very_high", "4", "max_harmonics", "64"]
    assert sonar.HRATIO_MAX_HARMONICS == 64 and sonar.HRATIO_NOISE_METHODS == {"median": 0, "percentile": 1, "minimum": 2}


def test_abi_version_and_symbols():
    assert sonar.abi_version() == 4
    lib = ctypes.CDLL(sonar.LIB_PATH)
    for n in ("sonar_hratio_params_default", "sonar_hratio_check", "sonar_hratio_from_spectrum", "sonar_hratio_frames",
              "sonar_hratio_track", "sonar_hratio", "sonar_hratio_average", "sonar_hratio_classify",
              "sonar_hratio_category_name", "sonar_hratio_voicing_quality"):
        assert n in sonar.EXPORTED_SYMBOLS and hasattr(lib, n)


# ------------------------------------- the GPU cases, as the checker sees them ----
@pytest.mark.parametrize("method,W,H,F", HC.PCM_CASES)
def test_pcm_cases_are_decided_in_the_reference(method, W, H, F):
    """at most 10 % of a case's frames are undecided (margin <= 1000 tol) under either transform, and at least
    four are decided; the two orderings agree on every discrete output of the decided frames"""
    tol, measured, decided = HC.pcm_tolerance(method, W, H, F)
    assert 0.0 < measured and tol < 1e-11
    assert np.count_nonzero(~decided) <= 0.1 * F and np.count_nonzero(decided) >= 4
    a, b = HC.pcm_ref(method, W, H, F, "numpy"), HC.pcm_ref(method, W, H, F, "go")
    for k in ("num_harmonics", "h_bin", "f0", "h_freq"):
        assert np.array_equal(a[k][decided], b[k][decided]), k
    assert a["num_harmonics"].max() > 0


@pytest.mark.parametrize("method,W,F,nf", HC.SPECTRUM_CASES)
def test_spectrum_cases_reach_their_code(method, W, F, nf):
    """the rows are compared bit for bit, so nothing is undecided; the cases must find harmonics, and the HNR
    ones a floor"""
    r = HC.spectrum_ref(method, W, F, nf)
    assert r["num_harmonics"].max() > 0 and np.count_nonzero(r["f0"]) > 0
    if method in ("hnr", "comb"):
        assert r["noise_floor"].max() > 0 and np.isfinite(r["snr"]).all() and r["noise_energy"].min() > 0
