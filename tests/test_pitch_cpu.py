"""The parts of the full pitch detector that need no GPU: known answers for the Python checker
(tests/pitch_ref.py) worked out by hand, the checker's YIN and tracker against the C oracle at the
constructor's defaults, the library's tracker and stability code (host_dsp.cpp, through the stand-alone
program tests/c_abi/pitch_track_check.cpp) against the checker exactly, the layout of sonar_pitch_params,
and the argument checks that need no device."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import oracle as O
import pitch_ref as R
import sonar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 16000


def _plain(**kw):
    """no pre-emphasis, rectangular window: the frame reaches the method as it is"""
    return R.Params(SR, pre_emphasis=False, window_function="rectangular", **kw)


# ----------------------------------------------------------- known answers ----
@pytest.mark.parametrize("method", [R.YIN, R.YIN_FFT, R.NSDF, R.MPM])
@pytest.mark.parametrize("W,P", [(256, 40), (1024, 100)])
def test_periodic_frame_gives_its_period(method, W, P):
    """x[n] = table[n mod P]: x[j + P] == x[j] exactly, so the YIN difference at lag P is 0 (cmndf 0, the
    first dip below the threshold that is a local minimum; confidence 1) and the NSDF there is 2 a / (a + a)
    = 1 exactly.  The frequency range keeps lag 2 P out (sr / 2P < min_freq < sr / P)."""
    table = np.sin(2.0 * np.pi * np.arange(P) / P)
    x = table[np.arange(W) % P]
    p = _plain(method=method, window_size=W, min_freq=0.75 * SR / P, max_freq=1.5 * SR / P)
    r = R.detect_frame(x, p)
    assert r["index"] == P and r["n_candidates"] == 1 and r["confidence"] == 1.0
    if method in (R.YIN, R.YIN_FFT):
        # the parabola through cmndf[P - 1], 0, cmndf[P + 1] is not symmetric (the running mean grows with the
        # lag), so the interpolated period sits a small fraction of a sample off P
        assert r["curve"][P] == 0.0 and abs(SR / r["pitch"] - P) < 0.05
    else:
        assert r["curve"][P] == 1.0 and r["pitch"] == SR / P


@pytest.mark.parametrize("k", [1, 7, 50])
def test_k_cycles_give_2k_minus_1_crossings(k):
    """k whole cycles are 2 k half-cycles of alternating sign: 2 k - 1 sign changes; the half-sample phase
    keeps every sample off zero.  Pitch = crossings sr / (2 W), confidence 0.3."""
    W = 512
    x = np.sin(2.0 * np.pi * k * (np.arange(W) + 0.5) / W)
    r = R.detect_frame(x, _plain(method=R.ZERO_CROSSING, window_size=W))
    assert r["index"] == 2 * k - 1 and r["confidence"] == 0.3 and r["n_candidates"] == 1
    assert r["pitch"] == (2 * k - 1) * SR / (2.0 * W) and len(r["curve"]) == 0


@pytest.mark.parametrize("method", [R.HPS, R.PEAKS])
@pytest.mark.parametrize("fft", ["numpy", "go"])
def test_comb_gives_its_hps_bin(method, fft):
    """Five harmonics of W-bin 8 (whole cycles in the frame, no leakage) under zero padding 2: lines at
    bins 16 h of the 512-point transform; only bin 16 has all of its harmonics 2..5 on a line."""
    W, b = 256, 8
    n = np.arange(W)
    x = sum(np.cos(2.0 * np.pi * h * b * n / W) for h in range(1, 6))
    r = R.detect_frame(x, _plain(method=method, window_size=W, zero_padding=2), fft=fft)
    assert r["index"] == 16 and r["pitch"] == 16.0 * SR / 512.0
    assert r["confidence"] == 1.0 and len(r["curve"]) == 256       # (W / 2)^5 / 1000 > 1


@pytest.mark.parametrize("fft", ["numpy", "go"])
def test_constant_frame_is_the_hps_bin_0_case(fft):
    """A constant frame has all its magnitude in bin 0: nothing in the scan range beats hps[0] = W^5, so the
    pitch is 0 Hz and the confidence min(W^5 / 1000, 1) = 1 is still reported."""
    r = R.detect_frame(np.ones(256), _plain(method=R.HPS, window_size=256, zero_padding=1), fft=fft)
    assert r["index"] == 0 and r["pitch"] == 0.0 and r["confidence"] == 1.0 and r["n_candidates"] == 1
    assert r["curve"][0] == 256.0 ** 5


@pytest.mark.parametrize("fft", ["numpy", "go"])
def test_impulse_train_gives_its_quefrency(fft):
    """Impulses every P = 32 samples of a 512-sample frame: |X| is 16 at every 16th bin and 0 between, so the
    log spectrum is a pulse train of period 16 bins and the cepstrum one of period 32, positive there
    ((ln 16 - ln 1e-10) / 16 = 1.612...) and equal to the floor's share elsewhere; the range 300-1000 Hz
    scans quefrencies 16..52, which hold P alone."""
    W, P = 512, 32
    x = (np.arange(W) % P == 0).astype(np.float64)
    r = R.detect_frame(x, _plain(method=R.CEPSTRUM, window_size=W, min_freq=300.0, max_freq=1000.0), fft=fft)
    assert r["index"] == P and r["pitch"] == SR / P and r["confidence"] == 1.0
    assert abs(r["curve"][P] - (math.log(16.0 + 1e-10) - math.log(1e-10)) / 16.0) < 1e-12


def _track(p, rows):
    rows = [(r + (1, 0.0))[:4] for r in rows]
    return R.track(p, *zip(*rows))


def _tp(**kw):
    return R.Params(SR, **kw)


@pytest.mark.parametrize("pitch,ratio,corrected", [(95.0, 0.5, 100.0), (410.0, 2.0, 400.0),
                                                  (64.0, 1.0 / 3.0, 200.0 * (1.0 / 3.0)), (630.0, 3.0, 600.0)])
def test_tracker_octave_ratios(pitch, ratio, corrected):
    """Three frames at 200 Hz make the median 200.  A pitch within 10 % of median * ratio moves there only when
    that is closer to the median than the pitch itself: 95 -> 100, 410 -> 400, 64 -> 66.7, 630 -> 600."""
    t = _track(_tp(temporal_smoothing=False), [(200.0, 0.9)] * 3 + [(pitch, 0.9)])
    assert t["pitch"][3] == corrected and t["f0_multiple"][3] == ratio
    assert np.all(t["f0_multiple"][:3] == 0.0)
    off = _track(_tp(temporal_smoothing=False, octave_correction=False), [(200.0, 0.9)] * 3 + [(pitch, 0.9)])
    assert off["pitch"][3] == pitch and off["f0_multiple"][3] == 0.0


def test_tracker_octave_keeps_the_closer_pitch():
    """105 is within 10 % of 100 = median / 2 but closer to the median than 100 is: it stays, and the loop ends
    at that ratio."""
    t = _track(_tp(temporal_smoothing=False), [(200.0, 0.9)] * 3 + [(105.0, 0.9)])
    assert t["pitch"][3] == 105.0 and t["f0_multiple"][3] == 0.0


def test_tracker_gate_spares_periodicity_and_the_quality_measures():
    """confidence 0.4 < 0.5: pitch, confidence and voicing are zeroed after clarity (one candidate: its
    confidence), strength ((0.4 + 0.4) / 2) and salience (0.4 * 1.2 at 200 Hz) were computed."""
    t = _track(_tp(), [(200.0, 0.4)])
    assert (t["pitch"][0], t["confidence"][0], t["voicing"][0]) == (0.0, 0.0, 0.0)
    assert t["periodicity"][0] == 0.4 and t["clarity"][0] == 0.4 and t["strength"][0] == 0.4
    assert t["salience"][0] == 0.4 * 1.2
    t = _track(_tp(min_confidence=0.3), [(1500.0, 0.4, 2, 0.1)])
    assert (t["pitch"][0], t["confidence"][0]) == (1500.0, 0.4)
    assert t["salience"][0] == 0.4 * 0.8 and t["clarity"][0] == (0.4 - 0.1) / 0.4


def test_tracker_exponential_branch_then_median():
    """Frame 1 is not smoothed (one history entry).  Frame 2 has two entries, fewer than three: 0.3 p + 0.7
    previous.  Frame 3 takes the median of three."""
    t = _track(_tp(octave_correction=False), [(200.0, 0.9), (300.0, 0.9), (400.0, 0.9)])
    assert list(t["pitch"]) == [200.0, 0.3 * 300.0 + (1 - 0.3) * 200.0, 300.0]
    # median_filter 2 never reaches three entries: always exponential, against the previous smoothed pitch
    t = _track(_tp(octave_correction=False, median_filter=2), [(200.0, 0.9), (300.0, 0.9), (400.0, 0.9)])
    second = 0.3 * 300.0 + (1 - 0.3) * 200.0
    assert list(t["pitch"]) == [200.0, second, 0.3 * 400.0 + (1 - 0.3) * second]
    t = _track(_tp(octave_correction=False, temporal_smoothing=False), [(200.0, 0.9), (300.0, 0.9)])
    assert list(t["pitch"]) == [200.0, 300.0]


def test_tracker_median_widths_3_and_5():
    rows = [(100.0 * k, 0.9) for k in range(1, 6)]
    assert list(_track(_tp(octave_correction=False, median_filter=3), rows)["pitch"][2:]) == [200.0, 300.0, 400.0]
    # width 5: three entries -> 200; four -> (200 + 300) / 2; five -> 300
    assert list(_track(_tp(octave_correction=False, median_filter=5), rows)["pitch"][2:]) == [200.0, 250.0, 300.0]
    # zeros (gated frames) are left out of the median: [100, 0, 300] -> (100 + 300) / 2
    t = _track(_tp(octave_correction=False), [(100.0, 0.9), (200.0, 0.1), (300.0, 0.9)])
    assert t["pitch"][2] == 200.0


def test_tracker_history_wraps_at_20_and_stability():
    """Stability is 1 - sd / mean over the history's positive entries.  After 25 frames of 100 + i the history
    holds 105..124: mean 114.5, and the variance of 20 consecutive integers is 20 * 21 / 12 = 35."""
    p = _tp(octave_correction=False, temporal_smoothing=False)
    t = _track(p, [(100.0 + i, 0.9) for i in range(25)])
    assert t["stability"][0] == 0.0 and t["stability"][1] == 0.0       # fewer than three entries
    assert abs(t["stability"][24] - (1.0 - math.sqrt(35.0) / 114.5)) < 1e-15
    assert abs(t["stability"][19] - (1.0 - math.sqrt(35.0) / 109.5)) < 1e-15
    assert list(_track(p, [(100.0, 0.9)] * 4)["stability"]) == [0.0, 0.0, 1.0, 1.0]
    # the history holds the UNSMOOTHED pitches: smoothing changes the pitch column, not the stability
    s = _track(_tp(octave_correction=False), [(100.0 + i, 0.9) for i in range(25)])
    assert np.array_equal(s["stability"], t["stability"]) and not np.array_equal(s["pitch"], t["pitch"])


def test_analyze_pitch_stability_known_answer():
    """Ten voiced values 100, 102, 100, 98, ... and two unvoiced: mean 100.2, every step 2 Hz (jitter 2), the
    detrended signs - + - - - + - - - + cross five times: 5 / (2 * 10 / (16000 / 512)) = 7.8125 Hz."""
    v = [100.0, 102.0, 100.0, 98.0, 100.0, 102.0, 100.0, 98.0, 100.0, 102.0]
    s = R.stability([0.0] + v + [0.0], SR, 512)
    assert abs(s["mean_pitch"] - 100.2) < 1e-12 and s["jitter"] == 2.0
    sd = math.sqrt(sum((x - 100.2) ** 2 for x in v) / 9.0)
    assert abs(s["pitch_std_dev"] - sd) < 1e-12
    assert abs(s["coefficient_of_variation"] - sd / 100.2) < 1e-14
    assert abs(s["stability"] - 1.0 / (1.0 + sd / 100.2)) < 1e-14
    assert s["vibrato_rate"] == 7.8125 and s["voiced_frames_ratio"] == 10.0 / 12.0
    assert R.stability(v[:9], SR, 512)["vibrato_rate"] == 0.0          # fewer than ten voiced frames
    assert R.stability([100.0], SR, 512) == {} and R.stability([0.0, 100.0, 0.0], SR, 512) == {}


# ------------------------------------------------------ checker vs oracle ----
def test_checker_yin_equals_oracle_yin_raw():
    x = R.make_signal(40, 1024, 512, seed=5)
    p = R.Params(SR)
    found = 0
    for f in range(40):
        frame = x[f * 512:f * 512 + 1024]
        r = R.detect_frame(frame, p)
        op, oc, ot = O.yin_raw(frame, SR)
        assert (r["pitch"], r["confidence"], r["index"]) == (op, oc, ot)
        found += r["n_candidates"]
    assert found >= 5                                                   # the comparison is not of zeros


def test_checker_detect_equals_oracle_pitch_track():
    """ProcessAudioStream at the defaults against the oracle's tracked rows (pitch, confidence, voicing)"""
    x = R.make_signal(40, 1024, 512, seed=6)
    got = R.detect(x, R.Params(SR))
    op, oc, ov = O.pitch_track(x, SR)
    assert np.array_equal(got["pitch"], op) and np.array_equal(got["confidence"], oc)
    assert np.array_equal(got["voicing"], ov)


# ------------------------------------------- library tracker vs the checker ----
@pytest.fixture(scope="module")
def track_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pitch") / "pitch_track_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O2", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "c_abi", "pitch_track_check.cpp"),
                    os.path.join(ROOT, "sonido-sonar_amd", "csrc", "host_dsp.cpp"), "-o", exe], check=True)
    return exe


def _run_track(exe, p, rows):
    text = "T %d %d %d %s %d\n" % (p.octave_correction, p.temporal_smoothing, p.median_filter,
                                   float(p.min_confidence).hex(), len(rows))
    text += "".join("%s %s %d %s\n" % (float(a).hex(), float(b).hex(), c, float(d).hex()) for a, b, c, d in rows)
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout
    vals = np.array([[float.fromhex(t) for t in line.split()] for line in out.splitlines()], dtype=np.float64)
    return vals.reshape(len(rows), 12)


def _random_rows(seed, F):
    """raw rows as the methods produce them: runs around one pitch with octave slips, unvoiced zeros, low
    confidences on both sides of the gate, one or several candidates"""
    rng = np.random.default_rng(seed)
    rows = []
    base = rng.uniform(90.0, 600.0)
    for f in range(F):
        if rng.random() < 0.1:
            base = rng.uniform(90.0, 600.0)
        u = rng.random()
        if u < 0.15:
            rows.append((0.0, 0.0, 0, 0.0))
            continue
        pitch = base * rng.choice([1.0, 1.0, 1.0, 0.5, 2.0, 1.0 / 3.0, 3.0]) * rng.uniform(0.93, 1.07)
        conf = rng.uniform(0.2, 1.0)
        nc = int(rng.integers(1, 4))
        rows.append((pitch, conf, nc, conf * rng.uniform(0.0, 1.0) if nc > 1 else 0.0))
    return rows


TRACK_PARAMS = [dict(), dict(octave_correction=False), dict(temporal_smoothing=False), dict(median_filter=0),
                dict(median_filter=2), dict(median_filter=5), dict(median_filter=20), dict(median_filter=25),
                dict(min_confidence=0.0), dict(min_confidence=0.9, median_filter=7)]


@pytest.mark.parametrize("kw", TRACK_PARAMS, ids=lambda kw: "-".join("%s=%s" % i for i in kw.items()) or "defaults")
def test_library_tracker_equals_checker(track_check, kw):
    p = _tp(**kw)
    rows = _random_rows(len(kw) * 17 + p.median_filter, 120)
    got = _run_track(track_check, p, rows)
    ref = R.track(p, *zip(*rows))
    for k, name in enumerate(R.TRACK_FIELDS):
        assert np.array_equal(got[:, k], ref[name], equal_nan=True), name
    assert np.count_nonzero(ref["f0_multiple"]) > 0 or not p.octave_correction
    if not kw:      # the constructor's defaults: YinTracker::step, the tracker the extractors use, agrees
        assert np.array_equal(got[:, 9], ref["pitch"]) and np.array_equal(got[:, 10], ref["confidence"])
        assert np.array_equal(got[:, 11], ref["voicing"])


def test_library_tracker_on_non_finite_rows(track_check):
    rows = [(200.0, 0.9, 1, 0.0)] * 3 + [(math.nan, math.nan, 1, 0.0), (math.inf, 0.9, 2, 0.5), (200.0, 0.9, 1, 0.0)]
    p = _tp()
    got = _run_track(track_check, p, rows)
    ref = R.track(p, *zip(*rows))
    for k, name in enumerate(R.TRACK_FIELDS):
        assert np.array_equal(got[:, k], ref[name], equal_nan=True), name


def test_library_stability_equals_checker(track_check):
    rng = np.random.default_rng(11)
    cases = [rng.uniform(80.0, 500.0, n) * (rng.random(n) > 0.2) for n in (0, 1, 2, 3, 9, 10, 11, 200)]
    cases += [np.zeros(5), np.array([0.0, 100.0, 0.0]), np.full(12, 220.0)]
    for seq in cases:
        text = "S %d %d %d\n" % (SR, 512, len(seq)) + " ".join(float(v).hex() for v in seq) + "\n"
        out = subprocess.run([track_check], input=text, check=True, capture_output=True, text=True).stdout.split()
        ok, vals = int(out[0]), [float.fromhex(t) for t in out[1:]]
        ref = R.stability(list(seq), SR, 512)
        assert ok == (1 if ref else 0)
        if ref:
            for k, name in enumerate(R.STABILITY_KEYS):
                assert vals[k] == ref[name] or (vals[k] != vals[k] and ref[name] != ref[name]), (name, len(seq))
        # the same through the library's entry
        got = sonar.pitch_stability(seq, SR, 512)
        assert set(got) == set(ref)
        for name in ref:
            assert got[name] == ref[name] or (got[name] != got[name] and ref[name] != ref[name])


def test_library_pitch_track_entry_equals_checker():
    """sonar_pitch_track itself (the loaded library), on one parameter set"""
    p = _tp(median_filter=5)
    rows = _random_rows(3, 80)
    ref = R.track(p, *zip(*rows))
    sp = sonar.pitch_params_default(SR, median_filter=5)
    got = sonar.pitch_track(sp, *[list(c) for c in zip(*rows)])
    for name in R.TRACK_FIELDS:
        assert np.array_equal(got[name], ref[name]), name


# ----------------------------------------------------------- ABI, arguments ----
def test_pitch_params_layout(tmp_path):
    """The ctypes mirror against the header as a C99 compiler lays it out (-pedantic -Werror)."""
    exe = str(tmp_path / "pitch_layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-O1",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_abi", "pitch_layout.c"),
                    "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert out[0].split() == ["size", "sonar_pitch_params", str(ctypes.sizeof(sonar.PitchParams))]
    offs = {line.split()[1]: int(line.split()[2]) for line in out if line.startswith("offset")}
    assert offs == {n: getattr(sonar.PitchParams, n).offset for n, _ in sonar.PitchParams._fields_}
    assert out[-1].split() == ["enum", "yin", "0", "praat", "10", "rectangular", "3"]
    assert sonar.PITCH_METHODS["yin"] == R.YIN and sonar.PITCH_METHODS["praat"] == R.PRAAT
    assert sonar.PITCH_METHODS["mpm"] == R.MPM and sonar.PITCH_WINDOWS == R.WINDOWS


def test_abi_version_and_symbols():
    assert sonar.abi_version() == 4
    names = ["sonar_pitch_params_default", "sonar_pitch_detect_frames", "sonar_pitch_curve_width",
             "sonar_pitch_frames_raw", "sonar_pitch_track", "sonar_pitch_detect", "sonar_pitch_stability"]
    lib = ctypes.CDLL(sonar.LIB_PATH)
    with open(os.path.join(ROOT, "include", "sonar_gpu.h")) as f:
        header = f.read()
    for n in names:
        assert n in sonar.EXPORTED_SYMBOLS and hasattr(lib, n)
        assert re.search(r"\b%s\s*\(" % n, header)


def test_defaults_are_new_pitch_detector():
    p, r = sonar.pitch_params_default(44100), R.Params(44100)
    for name in ("sample_rate", "method", "window_size", "hop_size", "min_freq", "max_freq", "yin_threshold",
                 "autocorr_threshold", "min_confidence", "zero_padding", "median_filter"):
        assert getattr(p, name) == getattr(r, name), name
    assert (p.pre_emphasis, p.temporal_smoothing, p.octave_correction, p.window_function) == (1, 1, 1, 0)
    assert (p.cepstral_threshold, p.min_salience, p.voicing_threshold, p.max_harmonics, p.harmonic_tolerance) == \
        (0.3, 0.1, 0.45, 10, 0.1)
    assert sonar.pitch_params_default(SR, window_function="kaiser").window_function == 0   # unknown: Hann
    assert sonar.pitch_method_name(2) == "Normalized Square Difference Function"
    assert sonar.pitch_method_name(11) == "Unknown"


def test_detect_frames_counts_whole_frames():
    for n, W, H in [(0, 64, 1), (63, 64, 1), (64, 64, 1), (65, 64, 1), (1024 + 3 * 512, 1024, 512),
                    (1024 + 3 * 512 - 1, 1024, 512), (5000, 128, 300)]:
        assert sonar.pitch_detect_frames(n, W, H) == R.detect_frames(n, W, H)
    assert sonar.pitch_detect_frames(1024 + 3 * 512, 1024, 512) == 4
    assert sonar.pitch_detect_frames(1024 + 3 * 512 - 1, 1024, 512) == 3
    assert sonar.pitch_detect_frames(100, 0, 1) == 0 and sonar.pitch_detect_frames(100, 64, 0) == 0


WIDTHS = [("yin", 1024, 2, 512), ("yin_fft", 64, 2, 32), ("nsdf", 128, 2, 64), ("mpm", 2048, 2, 1024),
          ("acf", 512, 2, 1023), ("acf", 1024, 2, 2047), ("hps", 1024, 2, 1024), ("hps", 1024, 4, 2048),
          ("peaks", 2048, 1, 1024), ("cepstrum", 256, 2, 256), ("zero_crossing", 64, 2, 0)]


@pytest.mark.parametrize("method,W,zp,width", WIDTHS)
def test_curve_width(method, W, zp, width):
    assert sonar.pitch_curve_width(sonar.pitch_params_default(SR, method=method, window_size=W, zero_padding=zp)) == width


ERRORS = [
    (dict(method=7), sonar.ERR_INVALID), (dict(method=10), sonar.ERR_INVALID), (dict(method=11), sonar.ERR_INVALID),
    (dict(method=-1), sonar.ERR_INVALID),
    (dict(method=7, window_size=100, hop_size=0), sonar.ERR_INVALID),          # the method comes first
    (dict(hop_size=0), sonar.ERR_INVALID), (dict(sample_rate=0), sonar.ERR_INVALID),
    (dict(min_freq=0.0), sonar.ERR_INVALID), (dict(min_freq=1000.0), sonar.ERR_INVALID),
    (dict(min_freq=2000.0), sonar.ERR_INVALID), (dict(max_freq=math.inf), sonar.ERR_INVALID),
    (dict(min_freq=math.nan), sonar.ERR_INVALID), (dict(min_freq=-5.0), sonar.ERR_INVALID),
    (dict(method="hps", zero_padding=0), sonar.ERR_PANIC), (dict(method="peaks", zero_padding=-1), sonar.ERR_PANIC),
    (dict(method="cepstrum", window_size=128, max_freq=125.0), sonar.ERR_PANIC),   # int(16000 / 125) = 128 >= W
    (dict(window_size=100), sonar.ERR_UNSUPPORTED), (dict(window_size=32), sonar.ERR_UNSUPPORTED),
    (dict(window_size=4096), sonar.ERR_UNSUPPORTED), (dict(window_size=0), sonar.ERR_UNSUPPORTED),
    (dict(method="hps", zero_padding=3), sonar.ERR_UNSUPPORTED),
    (dict(method="hps", window_size=2048, zero_padding=4), sonar.ERR_UNSUPPORTED),
    (dict(window_function=4), sonar.ERR_UNSUPPORTED),
]


@pytest.mark.parametrize("kw,code", ERRORS, ids=lambda v: str(v))
def test_parameter_errors_without_a_device(kw, code):
    p = sonar.pitch_params_default(kw.get("sample_rate", SR), **{k: v for k, v in kw.items() if k != "sample_rate"})
    with pytest.raises(sonar.SonarError) as e:
        sonar.pitch_curve_width(p)
    assert e.value.code == code
    if code == sonar.ERR_INVALID and "method" in kw and isinstance(kw["method"], int):
        assert e.value.msg == "unsupported pitch detection method: %d" % kw["method"]


def test_parameters_the_methods_do_not_read_are_not_checked():
    """zero_padding belongs to HPS / PEAKS alone; 127 = int(16000 / 125.5) is the last quefrency inside W"""
    assert sonar.pitch_curve_width(sonar.pitch_params_default(SR, zero_padding=0)) == 512
    assert sonar.pitch_curve_width(sonar.pitch_params_default(SR, method="cepstrum", window_size=128,
                                                              min_freq=80.0, max_freq=125.5)) == 128
    assert lib_track_rc(-1) == sonar.ERR_INVALID


def lib_track_rc(F):
    p = sonar.pitch_params_default(SR)
    return sonar.lib().sonar_pitch_track(ctypes.byref(p), F, None, None, None, None, *([None] * 9))
