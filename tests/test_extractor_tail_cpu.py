"""Known answers for the plain-Python restatement of the music, content and voice extractors' scalar tails
(tests/extractor_tail_ref.py), worked out by hand on tiny arrays, so the restatement is pinned independently of
the GPU; and the library's own tails and music plan (csrc/host_dsp.cpp, csrc/music_plan.h, compiled by the plain
host C++ compiler into tests/c_abi/build/extractor_tail_check) against the restatement on the same cases and on
seeded random arrays, exactly: both sides run the same IEEE double operations in the same order and call the
same libm, and every value travels as text that round-trips a double.  No GPU."""
import math
import os
import random
import subprocess

import extractor_tail_ref as R

CABI = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c_abi")
NAN, INF = math.nan, math.inf
FEATURES = ("zero_crossing_rate", "spectral_centroid", "energy_variance", "silence_ratio", "harmonic_ratio",
            "low_freq_energy", "high_freq_energy", "dynamic_range", "temporal_stability", "classification_confidence")
VOICE = ("jitter", "shimmer", "hnr", "noise_measure", "f0_stability", "amplitude_stability", "voicing_strength",
         "overall_quality", "num_periods", "mean_f0", "f0_range", "analysis_quality")


def same(a, b):
    a, b = [float(v) for v in a], [float(v) for v in b]
    return len(a) == len(b) and all(x == y or (math.isnan(x) and math.isnan(y)) for x, y in zip(a, b))


# ---- the restatement against answers worked out by hand ------------------------------------------

def test_go_int_known_answers():
    assert R.go_int(-3.7) == -3 and R.go_int(3.99) == 3 and R.go_int(0.0) == 0
    assert R.go_int(NAN) == R.MIN_INT64 and R.go_int(1e19) == R.MIN_INT64 and R.go_int(-INF) == R.MIN_INT64
    assert R.go_int(9223372036854775808.0) == R.MIN_INT64                       # 2^63 itself is out of range
    assert R.go_int(-9223372036854775808.0) == R.MIN_INT64                      # ... and -2^63 is in it


def test_contrast_edges_known_answers():
    assert R.contrast_edges(0, 513, 6) == [0, 1, 2, 3, 4, 5, 6]                 # Nyquist 0: every bin is int(Inf or NaN)
    # four bins: 200 Hz .. 10 kHz fall in bins 0 and 1, Nyquist in the last; then made strictly rising
    assert R.contrast_edges(44100, 4, 6) == [0, 1, 2, 3, 4, 5, 6]
    e = R.contrast_edges(44100, 513, 6)
    assert e[0] == 4 and e[6] in (511, 512) and all(b > a for a, b in zip(e, e[1:]))   # 200 Hz x 512 / 22050 = 4.6


def test_gonum_variance_known_answers():
    assert R.gonum_variance([]) == 0.0 and R.gonum_variance([3.0]) == 0.0       # fewer than two values
    assert R.gonum_variance([1.0, 2.0, 3.0, 4.0]) == 5.0 / 3.0                   # deviations 1.5, 0.5: 5 over n - 1
    assert R.gonum_variance([2.0, 2.0]) == 0.0


def test_crest_and_entropy_known_answers():
    assert R.crest_factors([1.0, 3.0, 5.0], [0.5, 0.0, 2.0]) == [2.0, 0.0, 2.5]   # no energy: 0
    assert R.energy_entropy([0.0, 0.0]) == ([0.0, 0.0], 0.0)                     # no positive energy: range 0
    assert R.energy_entropy([]) == ([], 0.0)
    ent, lr = R.energy_entropy([0.5, 2.0, 0.0])
    assert ent == [0.5, -2.0, 0.0] and lr == 20 * math.log10(4.0)                # the zero is not the minimum
    assert R.energy_entropy([1.0, 10.0])[1] == 20.0 and R.energy_entropy([3.0])[1] == 0.0


def test_panic_arguments_known_answers():
    assert R.percentile_panics(1536) == (10, 2)                                 # L = 2: int(10 (L - 1)) = 10
    assert R.percentile_panics(1535) == (None, 1) and R.percentile_panics(1023) == (None, 0)
    assert R.percentile_panics(88200) == (1700, 171)                            # 2 s at 44.1 kHz
    assert R.chroma_slice_panics(17, 512, 1300) == 3                            # frame 3 starts at 1536 > 1300
    assert R.chroma_slice_panics(17, 64, 1300) is None
    assert R.chroma_slice_panics(6, 256, 1280) is None                          # (F - 1) hop == n: an empty slice, no panic
    assert R.chroma_slice_panics(6, 256, 1279) == 5


def test_music_plan_known_answers():
    p = R.music_plan(1024, 1, 1024, 44100, 1024, 256)
    assert (p["K"], p["Fe"], p["fse"], p["Fenv"], p["harmonic_live"], p["L"]) == (513, 1, 1024, 1, 1, 1)
    p = R.music_plan(1536, 3, 1024, 44100, 1024, 256)
    assert (p["Fe"], p["fse"], p["Fenv"], p["harmonic_live"], p["L"], p["pct_index"]) == (3, 512, 5, 0, 2, 10)
    p = R.music_plan(512, 1, 512, 44100, 256, 64)
    assert (p["K"], p["Fe"], p["fse"], p["Fenv"], p["L"], p["chroma_bad"]) == (257, 5, 102, 7, 0, -1)
    p = R.music_plan(1300, 17, 256, 44100, 256, 512)                            # chroma panic: nothing after it
    assert (p["chroma_bad"], p["Fe"], p["Fenv"], p["harmonic_live"]) == (3, 0, 0, 0)
    p = R.music_plan(22050, 83, 1024, 44100, 0, 0)                              # hop 0
    assert (p["chroma_bad"], p["Fe"], p["fse"], p["Fenv"]) == (-1, 0, 0, 0)
    assert R.music_plan(44100, 169, 1024, 44100, 0, 256)["Fe"] == 0             # window 0: no energy frame


def _features(**kw):
    f = dict.fromkeys(FEATURES, 0.0)
    f.update(kw)
    return f


def test_content_features_known_answers():
    spec = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]                    # K = 10: one peak, at bin 3
    f = R.content_features(5, 1.0, 0.1, spec, [], [], 11, 2000)
    assert f["zero_crossing_rate"] == 0.5 and f["spectral_centroid"] == 300.0    # bin 3 of 2000 / 20 Hz each
    assert f["harmonic_ratio"] == 0.0                                           # fewer than two peaks
    assert f["low_freq_energy"] == 0.0 and f["high_freq_energy"] == 1.0          # split at bin 10 // 4 = 2
    assert f["dynamic_range"] == 20.0                                           # 1 / 0.1 is 10 in float64
    assert R.content_features(0, 1.0, 0.0, spec, [], [], 11, 2000)["dynamic_range"] == 0.0    # a zero minimum
    assert R.content_features(0, 1.0, INF, spec, [], [], 11, 2000)["dynamic_range"] == 0.0    # ... or an infinite one
    assert R.content_features(0, 0.0, 0.0, [0.0] * 10, [], [], 1, 2000)["zero_crossing_rate"] == 0.0
    spec = [0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0]          # peaks at 2, 6 (3x) and 9 (4.5x)
    assert R.content_features(0, 1.0, 1.0, spec, [], [], 22, 2000)["harmonic_ratio"] == 0.5
    # frames 1024 / 512: mean squares 1, 3 -> population variance 1; one of two frames under RMS 0.01
    f = R.content_features(0, 1.0, 1.0, [0.0] * 10, [1024.0, 3072.0], [], 2048, 2000)
    assert f["energy_variance"] == 1.0 and f["silence_ratio"] == 0.0
    assert R.content_features(0, 1.0, 1.0, [0.0] * 10, [1024.0, 3072.0], [], 2047, 2000)["energy_variance"] == 0.0
    assert R.content_features(0, 1.0, 1.0, [0.0] * 10, [0.0, 3072.0], [], 2048, 2000)["silence_ratio"] == 0.5
    # frames of 100 ms: sums 1, 3 -> mean 2, deviation 1 -> 1 - 1 / 2; three frames' worth of samples are needed
    assert R.content_features(0, 1.0, 1.0, [0.0] * 10, [], [1.0, 3.0], 600, 2000)["temporal_stability"] == 0.5
    assert R.content_features(0, 1.0, 1.0, [0.0] * 10, [], [1.0, 3.0], 599, 2000)["temporal_stability"] == 0.0
    assert R.content_features(0, 1.0, 1.0, [0.0] * 10, [], [0.0, 0.0, 9.0], 600, 2000)["temporal_stability"] == 0.0   # clamped


def test_classifier_known_answers():
    # speech 2 (crossing rate), talk 1.8, music 0, sports 0: a tie at the threshold is not above it
    f = _features(zero_crossing_rate=0.2, harmonic_ratio=0.25, temporal_stability=0.45)
    assert R.classify_content(f, 2.0) == (R.CT_UNKNOWN, 2.0 / 6.0)
    assert R.classify_content(f, 1.9) == (R.CT_NEWS, 2.0 / 6.0)
    assert R.classify_content(f, 3.0) == (R.CT_UNKNOWN, 0.5)
    # music 2 (crossing rate) + 1 (stability), speech 1 (no harmonics) + 2 (centroid): equal scores, music is first
    f = _features(zero_crossing_rate=0.01, temporal_stability=0.6, spectral_centroid=1000.0)
    assert R.classify_content(f, 2.0) == (R.CT_MUSIC, 0.5)
    # sports 2 + 1.5 + 1 against music 2 + 1 and speech 1
    f = _features(energy_variance=0.5, dynamic_range=31.0, temporal_stability=0.1)
    assert R.classify_content(f, 2.0) == (R.CT_SPORTS, 4.5 / 6.0)


def _ac(peak_lag, peak):
    ac = [0.0] * 2048
    ac[0], ac[peak_lag] = 1.0, peak
    return ac


def test_voice_quality_known_answers():
    q = R.voice_quality_from([100, 100, 100], [1.0, 1.0, 1.0], [160.0] * 3, None, [0.0] * 1000, 1000, 16000, 0.0)
    assert (q["jitter"], q["shimmer"], q["hnr"], q["noise_measure"]) == (0.0, 0.0, 0.0, 0.0)
    assert (q["f0_stability"], q["amplitude_stability"], q["mean_f0"], q["f0_range"]) == (1.0, 1.0, 160.0, 0.0)
    assert q["overall_quality"] == 0.75 and q["analysis_quality"] == (0.3 + 1.0 + 0.0) / 3.0 and q["num_periods"] == 3
    q = R.voice_quality_from([100, 110, 100], [1.0, 2.0, 1.0], [160.0] * 3, None, [0.0] * 1000, 1000, 16000, 0.7)
    assert q["jitter"] == (20.0 / 2.0) / (310.0 / 3.0) * 100.0 and q["shimmer"] == (2.0 / 2.0) / (4.0 / 3.0) * 100.0
    assert q["voicing_strength"] == 0.7
    head = [float(i % 2) for i in range(1024)]                                  # 1023 unit steps over 512 ones
    # mean F0 160 at 16 kHz: lag 100, searched over 75 .. 125
    q = R.voice_quality_from([100] * 3, [1.0] * 3, [160.0] * 3, _ac(100, 0.9), head, 4096, 16000, 0.0)
    assert q["hnr"] == 10.0 * math.log10(0.9 / (1.0 - 0.9)) and q["noise_measure"] == 1023.0 / 512.0
    for peak in (1.0, 2.0):                                                     # mc >= ac[0]: no ratio
        assert R.voice_quality_from([100] * 3, [1.0] * 3, [160.0] * 3, _ac(100, peak), head, 4096, 16000, 0.0)["hnr"] == 0.0
    assert R.voice_quality_from([100] * 3, [1.0] * 3, [160.0] * 3, _ac(126, 0.9), head, 4096, 16000, 0.0)["hnr"] == 0.0
    assert R.voice_quality_from([100] * 3, [1.0] * 3, [160.0] * 3, _ac(125, 0.9), head, 4096, 16000, 0.0)["hnr"] > 9.0


def test_period_walk_known_answers():
    st, ln, f0, v = R.period_walk([200.0] * 4, [0.9] * 4, 4, 2000, 16100)
    assert st == [0, 256, 512, 768] and ln == [80] * 4 and v == 0.0             # int(80.5), from each frame's start
    st, ln, f0, v = R.period_walk([50.0] * 4, [0.9] * 4, 4, 2000, 16010)
    assert st == [0, 320, 640, 960] and ln == [320] * 4                          # ... or from the last period's end
    assert R.period_walk([50.0] * 4, [0.9] * 4, 4, 1280, 16010)[0] == [0, 320, 640]   # one ending at n is dropped
    assert R.period_walk([200.0] * 4, [0.5] * 4, 4, 2000, 16100)[0] == []       # confidence must exceed 0.5
    assert R.period_walk([40.0] * 4, [0.9] * 4, 4, 2000, 16000)[0] == []        # below 50 Hz
    assert R.period_walk([200.0], [0.9], 0, 1024, 1000) == ([], [], [], 0.9)    # exactly 1024 samples: frame 0's voicing
    tr = R.YinTracker()
    assert tr.step(200.0, 0.4) == (0.0, 0.0, 0.0) and tr.step(100.0, 0.9) == (0.3 * 100.0, 0.9, 0.9)


# ---- the library's tails and plan against the restatement -----------------------------------------

def _run(binary, text):
    subprocess.run(["make", "-s", "-C", CABI, "build/" + binary], check=True)
    run = subprocess.run([os.path.join(CABI, "build", binary)], input=text, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    return [line.split() for line in run.stdout.splitlines()]


def _txt(values):
    return " ".join(repr(float(v)) for v in values)


def _counted(values):
    return "%d %s" % (len(values), _txt(values))


def _music_cases(rng):
    arrays = [[], [3.0], [2.0, 2.0], [1.0, 2.0, 3.0, 4.0], [0.0, 0.0], [0.5, 2.0, 0.0], [1e-300, 1e300], [5e-324, 1.0]]
    arrays += [[rng.uniform(0.0, 2.0) * (rng.random() > 0.2) for _ in range(n)] for n in (2, 7, 64, 1000)]
    return arrays


def test_library_music_tail_equals_restatement():
    rng = random.Random(7)
    ints = [-3.7, 3.99, 0.0, NAN, 1e19, -INF, INF, 9223372036854775808.0, -9223372036854775808.0, 9.2233720368547748e18]
    edges = [(0, 513, 6), (44100, 4, 6), (44100, 513, 6), (16000, 257, 6), (44100, 129, 6), (300, 65, 6), (22050, 2, 6)]
    arrays = [(a, [rng.uniform(0.0, 3.0) for _ in a]) for a in _music_cases(rng)]   # energies, frame peaks
    panics = [(17, 512, 1300), (17, 64, 1300), (6, 256, 1280), (6, 256, 1279), (341, 512, 88200), (1, 256, 1024),
              (3, 256, 1536), (1, 128, 512)]
    text = "".join("goint %r\n" % v for v in ints) + "".join("edges %d %d %d\n" % e for e in edges)
    for a, peaks in arrays:
        text += "variance %s\ncrest %d %s %s\nentropy %s\n" % (_counted(a), len(a), _txt(peaks), _txt(a), _counted(a))
    text += "".join("panics %d %d %d\n" % p for p in panics)
    lines = _run("extractor_tail_check", text)
    assert len(lines) == len(ints) + len(edges) + 4 * len(arrays) + 2 * len(panics)
    it = iter(lines)
    for v in ints:
        assert next(it) == ["goint", str(R.go_int(v))], v
    for e in edges:
        ln = next(it)
        assert ln[0] == "edges" and [int(v) for v in ln[2:]] == R.contrast_edges(*e), e
    for a, peaks in arrays:
        ent, lr = R.energy_entropy(a)
        assert same(next(it)[1:], [R.gonum_variance(a)]), a
        assert same(next(it)[2:], R.crest_factors(peaks, a)), a
        assert same(next(it)[2:], ent) and same(next(it)[1:], [lr]), a
    for F, hop, n in panics:
        frame, (index, L) = R.chroma_slice_panics(F, hop, n), R.percentile_panics(n)
        assert next(it) == ["chroma_panic", str(-1 if frame is None else frame)], (F, hop, n)
        assert next(it) == ["pct_panic", str(-1 if index is None else index), str(L)], n


PLAN_TUPLES = [(1024, 1024, 256, 1024, 256), (1300, 1024, 256, 512, 128), (1535, 512, 128, 1024, 128),
               (700, 512, 128, 256, 64), (1024, 512, 256, 256, 128),             # below 1536 samples
               (1300, 256, 64, 256, 512), (88200, 1024, 256, 1024, 512), (1535, 512, 128, 1024, 256),
               (5000, 1024, 256, 1024, 1000),                                    # chroma panics
               (88200, 1024, 256, 1024, 256), (441000, 1024, 256, 1024, 256), (44100, 1024, 256, 0, 256),
               (500, 256, 128, 256, 128), (22050, 1024, 256, 0, 0), (22050, 1024, 256, 1024, 0),   # a hop of 0
               (512, 512, 128, 256, 64), (512, 256, 64, 512, 128), (1535, 1024, 256, 1024, 256),
               (1536, 1024, 256, 1024, 256), (1536, 512, 128, 256, 64)]


def test_music_plan_equals_the_formulas_it_replaced():
    text, want = "", []
    for n, W, H, fw, fh in PLAN_TUPLES:
        for rate in (44100, 16000):
            F = (n - W) // H + 1
            text += "plan %d %d %d %d %d %d\n" % (n, F, W, rate, fw, fh)
            p = R.music_plan(n, F, W, rate, fw, fh)
            want.append(["plan"] + [str(p[k]) for k in ("F", "K", "chroma_bad", "Fe", "fse", "Fenv", "harmonic_live", "L",
                                                        "pct_index", "maxband")] + [str(e) for e in p["edges"]])
    assert _run("extractor_tail_check", text) == want
    live = [w for w in want if w[7] == "1"]
    assert len(live) == 2 and live[0][1:3] == ["1", "513"]                       # only n = 1024 with W = 1024


def _content_cases(rng):
    cases = [(5, 1.0, 0.1, [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], [], [], 11, 2000, 2.0),
             (0, 1.0, 0.0, [0.0] * 10, [], [], 11, 2000, 2.0), (0, 1.0, INF, [0.0] * 10, [], [], 11, 2000, 2.0),
             (0, 0.5, 0.5, [0.5], [], [], 1, 44100, 2.0),
             (0, 1.0, 1.0, [0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0], [], [], 22, 2000, 2.0),
             (0, 1.0, 1.0, [0.0] * 10, [1024.0, 3072.0], [1.0, 3.0], 2048, 2000, 2.0),
             (0, 1.0, 1.0, [0.0] * 10, [0.0, 3072.0], [0.0, 9.0], 2047, 2000, 2.0)]
    for n, sr in ((100, 8000), (2048, 44100), (3001, 22050), (44100, 44100), (160000, 16000)):
        N = min(2048, n)
        K = N // 2 + 1
        fe = (n - 1024 + 511) // 512 if n > 1024 else 0
        ts = sr // 10
        ft = (n - ts + ts - 1) // ts if n > ts else 0
        for thr in (2.0, 0.0, 3.0):
            scale = rng.choice((1e-3, 1.0, 30.0))
            spec = [rng.uniform(0.0, 1.0) ** 4 for _ in range(K)]
            es = [rng.uniform(0.0, scale) * 1024.0 * (rng.random() > 0.3) for _ in range(fe)]
            tsm = [rng.uniform(0.5, 1.5) * scale for _ in range(ft)]
            mn = rng.choice((0.0, 1e-6, 1e-3, 0.05))
            cases.append((rng.randrange(0, n), rng.uniform(0.1, 1.0), mn, spec, es, tsm, n, sr, thr))
    return cases


def test_library_content_tail_equals_restatement():
    cases = _content_cases(random.Random(11))
    text = "".join("content %d %r %r %d %d %r %s %s %s\n" % (cr, mx, mn, n, sr, thr, _counted(spec), _counted(es), _counted(ts))
                   for cr, mx, mn, spec, es, ts, n, sr, thr in cases)
    lines = _run("extractor_tail_check", text)
    assert len(lines) == 2 * len(cases)
    seen = set()
    for i, (cr, mx, mn, spec, es, ts, n, sr, thr) in enumerate(cases):
        f = R.content_features(cr, mx, mn, spec, es, ts, n, sr)
        kind, f["classification_confidence"] = R.classify_content(f, thr)
        assert same(lines[2 * i][1:], [f[k] for k in FEATURES]), (i, f, lines[2 * i])
        assert lines[2 * i + 1] == ["class", str(kind)], (i, f)
        seen.add(kind)
    assert {R.CT_UNKNOWN, R.CT_MUSIC} <= seen and len(seen) >= 3                 # the cases reach several classes


def _voice_cases(rng):
    head = [float(i % 2) for i in range(1024)]
    cases = [([100, 100, 100], [1.0] * 3, [160.0] * 3, None, [0.0] * 1000, 1000, 16000, 0.0),
             ([100, 110, 100], [1.0, 2.0, 1.0], [160.0] * 3, None, [0.0] * 1000, 1000, 16000, 0.7),
             ([100] * 3, [0.0] * 3, [160.0] * 3, None, head, 1500, 16000, 0.0)]
    cases += [([100] * 3, [1.0] * 3, [160.0] * 3, _ac(lag, peak), head, 4096, 16000, 0.0)
              for lag, peak in ((100, 0.9), (100, 1.0), (100, 2.0), (126, 0.9), (125, 0.9), (75, 0.3), (74, 0.3))]
    cases.append(([3000] * 3, [1.0] * 3, [5.0] * 3, _ac(100, 0.9), head, 4096, 16000, 0.0))   # lag 3200: no search
    for k in (3, 4, 10, 57):
        f0 = [rng.uniform(80.0, 400.0) for _ in range(k)]
        ac = [rng.uniform(-1.0, 1.0) for _ in range(2048)]
        ac[0] = rng.choice((0.5, 1.5))
        cases.append(([int(16000 / f) for f in f0], [rng.uniform(0.01, 1.0) for _ in range(k)], f0, ac,
                      [rng.uniform(-1.0, 1.0) for _ in range(1024)], 32000, 16000, rng.random()))
    return cases


def test_library_voice_tail_equals_restatement():
    rng = random.Random(13)
    cases = _voice_cases(rng)
    walks = [([200.0] * 4, [0.9] * 4, 4, 2000, 16100), ([50.0] * 4, [0.9] * 4, 4, 2000, 16010),
             ([50.0] * 4, [0.9] * 4, 4, 1280, 16010), ([200.0] * 4, [0.5] * 4, 4, 2000, 16100),
             ([200.0], [0.9], 0, 1024, 1000), ([], [], 0, 1000, 1000)]
    for rows in (5, 40, 121):
        n = 1025 + 256 * (rows - 1) + rng.randrange(0, 256)
        # a drifting pitch with octave jumps, dropouts and frames of low confidence: every branch of the tracker
        p = [rng.choice((1.0, 1.0, 1.0, 2.0, 0.5, 3.0, 0.0)) * (150.0 + 20.0 * math.sin(i / 5.0)) for i in range(rows)]
        c = [rng.choice((0.95, 0.8, 0.6, 0.45)) for _ in range(rows)]
        walks.append((p, c, rows, n, 16000))
    text = "".join("voice %d %d %r %d %s %s %s %s %s\n" % (n, sr, vstr, len(ln), _txt(ln), _txt(amp), _txt(f0),
                                                           _counted(ac or []), _counted(head))
                   for ln, amp, f0, ac, head, n, sr, vstr in cases)
    text += "".join("walk %d %d %d %d %s %s\n" % (Fv, n, sr, len(p), _txt(p), _txt(c)) for p, c, Fv, n, sr in walks)
    lines = _run("extractor_tail_check", text)
    assert len(lines) == len(cases) + 4 * len(walks)
    for i, (ln, amp, f0, ac, head, n, sr, vstr) in enumerate(cases):
        q = R.voice_quality_from(ln, amp, f0, ac, head, n, sr, vstr)
        assert lines[i][0] == "voice" and same(lines[i][1:], [q[k] for k in VOICE]), (i, q, lines[i])
    kept = 0
    for j, (p, c, Fv, n, sr) in enumerate(walks):
        got = lines[len(cases) + 4 * j: len(cases) + 4 * j + 4]
        st, ln, f0, v = R.period_walk(p, c, Fv, n, sr)
        assert [g[0] for g in got] == ["starts", "lengths", "f0", "voicing"]
        assert same(got[0][2:], st) and same(got[1][2:], ln) and same(got[2][2:], f0) and same(got[3][1:], [v]), j
        kept += len(st)
    assert kept > 60                                                            # the random walks keep periods
