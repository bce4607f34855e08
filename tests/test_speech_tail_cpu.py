"""Known answers for the speech-tail checker (tests/speech_tail_ref.py), worked out by hand on tiny arrays, so
the checker is pinned independently of the GPU; and the library's own tail (csrc/host_dsp.cpp, compiled by the
plain host C++ compiler into tests/c_abi/build/speech_tail_check) against the checker on the same cases,
exactly: every value travels as text that round-trips a double.  No GPU."""
import math
import os
import subprocess

import numpy as np

import oracle as O
import speech_tail_ref as R

CABI = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c_abi")
NAN, INF = math.nan, math.inf


def same(a, b):
    return np.array_equal(np.asarray(a, float), np.asarray(b, float), equal_nan=True)


# ---- the checker against answers worked out by hand ------------------------------------------------

def test_threshold_and_silence_ratio_known_answers():
    assert R.percentile10_threshold([5.0, 1.0, 4.0]) == 1.0                     # fewer than 10: index 0, the minimum
    assert R.percentile10_threshold([9.0, 8, 7, 6, 5, 4, 3, 2, 1, 0]) == 1.0    # 10 values: index 1
    assert R.percentile10_threshold([float(v) for v in range(29, -1, -1)]) == 3.0
    assert R.silence_ratio([]) == 0.0
    assert R.silence_ratio([1.0, 2.0, 3.0, 4.0]) == 0.25
    assert R.silence_ratio([2.0, 2.0, 2.0]) == 1.0                              # all equal: every frame is silent
    assert R.silence_ratio([1.0, 1.0, 2.0, 3.0]) == 0.5                         # a tie at the threshold counts


def test_pause_durations_known_answers():
    e = [0.0, 5.0, 0.0, 0.0, 5.0, 0.0, 0.0, 0.0]                                # hop 1 at rate 10: 0.1 s a frame
    assert R.pause_durations(e, 1, 10) == [0.2, 3 * 0.1]                        # the 0.1 s pause is not longer than 0.1
    assert R.pause_durations(e[:5], 1, 10) == [0.2]
    assert R.pause_durations([2.0, 2.0, 2.0], 1, 1) == [3.0]                    # one pause over the whole signal
    assert R.pause_durations([], 1, 10) == []
    assert R.pause_durations([0.0, 5.0, 0.0, 0.0, 5.0], 128, 0) == [INF, INF]   # rate 0: every pause is +Inf


def test_onsets_known_answers():
    assert R.adaptive_threshold([]) == 0.0 and R.adaptive_threshold([1.0, 1.0, 1.0, 1.0]) == 1.0
    assert R.adaptive_threshold([0.0, 2.0]) == 3.0                              # mean 1, population deviation 1
    assert R.detect_onsets([]) == [] and R.detect_onsets([0.0, 10.0]) == []
    assert R.detect_onsets([0.0, 10.0, 10.0]) == []                             # the first difference is never a peak
    # differences 0 x 8, 10, 0, 0: mean 10/11, deviation 2.87.., threshold 6.66 < 10; the rise 8 -> 9 is onset 8
    assert R.detect_onsets([0.0] * 9 + [10.0] * 3) == [8]
    assert R.detect_onsets([0.0] * 8 + [1.0] + [10.0] * 3) == [8]
    assert R.detect_onsets([0.0] * 9 + [10.0] * 2) == [8]
    assert R.detect_onsets([0.0] * 9 + [10.0]) == []                            # ... nor the last one
    assert R.detect_onsets([0.0, 1.0, 2.0, 3.0, 4.0]) == []                     # a plateau of differences: not strict
    assert R.onset_density([61, 124, 186], 32000, 16000) == 1.5


def test_attack_times_known_answers():
    e = [0.0] + [1.0] * 20
    assert R.attack_times([9], e, 1, 100) == [9 * 0.01]                         # back to frame 0, the 9th frame back
    assert R.attack_times([10], e, 1, 100) == [0.0]                             # frame 0 is 10 back: not looked at
    assert R.attack_times([15], e, 1, 100) == [0.0]
    assert R.attack_times([3], [1.0] * 4, 1, 100) == [0.0]                      # the search stops at frame 0
    assert R.attack_times([9], e, 1, 10) == [0.1]                               # 0.9 s is cut to 0.1
    assert R.attack_times([2, 3], [0.0, 0.0, 1.0, 1.0], 1, 100) == [0.01, 2 * 0.01]   # the nearest frame under a tenth
    assert R.attack_times([8], [0.0] * 9 + [10.0] * 3, 1, 100) == [0.0]         # the onset frame's own energy is 0
    assert same(R.attack_times([9, 15], e, 128, 0), [0.1, NAN])                 # rate 0: Inf is cut, 0 x Inf stays NaN
    assert R.attack_times([], e, 1, 100) == []


def test_speech_rate_known_answers():
    assert R.speech_rate([1.0, 2.0, 3.0, 4.0], 100, 10, True) == 3.0            # 10 s, silence 0.25: 4 x 7.5 / 10
    assert R.speech_rate([1.0, 1.0, 2.0, 3.0], 100, 10, True) == 2.0
    assert R.speech_rate([1.0, 2.0, 3.0, 4.0], 100, 10, False) == 0.0
    assert R.speech_rate([2.0, 2.0], 100, 10, True) == 3.0                      # no speech time: the default
    assert math.isnan(R.speech_rate([1.0, 2.0], 100, 0, True))                  # Inf / Inf
    assert R.speech_rate([2.0, 2.0], 100, 0, True) == 3.0                       # Inf x 0 is NaN, not above 0


def _sine(n, period, amp=0.5):
    return [amp * math.sin(2.0 * math.pi * i / period) for i in range(n)]


def _spikes_then_buzz(n=3000):
    """A head with no periodicity at lags 20 .. 399 (two spikes 10 apart), then enough sign changes."""
    x = [0.0] * n
    x[0], x[10] = 1.0, -1.0
    for i in range(1024, 1200):
        x[i] = 0.05 if i % 2 else -0.05
    return x


def test_detect_speech_known_answers():
    periodic = _sine(2048, 64)
    assert R.zero_crossings([1.0, -1.0, 0.0, -1.0, -2.0, 3.0]) == 4 and R.sum_squares([3.0, 4.0]) == 25.0
    assert R.check_periodicity(periodic) and not R.check_periodicity(periodic[:1023])
    assert R.detect_speech(periodic, 8000)
    assert not R.detect_speech(periodic, 8196) and R.detect_speech(periodic, 8195)      # n < rate / 4 on integers
    x = _spikes_then_buzz()
    assert 0.01 < R.zero_crossings(x) / (len(x) - 1) < 0.3 and math.sqrt(R.sum_squares(x) / len(x)) > 0.001
    assert not R.check_periodicity(x) and not R.detect_speech(x, 4000)
    assert R.detect_speech(periodic[:1024] + x[1024:], 4000)                    # the same tail after a periodic head
    head = periodic[:1024]
    assert R.detect_speech_from_sums(1001, 4000, 10, 1.0, head) and R.detect_speech_from_sums(1001, 4000, 300, 1.0, head)
    assert not R.detect_speech_from_sums(1001, 4000, 9, 1.0, head)              # z exactly 0.01 and 0.3 pass
    assert not R.detect_speech_from_sums(1001, 4000, 301, 1.0, head)
    assert not R.detect_speech_from_sums(1001, 4000, 100, 1001e-6 * (1 - 1e-9), head)   # RMS just under 0.001
    assert R.detect_speech_from_sums(1001, 4000, 100, 1001e-6 * (1 + 1e-9), head)
    assert not R.detect_speech_from_sums(1000, 4000, 100, 1.0, head[:1000])     # a head shorter than 1024


# ---- the library's tail against the checker --------------------------------------------------------

def _energy_cases():
    tone =O.short_time_energy(O.preemphasis(R.gated_tone(), 0.97), 512, 128)
    assert len(tone) == 247
    cases = [([], 1, 10), ([3.0], 1, 10), ([3.0, 1.0], 1, 10), ([3.0, 1.0, 2.0], 1, 10),        # 0 .. 3 frames
             ([2.0] * 12, 1, 10),                                                                # all equal
             ([1.0, 1.0, 2.0, 3.0, 1.0, 5.0, 1.0, 1.0, 1.0, 6.0, 7.0, 1.0, 1.0], 1, 10),         # ties, ends in a pause
             ([0.0, 5.0, 0.0, 0.0, 5.0, 0.0, 0.0, 0.0], 1, 10),                                  # a pause of exactly 0.1 s
             ([0.0, 5.0, 0.0, 0.0, 5.0], 128, 0),                                                # rate 0
             ([0.0] * 8 + [1.0] + [10.0] * 3, 1, 100),
             # the attack search gives up 9 frames back: the zero 10 frames before onset 12 is not seen
             ([1.0, 1.0, 0.0] + [1.0] * 9 + [0.5, 30.0, 30.0, 30.0], 1, 100),
             ([1.0, 1.0, 20.0, 20.0, 20.0, 20.0, 20.0, 20.0, 20.0, 20.0], 1, 100),   # ... and at frame 0
             ([1.0] * 12 + [0.5, 30.0, 30.0, 30.0], 128, 0),
             ([float(v) for v in tone], 128, 16000), ([float(v) for v in tone], 128, 0)]
    return cases


def _speech_cases():
    periodic = _sine(2048, 64)
    head = periodic[:1024]
    x = _spikes_then_buzz()
    mixed = head + x[1024:]
    cases = [(len(s), rate, R.zero_crossings(s), R.sum_squares(s), s[:1024])
             for s, rate in ((periodic, 8000), (periodic, 8196), (periodic, 8195), (x, 4000), (mixed, 4000),
                             (periodic[:1000], 3000))]
    for crossings in (9, 10, 300, 301):
        cases.append((1001, 4000, crossings, 1.0, head))
    cases.append((1001, 4000, 100, 1001e-6 * (1 - 1e-9), head))
    cases.append((1001, 4000, 100, 1001e-6 * (1 + 1e-9), head))
    cases.append((1000, 4000, 100, 1.0, head[:1000]))
    return cases


def _run(binary, text):
    subprocess.run(["make", "-s", "-C", CABI, "build/" + binary], check=True)
    run = subprocess.run([os.path.join(CABI, "build", binary)], input=text, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    return [line.split() for line in run.stdout.splitlines()]


def test_library_tail_equals_checker():
    n, sample_rate = 32000, 16000
    ecases, scases = _energy_cases(), _speech_cases()
    text = "".join("energy %d %d %d %d %d %s\n" % (hop, rate, n, sample_rate, len(e), " ".join(repr(v) for v in e))
                   for e, hop, rate in ecases)
    text += "".join("speech %d %d %d %r %d %s\n" % (m, rate, cr, ssq, len(h), " ".join(repr(v) for v in h))
                    for m, rate, cr, ssq, h in scases)
    lines = _run("speech_tail_check", text)
    assert len(lines) == 7 * len(ecases) + len(scases)
    seen_attack = set()
    for i, (e, hop, rate) in enumerate(ecases):
        got = {ln[0]: [float(v) for v in ln[1:]] for ln in lines[7 * i: 7 * i + 7]}
        what = (i, hop, rate)
        onsets = R.detect_onsets(e)
        attack = R.attack_times(onsets, e, hop, rate)
        assert same(got["threshold"], [R.percentile10_threshold(e) if e else 0.0]), what
        assert same(got["silence"], [R.silence_ratio(e)]), what
        assert same(got["pauses"][1:], R.pause_durations(e, hop, rate)) and got["pauses"][0] == len(got["pauses"]) - 1, what
        assert same(got["onsets"][1:], onsets), what
        assert same(got["attack"][1:], attack), what
        assert same(got["speech_rate"], [R.speech_rate(e, n, rate, True)]), what
        assert same(got["onset_density"], [R.onset_density(onsets, n, sample_rate)]), what
        seen_attack.update(repr(v) for v in attack)
    # the cases reach what they are there for
    assert {"0.0", "0.01", "0.024", "0.1", "nan"} <= seen_attack
    assert R.detect_onsets(ecases[9][0]) == [12] and R.attack_times([12], ecases[9][0], 1, 100) == [0.0]
    assert R.detect_onsets(ecases[10][0]) == [1] and R.attack_times([1], ecases[10][0], 1, 100) == [0.0]
    assert R.detect_onsets(ecases[12][0]) == [61, 124, 186]
    want = [R.detect_speech_from_sums(*c) for c in scases]
    assert [int(ln[1]) for ln in lines[7 * len(ecases):]] == [int(w) for w in want]
    assert want == [True, False, True, False, True, False, False, True, True, False, False, True, False]


def test_speech_layout_offsets():
    """csrc/speech_layout.h: sections 8-double aligned, disjoint, in order, the total their sum, the offsets those
    of the hand-written sequence it replaced; MFCC and speech on and off, Fe above and below F, n < 1024, rate 0."""
    assert _run("speech_layout_check", "") == [["speech_layout", "ok"]]
