"""Known answers of the key estimation checker (tests/key_ref.py), which test_gpu_key.py holds the GPU
entries to, and the host-only library entries (sonar_key_params_default, sonar_key_transition, the
layout of sonar_key_params) against it.  No GPU.  The DESIGN.md findings F42-F49 are pinned here."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import key_ref as R
import sonar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rotated(profile, tonic):
    """The profile with its first entry at pitch class `tonic`."""
    return [profile[(i - tonic) % 12] for i in range(12)]


def _ulps_from_one(x):
    return abs(x - 1.0) / 2.0 ** -52


# ---- F42: the profile is rotated the wrong way ---------------------------------------------------

@pytest.mark.parametrize("profile", range(7))
@pytest.mark.parametrize("mode", [0, 1])
def test_rotated_profile_is_reported_as_the_mirrored_key(profile, mode):
    for tonic in range(12):
        r = R.estimate_key(_rotated(R.PROFILES[profile][mode], tonic), R.params(profile=profile))
        assert (r["key"], r["mode"]) == ((12 - tonic) % 12, mode), (profile, mode, tonic)
        assert _ulps_from_one(r["confidence"]) <= 2 and r["known"] == 1
        assert r["strength"] == r["confidence"] == r["scores"][mode * 12 + r["key"]]
        assert r["candidates"][0] == r["code"] and len(r["candidates"]) == 5
        assert r["related"] == r["candidates"][1:4]


def test_krumhansl_major_on_d_is_a_sharp_major_above_one():
    r = R.estimate_key(_rotated(R.PROFILES[0][0], 2))
    assert R.key_name(r["code"]) == "A# major" and r["key"] == 10
    assert r["confidence"] == 1.0000000000000002 and r["confidence"] > 1.0


# ---- F43 / the profile fallback ------------------------------------------------------------------

@pytest.mark.parametrize("profile", [-1, 7, 1000])
def test_profile_outside_the_table_is_krumhansl(profile):
    row = np.random.default_rng(3).random(12)
    a, b = R.estimate_key(row, R.params(profile=profile)), R.estimate_key(row, R.params(profile=0))
    assert a == b


def test_params_hold_only_the_fields_the_reference_reads():
    """F43: there is no method field (every method runs the profile correlation), none of the unread ones."""
    names = [f[0] for f in sonar.KeyParams._fields_]
    assert names == ["profile", "hpcp_size", "normalize_chroma", "remove_mean", "binary_mode", "max_candidates",
                     "min_confidence"]
    assert set(names) == set(R.DEFAULT)


# ---- degenerate rows -----------------------------------------------------------------------------

def _all_zero(r):
    return (r["scores"] == [0.0] * 24 and r["code"] == 0 and r["confidence"] == 0.0 and r["known"] == 0 and
            r["strength"] == 0.0 and r["clarity"] == 0.0 and r["ambiguity"] == 0.0)


def test_zero_row_gives_c_major_unknown():
    r = R.estimate_key([0.0] * 12)
    assert _all_zero(r) and r["tonality"] == 0.0
    assert r["candidates"] == [0, 1, 2, 3, 4]                # F45: equal scores stay in creation order


@pytest.mark.parametrize("value", [0.5, 1.0, 3.0])
def test_constant_row_gives_c_major_unknown(value):
    """A row whose mean is exact (here: not normalised) has all 24 centred sums exactly 0."""
    r = R.estimate_key([value] * 12, R.params(normalize_chroma=0))
    assert _all_zero(r) and r["tonality"] == 0.0


def test_normalised_constant_row_scores_are_rounding_noise():
    """1 / sqrt(12) added twelve times is not 12 / sqrt(12): the centred row is a few 1e-17, the scores are
    ratios of rounding errors (about 1e-16), never a confident key."""
    r = R.estimate_key([1.0] * 12)
    assert max(abs(s) for s in r["scores"]) < 1e-14 and r["confidence"] == 0.0 and r["known"] == 0
    assert r["tonality"] == 0.0


def test_row_below_the_energy_floor_is_not_normalised():
    tiny = [2e-6, 1e-6] + [0.0] * 10                         # sum x^2 = 5e-12 < 1e-10
    assert R.preprocess(tiny, R.DEFAULT) == tiny
    above = [2e-5, 1e-5] + [0.0] * 10                        # 5e-10
    got = R.preprocess(above, R.DEFAULT)
    assert got != above and abs(sum(x * x for x in got) - 1.0) < 1e-15


def test_hpcp_size_24_scores_nothing_and_tonality_reads_24_bins():
    """F44: correlateWithProfile returns 0 on a length mismatch and every profile has 12 entries."""
    row = list(np.random.default_rng(5).random(24))
    r = R.estimate_key(row, R.params(hpcp_size=24))
    assert r["scores"] == [0.0] * 24 and r["code"] == 0 and r["known"] == 0
    assert len(r["processed"]) == 24
    assert r["tonality"] == 1.0 - R.uniformity(R.preprocess(row, R.params(hpcp_size=24))) > 0.0


def test_resize_indices():
    assert R.resize_indices(36, 12) == [3 * i for i in range(12)]
    assert R.resize_indices(13, 12) == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]
    assert R.resize_indices(11, 12) == [0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10]
    assert R.resize_indices(1, 12) == [0] * 12
    assert R.resize_indices(0, 12) == [-1] * 12              # int(0) < 0 is false: rows of zeros
    assert R.resize_indices(120, 12) == [10 * i for i in range(12)]
    row = [float(i) for i in range(36)]
    assert R.preprocess(row, R.params(normalize_chroma=0)) == [float(3 * i) for i in range(12)]


def test_preprocessing_switches():
    row = [3.0, 1.0] + [0.0] * 10
    p = R.params(normalize_chroma=0, remove_mean=1)
    assert R.preprocess(row, p) == [x - 4.0 / 12.0 for x in row]
    p = R.params(normalize_chroma=0, binary_mode=1)
    assert R.preprocess(row, p) == [1.0, 1.0] + [0.0] * 10
    p = R.params(normalize_chroma=0, remove_mean=1, binary_mode=1)      # the threshold is the new mean, about 0
    assert R.preprocess(row, p) == [1.0, 1.0] + [0.0] * 10


def test_frame_below_min_confidence_keeps_key_and_strength():
    """F46: only the confidence is zeroed."""
    row = _rotated(R.PROFILES[0][1], 4)
    lo, hi = R.estimate_key(row, R.params(min_confidence=0.0)), R.estimate_key(row, R.params(min_confidence=1.5))
    assert lo["known"] == 1 and hi["known"] == 0 and hi["confidence"] == 0.0
    for k in ("code", "key", "mode", "strength", "candidates", "scores", "clarity", "ambiguity", "tonality"):
        assert lo[k] == hi[k]
    assert hi["strength"] == lo["confidence"] > 0.99


def test_go_panics():
    row = [1.0] * 12
    with pytest.raises(IndexError, match=r"index out of range \[0\] with length 0"):
        R.estimate_key(row, R.params(max_candidates=0))
    with pytest.raises(IndexError, match=r"slice bounds out of range \[:-1\]"):
        R.estimate_key(row, R.params(max_candidates=-1))
    with pytest.raises(IndexError, match="makeslice: len out of range"):
        R.estimate_key(row, R.params(hpcp_size=-1))
    with pytest.raises(IndexError, match=r"index out of range \[0\] with length 0"):
        R.estimate_key(row, R.params(hpcp_size=0))
    assert len(R.estimate_key(row, R.params(max_candidates=25))["candidates"]) == 24


def test_clarity_and_ambiguity_by_hand():
    r = R.estimate_key(_rotated(R.PROFILES[5][0], 0), R.params(profile=5))
    srt = sorted(r["scores"], reverse=True)
    assert r["clarity"] == (srt[0] - srt[1]) / srt[0]
    pos = [s for s in r["scores"] if s > 0]
    want = -sum(s / sum(pos) * math.log2(s / sum(pos)) for s in pos) / math.log2(24)
    assert abs(r["ambiguity"] - want) < 1e-12 and 0.0 < r["ambiguity"] < 1.0


# ---- sequences: F45-F47 ----------------------------------------------------------------------------

def _seq(codes, profile=0):
    """One clean frame per code: key k's template has its tonic at (12 - k) % 12 (F42)."""
    return [_rotated(R.PROFILES[profile][c & 1], (12 - (c >> 1)) % 12) for c in codes]


@pytest.mark.parametrize("F,stable,may_modulate", [(2, False, False), (3, True, False), (10, True, False),
                                                   (11, True, False), (19, True, False), (20, True, False),
                                                   (21, True, False), (22, True, True)])
def test_sequence_thresholds(F, stable, may_modulate):
    """Stability from 3 frames on; the scan covers positions 10 .. F - 11 and position 10 has no predecessor,
    so the first length that can report anything is 22 (F47)."""
    rows = _seq([0] * (F - F // 2) + [14] * (F // 2))          # a jump from C major to G major at the middle
    r = R.estimate_key_sequence(rows)
    assert (r["stability"] > 0.0) == stable
    if stable:
        assert r["stability"] == float(F - F // 2) / float(F)
    if not may_modulate:
        assert r["modulations"] == []
    assert R.estimate_key_sequence([]) is None


def test_22_frames_report_exactly_position_11():
    # window 10 is rows [5, 15): five louder C major rows against five G major ones, still C major;
    # window 11 is rows [6, 16): four against six, G major
    rows = [[1.5 * x for x in r] for r in _seq([0] * 10)] + _seq([14] * 12)
    w10 = R.estimate_key(R.average_chroma(rows[5:15]))
    w11 = R.estimate_key(R.average_chroma(rows[6:16]))
    assert w10["code"] != w11["code"] and w11["confidence"] > 0.7
    assert R.estimate_key_sequence(rows)["modulations"] == [11]
    assert R.estimate_key_sequence(rows[:21])["modulations"] == []


def test_unknown_frames_still_vote_and_still_modulate():
    """F46: with min_confidence above every score each frame is Unknown, yet the stability counts their keys;
    the modulation test reads the zeroed confidence, so nothing is reported."""
    rows = _seq([0] * 10 + [14] * 12)
    r = R.estimate_key_sequence(rows, R.params(min_confidence=1.5))
    assert r["known"] == 0 and r["stability"] == 12.0 / 22.0 and r["modulations"] == []


def test_find_mode_takes_the_lowest_code_among_equals():
    assert R.find_mode([5, 3, 5, 3, 7]) == 3 and R.find_mode([]) == 0


# ---- batch ---------------------------------------------------------------------------------------

def test_no_confident_frame_gives_no_key_and_nan():
    frames = R.process_batch([[0.0] * 12, [1.0] * 12, [0.0] * 12])
    g = R.global_key(frames)
    assert g["code"] == -1 and math.isnan(g["confidence"]) and g["strength"] == 0.0 and g["votes"] == [0.0] * 24
    assert R.key_name(g["code"]) == "" and R.key_progression(frames) == []
    assert R.global_key([])["confidence"] == 0.0


def test_global_key_votes_in_order_and_ties_go_to_the_lowest_code():
    frames = R.process_batch(_seq([14, 0, 14, 0]), R.params(min_confidence=0.0))
    g = R.global_key(frames)
    c0, c14 = frames[1]["confidence"], frames[0]["confidence"]
    assert g["votes"][0] == c0 + c0 and g["votes"][14] == c14 + c14
    if g["votes"][0] == g["votes"][14]:
        assert g["code"] == 0
    assert g["strength"] == max(g["votes"]) / 4.0


def test_progression_records_every_confident_pair_same_key_included():
    frames = R.process_batch(_seq([0, 0, 14, 19]) + [[0.0] * 12] + _seq([0]))
    prog = R.key_progression(frames)
    assert [(p[0], p[1], p[2], R.TRANSITIONS[p[4]]) for p in prog] == [
        (1, 0, 0, "same_key"), (2, 0, 14, "dominant"), (3, 14, 19, "distant")]
    assert prog[0][3] == (frames[0]["confidence"] + frames[1]["confidence"]) / 2.0


def test_transition_table():
    t = R.analyze_key_transition
    assert t(0, 0, 9, 1)["transition_type"] == "relative" and t(0, 0, 9, 1)["fifths_distance"] == 1
    assert t(0, 0, 7, 0)["transition_type"] == "dominant"
    assert t(0, 0, 5, 0)["transition_type"] == "subdominant"
    assert t(0, 0, 0, 1)["transition_type"] == "parallel" and t(0, 0, 0, 1)["transition_strength"] == 1.0
    far = t(0, 0, 6, 0)
    assert far["transition_type"] == "distant" and far["fifths_distance"] == 6 and far["semitone_distance"] == 6
    assert far["transition_strength"] == 1.0 / 7.0
    assert t(9, 1, 0, 0)["transition_type"] == "relative" and t(4, 1, 4, 1)["transition_type"] == "same_key"


# ---- the library's host-only entries -------------------------------------------------------------

def test_library_defaults_are_new_key_estimators():
    p = sonar.key_params()
    assert {n: getattr(p, n) for n, _ in sonar.KeyParams._fields_} == R.DEFAULT
    assert sonar.key_params(profile="edma", max_candidates=24).profile == 3


def test_library_transition_matches_the_checker_on_every_pair():
    for a in range(24):
        for b in range(24):
            got = sonar.key_transition(a >> 1, a & 1, b >> 1, b & 1)
            assert got == R.analyze_key_transition(a >> 1, a & 1, b >> 1, b & 1), (a, b)
    assert [sonar.key_name(c) for c in (-1, 0, 21)] == [R.key_name(c) for c in (-1, 0, 21)] == ["", "C major", "A# minor"]


def test_key_params_layout(tmp_path):
    """sizeof and offsetof as a C99 compiler sees the header, against the ctypes mirror."""
    fields = [f[0] for f in sonar.KeyParams._fields_]
    src = tmp_path / "key_layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "sonar_gpu.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(sonar_key_params));\n' +
                   "".join(f'  printf("%zu\\n", offsetof(sonar_key_params, {f}));\n' for f in fields) +
                   "  return 0;\n}\n")
    exe = tmp_path / "key_layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == ctypes.sizeof(sonar.KeyParams) == 32
    assert out[1:] == [getattr(sonar.KeyParams, f).offset for f in fields] == [0, 4, 8, 12, 16, 20, 24]
