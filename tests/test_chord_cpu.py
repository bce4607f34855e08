"""Known answers of the chord detection checker (tests/chord_ref.py), which test_gpu_chord.py holds the GPU
entries to; the equality of its literal and reduced forms on every GPU test input (tests/chord_cases.py);
and the host-only library entries (sonar_chord_params_default, the struct layouts, the host-decidable
cases of sonar_chord_progression).  No GPU.  The DESIGN.md findings F50-F59 are pinned here, except F53
and F56, which are about sonar_chord_detect's audio side and are pinned in test_gpu_chord.py."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import chord_cases as K
import chord_ref as R
import sonar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_MAJOR = [1.0, 0, 0, 0, 1.0, 0, 0, 1.0, 0, 0, 0, 0]
X = 1.0 / math.sqrt(3.0)     # an entry of the normalised triad row
ULP = 2.0 ** -52             # of a value in [1, 2): the sums below take at most three roundings


def _slot(quality, root):
    return R.TEMPLATE_OF_QUALITY[quality] * 12 + root


# ---- known answers worked by hand ----------------------------------------------------------------------

def test_c_major_triad_scores():
    """Unit energy: every entry 1 / sqrt(3).  C major collects three of them, sqrt(3); C minor, Csus2, Csus4,
    C power and the triads on E and G two or one; the weights are the templates'."""
    r = R.Detector().detect(C_MAJOR)
    s = r["template_scores"]
    assert len(s) == 120
    assert s[_slot(0, 0)] == (X + X + X) * 1.0 and abs(s[_slot(0, 0)] - math.sqrt(3.0)) <= 3 * ULP
    assert s[_slot(1, 0)] == (X + X) * 1.0 and abs(s[_slot(1, 0)] - 2.0 / math.sqrt(3.0)) <= 3 * ULP
    assert s[_slot(6, 0)] == (X + X + X) * 0.85 and s[_slot(8, 0)] == (X + X + X) * 0.9
    assert s[_slot(23, 0)] == (X + X) * 0.6 and s[_slot(2, 0)] == X * 0.8 and s[_slot(3, 0)] == (X + X) * 0.7
    assert s[_slot(1, 4)] == (X + X) * 1.0          # E minor: E and G
    assert s[_slot(0, 1)] == 0.0                    # C# major: C#, F, G#
    assert s[_slot(7, 9)] == (X + X + X) * 0.85     # A minor 7: A, C, E, G
    assert (r["root"], r["quality"], r["inversion"], r["name"]) == (0, 0, 0, "C")
    assert r["confidence"] == 1.0 and r["strength"] == s[0] and r["consonance"] == 0.9
    assert r["stability"] == r["confidence"] and r["tension"] == 0.0 and r["extensions"] == 0 and r["role"] == 0


def test_unnormalised_triad_and_threshold():
    row = [0.25 * v for v in C_MAJOR]
    r = R.Detector(R.params(normalize_templates=0)).detect(row)
    assert r["template_scores"][0] == 0.75 and r["confidence"] == 0.75 and r["name"] == "C"
    # 0.25 + 0.25 = 0.5 for the two-tone matches; sus and power weights 0.7 / 0.6 -> 0.35, 0.3; one tone 0.25 * w
    assert r["cand_confidence"] == [0.75, 0.75 * 0.9, 0.75 * 0.85, 0.75 * 0.85, 0.5]
    assert [R.chord_name(R.slot_root(s), R.slot_quality(s), 0) for s in r["candidates"]] == \
        ["C", "Cdominant7", "Cmajor7", "Aminor7", "Cminor"]
    assert r["clarity"] == 0.75 - 0.75 * 0.9 and r["ambiguity"] == 1.0 - r["clarity"]
    # the threshold is >=: 0.25 * 0.8 = 0.2 is a candidate at min_chord_strength 0.2
    assert 0.25 * 0.8 == 0.2
    found = R.Detector(R.params(normalize_templates=0, max_candidates=120)).detect(row)
    assert _slot(2, 0) in found["candidates"] and _slot(2, 2) not in found["candidates"]     # C dim 0.2; D dim 0
    assert R.Detector(R.params(normalize_templates=0, min_chord_strength=5.0)).detect(row)["n_found"] == 0


def test_inversion_patterns():
    assert R.INVERSIONS[0] == [[1.0, 0, 0, 0, 1.0, 0, 0, 1.0, 0, 0, 0, 0], [1.0, 0, 0, 0, 1.5, 0, 0, 1.0, 0, 0, 0, 0],
                               [1.0, 0, 0, 0, 1.0, 0, 0, 1.5, 0, 0, 0, 0]]
    assert [len(v) for v in R.INVERSIONS] == [3, 3, 3, 3, 3, 3, 4, 4, 4, 2]
    assert R.INVERSIONS[8][3] == [1.0, 0, 0, 0, 1.0, 0, 0, 1.0, 0, 0, 1.5, 0]
    assert R.INVERSIONS[9] == [[1.0, 0, 0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0], [1.0, 0, 0, 0, 0, 0, 0, 1.5, 0, 0, 0, 0]]


def test_bass_bonus_and_inversion():
    """Bass E at confidence 0.9 under C major: the bonus is 0.3 * 0.9, the first inversion scores
    x + 1.5 x + x and wins; with the bass on the root the inversion score is the raw score, below the bonus."""
    p = R.params(max_candidates=120)
    r = R.Detector(p).detect(C_MAJOR, 4, 0.9)
    k = r["candidates"].index(0)
    assert r["cand_inversion"][k] == 1 and r["cand_strength"][k] == (X + 1.5 * X + X) * 1.0
    assert (X + 1.5 * X + X) > (X + X + X) + 0.3 * 0.9
    assert r["name"] == "C/1st" and r["template_scores"][0] == (X + X + X)
    r = R.Detector(p).detect(C_MAJOR, 0, 0.9)
    k = r["candidates"].index(0)
    assert r["cand_inversion"][k] == 0 and r["cand_strength"][k] == (X + X + X) + 0.3 * 0.9
    # at 0.3 the bass is off (the tests are > 0.3); above it, on
    assert R.Detector(p).detect(C_MAJOR, 4, 0.3) == R.Detector(p).detect(C_MAJOR)
    assert R.Detector(p).detect(C_MAJOR, 4, 0.30000000000000004) != R.Detector(p).detect(C_MAJOR)
    # a bass that is no chord tone of C major leaves it alone but lifts the chords that hold it
    r = R.Detector(p).detect(C_MAJOR, 2, 0.9)
    k = r["candidates"].index(0)
    assert r["cand_strength"][k] == (X + X + X) and r["cand_inversion"][k] == 0
    k = r["candidates"].index(_slot(4, 0))          # Csus2 holds D
    assert r["cand_strength"][k] == (X + X) * 0.7 + 0.3 * 0.9
    # a negative bass weight: the root-position "inversion" (the raw score) beats the lowered score
    r = R.Detector(R.params(max_candidates=120, bass_weight=-0.5)).detect(C_MAJOR, 0, 0.9)
    k = r["candidates"].index(0)
    assert r["cand_inversion"][k] == 0 and r["cand_strength"][k] == (X + X + X)
    # without use_inversions only the bonus
    r = R.Detector(R.params(max_candidates=120, use_inversions=0)).detect(C_MAJOR, 4, 0.9)
    k = r["candidates"].index(0)
    assert r["cand_inversion"][k] == 0 and r["cand_strength"][k] == (X + X + X) + 0.3 * 0.9


def test_tension():
    row = [0.0] * 12
    row[0], row[1] = 0.5, 0.4
    assert R.harmonic_tension(row) == 0.5 * 0.4                 # a minor second
    row[1], row[6] = 0.0, 0.4
    assert R.harmonic_tension(row) == 0.5 * 0.4                 # a tritone
    row[6], row[11] = 0.0, 0.4
    assert R.harmonic_tension(row) == 0.5 * 0.4                 # index difference 11
    row[11], row[2] = 0.0, 0.4
    assert R.harmonic_tension(row) == 0.0                       # a major second is not counted
    row = [0.0] * 12
    row[0], row[1] = 0.5, 0.2
    assert R.harmonic_tension(row) == 0.0                       # > 0.2, not >=
    assert R.harmonic_tension([1.0] * 12) == 1.0                # clipped
    assert R.harmonic_tension([0.5] * 36) == 1.0                # only bins 0..11 are read: 11 + 6 + 1 pairs * 0.25


def test_extension_masks():
    row = list(C_MAJOR)
    row[10] = 0.31                                              # Bb over C major
    p = R.params(normalize_templates=0)
    assert R.extensions_mask(row, _slot(0, 0), p) == 1 << 10
    assert R.extensions_mask(row, _slot(8, 0), p) == 0          # a chord tone of C dominant 7
    row[10] = 0.3
    assert R.extensions_mask(row, _slot(0, 0), p) == 0          # > 0.3, not >=
    row = [1.0] * 12
    assert R.extensions_mask(row, _slot(0, 0), p) == (1 << 10 | 1 << 11 | 1 << 2 | 1 << 5 | 1 << 9)
    assert R.extensions_mask(row, _slot(0, 0), R.params(max_extension=12)) == (1 << 10 | 1 << 11 | 1 << 2 | 1 << 5)
    assert R.extensions_mask(row, _slot(0, 0), R.params(max_extension=10)) == (1 << 10 | 1 << 11 | 1 << 2)
    assert R.extensions_mask(row, _slot(0, 0), R.params(max_extension=8)) == (1 << 10 | 1 << 11)
    assert R.extensions_mask(row, _slot(0, 0), R.params(max_extension=-1)) == (1 << 10 | 1 << 11)   # F57
    assert R.extensions_mask(row, _slot(4, 0), p) == (1 << 10 | 1 << 11 | 1 << 5 | 1 << 9)   # sus2 holds the 2
    assert R.extensions_mask(row, _slot(6, 3), p) == (1 << 10 | 1 << 2 | 1 << 5 | 1 << 9)    # maj7 holds the 11
    row = [0.0] * 12
    row[1] = 1.0                                                # root 11 + interval 2 wraps to pitch class 1
    assert R.extensions_mask(row, _slot(0, 11), p) == 1 << 2


def test_names_and_codes():
    assert R.chord_name(9, 7, 0) == "Aminor7" and R.chord_name(0, 0, 2) == "C/2nd" and R.chord_name(1, 23, 1) == "C#power/1st"
    assert R.chord_name(0, 9, 0) == "Cunknown"                  # a quality without a template (:953-957)
    assert R.quality_name(23) == "power" and R.quality_name(24) == "unknown" and R.quality_name(99) == "unknown"
    assert [R.method_name(m) for m in (0, 5, 6, -1)] == ["template_matching", "hybrid", "unknown", "unknown"]
    assert [R.ROLES[R.role_code(q)] for q in (0, 1, 8, 2, 6)] == ["tonic", "subdominant", "dominant", "leading_tone", "other"]
    for q in range(-1, 26):
        assert sonar.chord_quality_name(q) == R.quality_name(q)
        for root in (0, 11):
            for inv in range(5):
                if q >= 0:
                    assert sonar.chord_name(root, q, inv) == R.chord_name(root, q, inv), (root, q, inv)
    assert sonar.CHORD_SLOT_QUALITIES == R.QUALITY_CODES and sonar.CHORD_ROLES == R.ROLES
    assert sonar.chord_extensions(1 << 2 | 1 << 10) == R.extension_list(1 << 2 | 1 << 10) == [10, 2]


def test_checker_errors():
    with pytest.raises(ValueError, match="failed to extract chroma features: unsupported chroma size: 13"):
        R.Detector().detect([0.0] * 13)
    with pytest.raises(IndexError, match=r"slice bounds out of range \[:-1\]"):
        R.Detector(R.params(max_candidates=-1)).detect([0.0] * 12)     # even without candidates
    with pytest.raises(IndexError, match=r"slice bounds out of range \[:-3\]"):
        R.sequence_reduced([C_MAJOR], R.params(max_candidates=-3))
    d = R.Detector(R.params(temporal_window=-1))
    d.detect(C_MAJOR)
    with pytest.raises(IndexError, match=r"slice bounds out of range \[1:0\]"):
        d.detect([0.0] * 12)                                    # history[1:] of the empty candidate slice (:802)


# ---- the candidate findings -------------------------------------------------------------------------------

def test_f50_ties_decide_the_default_chord():
    """F50: under the defaults the first two confidences tie at 1.0 on nearly every row of input (a); the
    reported chord is then the lowest slot among the tied, clarity is 0 and ambiguity 1."""
    ref, _ = K.reference("a-F%d" % K.LONG, "frames")
    tied = [r for r in ref if len(r["cand_confidence"]) > 1 and r["cand_confidence"][0] == r["cand_confidence"][1]]
    assert len(tied) >= 0.95 * len(ref)
    for r in tied:
        assert r["confidence"] == 1.0 and r["clarity"] == 0.0 and r["ambiguity"] == 1.0
        at_one = [s for s in range(120) if min(r["template_scores"][s], 1.0) == 1.0]
        assert r["candidates"][0] == at_one[0] and r["candidates"][:len(at_one[:5])] == at_one[:5]
        assert r["strength"] == r["template_scores"][at_one[0]] >= 1.0


def test_f51_params_hold_only_the_fields_the_reference_reads():
    names = [f[0] for f in sonar.ChordParams._fields_]
    assert names == ["method", "normalize_templates", "use_inversions", "max_candidates", "use_bass_detection",
                     "detect_extensions", "max_extension", "use_temporal_smoothing", "temporal_window",
                     "use_functional_analysis", "min_chord_strength", "bass_weight"]
    assert sorted(names) == sorted(R.DEFAULT)
    for unread in ("min_confidence", "template_strength", "use_harmonics", "weight_harmonics", "detect_alterations",
                   "use_voice_leading", "context_weight", "model_path", "use_ensemble", "ensemble_weights",
                   "chroma_size", "bass_freq_range"):
        assert unread not in names


@pytest.mark.parametrize("window", [5, 50])
def test_f52_steady_row_alternates(window):
    """F52: the winner is dropped from its own history whenever a frame has more than temporal_window
    candidates, so on a steady row the first chord alternates for as long as the row repeats."""
    res = R.sequence([K.STEADY] * 20, R.params(normalize_templates=0, temporal_window=window))
    assert all(r["n_found"] == 67 for r in res)
    names = [r["name"] for r in res]
    conf = [r["confidence"] for r in res]
    assert names[:2] == ["C", "C"] and conf[:2] == [0.8200000000000001, 0.9020000000000001]
    for t in range(2, 20):
        assert (names[t], conf[t]) == (("Aminor7", 0.8789000000000001) if t % 2 == 0 else ("C", 0.9020000000000001))
    assert 0.8200000000000001 == 0.30 + 0.27 + 0.25 and 0.9020000000000001 == 0.8200000000000001 * 1.1
    assert 0.8789000000000001 == ((0.30 + 0.27 + 0.25 + 0.12) * 0.85) * 1.1


@pytest.mark.parametrize("window", [67, 68])
def test_f52_a_window_of_the_candidate_count_stops_it(window):
    res = R.sequence([K.STEADY] * 8, R.params(normalize_templates=0, temporal_window=window))
    assert [r["name"] for r in res] == ["C"] * 8
    assert [r["confidence"] for r in res] == [0.8200000000000001] + [0.9020000000000001] * 7


def test_f54_longer_rows_score_zero():
    """F54: a 24- or 36-value row makes every score 0: no candidate unless min_chord_strength <= 0, where
    all 120 appear with confidence 0; tension and extensions still read bins 0..11."""
    for dim in (24, 36):
        row = list(K.rows_a(K.PF, dim)[0])
        r = R.Detector().detect(row)
        assert r["template_scores"] == [0.0] * 120 and r["n_found"] == 0 and r["name"] == "" and r["tension"] == 0.0
        r = R.Detector(R.params(min_chord_strength=0.0, max_candidates=120)).detect(row)
        assert r["n_found"] == 120 and r["candidates"] == list(range(120)) and r["cand_confidence"] == [0.0] * 120
        assert (r["root"], r["quality"], r["confidence"], r["clarity"], r["ambiguity"]) == (0, 0, 0.0, 0.0, 1.0)
        assert r["tension"] == R.harmonic_tension(row[:12])
        hot = [1.0 if i < 12 else 0.0 for i in range(dim)]
        r = R.Detector(R.params(min_chord_strength=0.0)).detect(hot)
        assert r["extensions"] == (1 << 10 | 1 << 11 | 1 << 2 | 1 << 5 | 1 << 9) and r["tension"] == 1.0
        # the bass bonus is still added to the zero score
        r = R.Detector(R.params(max_candidates=120)).detect(row, 0, 0.9)
        assert r["n_found"] == sum(1 for t in R.TEMPLATES for root in range(12)
                                   if any((root + iv) % 12 == 0 for iv in t[3]))
        assert set(r["cand_strength"]) == {0.3 * 0.9} and set(r["cand_inversion"]) == {0}


def test_f55_frame_without_candidates():
    """F55: a frame without candidates is root 0, quality 0, an empty name and zero metrics; it empties the
    chord history and leaves the confidence history alone, so the next frame with candidates is a first
    call for the smoothing while its stability still sees the earlier frames."""
    p = R.params(normalize_templates=0)
    rows = [K.STEADY, K.STEADY, [0.0] * 12, K.STEADY, K.STEADY]
    res = R.sequence(rows, p)
    z = res[2]
    assert (z["root"], z["quality"], z["inversion"], z["name"], z["n_found"]) == (0, 0, 0, "", 0)
    for n in ("confidence", "strength", "clarity", "ambiguity", "consonance", "tension", "stability"):
        assert z[n] == 0.0, n
    assert z["candidates"] == [] and z["extensions"] == 0
    assert [r["confidence"] for r in res] == [0.8200000000000001, 0.9020000000000001, 0.0, 0.8200000000000001,
                                             0.9020000000000001]
    assert res[3]["stability"] == max(0.0, 1.0 - R.variance([0.8200000000000001, 0.9020000000000001]))
    assert res[3]["stability"] != res[3]["confidence"]


def test_f57_extensions_are_raw_intervals():
    """F57: the detector reports 10 / 11 / 2 / 5 / 9, the raw intervals; getExtensionNumber only gates them."""
    assert R.extension_list(0b111111111111) == [10, 11, 2, 5, 9]
    assert [R.extension_number(i) for i in (10, 11, 2, 5, 9)] == [7, 7, 9, 11, 13]
    assert R.extensions_mask([1.0] * 12, 0, R.params(max_extension=0)) == (1 << 10 | 1 << 11)


def test_f58_methods():
    """F58: harmonic_analysis, cqt_based and statistical are template matching with the bass forced to
    (0, 0.0); ml_based, hybrid and every other value are template matching with the bass."""
    rows, bn, bc = K.rows_b()[:40], K.bass()[0][:40], K.bass()[1][:40]
    p = R.params(normalize_templates=0)
    with_bass = R.sequence(rows, p, bn, bc)
    without = R.sequence(rows, p)
    assert with_bass != without
    for m in (1, 2, 3):
        assert R.sequence(rows, dict(p, method=m), bn, bc) == without
    for m in (4, 5, 6, -1, 99):
        assert R.sequence(rows, dict(p, method=m), bn, bc) == with_bass
    assert R.sequence(rows, dict(p, use_bass_detection=0), bn, bc) == without


def test_f59_max_candidates_zero():
    """F59: max_candidates 0 keeps nothing: no primary chord, no metric, no confidence history, while the
    smoothing history still advances."""
    p = R.params(normalize_templates=0, max_candidates=0)
    d = R.Detector(p)
    for t in range(4):
        r = d.detect(K.STEADY)
        assert r["n_found"] == 67 and r["candidates"] == [] and r["name"] == ""
        assert all(r[n] == 0.0 for n in ("confidence", "strength", "clarity", "ambiguity", "consonance", "tension",
                                         "stability"))
        assert d.confidence_history == []
        assert len(d.chord_history) == (67 if t == 0 else 66)


def test_stability_follows_the_history_without_smoothing():
    p = R.params(normalize_templates=0, use_temporal_smoothing=0, temporal_window=3)
    rows = K.rows_b()[:12]
    res = R.sequence(rows, p)
    firsts = [r["confidence"] for r in res]
    assert res[0]["stability"] == firsts[0]
    for t in range(1, 12):
        assert res[t]["stability"] == max(0.0, 1.0 - R.variance(firsts[max(t - 3, 0):t]))
        assert res[t]["confidence"] == R.Detector(p).detect(rows[t])["confidence"]     # no boost


def test_progression_checker():
    assert R.progression([], []) == dict(num_chords=0, insufficient_data=1)
    assert R.progression([3], [0.5]) == dict(num_chords=1, insufficient_data=1)
    r = R.progression([8, 1, 8, 1, 0], [0.1, 0.2, 0.3, 0.4, 0.5])
    assert r["most_common_quality"] == 1 and r["average_confidence"] == ((((0.1 + 0.2) + 0.3) + 0.4) + 0.5) / 5.0
    assert R.progression([23, 23, 0], [1.0, 1.0, 1.0])["most_common_quality"] == 23


# ---- the two forms of the chain ----------------------------------------------------------------------------

@pytest.mark.parametrize("cid", K.CASE_IDS)
def test_reduced_chain_equals_the_literal_loop(cid):
    lit, lit_err = K.reference(cid, "sequence")
    red, red_err = K.reference(cid, "reduced")
    assert (lit_err is None) == (red_err is None)
    if lit_err is not None:
        assert str(lit_err) == str(red_err)
    else:
        assert len(lit) == len(K.case(cid)[0]) and lit == red


def test_chain_states_on_the_steady_row():
    per_row = [R.template_matching(K.STEADY, 0, 0.0, R.params(normalize_templates=0))[0]] * 5
    recs = R.frame_records(per_row)
    c, am7 = _slot(0, 0), _slot(7, 9)
    assert recs[0] == (67, c, c, c) and recs[1] == (67, c, c, am7)
    states, firsts, kidx = R.resolve_chain(recs, R.params(normalize_templates=0))
    assert states == [R.HIST_EMPTY, R.HIST_FULL, c, am7, c] and firsts == [c, c, am7, c, am7] and kidx == [0, 1, 2, 3, 4]


def test_input_b_meets_its_conditions():
    ref, _ = K.reference("b-F%d" % K.LONG, "frames")
    n = len(ref)
    assert sum(r["confidence"] < 1.0 for r in ref) >= 0.95 * n
    assert sum(r["cand_confidence"][0] == r["cand_confidence"][1] for r in ref) <= 0.02 * n
    assert min(r["n_found"] for r in ref) >= 2 and sum(r["n_found"] > 5 for r in ref) >= 0.99 * n
    seq, _ = K.reference("b-F%d" % K.LONG, "sequence")
    assert seq[0] == ref[0] and sum(a != b for a, b in zip(seq, ref)) >= 0.9 * n


# ---- the library's host side ---------------------------------------------------------------------------------

def test_params_default_through_the_library():
    p = sonar.chord_params()
    assert {n: getattr(p, n) for n, _ in p._fields_} == R.DEFAULT
    assert sonar.chord_params(method="hybrid", temporal_window=9).method == 5
    assert sonar.CHORD_METHODS == {n: i for i, n in enumerate(R.METHODS)}


def test_chord_struct_layouts(tmp_path):
    """The ctypes mirrors against the header as a C99 compiler lays it out (-pedantic -Werror)."""
    exe = str(tmp_path / "chord_layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-O1",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_abi", "chord_layout.c"),
                    "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    sizes, offs = {}, {}
    for line in out.splitlines():
        kind, name, val = line.split()
        if kind == "struct":
            sizes[name] = int(val)
        else:
            s, m = name.split(".")
            offs.setdefault(s, []).append((m, int(val)))
    for cname, cls in (("sonar_chord_params", sonar.ChordParams), ("sonar_chord_out", sonar.ChordOut)):
        assert ctypes.sizeof(cls) == sizes[cname]
        assert [f[0] for f in cls._fields_] == [m for m, _ in offs[cname]]
        for m, off in offs[cname]:
            assert getattr(cls, m).offset == off, (cname, m)
    assert [f[0] for f in sonar.ChordOut._fields_] == list(sonar.CHORD_FIELDS)


def test_chord_symbols_are_exported():
    L = sonar.lib()
    for s in ("sonar_chord_params_default", "sonar_chord_frames", "sonar_chord_sequence", "sonar_chord_detect",
              "sonar_chord_progression"):
        assert s in sonar.EXPORTED_SYMBOLS and hasattr(L, s), s


@pytest.mark.parametrize("F", [0, 1])
def test_progression_below_two_chords_needs_no_device(F):
    """AnalyzeProgression's insufficient_data answer is decided on the host: no context, nothing else written."""
    L = sonar.lib()
    q, cf = np.zeros(F, np.int32), np.zeros(F)
    num, ins, avg, most = ctypes.c_int64(-1), ctypes.c_int32(-1), ctypes.c_double(-1.0), ctypes.c_int32(-1)
    rc = L.sonar_chord_progression(None, None, q.ctypes.data if F else None, None, cf.ctypes.data if F else None, F,
                                   ctypes.byref(num), ctypes.byref(ins), ctypes.byref(avg), ctypes.byref(most), 0)
    assert rc == 0 and (num.value, ins.value) == (F, 1) and (avg.value, most.value) == (-1.0, -1)
    assert R.progression([0] * F, [0.0] * F) == dict(num_chords=F, insufficient_data=1)
    assert L.sonar_chord_progression(None, None, None, None, None, -1, None, None, None, None, 0) == sonar.ERR_INVALID
    assert L.sonar_chord_progression(None, None, None, None, None, 2, None, None, None, None, 0) == sonar.ERR_INVALID
