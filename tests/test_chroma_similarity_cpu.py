"""CPU: known answers for the checker of the chroma sequence similarity (tests/chroma_similarity_ref.py),
worked out by hand from algorithms/chroma/chroma_similarity.go, and the product's host-only plan entry
against it.  No GPU."""
import ctypes
import math

import numpy as np
import pytest

import chroma_similarity_ref as R
import sonar


def _path(res):
    return list(zip(res["path_q"].tolist(), res["path_r"].tolist(), res["path_score"].tolist()))


def test_smith_waterman_2x2():
    """sim = [[1, 0], [0, 1]], gap 0.1, zero borders:
      S11 = max(0, 0 + 1, -0.1, -0.1) = 1                      match  -> code 1
      S12 = max(0, 0 + 0, 0 - 0.1, S11 - 0.1) = 0.9            insert -> code 3
      S21 = max(0, 0 + 0, S11 - 0.1, 0 - 0.1) = 0.9            delete -> code 2
      S22 = max(0, S11 + 1, S12 - 0.1, S21 - 0.1) = 2          match  -> code 1
    best = 2 at (2, 2); back: (1, 1, 2) -diag-> (0, 0, 1) -diag-> i = 0.  overall = 2 / 2."""
    res = R.smith_waterman(sim=[[1.0, 0.0], [0.0, 1.0]])
    assert res["matrix"].tolist() == [[1.0, 1.0 - 0.1], [1.0 - 0.1, 2.0]]
    assert res["best_cell"] == (2, 2) and res["max_score"] == 2.0
    assert _path(res) == [(0, 0, 1.0), (1, 1, 2.0)]
    assert res["overall"] == 1.0


def test_smith_waterman_3x2():
    """sim = [[.5, 0], [0, .5], [.5, 0]]:
      S11 = .5 (1)   S12 = max(0, 0, -.1, .5 - .1) = .4 (3)
      S21 = max(0, 0, S11 - .1, -.1) = .4 (2)      S22 = max(0, S11 + .5, S12 - .1, S21 - .1) = 1 (1)
      S31 = max(0, 0 + .5, S21 - .1, -.1) = .5 (1) S32 = max(0, S21 + 0, S22 - .1, S31 - .1) = .9 (2)
    The first maximum in row-major order is 1 at (2, 2); back: (1, 1, 1) -> (0, 0, .5).  overall = 1 / 2."""
    res = R.smith_waterman(sim=[[0.5, 0.0], [0.0, 0.5], [0.5, 0.0]])
    assert res["matrix"].tolist() == [[0.5, 0.5 - 0.1], [0.5 - 0.1, 1.0], [0.5, 1.0 - 0.1]]
    assert res["best_cell"] == (2, 2)
    assert _path(res) == [(0, 0, 0.5), (1, 1, 1.0)]
    assert res["overall"] == 0.5


def test_smith_waterman_nothing_scores_and_nan():
    """sim = [[-1]]: max(0, -1, -0.1, -0.1) = 0 equals none of the three -> code 0, nothing > 0: the path
    is empty and overall = 0 / 0 = NaN.  A NaN similarity gives a NaN score (math.Max propagates), code
    0; NaN > x is false, so it is never the best cell and a traceback reaching it stops (S > 0 fails)."""
    res = R.smith_waterman(sim=[[-1.0]])
    assert res["matrix"].tolist() == [[0.0]] and len(res["path_q"]) == 0 and math.isnan(res["overall"])
    res = R.smith_waterman(sim=[[1.0, 0.0], [0.0, math.nan], [0.0, 0.0]])
    assert math.isnan(res["matrix"][1, 1]) and res["best_cell"] == (1, 1)
    assert _path(res) == [(0, 0, 1.0)]
    # scores below a NaN are NaN too (delete = NaN - 0.1)
    assert math.isnan(res["matrix"][2, 1])


def test_dtw_2x2():
    """cost = [[1, 2], [3, 4]]: acc00 = 1, acc10 = 1 + 3 = 4, acc01 = 1 + 2 = 3,
    acc11 = 4 + min(up 3, min(left 4, diag 1)) = 5.  Back from (1, 1): diag 1 <= 3 and 1 <= 4 -> (0, 0),
    which is not appended: path = [(1, 1, 5)], distance = 5 / 1, overall = exp(-5)."""
    res = R.dtw(cost=[[1.0, 2.0], [3.0, 4.0]])
    assert res["acc"].tolist() == [[1.0, 3.0], [4.0, 5.0]]
    assert _path(res) == [(1, 1, 5.0)]
    assert res["distance"] == 5.0 and res["overall"] == math.exp(-5.0)
    assert res["matrix"].tolist() == [[math.exp(-1.0), math.exp(-2.0)], [math.exp(-3.0), math.exp(-4.0)]]


def test_dtw_3x2():
    """cost = [[0, 1], [1, 0], [2, 2]]: column 0 = 0, 1, 3; acc01 = 1;
    acc11 = 0 + min(up 1, min(left 1, diag 0)) = 0; acc21 = 2 + min(up 0, min(left 3, diag 1)) = 2.
    Back from (2, 1): diag 1 <= up 0 fails, up 0 <= left 3 -> (1, 1); there diag 0 <= 1, 0 <= 1 -> (0, 0).
    path = [(1, 1, 0), (2, 1, 2)], distance = 2 / 2 = 1."""
    res = R.dtw(cost=[[0.0, 1.0], [1.0, 0.0], [2.0, 2.0]])
    assert res["acc"].tolist() == [[0.0, 1.0], [1.0, 0.0], [3.0, 2.0]]
    assert _path(res) == [(1, 1, 0.0), (2, 1, 2.0)]
    assert res["distance"] == 1.0 and res["overall"] == math.exp(-1.0)


def test_dtw_traceback_prefers_diagonal_then_up_on_ties():
    """cost all 1 (2 x 2): acc = [[1, 2], [2, 2]]; from (1, 1) diag 1 wins.  cost = [[1, 0], [0, 5]]:
    acc = [[1, 1], [1, 6]]: diag = up = left = 1 -> diagonal by <=."""
    assert _path(R.dtw(cost=[[1.0, 0.0], [0.0, 5.0]])) == [(1, 1, 6.0)]
    # diag 2 > up = left = 1 -> up
    res = R.dtw(cost=[[2.0, -1.0], [-1.0, 5.0]])
    assert res["acc"].tolist() == [[2.0, 1.0], [1.0, 6.0]]
    assert _path(res) == [(0, 1, 1.0), (1, 1, 6.0)]


def test_dtw_band_rule_depends_on_j_only():
    assert R.dtw_skipped_columns(64, 64, 1) == [] and R.dtw_skipped_columns(300, 300, 50) == []
    assert R.dtw_skipped_columns(100, 300, 50) == list(range(76, 300))
    assert R.dtw_skipped_columns(300, 100, 50) == list(range(26, 100))
    assert R.dtw_skipped_columns(100, 300, 0) == [] and R.dtw_skipped_columns(100, 300, -3) == []
    assert R.dtw_skipped_columns(1, 300, 5) == []            # no row i >= 1


def test_dtw_band_100x300_is_exactly_one():
    """Columns 76..299 stay 0 in rows 1..99, so acc[99][299] = 0 and overall = exp(-0 / len) = 1."""
    rng = np.random.default_rng(5)
    q, r = rng.random((100, 12)), rng.random((300, 12))
    res = R.dtw(q, r, "cosine", 50)
    assert np.all(res["acc"][1:, 76:] == 0.0) and np.all(res["acc"][0, 1:] > 0)
    assert res["acc"][99, 299] == 0.0 and res["overall"] == 1.0
    assert R.dtw(q, r, "cosine", 0)["overall"] < 1.0         # R = 0: no band


def test_dtw_1x1_and_empty():
    """One cell: the path is empty, so acc / 0.  Identical frames (distance exactly 0): 0 / 0 = NaN.
    Cosine distance 0.5 ([1, 0, 0, 0] against [1, 1, 1, 1]: 1 - 1 / (1 * 2)): 0.5 / 0 = +Inf, exp(-Inf) = 0."""
    res = R.dtw([[3.0, 4.0]], [[3.0, 4.0]], "cosine")
    assert res["acc"].tolist() == [[0.0]] and len(res["path_q"]) == 0 and math.isnan(res["overall"])
    res = R.dtw([[1.0, 0.0, 0.0, 0.0]], [[1.0, 1.0, 1.0, 1.0]], "cosine")
    assert res["acc"].tolist() == [[0.5]] and res["overall"] == 0.0
    with pytest.raises(IndexError, match=r"index out of range \[0\] with length 0"):
        R.dtw(np.zeros((0, 12)), np.ones((3, 12)))


def test_qmax_is_the_clamped_matrix_maximum():
    rng = np.random.default_rng(7)
    q, r = rng.random((23, 12)), rng.random((17, 12))
    for metric in ("cosine", "pearson", "euclidean"):
        res = R.qmax(q, r, metric)
        assert res["overall"] == max(0.0, float(res["matrix"].max()))
    S = np.array([[-1.0, math.nan, -0.5], [math.nan, -2.0, -0.25]])
    assert R.qmax(sim=S)["overall"] == 0.0                   # all negative or NaN: the maxima stay 0
    S[1, 2] = 0.75
    assert R.qmax(sim=S)["overall"] == 0.75                  # NaNs are skipped


def test_oti_nil_matrix():
    """Cosine similarity of a constant frame and its negative: cos = -1 exactly (dim 4: norms 2 * 2),
    distance 2, similarity 1 - 2 / 2 = 0 for every shift: no average is > 0, bestMatrix stays nil."""
    q, r = np.ones((6, 4)), -np.ones((5, 4))
    res = R.oti(q, r, "cosine", 10)
    assert res["avgs"] == [0.0] * 12
    assert res["matrix"] is None and res["overall"] == 0.0 and res["best_transposition"] == 0
    res = R.oti(np.zeros((0, 12)), np.ones((3, 12)))         # 0 / 0: NaN never wins
    assert res["matrix"] is None and res["overall"] == 0.0
    assert R.oti(q, -r, "cosine", -1)["matrix"] is None      # a negative radius computes no cell


def test_oti_divides_by_the_full_grid():
    q = r = np.ones((8, 4))
    res = R.oti(q, r, "cosine", 0)                           # 8 diagonal cells of similarity 1
    assert res["overall"] == 8.0 / 64.0 and res["best_transposition"] == 0
    assert res["matrix"].tolist() == np.eye(8).tolist()


def test_sample_step():
    assert [R.sample_step(n) for n in (49, 50, 99, 100, 120, 151)] == [1, 1, 1, 2, 2, 3]
    assert R.sample_step(0) == 1


def test_best_transposition_of_a_rolled_copy():
    rng = np.random.default_rng(11)
    r = rng.random((120, 12))
    q = np.roll(r, 5, axis=1)                                # q[k] = r[k - 5]: shifting q by 5 undoes it
    best, mx, avgs = R.find_best_transposition(q, r, "cosine")
    assert best == 5 and mx == avgs[5] == max(avgs)
    d = R.direct(q, r, "cosine", True)
    assert d["best_transposition"] == 5 and d["overall"] == mx
    assert R.same_bits(d["matrix"], R.similarities(q, r, "cosine", 5))
    # empty query: every mean is 0 / 0, the best stays (0, 0.0)
    assert R.find_best_transposition(np.zeros((0, 12)), r)[:2] == (0, 0.0)


def test_js_second_normalisation_changes_bits():
    rng = np.random.default_rng(13)
    p, q = 0.05 + 0.95 * rng.random((40, 12)), 0.05 + 0.95 * rng.random((40, 12))
    twice, once = R.js_distances(p, q), R.js_distances(p, q, renormalize=False)
    assert np.any(twice != once)
    assert np.max(np.abs(twice - once)) < 1e-12              # ... by roundings only
    assert R.same_bits(R.distances(p, q, "js"), twice)


def test_metrics_known_values():
    a, b = np.array([[3.0, 4.0, 0.0]]), np.array([[0.0, 4.0, 3.0]])
    assert R.distances(a, b, "euclidean")[0, 0] == math.sqrt(18.0)
    assert R.distances(a, b, "manhattan")[0, 0] == 6.0
    assert R.distances(a, b, "cosine")[0, 0] == 1.0 - 16.0 / 25.0
    assert R.distances(a, np.zeros((1, 3)), "cosine")[0, 0] == 1.0           # a zero norm
    assert R.distances(a, b, 99)[0, 0] == math.sqrt(18.0)                    # unknown: Euclidean
    assert R.similarities(a, b, 99)[0, 0] == math.exp(-math.sqrt(18.0))      # ... with exp(-d)
    assert R.similarities(a, b, "cosine")[0, 0] == 1.0 - (1.0 - 16.0 / 25.0) / 2.0
    # Pearson is 1 - |corr|: a frame and its mirror image about the mean have corr = -1
    assert R.distances([[1.0, 2.0, 3.0]], [[3.0, 2.0, 1.0]], "pearson")[0, 0] == 0.0
    # normalizeToProbability: positives only; an all-non-positive frame becomes uniform
    assert R.normalize_to_probability([[1.0, -5.0, 3.0]]).tolist() == [[0.25, 0.0, 0.75]]
    assert R.normalize_to_probability([[0.0, -1.0]]).tolist() == [[0.5, 0.5]]
    # Hellinger of disjoint distributions is 1; KL of equal ones is 0
    assert abs(R.distances([[1.0, 0.0]], [[0.0, 1.0]], "hellinger")[0, 0] - 1.0) < 1e-15
    assert R.distances([[1.0, 3.0]], [[2.0, 6.0]], "kl")[0, 0] == 0.0
    assert R.circular_shift([[0.0, 1.0, 2.0, 3.0]], 1).tolist() == [[1.0, 2.0, 3.0, 0.0]]


def test_direct_go_order_mean_lies_within_the_bound():
    rng = np.random.default_rng(17)
    q, r = rng.random((66, 12)), rng.random((300, 12))
    for metric in R.METRICS:
        d = R.direct(q, r, metric)
        assert d["bound"] > 0 and abs(d["overall_go_order"] - d["overall_fsum"]) <= d["bound"], metric
    assert math.isnan(R.direct(np.zeros((0, 12)), r)["overall"])             # 0 / 0
    assert R.direct(np.zeros((0, 12)), r, "cosine", True)["overall"] == 0.0  # maxSimilarity stays 0.0


def test_binary_counts_matches():
    S = np.array([[0.5, 0.4, 0.39], [0.41, math.nan, 1.0]])
    res = R.binary(None, None, threshold=0.4, sim=S)
    assert res["matrix"].tolist() == [[1.0, 0.0, 0.0], [1.0, 0.0, 1.0]] and res["overall"] == 3.0 / 6.0


PLAN_SHAPES = [(49, 49), (50, 70), (99, 10), (100, 300), (120, 64), (151, 151), (300, 100), (64, 64), (1, 40), (40, 1)]


@pytest.mark.parametrize("nq,nr", PLAN_SHAPES)
@pytest.mark.parametrize("oti_radius,dtw_radius", [(10, 50), (0, 5), (-1, 0), (1000, 1)])
def test_plan_agrees_with_the_checker(nq, nr, oti_radius, dtw_radius):
    got = sonar.chroma_similarity_plan("dtw", nq, nr, 12, oti_radius, dtw_radius)
    ref = R.plan(nq, nr, oti_radius, dtw_radius)
    assert {k: got[k] for k in ref} == ref
    assert got["scratch_bytes"] >= nq * nr * 16


def test_plan_rejects_bad_sizes():
    with pytest.raises(sonar.SonarError):
        sonar.chroma_similarity_plan("direct", -1, 5)
    with pytest.raises(sonar.SonarError):
        sonar.chroma_similarity_plan("direct", 5, 5, dim=0)


def test_new_symbols_are_declared_and_exported():
    L = ctypes.CDLL(sonar.LIB_PATH)
    for s in ("sonar_chroma_frame_matrix", "sonar_chroma_similarity", "sonar_chroma_similarity_plan",
              "sonar_chroma_similarity_last_timing"):
        assert s in sonar.EXPORTED_SYMBOLS and hasattr(L, s), s
    assert sonar.CHROMA_SIM_METHODS == R.METHODS and sonar.CHROMA_DIST_METRICS == R.METRICS
    assert sonar.abi_version() == 4
