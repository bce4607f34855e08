"""The parts of the DTW step-pattern / metric feature that need no GPU: the Python checker
(tests/dtw_params_ref.py) pinned bit for bit against the C oracle where the two overlap (Euclidean,
symmetric2), sonar_dtw_quality (a pure host function) against a direct restatement of
GetAlignmentQuality (dtw.go:253-286), and the three new symbols in the header and the library."""
import ctypes
import math
import re

import numpy as np
import pytest

import dtw_params_ref as R
import oracle as O
import sonar


@pytest.mark.parametrize("nq,nr,band", [(130, 75, -1), (130, 75, 40), (300, 330, -1), (300, 330, 40), (10, 100, 5)])
def test_checker_equals_oracle_at_euclidean_symmetric2(nq, nr, band):
    """(10, 100, band 5) walks through +Inf cells to row 0: border points and zero costs."""
    rng = np.random.default_rng(nq * 3 + nr)
    q, r = rng.random((nq, 12)), rng.random((nr, 12))
    ref, got = O.dtw(q, r, band, want_cost=True), R.dtw(q, r, band, want_cost=True)
    assert R.same_result(got, ref, cost=True) == []


def test_checker_patterns_and_metrics_behave_as_the_reference():
    rng = np.random.default_rng(5)
    q, r = rng.random((40, 12)), rng.random((30, 12))
    a = R.dtw(q, r, step="asymmetric")                      # never reads C[0][0]: everything +Inf
    assert a["distance"] == math.inf and len(a["path_q"]) == 40 + 30 and a["path_q"][0] == -1
    assert np.isnan(a["path_cost"]).sum() == 40 and np.all(a["path_cost"][~np.isnan(a["path_cost"])] == 0)
    assert R.same_result(R.dtw(q, r, metric="mahalanobis"), R.dtw(q, r)) == []
    assert R.same_result(R.dtw(q, r, metric=99), R.dtw(q, r)) == []
    assert R.local_distances(q, q, "cosine").min() < 0       # identical rows: 1 - (1 + ulp)
    assert np.all(R.local_distances(np.zeros((3, 4)), q[:, :4], "cosine") == 1.0)
    assert np.all(R.local_distances(np.full((3, 4), 2.5), q[:, :4], "pearson") == 1.0)
    assert np.all(np.isnan(R.local_distances(q * 1e200, r * 1e200, "cosine")))
    assert np.all(np.isnan(R.local_distances(q * 1e200, r * 1e200, "pearson")))
    with pytest.raises(ValueError, match="failed to fill cost matrix: unknown step pattern: zigzag"):
        R.dtw(q, r, step="zigzag")
    with pytest.raises(ValueError, match="empty sequences provided"):
        R.dtw(np.zeros((0, 12)), r, step="zigzag")


def _res(pq, pr, pc, distance):
    return {"path_q": np.array(pq, np.int32), "path_r": np.array(pr, np.int32),
            "path_cost": np.array(pc, np.float64), "distance": distance}


def _same_quality(got, ref):
    assert list(got) == ["path_efficiency", "diagonal_ratio", "average_cost", "normalized_distance"]
    for k, v in ref.items():
        assert got[k] == v or (math.isnan(got[k]) and math.isnan(v)), (k, got[k], v)


def test_dtw_quality_against_the_restatement():
    rng = np.random.default_rng(2)
    diag = _res(range(50), range(50), rng.random(50), 0.37)
    _same_quality(sonar.dtw_quality(diag, 50, 50), R.alignment_quality(diag, 50, 50))
    assert sonar.dtw_quality(diag, 50, 50)["diagonal_ratio"] == 1.0
    # ragged: border points (-1), vertical and horizontal runs, lengths that differ
    pq = [-1, 0, 0, 1, 2, 2, 2, 3, 4, 5, 6, 6]
    pr = [0, 0, 1, 2, 2, 3, 4, 5, 5, 6, 7, 8]
    ragged = _res(pq, pr, rng.random(len(pq)) * 1e3, 12.5)
    _same_quality(sonar.dtw_quality(ragged, 7, 9), R.alignment_quality(ragged, 7, 9))
    one = _res([0], [0], [0.25], 0.25)                       # one point: 0 / 0
    got = sonar.dtw_quality(one, 1, 1)
    assert math.isnan(got["diagonal_ratio"]) and got["path_efficiency"] == 1.0 and got["average_cost"] == 0.25
    _same_quality(got, R.alignment_quality(one, 1, 1))
    nanc = _res([0, 1, 2], [0, 1, 1], [0.0, math.nan, 1.0], math.inf)
    got = sonar.dtw_quality(nanc, 3, 2)
    assert math.isnan(got["average_cost"]) and got["normalized_distance"] == math.inf
    _same_quality(got, R.alignment_quality(nanc, 3, 2))


def test_dtw_quality_of_an_empty_path_is_an_error():
    empty = _res([], [], [], 0.0)
    with pytest.raises(sonar.SonarError) as e:
        sonar.dtw_quality(empty, 3, 3)
    assert e.value.code == sonar.ERR_EMPTY
    assert R.alignment_quality(empty, 3, 3) == {}            # Go: an empty map


def test_average_cost_is_summed_serially_in_path_order():
    pc = [1e16, 1.0, -1e16, 1.0]                             # pairwise or reversed sums differ
    res = _res(range(4), range(4), pc, 0.0)
    assert sonar.dtw_quality(res, 4, 4)["average_cost"] == (((0.0 + 1e16) + 1.0) + -1e16 + 1.0) / 4.0


def test_new_symbols_are_declared_and_exported():
    names = ["sonar_dtw_params", "sonar_dtw_quality", "sonar_dtw_optimize_step_pattern"]
    with open(sonar._abi.HEADER) as f:
        text = f.read()
    lib = ctypes.CDLL(sonar.LIB_PATH)
    for n in names:
        assert n in sonar.EXPORTED_SYMBOLS
        assert re.search(r"^int " + n + r"\(", text, re.M)
        assert hasattr(lib, n)
    for k, v in {"SONAR_DTW_STEP_SYMMETRIC2": 0, "SONAR_DTW_STEP_ASYMMETRIC": 1, "SONAR_DTW_STEP_SYMMETRIC1": 2,
                 "SONAR_DTW_METRIC_EUCLIDEAN": 0, "SONAR_DTW_METRIC_MANHATTAN": 1, "SONAR_DTW_METRIC_COSINE": 2,
                 "SONAR_DTW_METRIC_PEARSON": 3, "SONAR_DTW_METRIC_MAHALANOBIS": 4}.items():
        assert re.search(r"^#define " + k + r" " + str(v) + r"$", text, re.M), k
    assert sonar.DTW_STEPS == {"symmetric2": 0, "asymmetric": 1, "symmetric1": 2}
    assert sonar.DTW_METRICS == R.METRICS
    assert sonar.abi_version() == 4
