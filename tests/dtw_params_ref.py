"""The checker of sonar_dtw_params / sonar_dtw_quality / sonar_dtw_optimize_step_pattern: a float64
restatement of the reference's DTW type for every step pattern and metric (test infrastructure,
never the product; the C oracle has only Euclidean / symmetric2 and is pinned against this file in
test_dtw_params_cpu.py).

  DTWAlignment.Align, fillCostMatrix, applyStepPattern, backtrack, findPreviousStep,
  GetAlignmentQuality, OptimizeStepPattern      (algorithms/stats/dtw.go:55-217, 253-311)
  Euclidean / Manhattan / Cosine / PearsonDistanceFunc, GetDistanceFunction
                                                (algorithms/stats/distance.go:10-107, 150-153)

The distance matrix is built with numpy one feature index at a time: elementwise numpy arithmetic is
unfused and keeps Go's summation order, and +, -, *, /, sqrt and abs are correctly rounded, so every
value has Go's bits.  The recurrence and the backtrack are plain Python loops with math.Min's NaN /
-Inf / -0 rules (as go_min in oracle/dtw_oracle.c)."""
import math

import numpy as np

STEPS = ("symmetric2", "asymmetric", "symmetric1")
METRICS = {"euclidean": 0, "manhattan": 1, "cosine": 2, "pearson": 3, "mahalanobis": 4}
_INF = math.inf
_NAN = math.nan


def go_min(x, y):
    """math.Min: -Inf wins, then NaN propagates, -0 < +0."""
    if x == -_INF or y == -_INF:
        return -_INF
    if x != x or y != y:
        return _NAN
    if x == 0 and y == 0:
        return x if math.copysign(1.0, x) < 0 else y
    return x if x < y else y


def _seq(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a[:, None] if a.ndim == 1 else a


def local_distances(q, r, metric="euclidean"):
    """D[i][j] = distanceFunc(q[i], r[j]) (nq x nr).  metric: a name or DistanceMetric's value;
    Mahalanobis and unknown values are Euclidean (distance.go:21-25)."""
    q, r = _seq(q), _seq(r)
    m = METRICS[metric] if isinstance(metric, str) else int(metric)
    nq, dim = q.shape
    nr = r.shape[0]
    with np.errstate(all="ignore"):
        if m == 1:                                           # ManhattanDistanceFunc :39-45
            s = np.zeros((nq, nr))
            for k in range(dim):
                s = s + np.abs(q[:, k, None] - r[None, :, k])
            return s
        if m == 2:                                           # CosineDistanceFunc :48-65
            dot, na, nb = np.zeros((nq, nr)), np.zeros(nq), np.zeros(nr)
            for k in range(dim):
                dot = dot + q[:, k, None] * r[None, :, k]
                na = na + q[:, k] * q[:, k]
                nb = nb + r[:, k] * r[:, k]
            sim = dot / (np.sqrt(na)[:, None] * np.sqrt(nb)[None, :])
            return np.where((na == 0)[:, None] | (nb == 0)[None, :], 1.0, 1.0 - sim)
        if m == 3:                                           # PearsonDistanceFunc :73-107
            ma, mb = np.zeros(nq), np.zeros(nr)
            for k in range(dim):
                ma = ma + q[:, k]
                mb = mb + r[:, k]
            ma = ma / float(dim)
            mb = mb / float(dim)
            num, sa, sb = np.zeros((nq, nr)), np.zeros(nq), np.zeros(nr)
            for k in range(dim):
                da, db = q[:, k] - ma, r[:, k] - mb
                num = num + da[:, None] * db[None, :]
                sa = sa + da * da
                sb = sb + db * db
            corr = num / np.sqrt(sa[:, None] * sb[None, :])
            return np.where((sa == 0)[:, None] | (sb == 0)[None, :], 1.0, 1.0 - np.abs(corr))
        s = np.zeros((nq, nr))                               # EuclideanDistanceFunc :29-36
        for k in range(dim):
            df = q[:, k, None] - r[None, :, k]
            s = s + df * df
        return np.sqrt(s)


def dtw(q, r, band=-1, step="symmetric2", metric="euclidean", want_cost=False):
    """NewDTWAlignmentWithParams(band, step, metric).Align -> the dict of sonar.Context.dtw."""
    q, r = _seq(q), _seq(r)
    nq, nr = (q.shape[0] if q.size else 0), (r.shape[0] if r.size else 0)
    if nq == 0 or nr == 0:
        raise ValueError("empty sequences provided")
    if step not in STEPS:                                    # at the first filled cell (:159-160, :78)
        raise ValueError(f"failed to fill cost matrix: unknown step pattern: {step}")
    D = local_distances(q, r, metric).tolist()
    Cm = [[_INF] * (nr + 1) for _ in range(nq + 1)]
    Cm[0][0] = 0.0
    pattern = STEPS.index(step)
    for i in range(1, nq + 1):                               # fillCostMatrix :106-135
        prev, cur, drow = Cm[i - 1], Cm[i], D[i - 1]
        lo, hi = 1, nr
        if band > 0:                                         # |i - j| > band: the cell stays +Inf
            lo, hi = max(1, i - band), min(nr, i + band)
        for j in range(lo, hi + 1):
            up, left, dg = prev[j], cur[j - 1], prev[j - 1]
            if pattern == 0:                                 # applyStepPattern :138-162
                best = go_min(go_min(up, left), dg)
            elif pattern == 1:
                best = go_min(up, left)
            else:
                best = go_min(up + 1, go_min(left + 1, dg))
            cur[j] = drow[j - 1] + best
    pq, pr, pc = [], [], []
    i, j = nq, nr
    while i > 0 or j > 0:                                    # backtrack :165-188
        pc.append(Cm[i][j] - Cm[i - 1][j - 1] if i > 0 and j > 0 else 0.0)
        pq.append(i - 1)
        pr.append(j - 1)
        if i == 0:                                           # findPreviousStep :191-217
            j -= 1
        elif j == 0:
            i -= 1
        else:
            up, left, dg = Cm[i - 1][j], Cm[i][j - 1], Cm[i - 1][j - 1]
            mi, best = 0, up
            if left < best:
                mi, best = 1, left
            if dg < best:
                mi = 2
            if mi == 0:
                i -= 1
            elif mi == 1:
                j -= 1
            else:
                i, j = i - 1, j - 1
    P = len(pq)
    return {"distance": Cm[nq][nr] / float(P), "path_q": np.array(pq[::-1], np.int32), "path_r": np.array(pr[::-1], np.int32),
            "path_cost": np.array(pc[::-1], np.float64),
            "cost": np.array(Cm[1:], np.float64) if want_cost else None}


def alignment_quality(res, nq, nr):
    """GetAlignmentQuality (dtw.go:253-286); {} for an empty path."""
    pq, pr, pc = res["path_q"], res["path_r"], res["path_cost"]
    P = len(pq)
    if P == 0:
        return {}
    diag = sum(1 for k in range(1, P) if pq[k] > pq[k - 1] and pr[k] > pr[k - 1])
    total = 0.0
    for c in pc:
        total += float(c)
    ratio = diag / float(P - 1) if P > 1 else _NAN         # one point: Go's 0 / 0
    return {"path_efficiency": float(max(nq, nr)) / float(P), "diagonal_ratio": ratio,
            "average_cost": total / float(P), "normalized_distance": float(res["distance"])}


def optimize_step_pattern(q, r, band=-1, metric="euclidean"):
    """OptimizeStepPattern (dtw.go:288-311) -> (best pattern, {pattern: distance})."""
    best, best_d, ds = STEPS[0], _INF, {}
    for step in STEPS:
        d = dtw(q, r, band, step, metric)["distance"]
        ds[step] = d
        if d < best_d:
            best, best_d = step, d
    return best, ds


def same_result(got, ref, cost=False):
    """Bit-exact comparison of two result dicts: distance equal or both NaN, equal paths, costs
    equal with NaN == NaN.  Returns the list of fields that differ."""
    bad = []
    gd, rd = float(got["distance"]), float(ref["distance"])
    if not (gd == rd or (gd != gd and rd != rd)):
        bad.append(f"distance {gd!r} != {rd!r}")
    for k in ("path_q", "path_r"):
        if not np.array_equal(got[k], ref[k]):
            bad.append(k)
    if not np.array_equal(got["path_cost"], ref["path_cost"], equal_nan=True):
        bad.append("path_cost")
    if cost and not np.array_equal(got["cost"], ref["cost"], equal_nan=True):
        bad.append("cost")
    return bad
