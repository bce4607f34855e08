"""The checker of sonar_chroma_frame_matrix / sonar_chroma_similarity / sonar_chroma_similarity_plan: a
float64 restatement of the reference's chroma sequence similarity (test infrastructure, never the
product).

  ChromaSequenceSimilarity.ComputeSimilarity, all six methods, findBestTransposition,
  tracebackAlignment, tracebackDTW               (algorithms/chroma/chroma_similarity.go:86-538)
  ChromaVectorAnalyzer.Distance / Similarity / CircularShift
                                                 (algorithms/chroma/chroma_vector.go:145-216)
  Euclidean / Manhattan / Cosine / Pearson / KLDivergence / JensenShannon / HellingerDistanceFunc,
  normalizeToProbability                         (algorithms/stats/distance.go:28-108, 247-294, 341-369)

The frame matrices are built with numpy one feature index at a time: elementwise numpy arithmetic is
unfused and keeps Go's summation order, and +, -, *, /, sqrt and abs are correctly rounded, so every
value of the five metrics without a logarithm has Go's bits (numpy's exp and log are within an ulp or
two of Go's).  Sums the reference takes serially are taken with np.cumsum, which adds in index order.
The two recurrences and their tracebacks are plain Python loops with math.Max / math.Min's rules."""
import math

import numpy as np

from dtw_params_ref import go_min, local_distances

METHODS = {"direct": 0, "binary": 1, "smith_waterman": 2, "dtw": 3, "qmax": 4, "oti": 5}
METRICS = {"euclidean": 0, "manhattan": 1, "cosine": 2, "pearson": 3, "kl": 4, "js": 5, "hellinger": 6}
EXACT_DISTANCES = ("euclidean", "manhattan", "cosine", "pearson", "hellinger")   # no exp / log inside
EXACT_SIMILARITIES = ("cosine", "pearson")                                        # 1 - d / 2
_NAN = math.nan
_INF = math.inf
U = 2.0 ** -53


def go_max(x, y):
    """math.Max: +Inf wins, then NaN propagates, +0 > -0."""
    if x == _INF or y == _INF:
        return _INF
    if x != x or y != y:
        return _NAN
    if x == 0 and y == 0:
        return y if math.copysign(1.0, x) < 0 else x
    return x if x > y else y


def _metric(m):
    m = METRICS[m] if isinstance(m, str) else int(m)
    return m if 0 <= m <= 6 else 0                            # Distance's default case: Euclidean


def _frames(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.size == 0:
        return a.reshape(0, a.shape[1] if a.ndim == 2 else 0)
    return a[:, None] if a.ndim == 1 else a


def _serial_sum(v):
    """0.0 + v[0] + v[1] + ... in index order."""
    v = np.ascontiguousarray(v, dtype=np.float64).ravel()
    return float(np.cumsum(v)[-1]) if v.size else 0.0


def _div(a, b):
    """Go's float64 division (x / 0 = +-Inf, 0 / 0 = NaN)."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def circular_shift(x, shift):
    """CircularShift on every row: value k is x[(k + shift) % dim] (chroma_vector.go:207-216)."""
    x = _frames(x)
    dim = x.shape[1]
    return x[:, (np.arange(dim) + shift) % dim] if dim else x


def normalize_to_probability(x):
    """normalizeToProbability on every row (distance.go:341-369)."""
    x = _frames(x)
    n, dim = x.shape
    with np.errstate(all="ignore"):
        s = np.zeros(n)
        for k in range(dim):
            s = np.where(x[:, k] > 0, s + x[:, k], s)
        out = np.empty_like(x)
        for k in range(dim):
            out[:, k] = np.where(s == 0, 1.0 / float(dim), np.where(x[:, k] > 0, x[:, k] / s, 0.0))
    return out


def js_distances(p, q, renormalize=True):
    """JensenShannonDistanceFunc of every pair of rows (distance.go:264-280).  renormalize=False is the
    textbook form that does not normalise KLDivergenceFunc's arguments a second time."""
    pn, qn = normalize_to_probability(p), normalize_to_probability(q)
    n, dim = pn.shape
    m_ = qn.shape[0]
    with np.errstate(all="ignore"):
        if renormalize:
            p2, q2 = normalize_to_probability(pn), normalize_to_probability(qn)
            msum = np.zeros((n, m_))
            for k in range(dim):
                m = (pn[:, k, None] + qn[None, :, k]) / 2.0
                msum = np.where(m > 0, msum + m, msum)
        else:
            p2, q2 = pn, qn
        kl1, kl2 = np.zeros((n, m_)), np.zeros((n, m_))
        for k in range(dim):
            m = (pn[:, k, None] + qn[None, :, k]) / 2.0
            m2 = np.where(msum == 0, 1.0 / float(dim), np.where(m > 0, m / msum, 0.0)) if renormalize else m
            pk, qk = p2[:, k, None], q2[None, :, k]
            kl1 = np.where((pk > 0) & (m2 > 0), kl1 + pk * np.log(pk / m2), kl1)
            kl2 = np.where((qk > 0) & (m2 > 0), kl2 + qk * np.log(qk / m2), kl2)
        return np.sqrt(0.5 * kl1 + 0.5 * kl2)


def distances(q, r, metric="cosine", shift=0):
    """Distance(CircularShift(q[i], shift), r[j]) for every pair (nq x nr)."""
    q, r = circular_shift(q, shift), _frames(r)
    m = _metric(metric)
    if m <= 3:
        return local_distances(q, r, m)
    nq, dim = q.shape
    nr = r.shape[0]
    with np.errstate(all="ignore"):
        if m == 5:
            return js_distances(q, r)
        p, pr = normalize_to_probability(q), normalize_to_probability(r)
        if m == 4:                                           # KLDivergenceFunc :248-261
            kl = np.zeros((nq, nr))
            for k in range(dim):
                pk, qk = p[:, k, None], pr[None, :, k]
                kl = np.where((pk > 0) & (qk > 0), kl + pk * np.log(pk / qk), kl)
            return kl
        s = np.zeros((nq, nr))                               # HellingerDistanceFunc :283-294
        sp, sq = np.sqrt(p), np.sqrt(pr)
        for k in range(dim):
            df = sp[:, k, None] - sq[None, :, k]
            s = s + df * df
        return np.sqrt(s) / np.sqrt(2.0)


def similarity_of(d, metric):
    """Similarity from Distance (chroma_vector.go:172-186)."""
    with np.errstate(all="ignore"):
        return 1.0 - (d / 2.0) if _metric(metric) in (2, 3) else np.exp(-d)


def similarities(q, r, metric="cosine", shift=0):
    return similarity_of(distances(q, r, metric, shift), metric)


def sample_step(nq):
    return int(max(1.0, float(nq) / 50.0))


def find_best_transposition(q, r, metric="cosine"):
    """findBestTransposition (:450-479) -> (bestShift, maxSimilarity, the 12 means)."""
    q, r = _frames(q), _frames(r)
    step = sample_step(q.shape[0])
    best, mx, avgs = 0, 0.0, []
    for shift in range(12):
        S = similarities(q[::step], r[::step], metric, shift) if q.shape[0] and r.shape[0] else np.zeros((0, 0))
        avg = _div(_serial_sum(S), float(S.size))
        avgs.append(avg)
        if avg > mx:
            best, mx = shift, avg
    return best, mx, avgs


def direct(q, r, metric="cosine", transposition_invariant=False):
    """computeDirectSimilarity (:106-159).  overall is Go's serial row-major mean; overall_fsum the
    exactly rounded mean and bound = N 2^-53 sum|sim| / N, which any summation order of the N terms
    obeys."""
    q, r = _frames(q), _frames(r)
    nq, nr = q.shape[0], r.shape[0]
    best, mx = (find_best_transposition(q, r, metric)[:2] if transposition_invariant else (0, 0.0))
    S = similarities(q, r, metric, best) if nq and nr else np.zeros((nq, nr))
    N = nq * nr
    flat = S.ravel()
    finite = bool(np.all(np.isfinite(flat)))
    go_order = _div(_serial_sum(flat), float(N))
    return {"matrix": S, "overall": mx if transposition_invariant else go_order,
            "overall_go_order": go_order,
            "overall_fsum": math.fsum(flat.tolist()) / N if N and finite else _NAN,
            "bound": N * U * math.fsum(np.abs(flat).tolist()) / N if N and finite else _NAN,
            "best_transposition": best}


def binary(q=None, r=None, metric="cosine", threshold=0.4, transposition_invariant=False, sim=None):
    """computeBinarySimilarity (:162-194); sim: a precomputed Direct matrix."""
    d = direct(q, r, metric, transposition_invariant) if sim is None else {"matrix": np.asarray(sim), "best_transposition": 0}
    B = (d["matrix"] > threshold).astype(np.float64)
    return {"matrix": B, "overall": _div(float(B.sum()), float(B.size)), "best_transposition": d["best_transposition"]}


def qmax(q=None, r=None, metric="cosine", transposition_invariant=False, sim=None):
    """computeQMaxSimilarity (:362-397), diagonal by diagonal as written."""
    d = direct(q, r, metric, transposition_invariant) if sim is None else {"matrix": np.asarray(sim), "best_transposition": 0}
    S = d["matrix"]
    nq, nr = S.shape
    rows = S.tolist()
    mx = 0.0
    for dd in range(-(nr - 1), nq):
        dmax = 0.0
        for i in range(max(0, dd), min(nq, nr + dd)):
            v = rows[i][i - dd]
            if v > dmax:
                dmax = v
        if dmax > mx:
            mx = dmax
    return {"matrix": S, "overall": mx, "best_transposition": d["best_transposition"]}


def oti_band(nq, nr, radius):
    """The cells OTI computes (:422): j from max(0, i - R) while j < min(nr, i + R + 1)."""
    i, j = np.arange(nq)[:, None], np.arange(nr)[None, :]
    return (j >= np.maximum(0, i - radius)) & (j < np.minimum(nr, i + radius + 1))


def oti(q, r, metric="cosine", radius=10):
    """computeOTISimilarity (:400-445).  matrix None = Go's nil.  avgs: the 12 averages; avg_bounds: what
    another order of each sum, of terms each within 1e-12 of these, can change its average by."""
    q, r = _frames(q), _frames(r)
    nq, nr = q.shape[0], r.shape[0]
    band = oti_band(nq, nr, radius)
    best, mx, bestM, avgs, bounds = 0, 0.0, None, [], []
    for shift in range(12):
        S = similarities(q, r, metric, shift) if nq and nr else np.zeros((nq, nr))
        terms = S[band]                                      # row-major: Go's order
        avg = _div(_serial_sum(terms), float(nq * nr))
        avgs.append(avg)
        with np.errstate(all="ignore"):
            bounds.append(_div(terms.size * (1e-12 + U * float(np.abs(terms).sum())), float(nq * nr)))
        if avg > mx:
            best, mx, bestM = shift, avg, np.where(band, S, 0.0)
    return {"matrix": bestM, "overall": mx, "best_transposition": best, "avgs": avgs, "avg_bounds": bounds}


def _path(pq, pr, ps):
    return {"path_q": np.array(pq[::-1], np.int32), "path_r": np.array(pr[::-1], np.int32),
            "path_score": np.array(ps[::-1], np.float64)}


def smith_waterman(q=None, r=None, metric="cosine", sim=None):
    """computeSmithWatermanSimilarity + tracebackAlignment (:197-271, :482-507).  sim: a precomputed
    frame similarity matrix.  matrix = scores[1:][1:]; best_cell = (maxI, maxJ), 1-based, (0, 0) when
    nothing scores."""
    S = (similarities(q, r, metric) if _frames(q).shape[0] and _frames(r).shape[0]
         else np.zeros((_frames(q).shape[0], _frames(r).shape[0]))) if sim is None else np.asarray(sim, np.float64)
    nq, nr = S.shape
    sim_rows = S.tolist()
    sc = [[0.0] * (nr + 1) for _ in range(nq + 1)]
    tb = [[0] * (nr + 1) for _ in range(nq + 1)]
    mx, mi, mj = 0.0, 0, 0
    for i in range(1, nq + 1):
        prev, cur, srow, trow = sc[i - 1], sc[i], sim_rows[i - 1], tb[i]
        for j in range(1, nr + 1):
            match = prev[j - 1] + srow[j - 1]
            delete = prev[j] - 0.1
            insert = cur[j - 1] - 0.1
            v = go_max(0.0, go_max(match, go_max(delete, insert)))
            cur[j] = v
            if v > mx:
                mx, mi, mj = v, i, j
            if v == match:                                   # switch maxVal: float equality, in this order
                trow[j] = 1
            elif v == delete:
                trow[j] = 2
            elif v == insert:
                trow[j] = 3
    pq, pr, ps = [], [], []
    i, j = mi, mj
    while i > 0 and j > 0 and sc[i][j] > 0:
        pq.append(i - 1)
        pr.append(j - 1)
        ps.append(sc[i][j])
        t = tb[i][j]
        if t == 1:
            i, j = i - 1, j - 1
        elif t == 2:
            i -= 1
        elif t == 3:
            j -= 1
        else:
            break
    out = {"matrix": np.array([row[1:] for row in sc[1:]], np.float64).reshape(nq, nr),
           "overall": _div(mx, float(len(pq))), "best_transposition": 0, "best_cell": (mi, mj), "max_score": mx}
    out.update(_path(pq, pr, ps))
    return out


def dtw_skipped_columns(nq, nr, radius):
    """The columns the band rule (:315-320) skips in every row i >= 1: it depends on j only."""
    if radius <= 0 or nq < 2:
        return []
    return [j for j in range(1, nr) if abs(j - int(float(j * nq) / float(nr))) > radius]


def dtw(q=None, r=None, metric="cosine", band_radius=50, cost=None):
    """computeDTWSimilarity + tracebackDTW (:274-352, :510-538).  cost: a precomputed distance matrix.
    acc: the accumulated costs; distance: acc[nq-1][nr-1] / len(path), the value before exp."""
    if cost is None:
        q, r = _frames(q), _frames(r)
        if q.shape[0] == 0 or r.shape[0] == 0:
            raise IndexError("runtime error: index out of range [0] with length 0")
        C = distances(q, r, metric)
    else:
        C = np.asarray(cost, np.float64)
    nq, nr = C.shape
    c = C.tolist()
    acc = [[0.0] * nr for _ in range(nq)]
    acc[0][0] = c[0][0]
    for i in range(1, nq):
        acc[i][0] = acc[i - 1][0] + c[i][0]
    for j in range(1, nr):
        acc[0][j] = acc[0][j - 1] + c[0][j]
    skipped = set(dtw_skipped_columns(nq, nr, band_radius))
    for i in range(1, nq):
        prev, cur, crow = acc[i - 1], acc[i], c[i]
        for j in range(1, nr):
            if j in skipped:
                continue                                     # the cell keeps 0, not +Inf
            cur[j] = crow[j] + go_min(prev[j], go_min(cur[j - 1], prev[j - 1]))
    pq, pr, ps = [], [], []
    i, j = nq - 1, nr - 1
    while i > 0 or j > 0:
        pq.append(i)
        pr.append(j)
        ps.append(acc[i][j])
        if i == 0:
            j -= 1
        elif j == 0:
            i -= 1
        else:
            dg, up, lf = acc[i - 1][j - 1], acc[i - 1][j], acc[i][j - 1]
            if dg <= up and dg <= lf:
                i, j = i - 1, j - 1
            elif up <= lf:
                i -= 1
            else:
                j -= 1
    dist = _div(acc[nq - 1][nr - 1], float(len(pq)))
    with np.errstate(all="ignore"):
        out = {"matrix": np.exp(-C), "overall": float(np.exp(np.float64(-dist))), "best_transposition": 0,
               "acc": np.array(acc, np.float64).reshape(nq, nr), "distance": dist}
    out.update(_path(pq, pr, ps))
    return out


def compute_similarity(q, r, method="direct", metric="cosine", binary_threshold=0.4, oti_radius=10,
                       dtw_band_radius=50, transposition_invariant=False):
    """ComputeSimilarity (:86-103) -> the dict of sonar.Context.chroma_similarity (plus the checker's
    extras); an unknown method runs Direct."""
    m = METHODS[method] if isinstance(method, str) else int(method)
    if m == 1:
        out = binary(q, r, metric, binary_threshold, transposition_invariant)
    elif m == 2:
        return smith_waterman(q, r, metric)
    elif m == 3:
        return dtw(q, r, metric, dtw_band_radius)
    elif m == 4:
        out = qmax(q, r, metric, transposition_invariant)
    elif m == 5:
        out = oti(q, r, metric, oti_radius)
    else:
        out = direct(q, r, metric, transposition_invariant)
    out.update(_path([], [], []))
    return out


def plan(nq, nr, oti_radius=10, dtw_band_radius=50):
    """The integer side sonar_chroma_similarity_plan exposes."""
    step = sample_step(nq)
    return {"sample_step": step, "sampled_pairs": len(range(0, nq, step)) * len(range(0, nr, step)),
            "oti_cells": int(oti_band(nq, nr, oti_radius).sum()),
            "dtw_skipped_columns": len(dtw_skipped_columns(nq, nr, dtw_band_radius))}


def same_bits(a, b):
    """Arrays (or scalars) equal bit for bit up to NaN == NaN and -0 == +0."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.array_equal(a, b, equal_nan=a.dtype.kind == "f"))


def close12(got, ref):
    """|got - ref| <= 1e-12 max(1, |ref|) elementwise, NaN == NaN, infinities equal."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.shape != ref.shape:
        return False
    with np.errstate(all="ignore"):
        ok = np.abs(got - ref) <= 1e-12 * np.maximum(1.0, np.abs(ref))
    return bool(np.all(ok | (got == ref) | (np.isnan(got) & np.isnan(ref))))
