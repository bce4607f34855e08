"""sonar_chroma_frame_matrix / sonar_chroma_similarity on the GPU against the Python checker
(tests/chroma_similarity_ref.py, held to hand-worked answers in test_chroma_similarity_cpu.py).

Comparison classes:
  bit-exact (NaN == NaN, integers equal): every value of Euclidean, Manhattan, Cosine, Pearson and
    Hellinger distances (each operation, sqrt included, is correctly rounded), of the Cosine / Pearson
    similarities 1 - d / 2, and everything decided from them: Binary, QMax, the transposition and its
    mean, OTI, the Smith-Waterman scores / best cell / path / overall, the DTW path and path scores.
  1e-12, |d| <= 1e-12 max(1, |ref|): what passes through a library exp / log: exp(-d) similarities, KL
    and JS distances, DTW's similarity matrix and overall.
  a recurrence over an inexact matrix: the device's own frame matrix is fed to the checker's
    smith_waterman(sim=) / dtw(cost=) / binary(sim=) / qmax(sim=); the result is then bit-exact.
  Direct's overall: |got - fsum mean| <= B = N 2^-53 sum|sim| / N over the matrix that was summed (the
    checker's for the exact metrics, the device's own for the exp-based ones: B bounds the order of the
    sum, not the exp).
Not tested: JS on identical frames (the sign of a rounding residue under the sqrt decides 0 against NaN
in the reference itself); non-finite inputs beyond one NaN frame for Cosine.

Shapes: the frame-matrix kernel tiles 64 x 64 per block, the DP kernels 64 x 64 per launch step
(T = 64): 63 / 64 / 65 in each dimension, (200, 129) = 4 x 3 tiles (six tile anti-diagonals), single
rows and columns, and (100, 300) / (300, 100) for the DTW band rule.  dim 12 runs the LDS instance,
24 and 7 the runtime-dimension one."""
import functools
import math

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library loads HIP (one HIP runtime in the process)

import chroma_similarity_ref as R
import sonar

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 40), (40, 1), (63, 5), (64, 64), (65, 2), (200, 129)]
EDGES = [(63, 65), (64, 64), (65, 63)]            # one below, at and above T in each dimension
ALL_METRICS = list(R.METRICS)
EXP_METRICS = ["euclidean", "kl", "js"]           # one plain exp(-d), the two with a log


@functools.lru_cache(maxsize=None)
def _inputs(nq, nr, dim=12, kind="plain"):
    """plain: uniform [0, 1); prob: [0.05, 1) for the probability metrics; rolled: the query is the
    reference rolled by 5 semitones plus 0.05 noise, the reference's frames one chroma profile plus 0.3
    noise each (so every frame pair, not only the aligned ones, tells the shift)."""
    rng = np.random.default_rng(1000003 * nq + 1009 * nr + dim)
    if kind == "rolled":
        base = 0.05 + rng.random(dim)[None, :] + 0.3 * rng.random((max(nq, nr), dim))
        r = base[:nr].copy()
        q = np.roll(base[:nq], 5, axis=1) + 0.05 * rng.random((nq, dim))
    else:
        lo = 0.05 if kind == "prob" else 0.0
        q, r = lo + (1.0 - lo) * rng.random((nq, dim)), lo + (1.0 - lo) * rng.random((nr, dim))
    q.setflags(write=False)
    r.setflags(write=False)
    return q, r


def _kind(metric):
    return "prob" if metric in ("kl", "js", "hellinger") else "plain"


@functools.lru_cache(maxsize=None)
def _ref(nq, nr, dim, kind, method, metric, **kw):
    q, r = _inputs(nq, nr, dim, kind)
    ref = R.compute_similarity(q, r, method, metric, **kw)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def _same_path(got, ref):
    assert got["path_q"].tolist() == ref["path_q"].tolist()
    assert got["path_r"].tolist() == ref["path_r"].tolist()
    assert R.same_bits(got["path_score"], ref["path_score"])


def _same_scalar(a, b):
    return a == b or (a != a and b != b)


def _check_direct_overall(got_overall, summed):
    flat = np.asarray(summed).ravel().tolist()
    n = len(flat)
    mean, bound = math.fsum(flat) / n, n * R.U * math.fsum(abs(v) for v in flat) / n
    print(f"direct overall {got_overall!r} fsum mean {mean!r} |d| {abs(got_overall - mean):.3e} B {bound:.3e}")
    assert abs(got_overall - mean) <= bound


# ---------------------------------------------------------------- the frame matrix ----
@pytest.mark.parametrize("nq,nr", SHAPES)
@pytest.mark.parametrize("metric", ALL_METRICS)
def test_frame_matrix(ctx, nq, nr, metric):
    q, r = _inputs(nq, nr, 12, _kind(metric))
    for shift in (0, 3):
        d, s = R.distances(q, r, metric, shift), R.similarities(q, r, metric, shift)
        gd = ctx.chroma_frame_matrix(q, r, metric, shift)
        gs = ctx.chroma_frame_matrix(q, r, metric, shift, as_similarity=True)
        if metric in R.EXACT_DISTANCES:
            assert R.same_bits(gd, d)
        else:
            assert R.close12(gd, d)
        if metric in R.EXACT_SIMILARITIES:
            assert R.same_bits(gs, s)
        else:
            assert R.close12(gs, s)


@pytest.mark.parametrize("dim", [24, 7])
@pytest.mark.parametrize("metric", ALL_METRICS)
def test_frame_matrix_runtime_dimension(ctx, dim, metric):
    q, r = _inputs(65, 70, dim, _kind(metric))
    d = R.distances(q, r, metric, 9)                          # shift 9 wraps at dim 7
    gd = ctx.chroma_frame_matrix(q, r, metric, 9)
    assert R.same_bits(gd, d) if metric in R.EXACT_DISTANCES else R.close12(gd, d)


def test_frame_matrix_unknown_metric_is_euclidean(ctx):
    q, r = _inputs(63, 5)
    assert R.same_bits(ctx.chroma_frame_matrix(q, r, 99), R.distances(q, r, "euclidean"))
    assert R.close12(ctx.chroma_frame_matrix(q, r, 99, as_similarity=True), R.similarities(q, r, "euclidean"))


def test_frame_matrix_device_pointers(ctx):
    q, r = _inputs(65, 63)
    dq, dr = torch.from_numpy(q.copy()).cuda(), torch.from_numpy(r.copy()).cuda()
    out = torch.zeros(65, 63, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.chroma_frame_matrix_device(dq.data_ptr(), 65, dr.data_ptr(), 63, 12, out.data_ptr(), "pearson", 2)
    assert R.same_bits(out.cpu().numpy(), R.distances(q, r, "pearson", 2))


# ---------------------------------------------------------------- every method ----
@pytest.mark.parametrize("method", list(R.METHODS))
def test_every_method_cosine_130x75(ctx, method):
    q, r = _inputs(130, 75)
    ref = _ref(130, 75, 12, "plain", method, "cosine")
    got = ctx.chroma_similarity(q, r, method, "cosine")
    if method == "dtw":
        assert R.close12(got["matrix"], ref["matrix"]) and R.close12(got["overall"], ref["overall"])
    else:
        assert R.same_bits(got["matrix"], ref["matrix"])
        if method == "direct":
            _check_direct_overall(got["overall"], ref["matrix"])
        else:
            assert _same_scalar(got["overall"], ref["overall"])
    assert got["best_transposition"] == ref["best_transposition"]
    _same_path(got, ref)
    if method in ("smith_waterman", "dtw"):
        assert len(got["path_q"]) > 0
    # the unknown method runs Direct
    if method == "direct":
        other = ctx.chroma_similarity(q, r, 17, "cosine")
        assert R.same_bits(other["matrix"], got["matrix"]) and other["overall"] == got["overall"]


@pytest.mark.parametrize("metric", ALL_METRICS)
def test_direct_every_metric_66x300(ctx, metric):
    q, r = _inputs(66, 300, 12, _kind(metric))
    ref = _ref(66, 300, 12, _kind(metric), "direct", metric)
    got = ctx.chroma_similarity(q, r, "direct", metric)
    if metric in R.EXACT_SIMILARITIES:
        assert R.same_bits(got["matrix"], ref["matrix"])
        _check_direct_overall(got["overall"], ref["matrix"])
    else:
        assert R.close12(got["matrix"], ref["matrix"])
        _check_direct_overall(got["overall"], got["matrix"])
        assert R.close12(got["overall"], ref["overall_fsum"])
    assert got["best_transposition"] == 0 and len(got["path_q"]) == 0


@pytest.mark.parametrize("nq,nr", SHAPES)
def test_direct_binary_qmax_shapes(ctx, nq, nr):
    q, r = _inputs(nq, nr)
    for metric in ("cosine", "pearson"):
        d = ctx.chroma_similarity(q, r, "direct", metric)
        assert R.same_bits(d["matrix"], R.similarities(q, r, metric))
        _check_direct_overall(d["overall"], d["matrix"])
        for thr in (0.4, 0.9):
            b, rb = ctx.chroma_similarity(q, r, "binary", metric, binary_threshold=thr), R.binary(q, r, metric, thr)
            assert R.same_bits(b["matrix"], rb["matrix"]) and b["overall"] == rb["overall"]
        assert ctx.chroma_similarity(q, r, "qmax", metric)["overall"] == R.qmax(q, r, metric)["overall"]


@pytest.mark.parametrize("metric", EXP_METRICS)
def test_binary_and_qmax_over_the_device_matrix(ctx, metric):
    q, r = _inputs(200, 129, 12, _kind(metric))
    sim = ctx.chroma_similarity(q, r, "direct", metric)["matrix"]
    assert R.close12(sim, R.similarities(q, r, metric))
    thr = float(np.median(sim))                               # half the cells on each side
    b, rb = ctx.chroma_similarity(q, r, "binary", metric, binary_threshold=thr), R.binary(threshold=thr, sim=sim)
    assert 0.3 < rb["overall"] < 0.7
    assert R.same_bits(b["matrix"], rb["matrix"]) and b["overall"] == rb["overall"]
    qm = ctx.chroma_similarity(q, r, "qmax", metric)
    assert R.same_bits(qm["matrix"], sim) and qm["overall"] == R.qmax(sim=sim)["overall"]


# ---------------------------------------------------------------- Smith-Waterman ----
@pytest.mark.parametrize("nq,nr", SHAPES + EDGES)
@pytest.mark.parametrize("metric", ["cosine", "pearson"])
def test_smith_waterman_exact(ctx, nq, nr, metric):
    q, r = _inputs(nq, nr)
    ref = _ref(nq, nr, 12, "plain", "smith_waterman", metric)
    got = ctx.chroma_similarity(q, r, "smith_waterman", metric)
    assert R.same_bits(got["matrix"], ref["matrix"])
    _same_path(got, ref)
    assert _same_scalar(got["overall"], ref["overall"]) and got["best_transposition"] == 0
    if len(ref["path_q"]):                                    # the best cell ends the path
        assert (got["path_q"][-1] + 1, got["path_r"][-1] + 1) == ref["best_cell"]
        assert got["path_score"][-1] == ref["max_score"]


@pytest.mark.parametrize("nq,nr", [(65, 63), (200, 129)])
@pytest.mark.parametrize("metric", EXP_METRICS)
def test_smith_waterman_over_the_device_matrix(ctx, nq, nr, metric):
    q, r = _inputs(nq, nr, 12, _kind(metric))
    sim = ctx.chroma_similarity(q, r, "direct", metric)["matrix"]
    ref = R.smith_waterman(sim=sim)
    got = ctx.chroma_similarity(q, r, "smith_waterman", metric)
    assert R.same_bits(got["matrix"], ref["matrix"])
    _same_path(got, ref)
    assert _same_scalar(got["overall"], ref["overall"])
    assert R.close12(got["matrix"], R.smith_waterman(q, r, metric)["matrix"])


def test_smith_waterman_nan_frame(ctx):
    """A NaN query frame makes its row of similarities NaN: those scores are NaN (math.Max), never the
    best cell, their code is 0, and every row below is NaN through delete = NaN - 0.1."""
    q, r = _inputs(70, 66)
    q = q.copy()
    q[40, 3] = math.nan
    ref = R.smith_waterman(q, r, "cosine")
    assert np.all(np.isnan(ref["matrix"][40:])) and ref["best_cell"][0] <= 40 and len(ref["path_q"]) > 0
    got = ctx.chroma_similarity(q, r, "smith_waterman", "cosine")
    assert R.same_bits(got["matrix"], ref["matrix"])
    _same_path(got, ref)
    assert got["overall"] == ref["overall"]


# ---------------------------------------------------------------- DTW ----
def _check_dtw(got, ref):
    _same_path(got, ref)
    assert R.close12(got["overall"], ref["overall"])
    assert R.close12(got["matrix"], ref["matrix"])
    if len(ref["path_q"]):                                    # the distance before exp
        assert got["path_score"][-1] == ref["acc"][-1, -1]
        assert _same_scalar(got["path_score"][-1] / len(got["path_q"]), ref["distance"])


@pytest.mark.parametrize("nq,nr", SHAPES + EDGES)
@pytest.mark.parametrize("metric", R.EXACT_DISTANCES)
def test_dtw_exact(ctx, nq, nr, metric):
    q, r = _inputs(nq, nr, 12, _kind(metric))
    ref = _ref(nq, nr, 12, _kind(metric), "dtw", metric)
    _check_dtw(ctx.chroma_similarity(q, r, "dtw", metric), ref)


@pytest.mark.parametrize("nq,nr", [(100, 300), (300, 100)])
@pytest.mark.parametrize("radius", [50, 0, 5])
def test_dtw_band_rule(ctx, nq, nr, radius):
    q, r = _inputs(nq, nr)
    ref = _ref(nq, nr, 12, "plain", "dtw", "cosine", dtw_band_radius=radius)
    got = ctx.chroma_similarity(q, r, "dtw", "cosine", dtw_band_radius=radius)
    _check_dtw(got, ref)
    plan = sonar.chroma_similarity_plan("dtw", nq, nr, 12, 10, radius)
    assert plan["dtw_skipped_columns"] == len(R.dtw_skipped_columns(nq, nr, radius))
    if radius > 0:                                            # the end cell is a skipped one: acc = 0
        assert plan["dtw_skipped_columns"] > 0 and got["overall"] == 1.0 and got["path_score"][-1] == 0.0


@pytest.mark.parametrize("nq,nr", [(65, 63), (200, 129)])
@pytest.mark.parametrize("metric", ["kl", "js"])
def test_dtw_over_the_device_matrix(ctx, nq, nr, metric):
    q, r = _inputs(nq, nr, 12, "prob")
    cost = ctx.chroma_frame_matrix(q, r, metric)
    assert R.close12(cost, R.distances(q, r, metric))
    ref = R.dtw(cost=cost)
    _check_dtw(ctx.chroma_similarity(q, r, "dtw", metric), ref)


def test_dtw_1x1(ctx):
    got = ctx.chroma_similarity([[3.0, 4.0]], [[3.0, 4.0]], "dtw", "cosine")
    assert math.isnan(got["overall"]) and len(got["path_q"]) == 0 and got["matrix"].tolist() == [[1.0]]
    got = ctx.chroma_similarity([[1.0, 0.0, 0.0, 0.0]], [[1.0, 1.0, 1.0, 1.0]], "dtw", "cosine")
    assert got["overall"] == 0.0 and len(got["path_q"]) == 0


# ---------------------------------------------------------------- transposition, OTI ----
@pytest.mark.parametrize("nq,nr", [(120, 75), (200, 129), (64, 64)])
@pytest.mark.parametrize("metric", ALL_METRICS)
def test_transposition_invariant_direct(ctx, nq, nr, metric):
    q, r = _inputs(nq, nr, 12, "rolled")
    best, mx, avgs = R.find_best_transposition(q, r, metric)
    assert best == 5                                          # not vacuous: a non-zero shift is expected
    got = ctx.chroma_similarity(q, r, "direct", metric, transposition_invariant=True)
    if metric in R.EXACT_SIMILARITIES:
        assert got["best_transposition"] == best and got["overall"] == mx
        assert R.same_bits(got["matrix"], R.similarities(q, r, metric, best))
        for method in ("binary", "qmax"):                     # the same shift, their own overall
            ref = R.compute_similarity(q, r, method, metric, transposition_invariant=True)
            g = ctx.chroma_similarity(q, r, method, metric, transposition_invariant=True)
            assert g["best_transposition"] == best and g["overall"] == ref["overall"]
            assert R.same_bits(g["matrix"], ref["matrix"])
    else:
        top = sorted(avgs, reverse=True)
        assert top[0] - top[1] > 1e-9                         # far beyond 1e-12 per term: the choice is safe
        assert got["best_transposition"] == best and R.close12(got["overall"], mx)
        assert R.close12(got["matrix"], R.similarities(q, r, metric, best))


@pytest.mark.parametrize("radius", [-1, 0, 10, 500])
@pytest.mark.parametrize("metric", ["cosine", "pearson"])
def test_oti_exact(ctx, radius, metric):
    q, r = _inputs(130, 75, 12, "rolled")
    ref = R.oti(q, r, metric, radius)
    got = ctx.chroma_similarity(q, r, "oti", metric, oti_radius=radius, transposition_invariant=True)
    if radius < 0:
        assert ref["matrix"] is None and got["matrix"] is None
        assert got["overall"] == 0.0 and got["best_transposition"] == 0
        return
    assert ref["best_transposition"] == 5
    assert got["best_transposition"] == 5 and got["overall"] == ref["overall"]
    assert R.same_bits(got["matrix"], ref["matrix"])
    assert sonar.chroma_similarity_plan("oti", 130, 75, 12, radius)["oti_cells"] == int(R.oti_band(130, 75, radius).sum())


@pytest.mark.parametrize("metric", EXP_METRICS)
def test_oti_exp_metrics(ctx, metric):
    q, r = _inputs(130, 75, 12, "rolled")
    ref = R.oti(q, r, metric, 10)
    order = np.argsort(ref["avgs"])[::-1]
    a, b = int(order[0]), int(order[1])
    assert ref["avgs"][a] - ref["avgs"][b] > ref["avg_bounds"][a] + ref["avg_bounds"][b]
    assert ref["best_transposition"] == 5
    got = ctx.chroma_similarity(q, r, "oti", metric, oti_radius=10)
    assert got["best_transposition"] == 5
    assert R.close12(got["overall"], ref["overall"]) and R.close12(got["matrix"], ref["matrix"])


def test_oti_nil(ctx):
    got = ctx.chroma_similarity(np.ones((6, 4)), -np.ones((5, 4)), "oti", "cosine")
    assert got["matrix"] is None and got["overall"] == 0.0 and got["best_transposition"] == 0


# ---------------------------------------------------------------- dimensions ----
@pytest.mark.parametrize("dim", [24, 7])
def test_methods_runtime_dimension(ctx, dim):
    q, r = _inputs(65, 70, dim, "rolled")
    for method in R.METHODS:
        ref = R.compute_similarity(q, r, method, "cosine", transposition_invariant=True)
        got = ctx.chroma_similarity(q, r, method, "cosine", transposition_invariant=True)
        if method == "dtw":
            assert R.close12(got["matrix"], ref["matrix"]) and R.close12(got["overall"], ref["overall"])
        else:
            assert R.same_bits(got["matrix"], ref["matrix"]) and _same_scalar(got["overall"], ref["overall"])
        assert got["best_transposition"] == ref["best_transposition"]
        _same_path(got, ref)
    assert R.find_best_transposition(q, r, "cosine")[0] == 5


# ---------------------------------------------------------------- matrix = NULL, repeatability ----
@pytest.mark.parametrize("method", list(R.METHODS))
def test_without_matrix_and_repeatable(ctx, method):
    q, r = _inputs(130, 75, 12, "rolled")
    kw = dict(method=method, metric="cosine", transposition_invariant=method in ("binary", "qmax"))
    full, again, lean = ctx.chroma_similarity(q, r, **kw), ctx.chroma_similarity(q, r, **kw), \
        ctx.chroma_similarity(q, r, matrix=False, **kw)
    assert R.same_bits(full["matrix"], again["matrix"]) and _same_scalar(full["overall"], again["overall"])
    _same_path(full, again)
    assert lean["matrix"] is None and lean["best_transposition"] == full["best_transposition"]
    _same_path(full, lean)
    if method == "direct":
        _check_direct_overall(full["overall"], full["matrix"])
        _check_direct_overall(lean["overall"], full["matrix"])
    else:
        assert _same_scalar(lean["overall"], full["overall"])


# ---------------------------------------------------------------- empty input, limits ----
def test_empty_inputs(ctx):
    e, r = np.zeros((0, 12)), _inputs(1, 40)[1]
    for a, b in ((e, r), (r, e), (e, e)):
        assert math.isnan(ctx.chroma_similarity(a, b, "direct")["overall"])
        assert ctx.chroma_similarity(a, b, "direct", transposition_invariant=True)["overall"] == 0.0
        assert math.isnan(ctx.chroma_similarity(a, b, "binary")["overall"])
        assert math.isnan(ctx.chroma_similarity(a, b, "smith_waterman")["overall"])
        assert ctx.chroma_similarity(a, b, "qmax")["overall"] == 0.0
        got = ctx.chroma_similarity(a, b, "oti")
        assert got["matrix"] is None and got["overall"] == 0.0 and got["best_transposition"] == 0
        with pytest.raises(sonar.SonarError, match=r"index out of range \[0\] with length 0") as ei:
            ctx.chroma_similarity(a, b, "dtw")
        assert ei.value.code == sonar.ERR_PANIC
        assert ctx.chroma_frame_matrix(a, b).shape == (a.shape[0], b.shape[0])


def test_cell_cap_and_arguments(ctx):
    q, r = np.zeros((40000, 1)), np.zeros((30000, 1))        # 1.2e9 cells > 2^30
    for method in ("smith_waterman", "dtw"):
        with pytest.raises(sonar.SonarError, match="2\\^30") as ei:
            ctx.chroma_similarity(q, r, method, matrix=False)
        assert ei.value.code == sonar.ERR_UNSUPPORTED
    with pytest.raises(sonar.SonarError) as ei:
        ctx.chroma_frame_matrix(_inputs(1, 40)[0], _inputs(1, 40)[1], "cosine", shift=-1)
    assert ei.value.code == sonar.ERR_PANIC


# ---------------------------------------------------------------- end to end on the device ----
def test_chroma_cqt_to_similarity_on_the_device(ctx):
    """Two tones and the same two tones five semitones up, through sonar_chroma_cqt and
    sonar_chroma_similarity without leaving the device; the checker runs on the same chroma rows."""
    cfg = dict(min_freq=200.0, max_freq=1600.0, bins_per_octave=12, q_factor=5.0, tuning_freq=440.0)
    t = np.arange(3000) / 8000.0
    up = 2.0 ** (5.0 / 12.0)
    xa = 0.5 + 0.3 * np.sin(2 * np.pi * 220.0 * t) + 0.2 * np.sin(2 * np.pi * 330.0 * t)
    xb = 0.5 + 0.3 * np.sin(2 * np.pi * 220.0 * up * t) + 0.2 * np.sin(2 * np.pi * 330.0 * up * t)
    F = sonar.chroma_cqt_plan(8000, n=3000, hop=64, **cfg)["n_frames"]
    da, db = torch.from_numpy(xa).cuda(), torch.from_numpy(xb).cuda()
    ca, cb = (torch.zeros(F, 12, dtype=torch.float64, device="cuda") for _ in range(2))
    mat = torch.zeros(F, F, dtype=torch.float64, device="cuda")
    pq, pr = (torch.zeros(2 * F, dtype=torch.int32, device="cuda") for _ in range(2))
    ps = torch.zeros(2 * F, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.chroma_cqt_device(da.data_ptr(), 3000, 64, 8000, ca.data_ptr(), **cfg)
    ctx.chroma_cqt_device(db.data_ptr(), 3000, 64, 8000, cb.data_ptr(), **cfg)
    got = ctx.chroma_similarity_device(ca.data_ptr(), F, cb.data_ptr(), F, 12, "dtw", "cosine", matrix_ptr=mat.data_ptr(),
                                       path_q_ptr=pq.data_ptr(), path_r_ptr=pr.data_ptr(), path_score_ptr=ps.data_ptr())
    ha, hb = ca.cpu().numpy(), cb.cpu().numpy()
    ref = R.dtw(ha, hb, "cosine", 50)
    P = got["path_len"]
    assert P == len(ref["path_q"]) > 0
    assert pq.cpu().numpy()[:P].tolist() == ref["path_q"].tolist() and pr.cpu().numpy()[:P].tolist() == ref["path_r"].tolist()
    assert R.same_bits(ps.cpu().numpy()[:P], ref["path_score"])
    assert R.close12(got["overall"], ref["overall"]) and R.close12(mat.cpu().numpy(), ref["matrix"])
    ti = ctx.chroma_similarity_device(ca.data_ptr(), F, cb.data_ptr(), F, 12, "direct", "cosine",
                                      transposition_invariant=True, matrix_ptr=mat.data_ptr())
    best, mx, _ = R.find_best_transposition(ha, hb, "cosine")
    assert (ti["best_transposition"], ti["overall"]) == (best, mx)
    assert R.same_bits(mat.cpu().numpy(), R.similarities(ha, hb, "cosine", best))
