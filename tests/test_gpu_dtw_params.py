"""sonar_dtw_params / sonar_dtw_optimize_step_pattern / sonar_dtw_quality on the GPU against the
float64 checker (tests/dtw_params_ref.py, pinned to the C oracle in test_dtw_params_cpu.py):
NewDTWAlignmentWithParams' three step patterns and four metrics (dtw.go:45-52, 137-162;
distance.go:10-107), with and without the cost matrix (full store / checkpoint columns + tile
recompute), banded and not, through the 12-dim and the runtime-dimension kernel instances.

Every comparison is bit-exact: distance equal or both NaN, equal paths, costs equal with NaN == NaN.
Shapes are the smallest that cross the pipeline's boundaries: 64-row bands, 8-step chunks, 16 moves
per code word, 64-column checkpoints and tiles, the 1,024-move flush of the walk."""
import functools
import math

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library loads HIP (one HIP runtime in the process)

import dtw_params_ref as R
import sonar

pytestmark = pytest.mark.gpu

METRICS = ["euclidean", "manhattan", "cosine", "pearson"]


def _data(nq, nr, dim=12, seed=0):
    rng = np.random.default_rng(1000 * nq + nr + 7 * dim + seed)
    return rng.random((nq, dim)), rng.random((nr, dim))


@functools.lru_cache(maxsize=None)
def _ref(nq, nr, dim, band, step, metric):
    """The checker's result (with the cost matrix) for _data(nq, nr, dim): computed once."""
    q, r = _data(nq, nr, dim)
    return R.dtw(q, r, band, step, metric, want_cost=True)


def _check(ctx, q, r, ref, band=-1, step="symmetric2", metric="euclidean", modes=(False, True)):
    for want_cost in modes:
        got = ctx.dtw_params(q, r, band=band, step=step, metric=metric, want_cost=want_cost)
        assert R.same_result(got, ref, cost=want_cost) == [], (step, metric, want_cost)


@pytest.mark.parametrize("want_cost", [False, True])
@pytest.mark.parametrize("nq,nr", [(66, 300), (700, 650)])
def test_defaults_equal_dtw(ctx, nq, nr, want_cost):
    q, r = _data(nq, nr)
    assert R.same_result(ctx.dtw_params(q, r, want_cost=want_cost), ctx.dtw(q, r, want_cost=want_cost),
                         cost=want_cost) == []


@pytest.mark.parametrize("want_cost", [False, True])
@pytest.mark.parametrize("nq,nr", [(130, 75), (66, 300)])
@pytest.mark.parametrize("step", R.STEPS)
@pytest.mark.parametrize("metric", METRICS)
def test_every_metric_and_step_pattern(ctx, metric, step, nq, nr, want_cost):
    q, r = _data(nq, nr)
    _check(ctx, q, r, _ref(nq, nr, 12, -1, step, metric), step=step, metric=metric, modes=(want_cost,))


@pytest.mark.parametrize("nq,nr", [(1, 1), (1, 40), (63, 5), (64, 64), (65, 2), (200, 129)])
@pytest.mark.parametrize("step,metric", [("symmetric1", m) for m in METRICS] + [("asymmetric", "euclidean")])
def test_edge_shapes(ctx, step, metric, nq, nr):
    q, r = _data(nq, nr)
    _check(ctx, q, r, _ref(nq, nr, 12, -1, step, metric), step=step, metric=metric)


@pytest.mark.parametrize("step,metric", [("symmetric2", m) for m in METRICS] +
                         [("asymmetric", "euclidean"), ("symmetric1", "euclidean")])
def test_700_by_650(ctx, step, metric):
    """The asymmetric path has 1,350 points: past the walk's 1,024-move flush, and along row 0."""
    q, r = _data(700, 650)
    ref = _ref(700, 650, 12, -1, step, metric)
    if step == "asymmetric":
        assert len(ref["path_q"]) == 1350 and ref["path_q"][0] == -1 and ref["distance"] == math.inf
    _check(ctx, q, r, ref, step=step, metric=metric)


@pytest.mark.parametrize("nq,nr,band", [(300, 330, 40), (10, 100, 5)])
def test_banded_cosine_symmetric1(ctx, nq, nr, band):
    q, r = _data(nq, nr)
    _check(ctx, q, r, _ref(nq, nr, 12, band, "symmetric1", "cosine"), band=band, step="symmetric1", metric="cosine")


@pytest.mark.parametrize("dim", [1, 5])
@pytest.mark.parametrize("step,metric", [("symmetric1", "euclidean"), ("symmetric2", "manhattan"),
                                         ("symmetric1", "cosine"), ("symmetric2", "pearson"),
                                         ("symmetric1", "pearson")])
def test_runtime_dimension(ctx, step, metric, dim):
    q, r = _data(130, 75, dim)
    ref = _ref(130, 75, dim, -1, step, metric)
    if metric == "pearson" and dim == 1:                     # one value per row: zero square sums
        assert np.all(R.local_distances(q, r, "pearson") == 1.0)
    _check(ctx, q, r, ref, step=step, metric=metric)


@pytest.mark.parametrize("dim", [12, 5])
def test_zero_and_constant_rows_take_the_exact_one_branch(ctx, dim):
    q, r = _data(130, 75, dim, seed=1)
    q[3] = 0.0; q[64:70] = 0.0; r[0] = 0.0; r[40:43] = 0.0
    assert (R.local_distances(q, r, "cosine") == 1.0).sum() >= 7 * 75
    _check(ctx, q, r, R.dtw(q, r, -1, "symmetric1", "cosine", want_cost=True), step="symmetric1", metric="cosine")
    q, r = _data(130, 75, dim, seed=2)
    q[5] = 0.25; q[100:104] = -3.0; r[74] = 1e-3; r[10:12] = 7.0
    assert (R.local_distances(q, r, "pearson") == 1.0).sum() >= 5 * 75
    _check(ctx, q, r, R.dtw(q, r, -1, "symmetric2", "pearson", want_cost=True), metric="pearson")


def test_identical_sequences_under_cosine_give_negative_costs(ctx):
    q, _ = _data(130, 75)
    ref = R.dtw(q, q, -1, "symmetric1", "cosine", want_cost=True)
    assert ref["path_cost"].min() < 0 and np.nanmin(ref["cost"]) < 0
    _check(ctx, q, q, ref, step="symmetric1", metric="cosine")


@pytest.mark.parametrize("metric", ["cosine", "pearson"])
def test_finite_rows_of_magnitude_1e200_give_nan_distances(ctx, metric):
    q, r = _data(130, 75)
    q, r = q * 1e200, r * 1e200
    ref = R.dtw(q, r, -1, "symmetric2", metric, want_cost=True)
    assert np.all(np.isfinite(q)) and math.isnan(ref["distance"])
    _check(ctx, q, r, ref, metric=metric)


@pytest.mark.parametrize("kind", ["nan", "inf", "ninf"])
def test_nonfinite_inputs_under_manhattan_symmetric1(ctx, kind):
    q, r = _data(130, 75, seed=3)
    v = {"nan": np.nan, "inf": np.inf, "ninf": -np.inf}[kind]
    q[17, 3] = v
    q[64:66, 0] = v
    q[0, 5] = v
    _check(ctx, q, r, R.dtw(q, r, -1, "symmetric1", "manhattan", want_cost=True), step="symmetric1",
           metric="manhattan")


@pytest.mark.parametrize("want_cost", [False, True])
def test_device_pointers_equal_host_pointers(ctx, want_cost):
    nq, nr = 130, 75
    q, r = _data(nq, nr)
    host = ctx.dtw_params(q, r, step="symmetric1", metric="cosine", want_cost=want_cost)
    dq, dr = torch.from_numpy(q).cuda(), torch.from_numpy(r).cuda()
    pq = torch.zeros(nq + nr + 1, dtype=torch.int32, device="cuda")
    pr = torch.zeros(nq + nr + 1, dtype=torch.int32, device="cuda")
    pc = torch.zeros(nq + nr + 1, dtype=torch.float64, device="cuda")
    cost = torch.zeros((nq, nr + 1), dtype=torch.float64, device="cuda") if want_cost else None
    torch.cuda.synchronize()
    dist, P = ctx.dtw_params_device(dq.data_ptr(), nq, dr.data_ptr(), nr, 12, pq.data_ptr(), pr.data_ptr(),
                                    pc.data_ptr(), step="symmetric1", metric="cosine",
                                    cost_ptr=cost.data_ptr() if want_cost else None)
    got = {"distance": dist, "path_q": pq[:P].cpu().numpy(), "path_r": pr[:P].cpu().numpy(),
           "path_cost": pc[:P].cpu().numpy(), "cost": cost.cpu().numpy() if want_cost else None}
    assert R.same_result(got, host, cost=want_cost) == []
    assert R.same_result(got, _ref(nq, nr, 12, -1, "symmetric1", "cosine"), cost=want_cost) == []


def test_unknown_step_pattern_and_empty_sequences(ctx):
    q, r = _data(20, 30)
    for bad in ("zigzag", 3, -1):
        with pytest.raises(sonar.SonarError) as e:
            ctx.dtw_params(q, r, step=bad)
        assert e.value.code == sonar.ERR_INVALID
        assert e.value.msg == f"failed to fill cost matrix: unknown step pattern: {bad}"   # Go: the name
    with pytest.raises(sonar.SonarError) as e:              # the empty-sequence error comes first
        ctx.dtw_params(np.zeros((0, 12)), r, step="zigzag")
    assert e.value.code == sonar.ERR_EMPTY and "empty sequences provided" in e.value.msg
    ok = ctx.dtw_params(q, r, step="symmetric1", metric="manhattan")     # the context stays usable
    assert R.same_result(ok, R.dtw(q, r, -1, "symmetric1", "manhattan")) == []


@pytest.mark.parametrize("metric", ["mahalanobis", 4, 99, -5])
@pytest.mark.parametrize("step", ["symmetric2", "symmetric1"])
def test_mahalanobis_and_unknown_metrics_are_euclidean(ctx, step, metric):
    q, r = _data(130, 75)
    got = ctx.dtw_params(q, r, step=step, metric=metric, want_cost=True)
    assert R.same_result(got, ctx.dtw_params(q, r, step=step, metric="euclidean", want_cost=True), cost=True) == []
    assert R.same_result(got, _ref(130, 75, 12, -1, step, "euclidean"), cost=True) == []


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_optimize_step_pattern(ctx, metric):
    q, r = _data(130, 75)
    best, dists = ctx.dtw_optimize_step_pattern(q, r, metric=metric)
    ref = {s: _ref(130, 75, 12, -1, s, metric)["distance"] for s in R.STEPS}
    assert dists == ref and list(dists) == list(R.STEPS)
    ref_best = R.STEPS[0]
    for s in R.STEPS:                                        # strict <, starting from symmetric2
        if ref[s] < ref[ref_best]:
            ref_best = s
    assert best == ref_best


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_optimize_step_pattern_on_device_pointers(ctx, metric):
    """The entry asks its three Align calls for no path: with device pointers the path kernels must
    write to the library's scratch, not through the null path pointers."""
    nq, nr = 130, 75
    q, r = _data(nq, nr)
    dq, dr = torch.from_numpy(q).cuda(), torch.from_numpy(r).cuda()
    torch.cuda.synchronize()
    got = ctx.dtw_optimize_step_pattern_device(dq.data_ptr(), nq, dr.data_ptr(), nr, 12, metric=metric)
    assert got == ctx.dtw_optimize_step_pattern(q, r, metric=metric)
    assert got[1] == {s: _ref(nq, nr, 12, -1, s, metric)["distance"] for s in R.STEPS}


@pytest.mark.parametrize("step,metric", [("symmetric2", "euclidean"), ("symmetric1", "cosine")])
def test_device_pointers_with_null_path_outputs(ctx, step, metric):
    """Distance and path length only (path_q / path_r / path_cost null), existing and new instances."""
    nq, nr = 130, 75
    q, r = _data(nq, nr)
    dq, dr = torch.from_numpy(q).cuda(), torch.from_numpy(r).cuda()
    torch.cuda.synchronize()
    ref = _ref(nq, nr, 12, -1, step, metric)
    dist, P = ctx.dtw_params_device(dq.data_ptr(), nq, dr.data_ptr(), nr, 12, None, None, None, step=step,
                                    metric=metric)
    assert dist == ref["distance"] and P == len(ref["path_q"])


def test_dtw_quality_of_a_gpu_result(ctx):
    q, r = _data(130, 75)
    for step in R.STEPS:                                     # asymmetric: NaN costs, +Inf distance
        res = ctx.dtw_params(q, r, step=step, metric="cosine")
        got, ref = sonar.dtw_quality(res, 130, 75), R.alignment_quality(res, 130, 75)
        for k, v in ref.items():
            assert got[k] == v or (math.isnan(got[k]) and math.isnan(v)), (step, k, got[k], v)


def test_no_band_pipeline_timeout(ctx):
    """No instance of the new family may report a timeout of the band pipeline's bounded waits."""
    q, r = _data(700, 650)
    before = ctx.dtw_counters()
    for metric in METRICS:
        ctx.dtw_params(q, r, step="symmetric1", metric=metric)
    after = ctx.dtw_counters()
    assert after["dtw_timeouts"] == before["dtw_timeouts"] and after["waves_timed_out"] == before["waves_timed_out"]
