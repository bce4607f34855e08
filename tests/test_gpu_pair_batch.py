"""The batched pair path of sonar_align_pairs (one band-kernel launch over a batch's chroma DTWs,
batched walk / path decode, one host sync per batch) against the unbatched path
(SONAR_PAIR_BATCH=0: one sonar_align_pair_device per pair).  Pairs are independent and both paths
run the same arithmetic, so records must be identical (NaN-aware), for pairs of different lengths,
any batch cut, and a pair whose chroma is not finite (the batch redoes it through the exact
math.Min path and flags the record SONAR_PAIR_REDONE_NONFINITE).  Every batched run here also
checks that no band pipeline timed out (the retry would hide it)."""
import numpy as np
import pytest
import torch  # noqa: F401 -- before the library loads HIP (one HIP runtime in the process)

import sonar
from sonar import synth

pytestmark = pytest.mark.gpu


def _same(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(
        np.nan_to_num(a), np.nan_to_num(b))


@pytest.fixture(scope="module")
def mixed_pairs():
    rng = np.random.default_rng(11)
    qs, rs = [], []
    for k, (sq, sr_) in enumerate([(6.0, 7.5), (9.0, 5.0), (3.3, 3.3), (12.0, 10.7), (4.1, 8.9)]):
        q, r = synth.c3_pair(max(sq, sr_), 0.4 + 0.3 * k)[:2]
        qs.append(np.ascontiguousarray(q[: int(sq * 44100)]))
        rs.append(np.ascontiguousarray(r[: int(sr_ * 44100)] + 1e-3 * rng.standard_normal(int(sr_ * 44100))))
    return qs, rs


def _run(ctx, monkeypatch, qs, rs, **env):
    env.setdefault("SONAR_PAIR_RETRY", 0)     # a timed-out pipeline is an error here, never a silent redo
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    try:
        ctx.dtw_counters(reset=True)
        out = ctx.align_pairs(qs, rs, max_lag_seconds=4.0, workers=4)
        assert ctx.dtw_counters(reset=True)["dtw_timeouts"] == 0
        return out
    finally:
        for k in env:
            monkeypatch.delenv(k)


@pytest.mark.parametrize("streams", [1, 2, 3])
def test_batched_equals_unbatched_mixed_lengths(ctx, monkeypatch, mixed_pairs, streams):
    qs, rs = mixed_pairs
    ref = _run(ctx, monkeypatch, qs, rs, SONAR_PAIR_BATCH=0)
    got = _run(ctx, monkeypatch, qs, rs, SONAR_PAIR_STREAMS=streams)
    assert np.all(ref["status"] == 0) and np.all(got["status"] == 0)
    for f in sonar.PAIR_FIELDS:
        assert _same(got[f], ref[f]), f


def test_batched_memory_budget_cut(ctx, monkeypatch, mixed_pairs):
    """A tiny device budget forces one pair per batch: same records."""
    qs, rs = mixed_pairs
    ref = _run(ctx, monkeypatch, qs, rs, SONAR_PAIR_BATCH=0)
    got = _run(ctx, monkeypatch, qs, rs, SONAR_PAIR_STREAMS=1, SONAR_PAIR_BATCH_GB=0.001)
    for f in sonar.PAIR_FIELDS:
        assert _same(got[f], ref[f]), f


def test_batched_nonfinite_pair_redone_exactly(ctx, monkeypatch, mixed_pairs):
    qs, rs = [x.copy() for x in mixed_pairs[0]], [x.copy() for x in mixed_pairs[1]]
    qs[1][5000] = np.nan                      # chroma frames around it become NaN
    rs[3][7000] = np.inf
    ref = _run(ctx, monkeypatch, qs, rs, SONAR_PAIR_BATCH=0)
    got = _run(ctx, monkeypatch, qs, rs, SONAR_PAIR_STREAMS=2)
    assert np.array_equal(got["status"], ref["status"])
    for f in sonar.PAIR_FIELDS:
        assert _same(got[f], ref[f]), f
    flagged = np.nonzero(got["flags"])[0].tolist()
    assert flagged == [1, 3], flagged
    assert np.all(got["flags"][[1, 3]] == sonar.PAIR_REDONE_NONFINITE)


def test_trim_releases_and_reallocates(ctx, monkeypatch, mixed_pairs):
    """sonar_trim frees the cached buffers of the context and its pair workers; the next call
    allocates again and gives the same records."""
    qs, rs = mixed_pairs
    ref = _run(ctx, monkeypatch, qs, rs, SONAR_PAIR_STREAMS=2)
    ctx.trim()
    got = _run(ctx, monkeypatch, qs, rs, SONAR_PAIR_STREAMS=2)
    for f in sonar.PAIR_FIELDS:
        assert _same(got[f], ref[f]), f


@pytest.fixture(scope="module")
def device_pairs():
    """Device-resident pairs of 5-12 s (chroma frames of 256 samples: the batched feature launches
    take the whole batch), plus the same with one 3.3 s pair (257-sample frames: per-pair path)."""
    rng = np.random.default_rng(12)
    qs, rs = [], []
    for k, (sq, sr_) in enumerate([(6.0, 7.5), (9.0, 5.0), (12.0, 10.7), (5.5, 8.9), (7.0, 7.0), (3.3, 3.3)]):
        q, r = synth.c3_pair(max(sq, sr_), 0.4 + 0.3 * k)[:2]
        qs.append(torch.from_numpy(np.ascontiguousarray(q[: int(sq * 44100)])).cuda())
        rs.append(torch.from_numpy(np.ascontiguousarray(r[: int(sr_ * 44100)] +
                                                        1e-3 * rng.standard_normal(int(sr_ * 44100)))).cuda())
    torch.cuda.synchronize()
    return qs, rs


def _run_dev(ctx, monkeypatch, qs, rs, **env):
    env.setdefault("SONAR_PAIR_RETRY", 0)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    try:
        ctx.dtw_counters(reset=True)
        out = ctx.align_pairs([q.data_ptr() for q in qs], [r.data_ptr() for r in rs],
                              nq=[q.numel() for q in qs], nr=[r.numel() for r in rs], max_lag_seconds=4.0,
                              workers=8, device_ptrs=True)
        assert ctx.dtw_counters(reset=True)["dtw_timeouts"] == 0
        assert np.all(out["flags"] == 0)
        return out
    finally:
        for k in env:
            monkeypatch.delenv(k)


@pytest.mark.parametrize("with_short", [False, True])
@pytest.mark.parametrize("streams", [1, 2])
def test_batched_features_equal_per_pair(ctx, monkeypatch, device_pairs, streams, with_short):
    """Device-resident pairs: the batch's music features and NCCs in batched launches (default)
    against the per-pair launches inside a batch (SONAR_FEAT_BATCH=0) and the unbatched path
    (SONAR_PAIR_BATCH=0): identical records.  with_short adds a pair whose chroma frames are 257
    samples, so its batch falls back to the per-pair launches."""
    qs, rs = device_pairs
    if not with_short:
        qs, rs = qs[:-1], rs[:-1]
    ref = _run_dev(ctx, monkeypatch, qs, rs, SONAR_PAIR_BATCH=0)
    per = _run_dev(ctx, monkeypatch, qs, rs, SONAR_PAIR_STREAMS=streams, SONAR_FEAT_BATCH=0)
    got = _run_dev(ctx, monkeypatch, qs, rs, SONAR_PAIR_STREAMS=streams)
    assert np.all(ref["status"] == 0) and np.all(got["status"] == 0) and np.all(per["status"] == 0)
    for f in sonar.PAIR_FIELDS:
        assert _same(got[f], ref[f]), f
        assert _same(per[f], ref[f]), f


@pytest.mark.parametrize("streams", [1, 3])
def test_device_scorer_equals_host_scorer(ctx, monkeypatch, device_pairs, streams):
    """The batch's scorer reductions on the device (pair_score_kernel: path sums, correlation
    peak / noise / sidelobes in Go's order) against the same batch scored on the host from the
    copied-back paths and correlations (SONAR_PAIR_HOST_SCORES=1): identical records, bit for bit."""
    qs, rs = device_pairs
    qs, rs = qs[:-1], rs[:-1]
    host = _run_dev(ctx, monkeypatch, qs, rs, SONAR_PAIR_STREAMS=streams, SONAR_PAIR_HOST_SCORES=1)
    dev = _run_dev(ctx, monkeypatch, qs, rs, SONAR_PAIR_STREAMS=streams)
    assert np.all(host["status"] == 0) and np.all(dev["status"] == 0)
    for f in sonar.PAIR_FIELDS:
        assert _same(dev[f], host[f]), f


def test_device_scorer_edge_pairs(ctx, monkeypatch):
    """Device vs host scorer on pairs whose paths and correlations are degenerate: identical
    streams (a pure diagonal, a correlation peak at lag 0), a silent query (an all-zero energy
    correlation: no peak beyond index 0, zero sidelobes), a constant tone against itself shifted,
    and the shortest streams the batch takes (paths of a few points)."""
    rng = np.random.default_rng(21)
    base, _ = synth.c3_pair(6.0, 0.7)[:2]
    tone = (0.3 * np.sin(2 * np.pi * 440.0 * np.arange(int(5.0 * 44100)) / 44100.0)).astype(np.float64)
    short = 0.2 * rng.standard_normal(1024 + 256 * 9)
    qs = [base[: 5 * 44100], np.zeros(5 * 44100), tone, short, base[: 6 * 44100]]
    rs = [base[: 5 * 44100].copy(), base[: 5 * 44100], np.roll(tone, 1234), short[::-1].copy(),
          base[44100: 6 * 44100] + 1e-3 * rng.standard_normal(5 * 44100)]
    qd = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda() for x in qs]
    rd = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda() for x in rs]
    torch.cuda.synchronize()

    def run(**env):
        env.setdefault("SONAR_PAIR_RETRY", 0)
        for k, v in env.items():
            monkeypatch.setenv(k, str(v))
        try:
            return ctx.align_pairs([q.data_ptr() for q in qd], [r.data_ptr() for r in rd],
                                   nq=[q.numel() for q in qd], nr=[r.numel() for r in rd],
                                   max_lag_seconds=2.0, workers=8, device_ptrs=True)
        finally:
            for k in env:
                monkeypatch.delenv(k)

    host = run(SONAR_PAIR_HOST_SCORES=1, SONAR_PAIR_STREAMS=1)
    dev = run(SONAR_PAIR_STREAMS=1)
    assert np.array_equal(host["status"], dev["status"])
    for f in sonar.PAIR_FIELDS:
        assert _same(dev[f], host[f]), f


# -- the smallest shapes at which the batch's layout, ticket map and decode can go wrong -------------
# Pairs of F chroma frames: 1024 + 256 (F - 1) samples of noise.  10 x 10 and 64 x 65 are one 64-row
# band (no edge buffer), 65 x 64 is the first two-band case.  Every case runs batched on 1 and 2
# streams against the unbatched path, with host and with device pointers, SONAR_PAIR_RETRY=0 and a
# check that no band pipeline timed out.
EDGE_FRAMES = [(10, 10), (64, 65), (65, 64)]
EDGE_BANDS = [1, 1, 2]


@pytest.fixture(scope="module")
def edge_pairs():
    rng = np.random.default_rng(31)
    host = [[0.2 * rng.standard_normal(1024 + 256 * (f - 1)) for f in fr] for fr in EDGE_FRAMES]
    dev = [[torch.from_numpy(x).cuda() for x in pr] for pr in host]
    torch.cuda.synchronize()
    return host, dev


def _edge_args(edge_pairs, dev, which):
    host, devp = edge_pairs
    nq, nr = [len(host[k][0]) for k in which], [len(host[k][1]) for k in which]
    if dev:
        return [devp[k][0].data_ptr() for k in which], [devp[k][1].data_ptr() for k in which], nq, nr
    return [host[k][0] for k in which], [host[k][1] for k in which], nq, nr


def _run_edge(ctx, monkeypatch, edge_pairs, dev, which=(0, 1, 2), feature_window=1024, **env):
    env.setdefault("SONAR_PAIR_RETRY", 0)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    try:
        qs, rs, nq, nr = _edge_args(edge_pairs, dev, which)
        ctx.dtw_counters(reset=True)
        out = ctx.align_pairs(qs, rs, nq=nq, nr=nr, feature_window=feature_window, max_lag_seconds=4.0, workers=4,
                              device_ptrs=dev)
        assert ctx.dtw_counters(reset=True)["dtw_timeouts"] == 0
        assert np.all(out["status"] == 0) and np.all(out["flags"] == 0)
        return out
    finally:
        for k in env:
            monkeypatch.delenv(k)


def _assert_records_equal(got, ref):
    for f in sonar.PAIR_FIELDS + ["status", "flags"]:
        assert _same(got[f], ref[f]), f


edge_cases = pytest.mark.parametrize("dev,streams", [(False, 1), (False, 2), (True, 1), (True, 2)])


@edge_cases
def test_band_and_batch_edges(ctx, monkeypatch, edge_pairs, dev, streams):
    """One band without an edge buffer and the first two-band pairs, as one batch per stream and (a
    tiny budget) as batches of one: records identical to the unbatched path."""
    ref = _run_edge(ctx, monkeypatch, edge_pairs, dev, SONAR_PAIR_BATCH=0)
    _assert_records_equal(_run_edge(ctx, monkeypatch, edge_pairs, dev, SONAR_PAIR_STREAMS=streams), ref)
    _assert_records_equal(_run_edge(ctx, monkeypatch, edge_pairs, dev, SONAR_PAIR_STREAMS=streams,
                                    SONAR_PAIR_BATCH_GB=0.001), ref)


@edge_cases
def test_no_correlation_candidate(ctx, monkeypatch, edge_pairs, dev, streams):
    """feature_window 4096 on the 10-frame pair (3,328 samples): no energy frames, so the chroma DTW
    is the only candidate.  Batched equals unbatched."""
    assert sonar.energy_frames(1024 + 256 * 9, 4096, 256) <= 0
    ref = _run_edge(ctx, monkeypatch, edge_pairs, dev, which=(0,), feature_window=4096, SONAR_PAIR_BATCH=0)
    got = _run_edge(ctx, monkeypatch, edge_pairs, dev, which=(0,), feature_window=4096, SONAR_PAIR_STREAMS=streams)
    _assert_records_equal(got, ref)
    assert np.isfinite(got["dtw_distance"][0])


def _align_pairs_c(ctx, qs, rs, nq, nr, dev):
    """sonar_align_pairs through the C entry: (return code, error text, records); the binding would
    raise on the code and drop the records."""
    from sonar import _abi
    n = len(qs)
    qp, rp, keep = _abi._pair_arrays(qs, rs)
    recs = (_abi.PairRecord * n)()
    L = _abi.lib()
    rc = L.sonar_align_pairs(ctx._h, n, qp, (_abi.C.c_int64 * n)(*nq), rp, (_abi.C.c_int64 * n)(*nr), 44100, 1024, 256,
                             1024, 4.0, 4, int(dev), recs)
    del keep
    return rc, L.sonar_last_error(ctx._h).decode(), _abi.records_dict(recs[:n])


@edge_cases
def test_bad_pair_among_good_ones(ctx, monkeypatch, edge_pairs, dev, streams):
    """Three pairs whose middle one has 100 samples: the call answers SONAR_ERR_TOO_SHORT with the
    text of pair 1, records 0 and 2 are those of a call with only these two pairs, and record 1 is
    what its path leaves: zeroed fields on the batched path (sized before any launch), NaN fields on
    the unbatched one (the single-pair entry's answer), the status on both."""
    qs, rs, nq, nr = _edge_args(edge_pairs, dev, (1, 1, 2))
    nq[1] = nr[1] = 100
    if not dev:
        qs[1], rs[1] = qs[1][:100].copy(), rs[1][:100].copy()
    for env, bad_field in (({"SONAR_PAIR_BATCH": 0}, np.nan), ({"SONAR_PAIR_STREAMS": streams}, 0.0)):
        env["SONAR_PAIR_RETRY"] = 0
        for k, v in env.items():
            monkeypatch.setenv(k, str(v))
        try:
            ctx.dtw_counters(reset=True)
            rc, text, got = _align_pairs_c(ctx, qs, rs, nq, nr, dev)
            rc2, _, two = _align_pairs_c(ctx, [qs[0], qs[2]], [rs[0], rs[2]], [nq[0], nq[2]], [nr[0], nr[2]], dev)
            assert ctx.dtw_counters(reset=True)["dtw_timeouts"] == 0
        finally:
            for k in env:
                monkeypatch.delenv(k)
        assert rc == sonar.ERR_TOO_SHORT and rc2 == 0
        assert text == "pair 1: signal too short for given window size and hop size", text
        assert got["status"].tolist() == [0, sonar.ERR_TOO_SHORT, 0] and got["flags"].tolist() == [0, 0, 0]
        for f in sonar.PAIR_FIELDS:
            assert _same(got[f][[0, 2]], two[f]), f
            assert _same(got[f][1], bad_field), (f, got[f][1])


@edge_cases
def test_small_dump_and_trace_files(ctx, monkeypatch, edge_pairs, dev, streams, tmp_path):
    """SONAR_PAIR_DUMP on the 64 x 65 pair: path, path costs and C[nq][nr] / P equal the oracle's
    serial DTW of the same chroma bit for bit.  SONAR_DTW_TRACE: exactly one 80-byte record per band
    of the batch, their (pair, band) headers the complete set.  Records equal the unbatched path's."""
    import oracle as O
    trace = tmp_path / "trace.bin"
    ref = _run_edge(ctx, monkeypatch, edge_pairs, dev, SONAR_PAIR_BATCH=0)
    got = _run_edge(ctx, monkeypatch, edge_pairs, dev, SONAR_PAIR_STREAMS=streams, SONAR_PAIR_DUMP=tmp_path,
                    SONAR_DTW_TRACE=trace)
    _assert_records_equal(got, ref)
    raw = np.fromfile(trace, dtype=np.uint64)
    assert raw.size * 8 == 80 * sum(EDGE_BANDS)
    heads = sorted((int(p), int(b)) for p, b in raw.reshape(-1, 10)[:, :2])
    assert heads == [(k, b) for k, nb in enumerate(EDGE_BANDS) for b in range(nb)]
    q, r = edge_pairs[0][1]
    cq, cr = ctx.music_alignment_features(q, 44100)[1], ctx.music_alignment_features(r, 44100)[1]
    assert cq.shape == (64, 12) and cr.shape == (65, 12)
    od = O.dtw(cq, cr)
    b = (tmp_path / "pair_1.bin").read_bytes()
    P, cnm = int(np.frombuffer(b[:8], np.int64)[0]), float(np.frombuffer(b[8:16], np.float64)[0])
    assert P == len(od["path_q"]) and len(b) == 16 + 16 * P
    assert np.array_equal(np.frombuffer(b[16:16 + 8 * P], np.float64), od["path_cost"])
    assert np.array_equal(np.frombuffer(b[16 + 8 * P:16 + 12 * P], np.int32), od["path_q"])
    assert np.array_equal(np.frombuffer(b[16 + 12 * P:], np.int32), od["path_r"])
    assert cnm / P == od["distance"]
