"""Timing probe of sonar_chroma_frame_matrix / sonar_chroma_similarity (diagnostics, not part of the
product or the tests, and no threshold: it reports).

One process, float64 chroma resident on the device (uniform [0.05, 1), 12 bins), two shapes:
10,332 x 10,332 frames (two 60 s chromagrams, the C5 shape) and 2,584 x 2,584.  Per case, after WARMUP
calls (default 2), ITERS calls (default 7); every figure is the median with minimum and maximum of the
library's HIP-event time of one kernel family (sonar_chroma_similarity_last_timing: frame matrix with
the row preparation | ordered sums | DP fill | traceback):

  frame matrix, stored   per metric, against the write floor 8 B / cell at 6.29 TB/s (the HBM rate this
                         project measured)
  frame matrix, fused    Direct with no matrix, per metric, against the FP64 VALU peak with the counted
                         float64 operations per cell (OPS below: add, mul, div, sqrt, abs, exp and log
                         one each; the per-row preparation is not counted)
  SW and DTW fill        cells / s of the tiled wavefront (Cosine; the DP matrix in library scratch), and
                         beside it sonar_dtw_params(cost matrix wanted, Cosine, symmetric2) on the same
                         shape: a different recurrence with its own kernel, for scale, not a bar
  ordered sums           the 12 OTI totals (R = 10) and the 12 sampled means of findBestTransposition
  traceback              the Smith-Waterman and DTW walks, with their path lengths

Beside them the Python checker's wall time (tests/chroma_similarity_ref.py: numpy and Python loops on
the host, not the Go reference) for the (200, 129) case of the tests.

Usage (GPU box): python3 tools/chroma_similarity_probe.py > profiles/chroma_similarity_probe.json
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sonido-sonar_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sonar  # noqa: E402
import chroma_similarity_ref as R  # noqa: E402

HBM_BPS = 6.29e12
FP64_VALU_PEAK = 78.6e12
DIM = 12
# float64 operations per cell and similarity, dim 12
OPS = {"euclidean": 3 * DIM + 1 + 1, "manhattan": 3 * DIM + 1, "cosine": 2 * DIM + 3 + 2, "pearson": 2 * DIM + 5 + 2,
       "kl": 4 * DIM + 1, "js": 2 * DIM + 12 * DIM + 4 + 1, "hellinger": 3 * DIM + 2 + 1}
iters = int(os.environ.get("ITERS", "7"))
warmup = int(os.environ.get("WARMUP", "2"))

ctx = sonar.Context(0)
gen = torch.Generator(device="cuda")
gen.manual_seed(7)


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def timed(call, family):
    """median / min / max of one family's event time (a tuple of families: of each) over ITERS calls,
    and the last call's return."""
    fams = family if isinstance(family, tuple) else (family,)
    ms, out = [[] for _ in fams], None
    for it in range(warmup + iters):
        out = call()
        if it >= warmup:
            t = ctx.chroma_similarity_last_timing()
            for k, f in enumerate(fams):
                ms[k].append(t[f])
    st = tuple(stats(v) for v in ms)
    return (st if isinstance(family, tuple) else st[0]), out


def case(n):
    q = 0.05 + 0.95 * torch.rand(n, DIM, dtype=torch.float64, device="cuda", generator=gen)
    r = 0.05 + 0.95 * torch.rand(n, DIM, dtype=torch.float64, device="cuda", generator=gen)
    mat = torch.zeros(n, n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    cells = float(n) * n
    qp, rp = q.data_ptr(), r.data_ptr()
    out = {"frames": n, "cells": cells, "write_floor_ms": cells * 8 / HBM_BPS * 1e3, "stored": {}, "fused": {}}
    for metric in R.METRICS:
        ms, _ = timed(lambda: ctx.chroma_frame_matrix_device(qp, n, rp, n, DIM, mat.data_ptr(), metric, 0, True), 0)
        out["stored"][metric] = {"ms": ms, "write_floor_fraction": out["write_floor_ms"] / ms["median"]}
        ms, _ = timed(lambda: ctx.chroma_similarity_device(qp, n, rp, n, DIM, "direct", metric), 0)
        flop = OPS[metric] * cells
        out["fused"][metric] = {"ms": ms, "ops_per_cell": OPS[metric], "tflops": flop / (ms["median"] * 1e-3) / 1e12,
                                "fp64_valu_fraction": flop / (ms["median"] * 1e-3) / FP64_VALU_PEAK}
    del mat
    torch.cuda.empty_cache()
    for method in ("smith_waterman", "dtw"):
        call = lambda: ctx.chroma_similarity_device(qp, n, rp, n, DIM, method, "cosine")  # noqa: E731
        (fill, walk), res = timed(call, (2, 3))
        out[method] = {"fill_ms": fill, "cells_per_s": cells / (fill["median"] * 1e-3), "traceback_ms": walk,
                       "path_len": res["path_len"], "tile_launches": 2 * ((n + 63) // 64) - 1}
    # sonar_dtw_params with the cost matrix, for scale
    pq, pr = (torch.zeros(2 * n + 1, dtype=torch.int32, device="cuda") for _ in range(2))
    pc = torch.zeros(2 * n + 1, dtype=torch.float64, device="cuda")
    cost = torch.zeros(n, n + 1, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    band = []
    for it in range(warmup + iters):
        ctx.dtw_params_device(qp, n, rp, n, DIM, pq.data_ptr(), pr.data_ptr(), pc.data_ptr(), band=-1,
                              step="symmetric2", metric="cosine", cost_ptr=cost.data_ptr())
        if it >= warmup:
            band.append(ctx.dtw_last_timing()[0])
    out["dtw_params_want_cost"] = {"band_sweep_ms": stats(band), "cells_per_s": cells / (np.median(band) * 1e-3)}
    del cost
    torch.cuda.empty_cache()
    ms, res = timed(lambda: ctx.chroma_similarity_device(qp, n, rp, n, DIM, "oti", "cosine", oti_radius=10), 1)
    terms = sonar.chroma_similarity_plan("oti", n, n, DIM, 10)["oti_cells"]
    out["oti_ordered_sums"] = {"ms": ms, "terms_per_shift": terms, "radius": 10,
                               "terms_per_s_per_chain": terms / (ms["median"] * 1e-3)}
    ms, res = timed(lambda: ctx.chroma_similarity_device(qp, n, rp, n, DIM, "direct", "cosine",
                                                         transposition_invariant=True), 1)
    out["find_best_transposition_sums"] = {"ms": ms, "terms_per_shift": sonar.chroma_similarity_plan("direct", n, n)["sampled_pairs"]}
    del q, r
    ctx.trim()
    torch.cuda.empty_cache()
    return out


cases = [case(n) for n in (2584, 10332)]

rng = np.random.default_rng(3)
hq, hr = rng.random((200, DIM)), rng.random((129, DIM))
checker = {}
for method in ("direct", "smith_waterman", "dtw", "oti"):
    t0 = time.perf_counter()
    R.compute_similarity(hq, hr, method, "cosine")
    checker[method] = time.perf_counter() - t0
print(json.dumps({
    "probe": "sonar_chroma_similarity / sonar_chroma_frame_matrix, device-resident float64 chroma, dim 12",
    "device": torch.cuda.get_device_name(0), "hbm_bytes_per_s": HBM_BPS, "fp64_valu_peak_tflops": FP64_VALU_PEAK / 1e12,
    "iters": iters, "warmup": warmup, "cases": cases,
    "python_checker_200x129_wall_s": checker,
    "note": "the checker is numpy and Python loops on the host, not the Go reference"}))
ctx.close()
