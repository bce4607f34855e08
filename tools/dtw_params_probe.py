"""Timing probe of sonar_dtw_params' kernel instances (diagnostics, not part of the product or the
tests, and no threshold: it reports).

One 12-dim shape (DTW_N rows each side, default 8192, no band, no cost matrix): every metric with
symmetric2, and Euclidean with every step pattern, through Context.dtw_params; the band sweep's
HIP-event time from sonar_dtw_last_timing (median of ITERS calls after one warm-up), as a ratio to
Euclidean / symmetric2 -- the existing FAST instance -- from the same run.

Usage (GPU box): python3 tools/dtw_params_probe.py [> profiles/<name>.txt]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sonido-sonar_amd"))
import sonar  # noqa: E402

n = int(os.environ.get("DTW_N", "8192"))
iters = int(os.environ.get("ITERS", "5"))
rng = np.random.default_rng(7)
q = rng.random((n, 12))
r = np.roll(q, 37, axis=0) + 0.01 * rng.random((n, 12))
ctx = sonar.Context(0)
cases = [("euclidean", "symmetric2"), ("manhattan", "symmetric2"), ("cosine", "symmetric2"),
         ("pearson", "symmetric2"), ("euclidean", "asymmetric"), ("euclidean", "symmetric1")]
rows = []
for metric, step in cases:
    ctx.dtw_params(q, r, step=step, metric=metric)           # warm-up (buffers, code load)
    ms = []
    for _ in range(iters):
        res = ctx.dtw_params(q, r, step=step, metric=metric)
        ms.append(ctx.dtw_last_timing())
    band, walk, decode = np.median(np.array(ms), axis=0)
    rows.append((metric, step, band, walk, decode, len(res["path_q"])))
base = rows[0][2]
print(f"sonar_dtw_params, {n} x {n} x 12, no band, no cost matrix, median of {iters}: kernel ms from "
      "sonar_dtw_last_timing", flush=True)
print(f"{'metric':<10} {'step':<11} {'band ms':>9} {'ratio':>6} {'walk ms':>8} {'decode ms':>9} {'path':>6}")
for metric, step, band, walk, decode, P in rows:
    print(f"{metric:<10} {step:<11} {band:9.3f} {band / base:6.2f} {walk:8.3f} {decode:9.3f} {P:6d}", flush=True)
t = ctx.dtw_counters()
print(f"band-pipeline timeouts: {t['dtw_timeouts']}", flush=True)
ctx.close()
