"""Timing probe of sonar_key_frames / sonar_key_sequence / sonar_key_batch (diagnostics, not part of the
product or the tests, and no threshold: it reports).

One process; a device-resident F x 12 float64 chromagram for F = 51,676 (10 minutes at 44.1 kHz, hop 512)
and F = 620,153 (two hours): a Krumhansl key template that changes every 40 frames, divided by its
maximum, plus 0.35 |N(0, 1)|, NewKeyEstimator's parameters, every array a device address.  Per case,
after WARMUP calls (default 3; the first builds the tables), ITERS calls (default 9): the kernel time of
the call's launch sequence from the library's HIP-event timers (sonar_enable_kernel_timing /
sonar_last_kernel_ms) and the host wall time of the call including its final stream synchronisation, each
as median, minimum and maximum; then the bytes the call must move (8 dim in per frame plus the outputs
asked for) and their fraction of the 8 TB/s HBM rate DESIGN.md section 5 uses.

  frames_all      sonar_key_frames, every output
  frames_scalars  sonar_key_frames, the eight per-frame values only
  frames_code     sonar_key_frames, key only (the cost of the per-frame kernel with next to no stores)
  sequence        sonar_key_sequence, every output
  sequence_avg    sonar_key_sequence, the average row's result only: the column sums, one row, and the
                  per-frame pass that looks for non-finite values
  batch           sonar_key_batch, every output
  batch_global    sonar_key_batch, the global key only: the per-frame kernel and the vote chain

The ordered sums are one block each, about F dependent float64 additions per chain.  Their time per
frame is estimated by difference: (sequence_avg - frames_code) / F for the column sums, (batch_global -
frames_code) / F for the votes.

Usage (GPU box): python3 tools/key_probe.py [--out profiles/key_probe.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sonido-sonar_amd"))
import sonar  # noqa: E402

KRUMHANSL = ([6.35, 2.23, 3.48, 2.33, 4.38, 4.09, 2.52, 5.19, 2.39, 3.66, 2.29, 2.88],
             [6.33, 2.68, 3.52, 5.38, 2.60, 3.53, 2.54, 4.75, 3.98, 2.69, 3.34, 3.17])
HBM_RATE = 8e12
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "key_probe.json"))
args = ap.parse_args()
iters = int(os.environ.get("ITERS", "9"))
warmup = int(os.environ.get("WARMUP", "3"))

ctx = sonar.Context(0)
ctx.enable_kernel_timing(True)


def tonal(F, seed=1):
    rng = np.random.default_rng(seed)
    rows = np.zeros((F, 12))
    for b in range(0, F, 40):
        code = int(rng.integers(0, 24))
        prof = np.array(KRUMHANSL[code & 1])
        rows[b:b + 40] = np.roll(prof, -(code >> 1)) / prof.max()
    return rows + 0.35 * np.abs(rng.standard_normal((F, 12)))


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def timed(fn):
    kernel, wall = [], []
    for it in range(warmup + iters):
        ctx.synchronize()
        ctx.last_kernel_ms()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        w = (time.perf_counter() - t0) * 1e3
        k = ctx.last_kernel_ms()
        if it >= warmup:
            kernel.append(k)
            wall.append(w)
    return {"kernel_ms": stats(kernel), "wall_ms": stats(wall)}


def with_bytes(r, F, out_bytes):
    r["algorithmic_bytes"] = float(F) * 96 + float(out_bytes)
    r["hbm_fraction"] = r["algorithmic_bytes"] / (r["kernel_ms"]["median"] * 1e-3) / HBM_RATE
    return r


def probe(F):
    i32, f64 = torch.int32, torch.float64
    x = torch.from_numpy(tonal(F)).cuda()
    fr = {n: torch.zeros(F, dtype=i32 if n in ("key", "mode", "known") else f64, device="cuda")
          for n in sonar.KEY_FRAME_FIELDS[:8]}
    fr.update(scores=torch.zeros(F, 24, dtype=f64, device="cuda"), candidates=torch.zeros(F, 5, dtype=i32, device="cuda"),
              processed=torch.zeros(F, 12, dtype=f64, device="cuda"))
    one = {n: torch.zeros(1, dtype=i32 if n in ("key", "mode", "known") else f64, device="cuda")
           for n in sonar.KEY_FRAME_FIELDS[:8]}
    one.update(scores=torch.zeros(24, dtype=f64, device="cuda"), processed=torch.zeros(12, dtype=f64, device="cuda"))
    seq = dict(one, stability=torch.zeros(1, dtype=f64, device="cuda"),
               modulations=torch.zeros(F - 20, dtype=i32, device="cuda"),
               n_modulations=torch.zeros(1, dtype=torch.int64, device="cuda"))
    glob = dict(global_code=torch.zeros(1, dtype=i32, device="cuda"), global_confidence=torch.zeros(1, dtype=f64, device="cuda"),
                global_strength=torch.zeros(1, dtype=f64, device="cuda"), votes=torch.zeros(24, dtype=f64, device="cuda"))
    trans = {n: torch.zeros(F - 1, dtype=f64 if n == "t_confidence" else i32, device="cuda")
             for n in ("t_frame", "t_from", "t_to", "t_confidence", "t_type")}
    trans["n_transitions"] = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def ptrs(d):
        return {n: t.data_ptr() for n, t in d.items()}

    xp = x.data_ptr()
    scalars = {n: fr[n] for n in sonar.KEY_FRAME_FIELDS[:8]}
    r = {"frames": F}
    r["frames_all"] = with_bytes(timed(lambda: ctx.key_frames_device(xp, F, 12, **ptrs(fr))), F, F * (52 + 192 + 20 + 96))
    r["frames_scalars"] = with_bytes(timed(lambda: ctx.key_frames_device(xp, F, 12, **ptrs(scalars))), F, F * 52)
    r["frames_code"] = with_bytes(timed(lambda: ctx.key_frames_device(xp, F, 12, key=fr["key"].data_ptr())), F, F * 4)
    r["sequence"] = timed(lambda: ctx.key_sequence_device(xp, F, 12, **ptrs(seq)))
    nm = int(seq["n_modulations"].cpu()[0])
    with_bytes(r["sequence"], F, 52 + 192 + 96 + 8 + 8 + 4 * nm)
    r["sequence"]["modulations"] = nm
    r["sequence"]["stability"] = float(seq["stability"].cpu()[0])
    r["sequence_avg"] = with_bytes(timed(lambda: ctx.key_sequence_device(xp, F, 12, **ptrs(one))), F, 52 + 192 + 96)
    r["batch"] = timed(lambda: ctx.key_batch_device(xp, F, 12, **ptrs(fr), **ptrs(glob), **ptrs(trans)))
    nt = int(trans["n_transitions"].cpu()[0])
    with_bytes(r["batch"], F, F * (52 + 192 + 20 + 96) + 4 + 8 + 8 + 192 + 8 + 24 * nt)
    r["batch"]["transitions"] = nt
    r["batch"]["global_key"] = sonar.key_name(int(glob["global_code"].cpu()[0]))
    r["batch_global"] = with_bytes(timed(lambda: ctx.key_batch_device(xp, F, 12, **ptrs(glob))), F, 4 + 8 + 8 + 192)
    base = r["frames_code"]["kernel_ms"]["median"]
    r["colsum_ns_per_frame_estimate"] = (r["sequence_avg"]["kernel_ms"]["median"] - base) * 1e6 / F
    r["votes_ns_per_frame_estimate"] = (r["batch_global"]["kernel_ms"]["median"] - base) * 1e6 / F
    return r


result = {"probe": "sonar_key_frames / sonar_key_sequence / sonar_key_batch, NewKeyEstimator's parameters, a "
                   "device-resident F x 12 float64 chromagram, device pointers",
          "device": torch.cuda.get_device_name(0), "hbm_rate_tb_s": HBM_RATE / 1e12, "iters": iters, "warmup": warmup,
          "cases": [probe(51676), probe(620153)]}
ctx.close()
with open(args.out, "w") as f:
    f.write(json.dumps(result) + "\n")
print(json.dumps(result))
