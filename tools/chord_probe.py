"""Timing probe of sonar_chord_frames / sonar_chord_sequence (diagnostics, not part of the product or the
tests, and no threshold: it reports).

One process; a device-resident F x 12 float64 chromagram for F = 51,676 (10 minutes at 44.1 kHz, hop 512)
and F = 620,153 (two hours), the sizes of tools/key_probe.py: 0.35 * U(0, 1)^2 per bin under
normalize_templates = 0 (first confidences below 1, about 60 candidates a row), NewChordDetector's other
parameters, no bass arrays, every array a device address.  Per case, after WARMUP calls (default 3), ITERS
calls (default 9): the kernel time of the call's launch sequence from the library's HIP-event timers
(sonar_enable_kernel_timing / sonar_last_kernel_ms) and the host wall time of the call including its
final stream synchronisation, each as median, minimum and maximum; then the bytes the call must move
(96 in per frame plus the outputs asked for) and their fraction of the 8 TB/s HBM rate DESIGN.md section
5 uses.

  frames_all        sonar_chord_frames, every output (template_scores is 960 of the 1,116 bytes a frame)
  frames_scalars    sonar_chord_frames, the thirteen per-frame values only
  frames_root       sonar_chord_frames, root only (the per-row kernel with next to no stores)
  sequence_all      sonar_chord_sequence, every output
  sequence_scalars  sonar_chord_sequence, the thirteen per-frame values only
  sequence_root     sonar_chord_sequence, root only: the record pass, the chain and the output pass

The chain is one lane walking F records.  Its time per frame is estimated by difference: the record pass
costs about what frames_root does (the same scores, three scans in place of the ranking), so
chain = (sequence_root - 2 * frames_root) / F.

Usage (GPU box): python3 tools/chord_probe.py [--out profiles/chord_probe.json]
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

HBM_RATE = 8e12
INTS = ("root", "quality", "inversion", "n_found", "extensions", "role", "candidates", "cand_inversion")
SCALARS = sonar.CHORD_FIELDS[:13]
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chord_probe.json"))
args = ap.parse_args()
iters = int(os.environ.get("ITERS", "9"))
warmup = int(os.environ.get("WARMUP", "3"))

ctx = sonar.Context(0)
ctx.enable_kernel_timing(True)
params = sonar.chord_params(normalize_templates=0)


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


def with_bytes(r, F, out_bytes_per_frame):
    r["algorithmic_bytes"] = float(F) * (96 + out_bytes_per_frame)
    r["hbm_fraction"] = r["algorithmic_bytes"] / (r["kernel_ms"]["median"] * 1e-3) / HBM_RATE
    return r


def probe(F):
    x = torch.from_numpy(0.35 * np.random.default_rng(2).random((F, 12)) ** 2).cuda()
    out = {}
    for n in sonar.CHORD_FIELDS:
        shape = (F, 120) if n == "template_scores" else (F, 5) if n.startswith("cand") else (F,)
        out[n] = torch.zeros(shape, dtype=torch.int32 if n in INTS else torch.float64, device="cuda")
    torch.cuda.synchronize()

    def call(sequence, names):
        return lambda: ctx.chord_rows_device(x.data_ptr(), F, 12, params, sequence=sequence,
                                             **{n: out[n].data_ptr() for n in names})

    scalar_bytes = 6 * 4 + 7 * 8
    all_bytes = scalar_bytes + 960 + 5 * (4 + 4 + 8 + 8)
    r = {"frames": F}
    for seq, tag in ((False, "frames"), (True, "sequence")):
        r[tag + "_all"] = with_bytes(timed(call(seq, sonar.CHORD_FIELDS)), F, all_bytes)
        r[tag + "_scalars"] = with_bytes(timed(call(seq, SCALARS)), F, scalar_bytes)
        r[tag + "_root"] = with_bytes(timed(call(seq, ("root",))), F, 4)
    r["mean_candidates"] = float(out["n_found"].double().mean().cpu())
    r["chain_ns_per_frame_estimate"] = (r["sequence_root"]["kernel_ms"]["median"]
                                        - 2 * r["frames_root"]["kernel_ms"]["median"]) * 1e6 / F
    return r


result = {"probe": "sonar_chord_frames / sonar_chord_sequence, NewChordDetector's parameters with normalize_templates "
                   "= 0, a device-resident F x 12 float64 chromagram, device pointers",
          "device": torch.cuda.get_device_name(0), "hbm_rate_tb_s": HBM_RATE / 1e12, "iters": iters, "warmup": warmup,
          "cases": [probe(51676), probe(620153)]}
ctx.close()
with open(args.out, "w") as f:
    f.write(json.dumps(result) + "\n")
print(json.dumps(result))
