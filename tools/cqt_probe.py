"""Timing probe of sonar_chroma_cqt (diagnostics, not part of the product or the tests, and no
threshold: it reports).

One process, NewChromaCQTDefault(44100) on 5 minutes and on 1 hour of 44.1 kHz float64 PCM resident on
the device (0.5 + 0.1 N(0, 1), generated there), at hop 512 and at hop 4096 (the chord detector's),
device pointers, the CQT magnitudes to library scratch.  Per case, after WARMUP calls (default 2; the
first builds and uploads the tap table), ITERS calls (default 7): the kernel time from the library's
HIP-event timers (sonar_enable_kernel_timing / sonar_last_kernel_ms: the filter-bank kernel and the
fold, not the non-finite scan before them) and the host wall time of the whole call, each as median,
minimum and maximum.  flop = 2 F sum(L_k), the useful multiply-adds (the kernel's zero padding of a
bin group to its longest member is not counted); fp64_valu_fraction = flop / kernel time / 78.6 TF,
the FP64 VALU peak DESIGN.md uses.

Beside it the Python checker's wall time (tests/chroma_cqt_ref.py: numpy FFTs on the host, not the Go
reference) for the 77-frame case of the tests (40,000 samples, hop 512), the only CPU figure at hand,
and the library's wall time for the same call with host pointers.

Usage (GPU box): python3 tools/cqt_probe.py > profiles/chroma_cqt_probe.json
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
import chroma_cqt_ref as R  # noqa: E402

SR = 44100
FP64_VALU_PEAK = 78.6e12
iters = int(os.environ.get("ITERS", "7"))
warmup = int(os.environ.get("WARMUP", "2"))

ctx = sonar.Context(0)
ctx.enable_kernel_timing(True)
plan = sonar.chroma_cqt_plan(SR)
gen = torch.Generator(device="cuda")
gen.manual_seed(5)


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def case(seconds, hop):
    n = seconds * SR
    x = 0.5 + 0.1 * torch.randn(n, dtype=torch.float64, device="cuda", generator=gen)
    F = sonar.chroma_cqt_plan(SR, n=n, hop=hop)["n_frames"]
    chroma = torch.zeros(F, 12, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    kernel, wall = [], []
    for it in range(warmup + iters):
        t0 = time.perf_counter()
        ctx.chroma_cqt_device(x.data_ptr(), n, hop, SR, chroma.data_ptr())
        w = (time.perf_counter() - t0) * 1e3
        k = ctx.last_kernel_ms()
        if it >= warmup:
            kernel.append(k)
            wall.append(w)
    flop = 2.0 * F * plan["sum_taps"]
    row_sums = chroma.sum(dim=1)
    out = {"seconds": seconds, "hop": hop, "samples": n, "frames": F, "flop": flop, "kernel_ms": stats(kernel),
           "wall_ms": stats(wall), "tflops": flop / (np.median(kernel) * 1e-3) / 1e12,
           "fp64_valu_fraction": flop / (np.median(kernel) * 1e-3) / FP64_VALU_PEAK,
           "chroma_row_sum_min_max": [float(row_sums.min()), float(row_sums.max())]}
    del x, chroma
    torch.cuda.empty_cache()
    return out


cases = [case(sec, hop) for sec in (300, 3600) for hop in (512, 4096)]

x = 0.5 + 0.1 * np.random.default_rng(40000).standard_normal(40000)
t0 = time.perf_counter()
ref = R.chroma_cqt(x, 512, SR)
checker_s = time.perf_counter() - t0
ctx.chroma_cqt(x, 512, SR)
host = []
for _ in range(iters):
    t0 = time.perf_counter()
    got = ctx.chroma_cqt(x, 512, SR)
    host.append((time.perf_counter() - t0) * 1e3)
print(json.dumps({
    "probe": "sonar_chroma_cqt, NewChromaCQTDefault(44100), device-resident float64 PCM",
    "device": torch.cuda.get_device_name(0), "total_bins": plan["total_bins"], "fft_size": plan["fft_size"],
    "sum_taps": plan["sum_taps"], "fp64_valu_peak_tflops": FP64_VALU_PEAK / 1e12, "iters": iters, "warmup": warmup,
    "cases": cases,
    "case_77_frames": {"samples": 40000, "hop": 512, "frames": int(ref["cqt"].shape[0]),
                       "numpy_checker_wall_s": checker_s,
                       "note": "the checker is numpy on the host (FFT-domain sums), not the Go reference",
                       "library_wall_ms_host_pointers": stats(host),
                       "max_abs_chroma_difference": float(np.max(np.abs(got - ref["chroma"])))}}))
ctx.close()
