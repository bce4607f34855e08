"""Timing probe of sonar_spectral_peaks / sonar_hpcp_from_spectrum / sonar_hpcp (diagnostics, not part
of the product or the tests, and no threshold: it reports).

One process, 10 minutes of 44.1 kHz float64 PCM resident on the device (four partials + noise,
generated there), W = 2048, H = 512, Hann: F = 51,676 frames of K = 1025 bins, NewHPCP's parameters.
Per case, after WARMUP calls (default 3; the first builds tables), ITERS calls (default 9): the
kernel time from the library's HIP-event timers (sonar_enable_kernel_timing / sonar_last_kernel_ms,
the mean over the call's timed launches, times their number: 1 for a, b and the peaks, 2 per chunk
for c) and the host wall time of the call including its final
stream synchronisation, each as median, minimum and maximum.

  a  sonar_fingerprint, SONAR_FP_MAGNITUDE only, float64, into a device buffer (the baseline)
  b  sonar_hpcp_from_spectrum on those rows, device pointers; algorithmic bytes F K 8 and the
     fraction of the 8 TB/s HBM rate DESIGN.md section 5 uses
  c  sonar_hpcp whole (chunked transform + profile); expected about a + b
  peaks_d1 / peaks_d5  sonar_spectral_peaks alone on the same rows (1e-5, 20 Hz, 60) at sample rate
     44,100 (min_distance_bins 1: no greedy) and 8,000 (5 bins: the serial greedy)

Usage (GPU box): python3 tools/hpcp_probe.py > profiles/hpcp_probe.json
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sonido-sonar_amd"))
import sonar  # noqa: E402

SR, W, H = 44100, 2048, 512
HBM_RATE = 8e12
iters = int(os.environ.get("ITERS", "9"))
warmup = int(os.environ.get("WARMUP", "3"))

ctx = sonar.Context(0)
ctx.enable_kernel_timing(True)
n = 600 * SR
plan = sonar.hpcp_plan(n, W, H)
F, K = plan["frames"], W // 2 + 1
gen = torch.Generator(device="cuda")
gen.manual_seed(11)
t = torch.arange(n, dtype=torch.float64, device="cuda") / SR
x = sum(a * torch.sin(2 * np.pi * f * t) for a, f in [(0.5, 220.0), (0.3, 554.37), (0.2, 1318.5), (0.1, 3520.0)])
x = x + 0.01 * torch.randn(n, dtype=torch.float64, device="cuda", generator=gen)
del t
mag = torch.zeros(F, K, dtype=torch.float64, device="cuda")
hp, hp2 = (torch.zeros(F, 12, dtype=torch.float64, device="cuda") for _ in range(2))
count = torch.zeros(F, dtype=torch.int32, device="cuda")
bins = torch.zeros(F, 60, dtype=torch.int32, device="cuda")
pm, pf = (torch.zeros(F, 60, dtype=torch.float64, device="cuda") for _ in range(2))
torch.cuda.synchronize()
cfg = ctx.config(window_size=W, hop_size=H, window_type="hann", sample_rate=SR, flags=sonar.FP_MAGNITUDE,
                 precision=sonar.F64, pcm_dtype=sonar.F64, out_dtype=sonar.F64)


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def timed(fn, launches=1):
    kernel, wall = [], []
    for it in range(warmup + iters):
        ctx.synchronize()
        ctx.last_kernel_ms()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        w = (time.perf_counter() - t0) * 1e3
        k = ctx.last_kernel_ms() * launches
        if it >= warmup:
            kernel.append(k)
            wall.append(w)
    return {"kernel_ms": stats(kernel), "wall_ms": stats(wall)}


a = timed(lambda: ctx.fingerprint_device(x.data_ptr(), n, cfg, magnitude=mag.data_ptr()))
b = timed(lambda: ctx.hpcp_from_spectrum_device(mag.data_ptr(), F, K, W, SR, hp.data_ptr()))
c = timed(lambda: ctx.hpcp_device(x.data_ptr(), n, SR, hp2.data_ptr(), W, H, "hann"), 2 * plan["n_chunks"])
same = bool(torch.equal(hp, hp2))
peaks = {}
for name, sr in (("peaks_d1", SR), ("peaks_d5", 8000)):
    peaks[name] = timed(lambda: ctx.spectral_peaks_device(mag.data_ptr(), F, K, W, sr, count.data_ptr(), bins.data_ptr(),
                                                          pm.data_ptr(), pf.data_ptr()))
    peaks[name]["sample_rate"] = sr
    peaks[name]["mean_peaks_per_row"] = float(count.double().mean())
row_bytes = float(F) * K * 8
b["algorithmic_bytes"] = row_bytes
b["hbm_fraction"] = row_bytes / (b["kernel_ms"]["median"] * 1e-3) / HBM_RATE
for v in peaks.values():
    v["hbm_fraction"] = row_bytes / (v["kernel_ms"]["median"] * 1e-3) / HBM_RATE
print(json.dumps({
    "probe": "sonar_hpcp, NewHPCP(44100), 10 min of device-resident float64 PCM, W 2048, H 512, Hann",
    "device": torch.cuda.get_device_name(0), "samples": n, "frames": F, "bins": K, "chunk_frames": plan["chunk_frames"],
    "n_chunks": plan["n_chunks"], "hbm_rate_tb_s": HBM_RATE / 1e12, "iters": iters, "warmup": warmup,
    "a_fingerprint_magnitude": a, "b_hpcp_from_spectrum": b, "c_hpcp": c,
    "c_over_a_plus_b_kernel": c["kernel_ms"]["median"] / (a["kernel_ms"]["median"] + b["kernel_ms"]["median"]),
    "c_over_a_plus_b_wall": c["wall_ms"]["median"] / (a["wall_ms"]["median"] + b["wall_ms"]["median"]),
    "c_equals_b_bitwise": same, **peaks}))
ctx.close()
