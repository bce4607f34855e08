"""Timing probe of sonar_inharm_frames (diagnostics, not part of the product or the tests, and no threshold: it
reports).

One process, 10 minutes and 1 hour of 44.1 kHz float64 PCM resident on the device (eight stretched partials +
noise, generated there), W = 1024 (the only window the analyzer's detector takes), H = 512.  Per leg and length,
after WARMUP calls (default 2), ITERS calls (default 7) of sonar_inharm_frames with device pointers: the kernel
time from the library's HIP-event timers (sonar_enable_kernel_timing / sonar_last_kernel_ms) and the host wall
time of the call including its final stream synchronisation, each as median, minimum and maximum.

Legs: every method with every per-frame output.  sonar_last_kernel_ms averages over the timed sections since the
last query, and a sonar_inharm_frames call has two: its f0 leg (the default detector's YIN kernels under
sonar_pitch_detect, one section) and the analyzer's own stage (the transform and everything after it in
inharm_kernel; for BeatPattern also the correlation launches and their tail).  The f0 leg is measured next to it in
the same process (`f0_leg_pitch_detect_defaults`) and each leg reports `kernel_ms_stage` = 2 x its median - the f0
leg's median.  The yardstick is sonar_pitch_frames_raw with the cepstrum method at W 1024, zero padding 1, code this
feature does not touch: a forward and an inverse W-point transform with a logarithm between them
(`stage_over_yardstick`).

Usage (GPU box): python3 tools/inharm_probe.py > profiles/inharm_probe.json
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

SR, W, H, MH = 44100, 1024, 512, 20
iters = int(os.environ.get("ITERS", "7"))
warmup = int(os.environ.get("WARMUP", "2"))
LEGS = ["spectral_deviation", "railsback", "fletcher_munson", "partial_tracking", "statistical", "beat_pattern"]
INT = ("status", "num_harmonics", "n_deviations", "h_number", "quality")
ROWS = ("h_number", "h_freq", "h_ideal", "h_amp", "h_deviation")

ctx = sonar.Context(0)
ctx.enable_kernel_timing(True)


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


def signal(n):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    t = torch.arange(n, dtype=torch.float64, device="cuda") / SR
    x = 0.002 * torch.randn(n, dtype=torch.float64, device="cuda", generator=gen)
    for k in range(1, 9):
        x += 0.8 ** k * torch.sin(2 * np.pi * k * float(np.sqrt(1.0 + 4e-4 * k * k)) * 300.0 * t)
    return x


out = {"probe": "sonar_inharm_frames, NewInharmonicityAnalyzer(44100) at window 1024 with each method, device-resident "
                "float64 PCM, W 1024, H 512", "library": os.path.relpath(sonar.LIB_PATH, ROOT),
       "device": torch.cuda.get_device_name(0), "iters": iters, "warmup": warmup,
       "lds_bytes_per_block": 8 * (5 * (W // 2) + 6 * 64 + 256 + 8) + 4 * 72, "lengths": {}}
for label, seconds in (("10min", 600), ("1h", 3600)):
    n = seconds * SR
    x = signal(n)
    F = sonar.pitch_detect_frames(n, W, H)
    bufs = {k: torch.zeros(F * (MH if k in ROWS else 1), dtype=torch.int32 if k in INT else torch.float64, device="cuda")
            for k in sonar.INHARM_FRAME_FIELDS}
    yp, yc = (torch.zeros(F, dtype=torch.float64, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    yprm = sonar.pitch_params_default(SR, method="cepstrum", window_size=W, hop_size=H, zero_padding=1)
    yard = timed(lambda: ctx.pitch_frames_raw_device(x.data_ptr(), n, yprm, yp.data_ptr(), yc.data_ptr()))
    dprm = sonar.pitch_params_default(SR, hop_size=H)
    f0leg = timed(lambda: ctx.pitch_detect_device(x.data_ptr(), n, dprm, {"pitch": yp.data_ptr(), "confidence": yc.data_ptr()}))
    ym, fm = yard["kernel_ms"]["median"], f0leg["kernel_ms"]["median"]
    legs = {}
    for name in LEGS:
        prm = sonar.inharm_params_default(SR, method=name, window_size=W)
        ptrs = {k: v.data_ptr() for k, v in bufs.items()}
        leg = timed(lambda: ctx.inharm_device("frames", x.data_ptr(), n, H, prm, ptrs))
        stage = 2.0 * leg["kernel_ms"]["median"] - fm
        leg["kernel_ms_stage"] = stage
        leg["stage_over_yardstick"] = stage / ym
        leg["ns_per_frame_stage"] = stage * 1e6 / F
        leg["ok_fraction"] = float((bufs["status"] == 0).double().mean())
        leg["mean_harmonics"] = float(bufs["num_harmonics"].double().mean())
        legs[name] = leg
    out["lengths"][label] = {"samples": n, "frames": F, "yardstick_pitch_cepstrum_w1024": yard,
                             "f0_leg_pitch_detect_defaults": f0leg, **legs}
    del x, bufs, yp, yc
    torch.cuda.empty_cache()
print(json.dumps(out))
ctx.close()
