"""Timing probe of sonar_pitch_frames_raw / sonar_pitch_detect (diagnostics, not part of the product or
the tests, and no threshold: it reports).

One process, 10 minutes and 1 hour of 44.1 kHz float64 PCM resident on the device (six partials + noise,
generated there), NewPitchDetector's W = 1024, H = 512.  Per method and length, after WARMUP calls
(default 2), ITERS calls (default 7) of sonar_pitch_frames_raw with device pointers, pitch and confidence
only: the kernel time from the library's HIP-event timers (sonar_enable_kernel_timing /
sonar_last_kernel_ms) and the host wall time of the call including its final stream synchronisation,
each as median, minimum and maximum.  For the lag-domain methods also the unfused float64 operations of
the lag sums (YIN 3 a term, NSDF 4 a term by the issue's count, F W^2 / 4 terms) and their fraction of the
FP64 vector rate for unfused operations (39.3e12 / s, half the 78.6 TF fused peak).

The yardstick is sonar_pitch_yin on the same PCM in the same process (wall time; that entry has no event
timer), whose code this feature does not touch.  `detect` is sonar_pitch_detect with host outputs: the raw
pass, the copy back and the host tracker.

Usage (GPU box): python3 tools/pitch_probe.py > profiles/pitch_probe.json
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sonido-sonar_amd"))
import sonar  # noqa: E402

SR, W, H = 44100, 1024, 512
UNFUSED_RATE = 39.3e12
iters = int(os.environ.get("ITERS", "7"))
warmup = int(os.environ.get("WARMUP", "2"))
METHODS = ["yin", "nsdf", "acf", "hps", "cepstrum", "zero_crossing"]
TERM_OPS = {"yin": 3, "nsdf": 4}

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
    x = 0.05 * torch.randn(n, dtype=torch.float64, device="cuda", generator=gen)
    for h in range(1, 7):
        x += 0.7 ** h * torch.sin(2 * np.pi * h * 196.0 * t)
    return x


out = {"probe": "sonar_pitch_frames_raw, NewPitchDetector(44100) with each method, device-resident float64 PCM, "
                "W 1024, H 512", "library": os.path.relpath(sonar.LIB_PATH, ROOT),
       "device": torch.cuda.get_device_name(0), "iters": iters, "warmup": warmup,
       "unfused_fp64_rate_per_s": UNFUSED_RATE, "lengths": {}}
for label, seconds in (("10min", 600), ("1h", 3600)):
    n = seconds * SR
    x = signal(n)
    F = sonar.pitch_detect_frames(n, W, H)
    Fy = sonar.pitch_frames(n)
    p_d, c_d = (torch.zeros(max(F, Fy), dtype=torch.float64, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    legs = {}
    yin_old = timed(lambda: ctx._check(ctx._L.sonar_pitch_yin(ctx._h, C.c_void_p(x.data_ptr()), n, SR,
                                                                C.c_void_p(p_d.data_ptr()), C.c_void_p(c_d.data_ptr()),
                                                                None, 1)))
    del yin_old["kernel_ms"]
    yard = yin_old["wall_ms"]["median"]
    old_rows = (p_d[:F].clone(), c_d[:F].clone())
    for m in METHODS:
        prm = sonar.pitch_params_default(SR, method=m)
        leg = timed(lambda: ctx.pitch_frames_raw_device(x.data_ptr(), n, prm, p_d.data_ptr(), c_d.data_ptr()))
        leg["wall_over_pitch_yin"] = leg["wall_ms"]["median"] / yard
        if m in TERM_OPS:
            ops = float(F) * (W // 2) ** 2 * TERM_OPS[m]
            leg["lag_sum_ops"] = ops
            leg["unfused_fp64_fraction"] = ops / (leg["kernel_ms"]["median"] * 1e-3) / UNFUSED_RATE
        if m == "yin":
            leg["rows_equal_pitch_yin_bitwise"] = bool(torch.equal(p_d[:F], old_rows[0]) and
                                                       torch.equal(c_d[:F], old_rows[1]))
        leg["voiced_fraction"] = float((p_d[:F] > 0).double().mean())
        legs[m] = leg
    if label == "10min":
        xh = x.cpu().numpy()
        prm = sonar.pitch_params_default(SR)
        legs["detect_host_yin"] = timed(lambda: ctx.pitch_detect(xh, prm))
        legs["detect_host_yin"]["note"] = "host PCM: includes the upload of n doubles, the copy back and the tracker"
        del xh
    out["lengths"][label] = {"samples": n, "frames": F, "pitch_yin_frames": Fy, "pitch_yin": yin_old, **legs}
    del x, p_d, c_d
    torch.cuda.empty_cache()
print(json.dumps(out))
ctx.close()
