"""Timing probe of sonar_hratio_frames (diagnostics, not part of the product or the tests, and no threshold: it
reports).

One process, 10 minutes and 1 hour of 44.1 kHz float64 PCM resident on the device (six partials + noise,
generated there), NewHarmonicRatioAnalyzer's W = 2048, H = 512.  Per leg and length, after WARMUP calls (default
2), ITERS calls (default 7) of sonar_hratio_frames with device pointers: the kernel time from the library's
HIP-event timers (sonar_enable_kernel_timing / sonar_last_kernel_ms) and the host wall time of the call
including its final stream synchronisation, each as median, minimum and maximum.

Legs.  Each method with every per-frame output but the F x K noise_floor rows (`hnr`, `comb`, `hps`, `spectral`,
`acf`, `yin`), and, to split the HNR time by measurement, HNR variants that switch one stage off:
  hnr_with_floor_rows   the F x K noise_floor rows written as well
  hnr_no_floor          snr and noise_floor not asked for: no quantile selection, no second smoothing, and the
                        chain of the floor's energy adds zeros
  hnr_minimum_floor     noise_floor_method "minimum": the window scan instead of the rank selection
  hnr_no_smoothing      spectral_smoothing_len 1
  hnr_ratio_only        harmonic_ratio alone (the stage runs whole but for the floor; one output row)
  hnr_0_harmonics       max_harmonics 0: no findHarmonicPeaks, no mask, no roughness
The yardstick, in the same process, is sonar_pitch_frames_raw with method HPS at W 1024, zero padding 2, H 512:
the same 2048-point transform by code this feature does not touch.

Usage (GPU box): python3 tools/hratio_probe.py > profiles/hratio_probe.json
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
K, MH = W // 2, 20
iters = int(os.environ.get("ITERS", "7"))
warmup = int(os.environ.get("WARMUP", "2"))
SCALARS = [k for k in sonar.HRATIO_FRAME_FIELDS if k != "noise_floor"]
LEGS = [("hnr", dict(method="hnr"), SCALARS), ("comb", dict(method="comb"), SCALARS), ("hps", dict(method="hps"), SCALARS),
        ("spectral", dict(method="spectral"), SCALARS), ("acf", dict(method="acf"), SCALARS),
        ("yin", dict(method="yin"), SCALARS),
        ("hnr_with_floor_rows", dict(method="hnr"), list(sonar.HRATIO_FRAME_FIELDS)),
        ("hnr_no_floor", dict(method="hnr"), [k for k in SCALARS if k != "snr"]),
        ("hnr_minimum_floor", dict(method="hnr", noise_floor_method="minimum"), SCALARS),
        ("hnr_no_smoothing", dict(method="hnr", spectral_smoothing_len=1), SCALARS),
        ("hnr_ratio_only", dict(method="hnr"), ["harmonic_ratio"]),
        ("hnr_0_harmonics", dict(method="hnr", max_harmonics=0), SCALARS)]

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


out = {"probe": "sonar_hratio_frames, NewHarmonicRatioAnalyzer(44100) with each method, device-resident float64 PCM, "
                "W 2048, H 512", "library": os.path.relpath(sonar.LIB_PATH, ROOT),
       "device": torch.cuda.get_device_name(0), "iters": iters, "warmup": warmup,
       "lds_bytes_per_block": 8 * (5 * K + K // 2 + 64 + 64 + 128 + 8) + 4 * 72 + 2 * (K // 2 + 256) + K, "lengths": {}}
for label, seconds in (("10min", 600), ("1h", 3600)):
    n = seconds * SR
    x = signal(n)
    F = sonar.pitch_detect_frames(n, W, H)
    Fy = sonar.pitch_detect_frames(n, 1024, H)
    bufs = {k: torch.zeros(F, dtype=torch.float64, device="cuda") for k in sonar.HRATIO_FRAME_FIELDS[:11]}
    bufs["num_harmonics"] = torch.zeros(F, dtype=torch.int32, device="cuda")
    bufs["h_bin"] = torch.zeros(F * MH, dtype=torch.int32, device="cuda")
    for k in ("h_freq", "h_amp", "h_phase"):
        bufs[k] = torch.zeros(F * MH, dtype=torch.float64, device="cuda")
    bufs["noise_floor"] = torch.zeros(F * K, dtype=torch.float64, device="cuda")
    yp, yc = (torch.zeros(Fy, dtype=torch.float64, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    yprm = sonar.pitch_params_default(SR, method="hps", window_size=1024, hop_size=H, zero_padding=2)
    yard = timed(lambda: ctx.pitch_frames_raw_device(x.data_ptr(), n, yprm, yp.data_ptr(), yc.data_ptr()))
    ym = yard["kernel_ms"]["median"]
    legs = {}
    for name, kw, want in LEGS:
        prm = sonar.hratio_params_default(SR, **kw)
        ptrs = {k: bufs[k].data_ptr() for k in want}
        leg = timed(lambda: ctx.hratio_device("frames", x.data_ptr(), n, prm, ptrs))
        leg["kernel_over_yardstick_per_frame"] = (leg["kernel_ms"]["median"] / F) / (ym / Fy)
        leg["ns_per_frame"] = leg["kernel_ms"]["median"] * 1e6 / F
        if "harmonic_ratio" in want:
            r = bufs["harmonic_ratio"]
            leg["finite_ratio_fraction"] = float(torch.isfinite(r).double().mean())
        if "num_harmonics" in want:
            leg["mean_harmonics"] = float(bufs["num_harmonics"].double().mean())
        legs[name] = leg
    out["lengths"][label] = {"samples": n, "frames": F, "yardstick_frames": Fy,
                             "yardstick_pitch_hps_w1024_zp2": yard, **legs}
    del x, bufs, yp, yc
    torch.cuda.empty_cache()
print(json.dumps(out))
ctx.close()
