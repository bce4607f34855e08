"""Timing probe of sonar_hps_from_spectrum / sonar_hps (diagnostics, not part of the product or the
tests, and no threshold: it reports).

One process, 10 minutes of 44.1 kHz float64 PCM resident on the device (four partials + noise,
generated there), W = 2048, H = 512: F = 51,676 frames of K = 1025 bins, the music extractor's
NewHarmonicProduct(sampleRate, 10, 80.0, 2000.0).  Per leg, after WARMUP calls (default 3), ITERS calls
(default 9): the kernel time from the library's HIP-event timers (sonar_enable_kernel_timing /
sonar_last_kernel_ms, the mean over the call's timed regions times their number) and the host wall
time of the call including its final stream synchronisation, each as median, minimum and maximum;
the algorithmic bytes (F K 8 read plus what the leg writes) and their fraction of the 8 TB/s HBM rate.

  transform            sonar_fingerprint, SONAR_FP_MAGNITUDE only, float64, into a device buffer
  f0                   sonar_hps_from_spectrum, f0_bin and f0 only
  f0_conf              ... with confidence (the ordered sum of mag^2 runs)
  f0_conf_strengths    ... with confidence and strengths
  f0_rows              ... f0 and the HPS rows written
  *_interp             the same legs with ComputeHPSWithInterpolation
  f0_conf_2h           f0 and confidence on F = 620,153 rows (2 h), the 10 min rows repeated
  hps                  sonar_hps whole (chunked transform + estimate), against transform + f0_conf
  peaks_d1, hpcp       sonar_spectral_peaks and sonar_hpcp_from_spectrum on the same rows, as hpcp_probe

The chain layout behind the confidence is a build-time choice (SONAR_HPS_CHAIN_ROWS_PER_LANE); run the
probe once per build (SONAR_LIB) to compare them.

Usage (GPU box): python3 tools/hps_probe.py > profiles/hps_probe.json
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

SR, W, H, NH, LO, HI = 44100, 2048, 512, 10, 80.0, 2000.0
HBM_RATE = 8e12
iters = int(os.environ.get("ITERS", "9"))
warmup = int(os.environ.get("WARMUP", "3"))

ctx = sonar.Context(0)
ctx.enable_kernel_timing(True)
n = 600 * SR
plan = sonar.hps_plan(n, W, H)
F, K = plan["frames"], W // 2 + 1
F2H = 620_153
gen = torch.Generator(device="cuda")
gen.manual_seed(11)
t = torch.arange(n, dtype=torch.float64, device="cuda") / SR
x = sum(a * torch.sin(2 * np.pi * f * t) for a, f in [(0.5, 220.0), (0.3, 554.37), (0.2, 1318.5), (0.1, 3520.0)])
x = x + 0.01 * torch.randn(n, dtype=torch.float64, device="cuda", generator=gen)
del t
mag = torch.zeros(F, K, dtype=torch.float64, device="cuda")
b1, b2 = (torch.zeros(F, dtype=torch.int32, device="cuda") for _ in range(2))
f1, f2, c1, c2 = (torch.zeros(F, dtype=torch.float64, device="cuda") for _ in range(4))
st = torch.zeros(F, NH, dtype=torch.float64, device="cuda")
rows = torch.zeros(F, K, dtype=torch.float64, device="cuda")
hp = torch.zeros(F, 12, dtype=torch.float64, device="cuda")
count = torch.zeros(F, dtype=torch.int32, device="cuda")
bins = torch.zeros(F, 60, dtype=torch.int32, device="cuda")
pm, pf = (torch.zeros(F, 60, dtype=torch.float64, device="cuda") for _ in range(2))
torch.cuda.synchronize()
cfg = ctx.config(window_size=W, hop_size=H, window_type="hann", sample_rate=SR, flags=sonar.FP_MAGNITUDE,
                 precision=sonar.F64, pcm_dtype=sonar.F64, out_dtype=sonar.F64)


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def timed(fn, regions=1, written=0.0, frames=F):
    kernel, wall = [], []
    for it in range(warmup + iters):
        ctx.synchronize()
        ctx.last_kernel_ms()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        w = (time.perf_counter() - t0) * 1e3
        k = ctx.last_kernel_ms() * regions
        if it >= warmup:
            kernel.append(k)
            wall.append(w)
    out = {"kernel_ms": stats(kernel), "wall_ms": stats(wall)}
    out["algorithmic_bytes"] = float(frames) * K * 8 + written
    out["hbm_fraction"] = out["algorithmic_bytes"] / (out["kernel_ms"]["median"] * 1e-3) / HBM_RATE
    return out


def spectrum(m, frames, bp, fp, interp, conf=None, strengths=None, hps=None):
    return lambda: ctx.hps_from_spectrum_device(m.data_ptr(), frames, K, W, SR, bp.data_ptr(), fp.data_ptr(), NH, LO, HI,
                                                interp, conf.data_ptr() if conf is not None else None,
                                                strengths.data_ptr() if strengths is not None else None,
                                                hps.data_ptr() if hps is not None else None)


legs = {"transform": timed(lambda: ctx.fingerprint_device(x.data_ptr(), n, cfg, magnitude=mag.data_ptr()),
                           written=0.0)}
legs["transform"]["note"] = "normalised Hann; algorithmic_bytes is the F K 8 written, nothing of the PCM"
for tag, interp in (("", False), ("_interp", True)):
    legs["f0" + tag] = timed(spectrum(mag, F, b1, f1, interp), written=F * 12.0)
    legs["f0_conf" + tag] = timed(spectrum(mag, F, b1, f1, interp, c1), written=F * 20.0)
    legs["f0_conf_strengths" + tag] = timed(spectrum(mag, F, b1, f1, interp, c1, st), written=F * (20.0 + 8 * NH))
    legs["f0_rows" + tag] = timed(spectrum(mag, F, b1, f1, interp, hps=rows), written=F * (12.0 + 8 * K))
del rows
legs["hps"] = timed(lambda: ctx.hps_device(x.data_ptr(), n, SR, b2.data_ptr(), f2.data_ptr(), W, H, NH, LO, HI, False,
                                           c2.data_ptr()), regions=2 * plan["n_chunks"], written=F * 20.0)
# sonar_hps works on the unnormalised window's rows: the same estimate from those rows for the comparison
ctx.hps_device(x.data_ptr(), n, SR, b2.data_ptr(), f2.data_ptr(), W, H, NH, LO, HI, False, c2.data_ptr(), None,
               mag.data_ptr())
spectrum(mag, F, b1, f1, False, c1)()
ctx.synchronize()
same = bool(torch.equal(b1, b2) and torch.equal(f1, f2) and torch.equal(c1, c2))
voiced = float((b2 > 0).double().mean())
ctx.fingerprint_device(x.data_ptr(), n, cfg, magnitude=mag.data_ptr())
legs["peaks_d1"] = timed(lambda: ctx.spectral_peaks_device(mag.data_ptr(), F, K, W, SR, count.data_ptr(), bins.data_ptr(),
                                                           pm.data_ptr(), pf.data_ptr()), written=F * (4.0 + 60 * 20))
legs["hpcp"] = timed(lambda: ctx.hpcp_from_spectrum_device(mag.data_ptr(), F, K, W, SR, hp.data_ptr()),
                     written=F * 96.0)
reps = -(-F2H // F)
big = mag.repeat(reps, 1)[:F2H].contiguous()
bb = torch.zeros(F2H, dtype=torch.int32, device="cuda")
fb, cb = (torch.zeros(F2H, dtype=torch.float64, device="cuda") for _ in range(2))
torch.cuda.synchronize()
legs["f0_2h"] = timed(spectrum(big, F2H, bb, fb, False), written=F2H * 12.0, frames=F2H)
legs["f0_conf_2h"] = timed(spectrum(big, F2H, bb, fb, False, cb), written=F2H * 20.0, frames=F2H)
sum_ms = legs["transform"]["kernel_ms"]["median"] + legs["f0_conf"]["kernel_ms"]["median"]
print(json.dumps({
    "probe": "sonar_hps, NewHarmonicProduct(44100, 10, 80, 2000), 10 min of device-resident float64 PCM, W 2048, H 512",
    "library": os.path.relpath(sonar.LIB_PATH, ROOT), "device": torch.cuda.get_device_name(0), "samples": n, "frames": F,
    "bins": K, "frames_2h": F2H, "chunk_frames": plan["chunk_frames"], "n_chunks": plan["n_chunks"],
    "scan_bins": sonar.hps_bins(SR, W, K, LO, HI), "hbm_rate_tb_s": HBM_RATE / 1e12, "iters": iters, "warmup": warmup,
    "voiced_fraction": voiced, "hps_equals_from_spectrum_bitwise": same,
    "hps_over_transform_plus_f0_conf_kernel": legs["hps"]["kernel_ms"]["median"] / sum_ms,
    "chain_ms": legs["f0_conf"]["kernel_ms"]["median"] - legs["f0"]["kernel_ms"]["median"],
    "f0_over_peaks_d1": legs["f0"]["kernel_ms"]["median"] / legs["peaks_d1"]["kernel_ms"]["median"],
    **legs}))
ctx.close()
