"""Timing probe of the onset and tempo entries (diagnostics, not part of the product or the tests, and no
threshold: it reports).

One process, device-resident float64 data at 44.1 kHz: 10 minutes (F = 51,678 rows of 513 at 1024 / 512)
and 2 hours (F = 620,155).  The PCM is a floor of noise with a decaying burst every 0.5 s, generated on
the device.  Per leg, after WARMUP calls (default 3), ITERS calls (default 9): the kernel time from the
library's HIP-event timers (sonar_enable_kernel_timing / sonar_last_kernel_ms, the mean over the call's
timed regions times their number) and the host wall time of the call including its final stream
synchronisation, each as median, minimum and maximum.

  flux                 sonar_spectral_flux on the unwindowed STFT rows; bytes = F K 8 (each row once), their
                       fraction of the 8 TB/s HBM rate
  peaks_mif2 / _mif4   sonar_onset_peaks on that flux at minIntervalFrames 2 (nothing walks) and 4 (the
                       default's: one thread walks the candidate words); chain_ns_per_frame is their
                       difference over the frames
  peaks_sawtooth_mif4  the same on a curve whose every second value is a candidate (the longest chain)
  rms_512_256, rms_4410_1102   sonar_rms_envelope
  autocorr_narrow / _full      sonar_tempo_autocorrelation without and with the whole curve
  transform            sonar_fingerprint, SONAR_FP_MAGNITUDE only, rectangular window, float64, device buffer
  onsets_flux          sonar_onsets_flux whole (chunked), against transform + flux + peaks_mif4
  tempo                sonar_tempo whole

Usage (GPU box): python3 tools/onset_probe.py > profiles/onset_probe.json
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

SR, W, H = 44100, 1024, 512
K = W // 2 + 1
HBM_RATE = 8e12
iters = int(os.environ.get("ITERS", "9"))
warmup = int(os.environ.get("WARMUP", "3"))
durations = {"10min": 600, "2h": 7200}
if os.environ.get("PROBE_SECONDS"):                          # a rehearsal size
    durations = {"short": int(os.environ["PROBE_SECONDS"])}

ctx = sonar.Context(0)
ctx.enable_kernel_timing(True)
cfg = ctx.config(window_size=W, hop_size=H, window_type="rectangular", sample_rate=SR, flags=sonar.FP_MAGNITUDE,
                 precision=sonar.F64, pcm_dtype=sonar.F64, out_dtype=sonar.F64)


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def timed(fn, regions=1):
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
    return {"kernel_ms": stats(kernel), "wall_ms": stats(wall), "timed_regions": regions}


def pcm(seconds):
    n = seconds * SR
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seconds)
    x = 1e-3 * torch.randn(n, dtype=torch.float64, device="cuda", generator=gen)
    t = torch.arange(n, device="cuda") % (SR // 2)
    x += 0.5 * torch.exp(-t.double() / (0.01 * SR)) * torch.randn(n, dtype=torch.float64, device="cuda", generator=gen)
    return x


def probe(seconds):
    n = seconds * SR
    x = pcm(seconds)
    plan = sonar.hpcp_plan(n, W, H)
    F = plan["frames"]
    mag = torch.zeros(F, K, dtype=torch.float64, device="cuda")
    flux = torch.zeros(F - 1, dtype=torch.float64, device="cuda")
    width = sonar.onset_peaks_width(F - 1)
    index = torch.zeros(width, dtype=torch.int64, device="cuda")
    onsets = torch.zeros(width, dtype=torch.int64, device="cuda")
    saw = (torch.arange(F - 1, device="cuda") % 2).double()
    torch.cuda.synchronize()
    legs = {}
    legs["transform"] = timed(lambda: ctx.fingerprint_device(x.data_ptr(), n, cfg, magnitude=mag.data_ptr()))
    legs["flux"] = timed(lambda: ctx.spectral_flux_device(mag.data_ptr(), F, K, flux.data_ptr()))
    legs["flux"]["algorithmic_bytes"] = float(F) * K * 8 + (F - 1) * 8.0
    legs["flux"]["hbm_fraction"] = legs["flux"]["algorithmic_bytes"] / (legs["flux"]["kernel_ms"]["median"] * 1e-3) / HBM_RATE
    counts = {}
    for name, curve, mif in (("peaks_mif2", flux, 2), ("peaks_mif4", flux, 4), ("peaks_sawtooth_mif2", saw, 2),
                             ("peaks_sawtooth_mif4", saw, 4)):
        legs[name] = timed(lambda: counts.__setitem__(name, ctx.onset_peaks_device(curve.data_ptr(), F - 1, 0.3, float(mif), 1, 1,
                                                                                  index.data_ptr())))
        legs[name]["count"] = counts[name]
    for frame, hop in ((512, 256), (4410, 1102)):
        env = torch.zeros(sonar.rms_envelope_frames(n, frame, hop), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        name = f"rms_{frame}_{hop}"
        legs[name] = timed(lambda: ctx.rms_envelope_device(x.data_ptr(), n, frame, hop, env.data_ptr()))
        legs[name]["frames"] = len(env)
        legs[name]["algorithmic_bytes"] = n * 8.0 + len(env) * 8.0
        legs[name]["hbm_fraction"] = legs[name]["algorithmic_bytes"] / (legs[name]["kernel_ms"]["median"] * 1e-3) / HBM_RATE
    ap = sonar.tempo_autocorr_plan(n, SR)
    tempo = torch.zeros(1, dtype=torch.float64, device="cuda")
    lag = torch.zeros(1, dtype=torch.int64, device="cuda")
    ac = torch.zeros(ap["n_autocorr"], dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    legs["autocorr_narrow"] = timed(lambda: ctx.tempo_autocorrelation_device(x.data_ptr(), n, SR, tempo.data_ptr(), lag.data_ptr()))
    narrow = (tempo.item(), lag.item())
    legs["autocorr_full"] = timed(lambda: ctx.tempo_autocorrelation_device(x.data_ptr(), n, SR, tempo.data_ptr(), lag.data_ptr(),
                                                                          ac.data_ptr()))
    full = (tempo.item(), lag.item())
    got = {}
    legs["onsets_flux"] = timed(lambda: got.__setitem__("flux", ctx.onsets_flux_device(x.data_ptr(), n, SR, 0.3, 0.05,
                                                                                       onsets.data_ptr())),
                                regions=2 * plan["n_chunks"] + 1)
    legs["onsets_flux"]["count"] = got["flux"][0]
    # the same onsets from the three entries one after the other
    ctx.fingerprint_device(x.data_ptr(), n, cfg, magnitude=mag.data_ptr())
    ctx.spectral_flux_device(mag.data_ptr(), F, K, flux.data_ptr())
    c = ctx.onset_peaks_device(flux.data_ptr(), F - 1, 0.3, 0.05, H, SR, index.data_ptr())
    ctx.synchronize()
    same = bool(c == got["flux"][0] and torch.equal(index * H, onsets))
    res = {}
    legs["tempo"] = timed(lambda: res.__setitem__("tempo", ctx.tempo(x.data_ptr(), SR, device_n=n)),
                          regions=2 * plan["n_chunks"] + 4)
    parts = sum(legs[k]["kernel_ms"]["median"] for k in ("transform", "flux", "peaks_mif4"))
    chain = (legs["peaks_mif4"]["kernel_ms"]["median"] - legs["peaks_mif2"]["kernel_ms"]["median"]) * 1e6 / (F - 1)
    saw_chain = (legs["peaks_sawtooth_mif4"]["kernel_ms"]["median"] - legs["peaks_sawtooth_mif2"]["kernel_ms"]["median"]) * 1e6 / (F - 1)
    return {"samples": n, "frames": F, "bins": K, "chunk_frames": plan["chunk_frames"], "n_chunks": plan["n_chunks"],
            "autocorr_plan": ap, "autocorr_tempo_narrow": narrow, "autocorr_tempo_full": full,
            "onsets_flux_equals_the_three_entries": same,
            "onsets_flux_over_transform_plus_flux_plus_peaks_kernel": legs["onsets_flux"]["kernel_ms"]["median"] / parts,
            "onsets_flux_over_transform_plus_flux_plus_peaks_wall": legs["onsets_flux"]["wall_ms"]["median"] /
            sum(legs[k]["wall_ms"]["median"] for k in ("transform", "flux", "peaks_mif4")),
            "chain_ns_per_frame": chain, "chain_ns_per_frame_sawtooth": saw_chain, "tempo_result": res["tempo"], **legs}


out = {"probe": "onset and tempo entries, device-resident float64 PCM at 44.1 kHz, W 1024, H 512",
       "library": os.path.relpath(sonar.LIB_PATH, ROOT), "device": torch.cuda.get_device_name(0),
       "hbm_rate_tb_s": HBM_RATE / 1e12, "iters": iters, "warmup": warmup,
       "key_vote_chain_ns_per_frame": 20.0, "chord_chain_ns_per_frame": 19.4}
for name, seconds in durations.items():
    out[name] = probe(seconds)
    torch.cuda.empty_cache()
print(json.dumps(out))
ctx.close()
