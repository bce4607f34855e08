"""Timing probe of sonar_xcorr_params against sonar_ncc (diagnostics, not part of the product or the
tests, and no threshold: it reports).

One process, the C3 energy-sized inputs (XCORR_N samples each side, default 51,676; max_lag 10,335),
device pointers, a null correlation pointer (library scratch).  Per configuration: the kernel time of
a call from the library's HIP-event timers (sonar_enable_kernel_timing / sonar_last_kernel_ms) and
the host wall time of the call, each the median of ITERS calls (default 25) after WARMUP (default 3).
sonar_ncc runs on the same device arrays, in the same process, before and after the new calls.  The FFT method's first call (twiddle table built on the
host and uploaded, scratch allocated) is timed apart from its steady state.

Usage (GPU box): python3 tools/xcorr_probe.py [> profiles/<name>.txt]
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sonido-sonar_amd"))
import sonar  # noqa: E402

n = int(os.environ.get("XCORR_N", "51676"))
max_lag = int(os.environ.get("XCORR_MAX_LAG", "10335"))
iters = int(os.environ.get("ITERS", "25"))
warmup = int(os.environ.get("WARMUP", "3"))

rng = np.random.default_rng(3)
base = np.convolve(rng.random(n + 400) ** 2, np.ones(9) / 9, "same")      # smooth, positive: energy-like
a, b = base[137:137 + n].copy(), base[:n] + 0.02 * rng.random(n)
da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
torch.cuda.synchronize()
ctx = sonar.Context(0)
ctx.enable_kernel_timing(True)


def ncc_call():
    met = np.zeros(10)
    ctx._check(ctx._L.sonar_ncc(ctx._h, da.data_ptr(), n, db.data_ptr(), n, max_lag, None,
                                met.ctypes.data_as(C.c_void_p), 1))
    return met[0], int(met[1])


def xcorr_call(corr_type, method):
    def f():
        m = ctx.xcorr_params_device(da.data_ptr(), n, db.data_ptr(), n, max_lag, corr_type, method)
        return m["peak_correlation"], m["peak_lag"]
    return f


def auto_call():
    m = ctx.autocorr_device(da.data_ptr(), n, max_lag)
    return m["peak_correlation"], m["peak_lag"]


def timed(f):
    t0 = time.perf_counter()
    r = f()
    wall = (time.perf_counter() - t0) * 1e3
    return ctx.last_kernel_ms(), wall, r


def steady(f):
    for _ in range(warmup):
        timed(f)
    runs = [timed(f) for _ in range(iters)]
    return float(np.median([r[0] for r in runs])), float(np.median([r[1] for r in runs])), runs[-1][2]


rows = []
rows.append(("sonar_ncc (before)",) + steady(ncc_call))
rows.append(("xcorr ncc / time",) + steady(xcorr_call("ncc", "time")))
rows.append(("xcorr pearson / time",) + steady(xcorr_call("pearson", "time")))
rows.append(("xcorr zncc / time",) + steady(xcorr_call("zncc", "time")))
first = timed(xcorr_call("pearson", "frequency"))
rows.append(("xcorr fft, first call",) + first)
rows.append(("xcorr fft, steady",) + steady(xcorr_call("pearson", "frequency")))
rows.append(("autocorr fft, steady",) + steady(auto_call))
rows.append(("sonar_ncc (after)",) + steady(ncc_call))
base_ms = rows[0][1]
N = 1
while N < 2 * n - 1:
    N <<= 1
print(f"sonar_xcorr_params vs sonar_ncc, n = {n} both, max_lag {max_lag} ({2 * min(max_lag, n - 1) + 1} lags), "
      f"FFT size {N}, device pointers, median of {iters} after {warmup} warm-up calls (first call: one call)")
print(f"{'configuration':<24} {'kernel ms':>10} {'x ncc':>7} {'wall ms':>9}   peak (value, lag)")
for name, k, w, (pk, lag) in rows:
    print(f"{name:<24} {k:10.4f} {k / base_ms:7.3f} {w:9.4f}   ({pk:.6g}, {lag})", flush=True)
ctx.close()
