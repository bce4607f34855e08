"""The cases the harmonic-ratio tests share (tests/test_hratio_cpu.py, tests/test_gpu_hratio.py): the signals,
the parameter pairs (checker, library), the cached reference of every case and, for the PCM cases, the measured
tolerance and the frames it leaves decided.

Tolerance of the PCM cases.  The reference's transform is go-dsp's, whose source is not in the tree, so the
spectral methods are held to FACTOR x the largest difference, on the case's own frames, between the checker's
|X| on numpy's FFT and on xcorr_params_ref.go_fft, relative to the row's peak (FACTOR is test_gpu_pitch.py's).
Per output that relative tolerance `tol` is scaled by what the output is made of (scales(), below); a frame
whose margin (hratio_ref.py) is not above 1000 tol is undecided and skipped, under a cap of 10 % per case."""
import functools
import math

import numpy as np

import hratio_ref as R
import pitch_ref as PR

SR = 16000
FACTOR = 16
ULP16 = 16 * 2.0 ** -52         # outputs through log10 / exp: two libraries of <= 2 ulp over <= 3 chained operations
METHODS = {"hnr": R.HNR, "acf": R.ACF, "hps": R.HPS, "comb": R.COMB, "spectral": R.SPECTRAL, "yin": R.YIN}
EXACT_KEYS = ("num_harmonics", "h_bin", "harmonic_energy", "noise_energy", "total_energy", "periodicity", "roughness",
              "noise_floor", "h_freq", "h_amp", "f0", "f0_confidence")
LOG_KEYS = ("harmonic_ratio", "snr", "voicing", "harmonicity")
# from spectrum: (W, F); K = 32 is where the 20-wide window and the L = 5 / 10 edge rules dominate.  One frame
# per block, so there is no frames-per-block or frames-per-lane boundary to straddle.
SPECTRUM_SHAPES = [(64, 1), (64, 65), (256, 5), (2048, 5), (2048, 130)]
SPECTRUM_CASES = [(m, W, F, "percentile") for W, F in SPECTRUM_SHAPES for m in ("hnr", "comb", "hps", "spectral")] + \
                 [("hnr", W, F, nf) for W, F in SPECTRUM_SHAPES[1:4] for nf in ("median", "minimum")]
# from PCM: W x H in {W / 4, W, W + 76} at F = 5, and one F >= 65
PCM_CASES = [(m, W, H, 5) for W in (64, 256, 2048) for H in (W // 4, W, W + 76) for m in ("hnr", "hps", "spectral")] + \
            [("comb", 256, 64, 5)] + [(m, 256, 64, 66) for m in ("hnr", "hps", "spectral")]


@functools.lru_cache(maxsize=None)
def signal(W, H, F):
    x = PR.make_signal(F, W, H, seed=W * 11 + H + F, sample_rate=SR)
    x.setflags(write=False)
    return x


def ref_params(method, W, H, **kw):
    return R.Params(SR, method=METHODS[method], window_size=W, hop_size=H, autocorr_max_lag=max(W, 2048), **kw)


def lib_params(sonar, method, W, H, **kw):
    kw = {k: (int(v) if isinstance(v, bool) else v) for k, v in kw.items()}
    return sonar.hratio_params_default(SR, method=method, window_size=W, hop_size=H, autocorr_max_lag=max(W, 2048), **kw)


@functools.lru_cache(maxsize=None)
def spectrum_rows(W, F):
    """|X| and phase rows (numpy's transform) of the F frames of signal(W, W // 2, F)"""
    x, win = signal(W, W // 2, F), R.window(W)
    rows = [R.spectrum(x[f * (W // 2):f * (W // 2) + W] * win) for f in range(F)]
    mag, ph = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    mag.setflags(write=False), ph.setflags(write=False)
    return mag, ph


@functools.lru_cache(maxsize=None)
def spectrum_ref(method, W, F, nf):
    mag, ph = spectrum_rows(W, F)
    return R.from_spectrum(mag, ph, ref_params(method, W, W // 2, noise_floor_method=nf))


@functools.lru_cache(maxsize=None)
def pcm_ref(method, W, H, F, fft="numpy"):
    return R.frames(signal(W, H, F), ref_params(method, W, H), fft)


def pcm_tolerance(method, W, H, F):
    """(tol, measured, decided): the relative tolerance, the numpy-vs-go difference it comes from, and the mask
    of the frames both orderings decide"""
    a, b = pcm_ref(method, W, H, F, "numpy"), pcm_ref(method, W, H, F, "go")
    peak = a["raw_magnitude"].max(axis=1, keepdims=True)
    measured = float(np.max(np.abs(a["raw_magnitude"] - b["raw_magnitude"]) / peak))
    tol = FACTOR * measured
    decided = (a["margin"] > 1000 * tol) & (b["margin"] > 1000 * tol)
    return tol, measured, decided


def scales(ref, f, p):
    """What one unit of relative |X| error (in units of the row's peak) can move each tolerance-held output of
    frame f by, absolutely, from the reference's own values.  One magnitude, smoothed or a floor value, moves by
    peak.  A sum of <= K squares moves by E = 2 K peak^2; 10 log10 of a ratio of two such sums a / b by
    (10 / ln 10) (E / a + E / |b|); the sigmoid's slope is at most 0.025 of that.  The periodicity is a ratio of
    two sums of <= K magnitudes, the lower one at least sqrt(total_energy).  The roughness has n (n - 1) / 2 terms
    m_i m_j / (d + 1), each moving by at most 2 peak^2.  The HPS ratio is 20 log10 of a product of magnitudes
    (hps_rel: the sum of peak / m over its factors)."""
    K = p.window_size // 2
    peak = float(ref["scale"][f])
    E = 2.0 * K * peak * peak
    db = 10.0 / math.log(10.0)
    inv = lambda v: E / abs(v) if v != 0 else math.inf                 # noqa: E731
    s = {"h_amp": peak, "f0_confidence": peak, "noise_floor": peak, "harmonic_energy": E, "noise_energy": E,
         "total_energy": E}
    he, ne, te = (float(ref[k][f]) for k in ("harmonic_energy", "noise_energy", "total_energy"))
    if p.method == R.HPS:
        s["harmonic_ratio"] = 2.0 * db * float(ref["hps_rel"][f])
    else:
        s["harmonic_ratio"] = db * (inv(he) + inv(ne))
    s["voicing"] = 0.025 * s["harmonic_ratio"]
    s["periodicity"] = 2.0 * K * peak / math.sqrt(te) if te > 0 else math.inf
    n = int(ref["num_harmonics"][f])
    s["roughness"] = max(n * (n - 1) // 2, 1) * 2.0 * peak * peak
    freq = np.arange(K) * float(p.sample_rate) / float(p.window_size)
    fe = float(np.sum(ref["noise_floor"][f][(freq >= p.min_freq) & (freq <= p.max_freq)] ** 2))
    s["snr"] = db * (inv(te) + inv(fe))
    return s
