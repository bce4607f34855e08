"""The checker of sonar_xcorr_params / sonar_autocorr: a float64 restatement of the reference's
cross-correlation type for every correlation type, method and constructor (test infrastructure,
never the product; the C oracle has NormalizedCrossCorrelation / TimeDomain and the FFT method on
(x, x), and is pinned against this file in test_xcorr_params_cpu.py).

  NewCrossCorrelation, NewCrossCorrelationWithParams, Compute, computeTimeDomain, computeFFT,
  computeSlidingWindow, computeAtLag, pearsonCorrelation, normalizedCrossCorrelation,
  zeroNormalizedCrossCorrelation, calculateOverlapRegion, calculateActualMaxLag, normalize,
  subtractMean, findPeak, calculatePValue, calculateSNR, calculateSharpness, findSecondPeak,
  calculatePeakToSidelobe, calculateOverlapLength, AutoCorrelation
                                                (algorithms/stats/correlation.go:103-690)
  clampCorrelation, nextPowerOf2, fft, ifft     (correlation.go:694-774)

Sums are np.add.accumulate from 0.0 (strictly sequential, Go's index order); elementwise numpy *, +,
-, / are unfused and correctly rounded.  The FFT is the recursion unrolled one level at a time, the
twiddles of every level from libm's sincos of Go's own angle -2 pi i / n.  sincos, not math.cos and
math.sin: the C oracle's cos(th), sin(th) pair compiles to one sincos call, and glibc's sincos differs
from its sin / cos in the last bit for a few angles (86 of the 65,536 at n = 2^17), so only sincos
keeps this file bit-identical to the oracle.  (Go's own math.Sincos is a third implementation; libm
is the project's stand-in for it, as in the oracle.)"""
import ctypes
import ctypes.util
import functools
import math

import numpy as np

TYPES = {"pearson": 0, "spearman": 1, "kendall": 2, "ncc": 3, "zncc": 4}
METHODS = {"time": 0, "frequency": 1, "sliding": 2}
KEYS = ["peak_correlation", "peak_lag", "peak_index", "p_value", "snr", "sharpness", "second_peak",
        "peak_to_sidelobe", "overlap_length", "num_lags", "method", "type"]
FFT_THRESHOLD = 1000
MIN_STD = 1e-10


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _sum(v):
    """var s float64; for _, x := range v { s += x }"""
    return float(np.add.accumulate(np.concatenate(([0.0], v)))[-1])


def _sqrt(x):
    return math.sqrt(x) if x >= 0 else math.nan           # math.Sqrt: NaN for negative and NaN


def _log10(x):
    if x != x:
        return math.nan
    return -math.inf if x == 0 else math.log10(x)         # math.Log10(0) = -Inf


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))        # IEEE: x / 0 = +-Inf, 0 / 0 = NaN


def normalize(x):
    """normalize (:464-501): zero mean, unit population std; a constant signal is only centred."""
    x = _f64(x)
    n = len(x)
    mean = _sum(x) / n
    d = x - mean
    sd = _sqrt(_sum(d * d) / n)
    return d if sd < MIN_STD else d / sd


def subtract_mean(x):
    """subtractMean (:504-523)"""
    return x - _sum(x) / len(x)


def overlap_region(l1, l2, lag):
    """calculateOverlapRegion (:421-449)"""
    if lag >= 0:
        return 0, min(l1, l2 - lag), lag, l2
    return -lag, l1, 0, min(l2, l1 + lag)


def actual_max_lag(max_lag, l1, l2):
    return max(0, min(max_lag, l1 - 1, l2 - 1))


def _overlap(x, y, lag):
    s1, e1, s2, e2 = overlap_region(len(x), len(y), lag)
    ov = min(e1 - s1, e2 - s2)
    return ov, x[s1:s1 + max(ov, 0)], y[s2:s2 + max(ov, 0)]


def ncc_at_lag(x, y, lag):
    """normalizedCrossCorrelation (:373-409)"""
    ov, u, v = _overlap(x, y, lag)
    if ov <= 0:
        return 0.0
    dn = _sqrt(_sum(u * u) * _sum(v * v))
    return 0.0 if dn < MIN_STD else _div(_sum(u * v), dn)


def pearson_at_lag(x, y, lag):
    """pearsonCorrelation (:314-370): the means of the overlap, then the centred sums"""
    ov, u, v = _overlap(x, y, lag)
    if ov <= 1:
        return 0.0
    d1, d2 = u - _sum(u) / ov, v - _sum(v) / ov
    dn = _sqrt(_sum(d1 * d1) * _sum(d2 * d2))
    if dn < MIN_STD:
        return 0.0
    c = _div(_sum(d1 * d2), dn)
    return 1.0 if c > 1.0 else -1.0 if c < -1.0 else c      # clampCorrelation: NaN passes


def time_domain(a, b, max_lag, corr_type):
    """computeTimeDomain (:203-228) with computeAtLag's dispatch (:300-311)"""
    x, y = normalize(a), normalize(b)
    L = actual_max_lag(max_lag, len(x), len(y))
    if corr_type == TYPES["ncc"]:
        f = ncc_at_lag
    elif corr_type == TYPES["zncc"]:                         # :412-418, the same subtraction at every lag
        x, y = subtract_mean(x), subtract_mean(y)
        f = ncc_at_lag
    else:
        f = pearson_at_lag
    return np.array([f(x, y, i - L) for i in range(2 * L + 1)], dtype=np.float64), L


def next_pow2(n):
    p = 1
    while p < n:
        p <<= 1
    return p


_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.sincos.argtypes = [ctypes.c_double, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
_libm.sincos.restype = None


@functools.lru_cache(maxsize=None)
def _twiddles(n):
    """cmplx.Exp(complex(0, -2 pi i / n)) for i < n / 2 (:748): (cos, sin) of Go's angle"""
    c, s = np.zeros(n // 2), np.zeros(n // 2)
    sv, cv = ctypes.c_double(), ctypes.c_double()
    for i in range(n // 2):
        _libm.sincos(-2.0 * math.pi * float(i) / float(n), ctypes.byref(sv), ctypes.byref(cv))
        c[i], s[i] = cv.value, sv.value
    return c, s


def _bit_reverse(N):
    idx = np.zeros(N, dtype=np.int64)
    bits = N.bit_length() - 1
    for k in range(bits):
        idx |= ((np.arange(N) >> k) & 1) << (bits - 1 - k)
    return idx


def go_fft(re, im):
    """fft (:726-754).  The recursion's leaves are the input in bit-reversed order; its combine step
    at size n acts on every group of n consecutive points at once."""
    N = len(re)
    perm = _bit_reverse(N)
    re, im = re[perm].copy(), im[perm].copy()
    n = 2
    while n <= N:
        h = n // 2
        c, s = _twiddles(n)
        R, I = re.reshape(-1, n), im.reshape(-1, n)
        er, ei, odr, odi = R[:, :h], I[:, :h], R[:, h:], I[:, h:]
        tr = c * odr - s * odi
        ti = c * odi + s * odr
        re = np.concatenate((er + tr, er - tr), axis=1).reshape(-1)
        im = np.concatenate((ei + ti, ei - ti), axis=1).reshape(-1)
        n *= 2
    return re, im


def frequency_domain(a, b, max_lag):
    """computeFFT (:231-291): the correlation type is not consulted"""
    x, y = normalize(a), normalize(b)
    n1, n2 = len(x), len(y)
    N = next_pow2(n1 + n2 - 1)
    p1, p2 = np.zeros(N), np.zeros(N)
    p1[:n1], p2[:n2] = x, y
    ar, ai = go_fft(p1, np.zeros(N))
    br, bi = go_fft(p2, np.zeros(N))
    c, d = br, -bi                                           # cmplx.Conj(fft2[i])
    pr, pi = ar * c - ai * d, ar * d + ai * c                # Go's complex product
    yr, _ = go_fft(pr, -pi)                                  # ifft: conjugate, fft, conjugate / n
    L = actual_max_lag(max_lag, n1, n2)
    lags = np.arange(-L, L + 1)
    return yr[np.where(lags >= 0, lags, N + lags)] / float(N), L


def metrics(corr, L, n1, n2):
    """findPeak .. calculateOverlapLength (:526-667) -> the first ten KEYS"""
    nl = len(corr)
    a = np.abs(corr)
    pidx = 0 if a[0] != a[0] else int(np.nanargmax(a))       # strict >: the first maximum; NaN never wins
    pk = float(corr[pidx])
    n = min(n1, n2)
    pv = 1.0
    if n > 2:
        t = _div(abs(pk) * math.sqrt(float(n - 2)), _sqrt(1.0 - pk * pk))
        pv = 0.01 if t > 2.0 else 0.05 if t > 1.5 else 0.1 if t > 1.0 else 0.5
    dist = np.abs(np.arange(nl) - pidx)
    snr = 0.0
    noise = corr[dist > 5]
    if len(noise):
        lvl = _sqrt(_sum(noise * noise) / float(len(noise)))
        snr = math.inf if lvl < 1e-10 else 20.0 * _log10(_div(abs(pk), lvl))
    sharp = 0.0
    if nl >= 3 and 0 < pidx < nl - 1:
        sharp = -float(corr[pidx + 1] - 2 * corr[pidx] + corr[pidx - 1])
    others = a.copy()
    others[pidx] = math.nan
    second = 0.0
    if np.any(others > 0):
        second = float(corr[int(np.nanargmax(others))])
    side = a[dist > 10]
    ms = float(np.nanmax(side)) if np.any(side > 0) else 0.0
    psl = math.inf if ms < 1e-10 else 20.0 * _log10(_div(abs(pk), ms))
    plag = pidx - L
    s1, e1, s2, e2 = overlap_region(n1, n2, plag)
    return [pk, plag, pidx, pv, snr, sharp, second, psl, min(e1 - s1, e2 - s2), nl]


def xcorr_params(a, b, max_lag, corr_type="pearson", method="time", use_fft=None):
    """CrossCorrelation.Compute (:131-200) -> {"corr", "lags", "metrics"}.  use_fft None is
    NewCrossCorrelationWithParams' rule; ValueError carries Go's error text."""
    a, b = _f64(a), _f64(b)
    t = TYPES[corr_type] if isinstance(corr_type, str) else int(corr_type)
    m = METHODS[method] if isinstance(method, str) else int(method)
    if use_fft is None:
        use_fft = m == METHODS["frequency"]
    if len(a) == 0 or len(b) == 0:
        raise ValueError("empty signals provided")
    if use_fft and (len(a) > FFT_THRESHOLD or len(b) > FFT_THRESHOLD):
        m = METHODS["frequency"]
    if m == METHODS["frequency"]:
        corr, L = frequency_domain(a, b, max_lag)
    elif m in (METHODS["time"], METHODS["sliding"]):
        corr, L = time_domain(a, b, max_lag, t)
    else:
        raise ValueError("unsupported correlation method")
    met = metrics(corr, L, len(a), len(b)) + [m, t]
    return {"corr": corr, "lags": np.arange(-L, L + 1), "metrics": dict(zip(KEYS, met))}


def xcorr(a, b, max_lag):
    """NewCrossCorrelation(max_lag).Compute(a, b)"""
    return xcorr_params(a, b, max_lag, "pearson", "time", use_fft=True)


def autocorr(x, max_lag, corr_type="pearson", method="time"):
    """NewAutoCorrelation(max_lag) [+ SetParameters].Compute(x): useFFT stays true"""
    return xcorr_params(x, x, max_lag, corr_type, method, use_fft=True)


def same(got_corr, got_metrics, ref):
    """Differences between a library result and a checker result, bit for bit (NaN equals NaN)."""
    bad = []
    if not np.array_equal(np.asarray(got_corr), ref["corr"], equal_nan=True):
        bad.append("corr")
    for k in KEYS:
        g, r = got_metrics[k], ref["metrics"][k]
        if not (g == r or (g != g and r != r)):
            bad.append((k, g, r))
    return bad
