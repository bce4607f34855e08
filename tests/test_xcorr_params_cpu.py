"""The parts of the full cross-correlation feature that need no GPU: the Python checker
(tests/xcorr_params_ref.py) pinned bit for bit against the C oracle where the two overlap
(NormalizedCrossCorrelation / TimeDomain; the FFT method on (x, x)), known answers for what the
oracle does not have, and the two new symbols in the header and the library."""
import ctypes
import math
import re

import numpy as np
import pytest

import oracle as O
import sonar
import xcorr_params_ref as R


def _pair(na, nb, seed=None):
    rng = np.random.default_rng(na * 7 + nb if seed is None else seed)
    return rng.standard_normal(na), rng.standard_normal(nb)


@pytest.mark.parametrize("max_lag", [0, 5, 400, 10**6])
@pytest.mark.parametrize("na,nb", [(1, 1), (2, 3), (300, 257), (1500, 1100)])
def test_checker_equals_oracle_at_ncc_time_domain(na, nb, max_lag):
    a, b = _pair(na, nb)
    rc, rm = O.ncc(a, b, max_lag)
    got = R.xcorr_params(a, b, max_lag, "ncc", "time")
    assert np.array_equal(got["corr"], rc)
    for k, v in rm.items():
        g = got["metrics"][k]
        assert g == v or (math.isnan(g) and math.isnan(v)), (k, g, v)
    assert got["metrics"]["method"] == 0 and got["metrics"]["type"] == 3
    assert np.array_equal(got["lags"], np.arange(len(rc)) - len(rc) // 2)


@pytest.mark.parametrize("n", [3, 1000, 2048, 2049])
def test_checker_fft_equals_oracle_autocorr_fft(n):
    x = np.random.default_rng(n).standard_normal(n)
    for max_lag in (n - 1, 10**6, 7):                        # the full-lag range, beyond it, a few lags
        got = R.xcorr_params(x, x, max_lag, "pearson", "frequency")
        assert np.array_equal(got["corr"], O.autocorr_fft(x, max_lag))
        assert got["metrics"]["method"] == 1


@pytest.mark.parametrize("na,nb", [(1, 1), (5, 3), (100, 157), (700, 325)])
def test_fft_correlations_are_the_direct_sums(na, nb):
    """real(ifft(fft(x) conj(fft(y))))[lag] = sum_k x[k + lag] y[k], for the z-scored inputs; the bound
    is the one test_autocorr_fft_matches_direct_sums holds the oracle to: 1e-10 of the largest value."""
    a, b = _pair(na, nb)
    x, y = R.normalize(a), R.normalize(b)
    got = R.xcorr_params(a, b, 10**6, "zncc", "frequency")
    L = min(na, nb) - 1
    assert len(got["corr"]) == 2 * L + 1
    direct = np.array([math.fsum(x[k + lag] * y[k] for k in range(nb) if 0 <= k + lag < na)
                       for lag in range(-L, L + 1)])
    assert np.max(np.abs(got["corr"] - direct)) <= 1e-10 * max(np.max(np.abs(direct)), 1.0)


@pytest.mark.parametrize("d", [0, 3, 17])
def test_pearson_of_a_delayed_copy_peaks_at_the_delay(d):
    rng = np.random.default_rng(d)
    base = rng.standard_normal(400 + d)
    a, b = base[d:d + 400], base[:400]                       # b[i] = a[i - d]: the overlap windows coincide at lag d
    got = R.xcorr_params(a, b, 50, "pearson", "time")
    m = got["metrics"]
    assert m["peak_lag"] == d and m["peak_index"] == 50 + d and m["overlap_length"] == 400 - d
    assert abs(m["peak_correlation"] - 1.0) <= 1e-12 and m["peak_correlation"] <= 1.0
    assert np.all(np.abs(got["corr"]) <= 1.0)
    assert m["p_value"] == 0.01                              # t large, or +Inf at exactly 1.0


def test_default_object_changes_meaning_between_1000_and_1001_samples():
    for n, method in ((1000, 0), (1001, 1)):
        a, b = _pair(n, n, seed=4)
        b = np.roll(a, 3) + 0.01 * b
        got = R.xcorr(a, b, 20)
        m = got["metrics"]
        assert m["method"] == method and m["type"] == 0
        if method == 0:
            assert np.all(np.abs(got["corr"]) <= 1.0) and m["p_value"] == 0.01
        else:                                                # un-normalised sums: the peak is ~ the overlap count
            assert 0.9 * n < m["peak_correlation"] < 1.1 * n
            assert m["p_value"] == 0.5                       # sqrt(1 - peak^2) is NaN: every comparison false


def test_types_and_methods_that_fall_through():
    a, b = _pair(120, 90)
    ref = R.xcorr_params(a, b, 30, "pearson", "time")
    for t in ("spearman", "kendall", 9):
        got = R.xcorr_params(a, b, 30, t, "time")
        assert np.array_equal(got["corr"], ref["corr"], equal_nan=True)
        assert got["metrics"]["type"] == (t if isinstance(t, int) else R.TYPES[t])
    for t in ("pearson", "ncc", "zncc"):
        s, u = R.xcorr_params(a, b, 30, t, "sliding"), R.xcorr_params(a, b, 30, t, "time")
        assert np.array_equal(s["corr"], u["corr"]) and s["metrics"]["method"] == 2
    with pytest.raises(ValueError, match="unsupported correlation method"):
        R.xcorr_params(a, b, 30, "pearson", 7, use_fft=False)
    with pytest.raises(ValueError, match="unsupported correlation method"):
        R.xcorr_params(a, b, 30, "pearson", 7, use_fft=True)    # 120 samples: the switch does not fire
    with pytest.raises(ValueError, match="empty signals provided"):
        R.xcorr_params(np.zeros(0), b, 30, "pearson", 7)
    big, _ = _pair(1001, 1)
    got = R.xcorr_params(big, b, 30, "pearson", 7, use_fft=True)
    assert got["metrics"]["method"] == 1
    assert np.array_equal(got["corr"], R.xcorr_params(big, b, 30, "ncc", "frequency")["corr"])


def test_zncc_is_ncc_of_the_mean_subtracted_z_scores():
    a, b = _pair(200, 140)
    a += 3.0
    got = R.xcorr_params(a, b, 60, "zncc", "time")
    x, y = R.subtract_mean(R.normalize(a)), R.subtract_mean(R.normalize(b))
    want = np.array([R.ncc_at_lag(x, y, lag) for lag in range(-60, 61)])
    assert np.array_equal(got["corr"], want)
    # per lag, spelled out as Go does it
    for lag in (-60, -1, 0, 17):
        s1, e1, s2, e2 = R.overlap_region(200, 140, lag)
        sm = q1 = q2 = 0.0
        for i in range(min(e1 - s1, e2 - s2)):
            v1, v2 = float(x[s1 + i]), float(y[s2 + i])
            sm += v1 * v2
            q1 += v1 * v1
            q2 += v2 * v2
        assert got["corr"][lag + 60] == sm / math.sqrt(q1 * q2)


def test_pearson_edge_rules():
    assert np.array_equal(R.xcorr_params([1.0, 2.0], [3.0, 1.0], 10)["corr"], [0.0, -1.0, 0.0])   # overlap 1 at +-1
    edge = R.xcorr_params([1.0, 2.0], [3.0, 1.0, 2.0], 10)["corr"]                      # overlaps 1, 2, 2
    assert edge[0] == 0.0 and abs(edge[2] - 1.0) <= 1e-15 and edge[2] <= 1.0
    const = R.xcorr_params(np.full(50, 2.5), _pair(50, 50)[1], 10)
    assert np.all(const["corr"] == 0.0) and const["metrics"]["peak_index"] == 0      # denominator < 1e-10
    a, b = _pair(40, 40)
    a[7] = math.nan
    got = R.xcorr_params(a, b, 5)
    assert np.all(np.isnan(got["corr"])) and math.isnan(got["metrics"]["peak_correlation"])   # the clamp lets NaN through
    assert got["metrics"]["p_value"] == 0.5


def test_autocorr_constructor_keeps_the_fft_switch():
    x = _pair(1200, 1)[0]
    got = R.autocorr(x, 64, "ncc", "time")
    assert got["metrics"]["method"] == 1 and got["metrics"]["type"] == 3
    assert np.array_equal(got["corr"], O.autocorr_fft(x, 64))
    small = R.autocorr(x[:900], 64, "ncc", "time")
    assert small["metrics"]["method"] == 0
    assert np.array_equal(small["corr"], O.ncc(x[:900], x[:900], 64)[0])


def test_new_symbols_are_declared_and_exported():
    names = ["sonar_xcorr_params", "sonar_autocorr"]
    with open(sonar._abi.HEADER) as f:
        text = f.read()
    lib = ctypes.CDLL(sonar.LIB_PATH)
    for n in names:
        assert n in sonar.EXPORTED_SYMBOLS
        assert re.search(r"^int " + n + r"\(", text, re.M)
        assert hasattr(lib, n)
    for k, v in {"SONAR_CORR_PEARSON": 0, "SONAR_CORR_SPEARMAN": 1, "SONAR_CORR_KENDALL": 2, "SONAR_CORR_NCC": 3,
                 "SONAR_CORR_ZNCC": 4, "SONAR_CORR_TIME_DOMAIN": 0, "SONAR_CORR_FREQUENCY_DOMAIN": 1,
                 "SONAR_CORR_SLIDING_WINDOW": 2}.items():
        assert re.search(r"\b" + k + r" = " + str(v) + r"\b", text), k
    assert sonar.CORR_TYPES == R.TYPES and sonar.CORR_METHODS == R.METHODS
    assert sonar.abi_version() == 4
