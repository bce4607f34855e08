"""sonar_xcorr_params / sonar_autocorr on the GPU against the Python checker
(tests/xcorr_params_ref.py, pinned to the C oracle in test_xcorr_params_cpu.py).  Every comparison is
bit-exact: correlations equal (NaN == NaN); peak index, lag, overlap, method and type equal; the
float metrics equal.

The shapes are the smallest that cross the kernels' boundaries: 256 lags per block and the
1,024-sample staging tile of the lag kernels; the 4,096-point LDS tile of the FFT and one or two
global passes above it (N = 2^13 .. 2^16 one pass of 1 .. 4 levels, 2^17 two passes)."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library loads HIP (one HIP runtime in the process)

import sonar
import xcorr_params_ref as R

pytestmark = pytest.mark.gpu

TILE = 4096                                                  # XCORR_FFT_TILE


@functools.lru_cache(maxsize=None)
def _data(na, nb, kind="noise"):
    rng = np.random.default_rng(na * 31 + nb)
    base = np.convolve(rng.standard_normal(max(na, nb) + 40), np.ones(5) / 5, "same")
    a, b = base[11:11 + na].copy(), base[:nb] + 0.05 * rng.standard_normal(nb)
    if kind == "constant":
        a[:] = 2.5                                           # std < 1e-10: only centred, every sum 0
    elif kind == "nan":
        b[nb // 3] = np.nan
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def _ref(na, nb, max_lag, corr_type, method, use_fft=None, kind="noise"):
    a, b = _data(na, nb, kind)
    return R.xcorr_params(a, b, max_lag, corr_type, method, use_fft)


def _check(got, ref):
    corr, lags, met = got
    assert R.same(corr, met, ref) == []
    assert np.array_equal(lags, ref["lags"])


TIME_SHAPES = [(1, 1, 5), (2, 3, 10), (64, 64, -3), (300, 257, 1000), (1500, 1100, 400)]


@pytest.mark.parametrize("corr_type", ["pearson", "ncc", "zncc"])
@pytest.mark.parametrize("na,nb,max_lag", TIME_SHAPES)
def test_time_domain_matches_checker(ctx, na, nb, max_lag, corr_type):
    """(2, 3): overlap <= 1 at an edge lag; (300, 257, 1000): L = 256, 513 lags, three lag blocks;
    (1500, 1100, 400) crosses the 1,024-sample tile (use_fft 0: NewCrossCorrelationWithParams)."""
    a, b = _data(na, nb)
    _check(ctx.xcorr_params(a, b, max_lag, corr_type, "time"), _ref(na, nb, max_lag, corr_type, "time"))


@pytest.mark.parametrize("corr_type", ["pearson", "ncc", "zncc"])
@pytest.mark.parametrize("kind", ["constant", "nan"])
def test_time_domain_constant_and_nan_inputs(ctx, kind, corr_type):
    a, b = _data(300, 257, kind)
    ref = _ref(300, 257, 40, corr_type, "time", None, kind)
    _check(ctx.xcorr_params(a, b, 40, corr_type, "time"), ref)
    if kind == "constant":
        assert np.all(ref["corr"] == 0.0)
    else:
        assert np.all(np.isnan(ref["corr"])) and ref["metrics"]["p_value"] == 0.5


@pytest.mark.parametrize("na,nb,max_lag", TIME_SHAPES)
def test_ncc_time_domain_is_sonar_ncc(ctx, na, nb, max_lag):
    a, b = _data(na, nb)
    corr, _, met = ctx.xcorr_params(a, b, max_lag, "ncc", "time")
    c0, m0 = ctx.ncc(a, b, max_lag)
    assert np.array_equal(corr, c0)
    assert all(met[k] == v for k, v in m0.items())
    assert met["method"] == 0 and met["type"] == 3


def test_types_and_methods_that_fall_through(ctx):
    a, b = _data(300, 257)
    ref = _ref(300, 257, 1000, "pearson", "time")
    for t in ("spearman", "kendall", 9):
        corr, _, met = ctx.xcorr_params(a, b, 1000, t, "time")
        assert np.array_equal(corr, ref["corr"]) and met["type"] == (t if isinstance(t, int) else R.TYPES[t])
    for t in ("pearson", "zncc"):
        _check(ctx.xcorr_params(a, b, 1000, t, "sliding"), _ref(300, 257, 1000, t, "sliding"))
    for use_fft in (False, True):                            # 300 samples: the switch does not fire
        with pytest.raises(sonar.SonarError, match="unsupported correlation method") as e:
            ctx.xcorr_params(a, b, 10, "pearson", 7, use_fft=use_fft)
        assert e.value.code == sonar.ERR_INVALID
    with pytest.raises(sonar.SonarError, match="empty signals provided") as e:
        ctx.xcorr_params(np.zeros(0), b, 10, "pearson", 7)
    assert e.value.code == sonar.ERR_EMPTY
    a2, b2 = _data(1001, 40)                                 # method 7 with use_fft and n > 1000: the FFT runs
    _check(ctx.xcorr_params(a2, b2, 10, "pearson", 7, use_fft=True), _ref(1001, 40, 10, "pearson", 7, True))


def test_fft_limit_is_reported(ctx):
    d = torch.zeros(8, dtype=torch.float64, device="cuda")  # the lengths are refused before anything is read
    with pytest.raises(sonar.SonarError, match="exceeds the FFT limit") as e:
        ctx.xcorr_params_device(d.data_ptr(), (1 << 21) + 1, d.data_ptr(), (1 << 21) + 1, 5, "pearson", "frequency")
    assert e.value.code == sonar.ERR_UNSUPPORTED


# (na, nb) -> N: 1, 2, 8; na + nb - 1 = TILE exactly and TILE + 1 (one global pass of one level);
# 2^14 .. 2^16 (one pass of 2, 3, 4 levels); unequal lengths both ways
FFT_SHAPES = [(1, 1), (1, 2), (2, 1), (3, 5), (2048, 2049), (2049, 2049), (700, 3397), (3500, 598), (9000, 5000),
              (10000, 20000), (40000, 20000)]


@pytest.mark.parametrize("max_lag", [0, 7, 10**6])
@pytest.mark.parametrize("na,nb", FFT_SHAPES)
def test_frequency_domain_matches_checker(ctx, na, nb, max_lag):
    a, b = _data(na, nb)
    ref = _ref(na, nb, max_lag, "ncc", "frequency")
    assert ref["metrics"]["method"] == 1 and ref["metrics"]["type"] == 3
    _check(ctx.xcorr_params(a, b, max_lag, "ncc", "frequency"), ref)


C3 = 51_676                                                  # energy frames of the C3 pair: N = 2^17, two global passes


@pytest.mark.parametrize("max_lag", [0, 10_335, C3])
def test_frequency_domain_c3_shape(ctx, max_lag):
    a, b = _data(C3, C3)
    _check(ctx.xcorr_params(a, b, max_lag, "pearson", "frequency"), _ref(C3, C3, max_lag, "pearson", "frequency"))


def test_frequency_domain_ignores_the_type_and_takes_nan(ctx):
    a, b = _data(700, 3397)
    ref = _ref(700, 3397, 50, "ncc", "frequency")
    for t in ("pearson", "zncc", 9):
        corr, _, met = ctx.xcorr_params(a, b, 50, t, "frequency")
        assert np.array_equal(corr, ref["corr"]) and met["peak_correlation"] == ref["metrics"]["peak_correlation"]
    a, b = _data(300, 257, "nan")
    _check(ctx.xcorr_params(a, b, 20, "pearson", "frequency"), _ref(300, 257, 20, "pearson", "frequency", None, "nan"))


@pytest.mark.parametrize("n,method", [(1000, 0), (1001, 1)])
def test_default_constructor_switches_above_1000_samples(ctx, n, method):
    a, b = _data(n, n)
    ref = R.xcorr(a, b, 25)
    got = ctx.xcorr(a, b, 25)
    _check(got, ref)
    assert got[2]["method"] == method and got[2]["type"] == 0
    if method:
        assert got[2]["peak_correlation"] > 1.0 and got[2]["p_value"] == 0.5
    else:
        assert np.all(np.abs(got[0]) <= 1.0)


@pytest.mark.parametrize("n", [900, 1001, 5000])
@pytest.mark.parametrize("corr_type,method", [("pearson", "time"), ("zncc", "sliding"), ("ncc", "frequency")])
def test_autocorr_is_xcorr_of_x_with_itself(ctx, n, corr_type, method):
    x, _ = _data(n, 1)
    got = ctx.autocorr(x, 300, corr_type, method)
    two = ctx.xcorr_params(x, x.copy(), 300, corr_type, method, use_fft=True)   # two arrays: two transforms
    assert np.array_equal(got[0], two[0], equal_nan=True) and got[2] == two[2]
    _check(got, R.autocorr(x, 300, corr_type, method))
    assert got[2]["method"] == (1 if n > 1000 or method == "frequency" else R.METHODS[method])


@pytest.mark.parametrize("corr_type,method,na,nb", [("pearson", "time", 300, 257), ("zncc", "time", 1500, 1100),
                                                    ("ncc", "frequency", 9000, 5000)])
def test_device_pointers_give_the_same_bits(ctx, corr_type, method, na, nb):
    a, b = _data(na, nb)
    corr, _, met = ctx.xcorr_params(a, b, 400, corr_type, method)
    da, db = torch.from_numpy(a.copy()).cuda(), torch.from_numpy(b.copy()).cuda()
    dc = torch.zeros(len(corr), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    dmet = ctx.xcorr_params_device(da.data_ptr(), na, db.data_ptr(), nb, 400, corr_type, method, corr_ptr=dc.data_ptr())
    assert np.array_equal(dc.cpu().numpy(), corr) and dmet == met
    assert ctx.xcorr_params_device(da.data_ptr(), na, db.data_ptr(), nb, 400, corr_type, method) == met   # null corr
    ac, _, am = ctx.autocorr(a, 400, corr_type, method)
    dac = torch.zeros(len(ac), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    amet = ctx.autocorr_device(da.data_ptr(), na, 400, corr_type, method, corr_ptr=dac.data_ptr())
    assert np.array_equal(dac.cpu().numpy(), ac) and amet == am


def test_table_cache_and_trim(ctx):
    """A second N after a first one, the first again (its table is cached), then sonar_trim and both again."""
    shapes = [(3500, 598), (9000, 5000), (3500, 598)]
    for _ in range(2):
        for na, nb in shapes:
            a, b = _data(na, nb)
            _check(ctx.xcorr_params(a, b, 7, "ncc", "frequency"), _ref(na, nb, 7, "ncc", "frequency"))
        ctx.trim()
    a, b = _data(300, 257)
    _check(ctx.xcorr_params(a, b, 1000, "pearson", "time"), _ref(300, 257, 1000, "pearson", "time"))
