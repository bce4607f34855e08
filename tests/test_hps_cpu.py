"""CPU: the harmonic product checker (tests/hps_ref.py) against known answers worked out by hand from
harmonic_product.go, and the host-only side of the library (sonar_hps_bins,
sonar_hps_optimal_harmonics, sonar_hps_plan) against the checker.  Everything here is integers and
exact float64 values, so every comparison is an equality."""
import math

import numpy as np
import pytest

import hps_ref as R
import sonar


# ---- checker known answers ---------------------------------------------------------------------

def test_comb_gives_its_base_bin():
    # window_size = sample_rate: bin i is i Hz.  Ten partials of bin 12 over a floor of 0.01.
    row = np.full(257, 0.01)
    for k in range(1, 11):
        row[12 * k] = 0.8 ** k
    got = R.estimate_row(R.analyzer(256, 10, 5.0, 100.0), row, 256)
    assert got["f0_bin"] == 12 and got["f0"] == 12.0
    assert got["strengths"] == [0.8 ** k for k in range(1, 11)]              # integer indices: frac is 0
    comb = sum(0.64 ** k for k in range(1, 11))                              # over comb + 247 floor bins of 1e-4
    assert abs(got["confidence"] - comb / (comb + 247 * 1e-4)) < 1e-12
    hps = R.compute_hps(R.analyzer(256, 10), row)
    want = 1.0
    for k in range(1, 11):
        want = want * ((0.8 ** k) * (0.8 ** k))                              # left to right, one rounding each
    assert hps[12] == want


def test_harmonic_above_K_is_a_no_op():
    row = [1.0, 2.0, 3.0, 4.0]
    assert R.compute_hps(R.analyzer(64, 2), row) == [1.0, 36.0, 0.0, 0.0]    # L = 2: p[1] * p[2], zeros from L on
    assert R.compute_hps(R.analyzer(64, 4), row) == [1.0, 0.0, 0.0, 0.0]     # h = 3, 4: L = 1
    assert R.compute_hps(R.analyzer(64, 10), row) == R.compute_hps(R.analyzer(64, 4), row)   # h = 5..10: L = 0
    assert R.downsample_spectrum(row, 5) == []
    assert R.compute_hps(R.analyzer(64, 1), row) == [1.0, 4.0, 9.0, 16.0]    # the power spectrum
    assert R.compute_hps(R.analyzer(64, -3), row) == [1.0, 4.0, 9.0, 16.0]
    # ComputeHPSWithInterpolation reads p at bin / h, the sub-harmonics: 1, 4 * 2.5, 9 * 4, 16 * 6.5
    assert R.compute_hps_interpolated(R.analyzer(64, 2), row) == [1.0, 10.0, 36.0, 104.0]
    # and it has no such rule: h = 5 multiplies bin 0 by p[0] and the rest by values below p[1]
    a, b = R.compute_hps_interpolated(R.analyzer(64, 4), row), R.compute_hps_interpolated(R.analyzer(64, 5), row)
    assert a[0] == b[0] and all(x != y for x, y in zip(a[1:], b[1:]))


def test_zero_region_multiplies():
    hps = R.compute_hps(R.analyzer(64, 2), [1.0, 1.0, math.inf, 1.0])
    assert hps[0] == 1.0 and hps[1] == math.inf and math.isnan(hps[2]) and hps[3] == 0.0   # Inf * 0.0
    hps = R.compute_hps(R.analyzer(64, 2), [1.0, 1.0, 1.0, math.nan])
    assert hps[:3] == [1.0, 1.0, 0.0] and math.isnan(hps[3])
    # a NaN is never the peak, an Inf is
    got = R.estimate_row(R.analyzer(64, 2, 1.0, 3.0), [1.0, 1.0, math.inf, 1.0], 64)
    assert got["f0_bin"] == 1 and got["f0"] == 1.0


def test_equal_maxima_resolve_to_the_lower_bin():
    row = np.full(33, 0.5)
    row[[7, 19]] = 2.0
    got = R.estimate_row(R.analyzer(64, 1, 1.0, 30.0), row, 64)
    assert got["f0_bin"] == 7 and got["hps"][7] == got["hps"][19] == 4.0
    assert R.estimate_row(R.analyzer(64, 1, 8.0, 30.0), row, 64)["f0_bin"] == 19


def test_subnormal_products_survive():
    row = np.full(65, 1e-16)
    row[5] = 3e-16
    got = R.estimate_row(R.analyzer(64, 10, 1.0, 40.0), row, 64)
    # bins 1..6 have all ten harmonics in range: (1e-32)^10 = 1e-320, and bin 1 has p[5] = 9e-32 among them
    assert got["hps"][1] == 9e-320 and got["hps"][5] == 9e-320 and got["hps"][2] == 1e-320
    assert 0.0 < got["hps"][1] < 2.3e-308                                    # a subnormal, not zero
    assert got["f0_bin"] == 1 and got["f0"] == 1.0


def test_empty_ranges_give_bin_0():
    row = np.linspace(1.0, 2.0, 65)
    for lo, hi in [(50.0, 10.0), (0.0, 0.0), (100.0, 200.0)]:               # min > max; max_bin 0; min_bin past K - 1
        got = R.estimate_row(R.analyzer(64, 3, lo, hi), row, 64)
        assert got["f0_bin"] == 0 and got["f0"] == 0.0 and got["confidence"] == 0.0
        assert got["strengths"] == [0.0, 0.0, 0.0]
    assert R.estimate_row(R.analyzer(64, 3, 1.0, 40.0), np.zeros(65), 64)["f0_bin"] == 0   # nothing above 0.0
    assert R.estimate_row(R.analyzer(64, 3, 1.0, 40.0), [], 64)["f0_bin"] == 0


def test_strength_index_is_not_bin_times_h():
    # 44.1 Hz per bin: float64(7) * 44.1 / 44.1 is 6.999999999999999, so the first harmonic of bin 7 is
    # interpolated between bins 6 and 7 with frac just under 1 and is not mag[7]
    hp = R.analyzer(44100, 3, 300.0, 320.0)
    res = 44100.0 / 1000.0
    assert (7.0 * res) / res < 7.0 and int((7.0 * res) / res) == 6
    row = np.full(501, 0.25)
    row[7], row[14], row[21] = 1.0, 0.5, 0.125
    got = R.estimate_row(hp, row, 1000)
    assert got["f0_bin"] == 7 and got["f0"] == 7.0 * res
    frac = (7.0 * res) / res - 6.0
    assert got["strengths"][0] == 0.25 + frac * (1.0 - 0.25) and got["strengths"][0] != 1.0
    assert got["strengths"][1] == R.interpolate_spectrum(list(row), (7.0 * res * 2.0) / res)
    # past the row: 0
    assert R.compute_harmonic_strength(R.analyzer(44100, 3), row, 200.0 * res, 1000) == [0.25, 0.25, 0.0]
    assert R.interpolate_spectrum([1.0, 2.0], 1.0) == 0.0 and R.interpolate_spectrum([1.0, 2.0], 0.5) == 1.5
    assert R.interpolate_spectrum([3.0], 0.0) == 0.0


def test_harmonicity_of_zero_harmonics_and_zero_energy():
    row = np.zeros(65)
    row[4] = 1.0
    assert R.estimate_row(R.analyzer(64, 0, 1.0, 40.0), row, 64)["confidence"] == 0.0     # no strengths
    got = R.estimate_row(R.analyzer(64, 1, 1.0, 40.0), row, 64)
    assert got["f0_bin"] == 4 and got["confidence"] == 1.0 and got["strengths"] == [1.0]
    assert R.compute_harmonicity(R.analyzer(64, 2), np.zeros(65), 4.0, 64) == 0.0


# ---- the library's host-only entries against the checker ---------------------------------------

RES_2048 = 44100.0 / 2048.0      # 21.533203125, exact in binary


@pytest.mark.parametrize("sr,ws,K,lo,hi", [
    (44100, 2048, 1025, 80.0, 2000.0),                       # the music extractor's: bins 3..92
    (44100, 2048, 1025, 4 * RES_2048, 10 * RES_2048),        # exact bin multiples truncate to themselves
    (44100, 2048, 1025, np.nextafter(4 * RES_2048, 0.0), np.nextafter(10 * RES_2048, 0.0)),   # one ulp below: 3, 9
    (44100, 1000, 501, 7 * 44.1, 10 * 44.1),                 # 308.7 / 44.1 is 6.999999999999999: bin 6
    (44100, 2048, 1025, 0.0, 2000.0),                        # min_bin raised to 1
    (44100, 2048, 1025, 10.0, 30000.0),                      # both clamps
    (44100, 2048, 64, 80.0, 2000.0),                         # max_bin lowered to K - 1
    (44100, 2048, 3, 80.0, 2000.0),                          # min_bin 3 > max_bin 2
    (44100, 2048, 1025, 500.0, 100.0),                       # empty
    (44100, 2048, 0, 80.0, 2000.0),                          # K == 0: max_bin -1
    (64, 64, 65, 1.0, 40.0), (8000, 128, 65, -0.0, 1e9), (1, 2147483647, 8192, 0.0, 1.0),
])
def test_bins_match_checker(sr, ws, K, lo, hi):
    assert sonar.hps_bins(sr, ws, K, lo, hi) == R.scan_bins(R.analyzer(sr, 10, lo, hi), K, ws)


def test_bins_known_values():
    assert sonar.hps_bins(44100, 2048, 1025) == (3, 92)
    assert sonar.hps_bins(44100, 2048, 1025, 4 * RES_2048, 10 * RES_2048) == (4, 10)
    assert sonar.hps_bins(44100, 1000, 501, 7 * 44.1, 10 * 44.1)[0] == 6
    assert sonar.hps_bins(44100, 2048, 64, 0.0, 1e6) == (1, 63)


@pytest.mark.parametrize("args", [(0, 2048, 65, 80.0, 2000.0), (-1, 2048, 65, 80.0, 2000.0), (44100, 0, 65, 80.0, 2000.0),
                                  (44100, 2048, 65, math.nan, 2000.0), (44100, 2048, 65, 80.0, math.inf),
                                  (44100, 2048, 65, -1.0, 2000.0), (44100, 2048, 65, 80.0, -2000.0),
                                  (44100, 2048, 65, 80.0, 1e300), (1, 2147483647, 65, 1.0, 2.0),
                                  (44100, 2048, 65, 2147483648.0 * RES_2048, 2000.0)])
def test_bins_unsupported(args):
    with pytest.raises(sonar.SonarError) as e:
        sonar.hps_bins(*args)
    assert e.value.code == sonar.ERR_UNSUPPORTED
    sr, ws, K, lo, hi = args
    if sr > 0 and ws > 0 and lo >= 0 and hi >= 0:            # the checker refuses the same conversions
        with pytest.raises(ValueError):
            R.scan_bins(R.analyzer(sr, 10, lo, hi), K, ws)


def test_bins_largest_quotient_that_fits():
    assert sonar.hps_bins(44100, 2048, 8192, 0.0, 2147483647.0 * RES_2048) == (1, 8191)
    with pytest.raises(sonar.SonarError) as e:
        sonar.hps_bins(44100, 2048, -1, 80.0, 2000.0)
    assert e.value.code == sonar.ERR_INVALID


@pytest.mark.parametrize("sr,min_f0,want", [(44100, 80.0, 5), (16000, 1000.0, 5), (16000, 1000.1, 6), (1000, 100.0, 4),
                                            (1000, 125.0, 3), (1000, 125.1, 2), (1000, 166.0, 2), (1000, 600.0, 2),
                                            (8000, 571.4, 6), (8000, 571.5, 5)])
def test_optimal_harmonics(sr, min_f0, want):
    assert R.optimal_num_harmonics(R.analyzer(sr, 10, min_f0)) == want       # m: 275, 8, 7, 5, 4, 3, 3, 0, 7, 6
    assert sonar.hps_optimal_harmonics(sr, min_f0) == want


@pytest.mark.parametrize("sr,min_f0", [(0, 80.0), (-5, 80.0), (44100, 0.0), (44100, -80.0), (44100, math.nan),
                                       (44100, math.inf), (44100, 1e-6)])
def test_optimal_harmonics_unsupported(sr, min_f0):
    with pytest.raises(sonar.SonarError) as e:
        sonar.hps_optimal_harmonics(sr, min_f0)
    assert e.value.code == sonar.ERR_UNSUPPORTED


@pytest.mark.parametrize("n,W,H", [(140_000, 128, 1), (26_460_000, 2048, 512), (2048, 2048, 512), (5000, 1000, 250),
                                   (100, 2, 1), (8192, 8192, 1)])
def test_plan_is_the_hpcp_plan(n, W, H):
    plan = sonar.hps_plan(n, W, H)
    assert plan == sonar.hpcp_plan(n, W, H)
    assert plan["frames"] == (n - W) // H + 1
    assert plan["n_chunks"] == -(-plan["frames"] // plan["chunk_frames"])


@pytest.mark.parametrize("n,W,H,code", [(0, 1024, 256, sonar.ERR_EMPTY), (1000, 0, 256, sonar.ERR_INVALID),
                                        (1000, 1024, 0, sonar.ERR_INVALID), (768, 1024, 256, sonar.ERR_TOO_SHORT),
                                        (10000, 8193, 256, sonar.ERR_UNSUPPORTED), (10, 1, 1, sonar.ERR_UNSUPPORTED)])
def test_plan_errors(n, W, H, code):
    with pytest.raises(sonar.SonarError) as e:
        sonar.hps_plan(n, W, H)
    assert e.value.code == code


def test_window_is_the_unnormalised_symmetric_hann():
    w = R.apply_window([1.0] * 9)
    assert w[0] == 0.0 and w[4] == 1.0 and abs(w[8]) < 1e-30 and w[1] == 0.5 * (1.0 - math.cos(2.0 * math.pi / 8.0))
    assert np.allclose(w, np.hanning(9), rtol=0, atol=1e-15)
