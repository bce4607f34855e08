"""CPU: the HPCP / spectral peaks checker (tests/hpcp_ref.py) against known answers, the two forms of
the distance rule against each other, MaxShifted's identity, and the host-only side of the library
(sonar_hpcp_table, sonar_hpcp_plan, sonar_spectral_peaks_width, the defaults) against the checker.

Table bounds: window weights pass through log2 and cos, so 1e-12 absolute (the project's bound for
values through log / exp); factors are exact; the (row, wrapped_bin) sequences are identical except
that an entry whose checker weight is <= 1e-12 (a cosine window's edge, where `distance <= w/2`
hangs on the last bit of log2) may be on one side only.  For the weight type "none" the edge weight
is 1, so that case first asserts on the checker alone that every decision of every used bin is at
least 1e-9 from its boundary, then requires identical sequences."""
import math

import numpy as np
import pytest

import hpcp_ref as R
import sonar


def _spectrum(K, peaks):
    m = np.zeros(K)
    for b, v in peaks:
        m[b] = v
    return m


# ---- checker known answers ---------------------------------------------------------------------

def test_one_440_peak_is_bin_9():
    # window_size = sample_rate: bin i is i Hz
    h, e, ent = R.hpcp_from_spectrum(_spectrum(1024, [(440, 0.7)]), 8000, 8000, R.params(normalized=0))
    want = np.zeros(12)
    want[9] = 0.7                                            # pc = 9 exactly, cos(0) = 1, f < 500 is doubled
    assert np.array_equal(h, want * 2)
    h, e, ent = R.hpcp_from_spectrum(_spectrum(1024, [(440, 0.7)]), 8000, 8000, R.params())
    want[9] = 1.0
    assert np.array_equal(h, want) and e == 1.0 and ent == 0.0


def test_band_preset_doubles_below_split():
    lo = R.hpcp_from_spectrum(_spectrum(1024, [(220, 0.25)]), 8000, 8000, R.params(normalized=0))[0]
    off = R.hpcp_from_spectrum(_spectrum(1024, [(220, 0.25)]), 8000, 8000, R.params(normalized=0, band_preset=0))[0]
    hi = R.hpcp_from_spectrum(_spectrum(1024, [(880, 0.25)]), 8000, 8000, R.params(normalized=0))[0]
    assert lo[9] == 0.5 and off[9] == 0.25 and hi[9] == 0.25
    assert np.count_nonzero(lo) == np.count_nonzero(off) == np.count_nonzero(hi) == 1


def test_third_harmonic_adds_the_fifth():
    p = R.params(normalized=0, band_preset=0, max_harmonics=3)
    h = R.hpcp_from_spectrum(_spectrum(2048, [(440, 0.9)]), 8000, 8000, p)[0]
    # 880 Hz is A again (0.9 / 2); 1320 Hz is 19.02 semitones up: bin 4 (E), at 0.9 / 3 times its cosine
    pc = R.frequency_to_pitch_class(p, 1320.0)
    assert round(pc) == 4
    assert h[9] == 0.9 + (0.9 * (1.0 / 2.0)) * 1.0
    assert h[4] == (0.9 * (1.0 / 3.0)) * math.cos(math.pi * abs(4 - pc) / 1.0)
    assert np.count_nonzero(h) == 2
    removed = R.hpcp_from_spectrum(_spectrum(2048, [(440, 0.9)]), 8000, 8000, dict(p, harmonics_removal=1))[0]
    assert removed[9] == 0.9 and np.count_nonzero(removed) == 1   # nothing is removed, only not added (F40)


def test_half_bin_gives_two_bins_at_cos_half_pi():
    got = [(b, w) for b, w, _ in R.contribution(R.params(), 8.5) if b is not None]
    assert got == [(8, math.cos(math.pi / 2)), (9, math.cos(math.pi / 2))]
    assert 0 < got[0][1] < 1e-16


def test_wrapping_and_collisions():
    # a 12-semitone window around 0.25: unwrapped bins -6 .. 7; the distance fold at size / 2 lets the
    # outermost ones (6.25 and 6.75 away, folded to 5.75 and 5.25) pass, so bins 6 and 7 are added twice
    rows = [b for b, _, _ in R.contribution(R.params(window_size=12.0, weight_type=0), 0.25)]
    assert rows == [6, 7, 8, 9, 10, 11, 0, 1, 2, 3, 4, 5, 6, 7]


def test_quiet_frame_is_not_normalised():
    # 450 Hz is 0.39 bins off A: 1.2e-5 * cos(0.39 pi) = 4.1e-6, its square is below 1e-10
    quiet = _spectrum(1024, [(450, 1.2e-5)])
    raw = R.hpcp_from_spectrum(quiet, 8000, 8000, R.params(band_preset=0, normalized=0))
    h, e, _ = R.hpcp_from_spectrum(quiet, 8000, 8000, R.params(band_preset=0))
    assert 0 < raw[0][9] < 1e-5 and np.array_equal(h, raw[0]) and e == raw[1]
    h, e, _ = R.hpcp_from_spectrum(quiet * 10, 8000, 8000, R.params(band_preset=0))
    assert h[9] == 1.0 and e == 1.0


# ---- the distance rule ------------------------------------------------------------------------

def test_two_greedy_outcomes():
    # replacement moves the reference point: 10 (1.0) is replaced by 13 (2.0), so 17 (1.5) is 4 away and kept
    m = _spectrum(32, [(10, 1.0), (13, 2.0), (17, 1.5)])
    assert [p[0] for p in R.detect_peaks(m, 64, 64, 0.0, 4.5, 60)] == [13, 17]
    # a drop keeps it: 13 (0.5) is dropped, 10 stays the reference, 15 (0.7) is 5 away and kept
    m = _spectrum(32, [(10, 1.0), (13, 0.5), (15, 0.7)])
    assert [p[0] for p in R.detect_peaks(m, 64, 64, 0.0, 4.5, 60)] == [10, 15]
    # not a cluster maximum: 13 replaces 10, 16 (3.0) replaces 13, although 16 is 6 away from 10
    m = _spectrum(32, [(10, 1.0), (13, 2.0), (16, 3.0)])
    assert [p[0] for p in R.detect_peaks(m, 64, 64, 0.0, 4.5, 60)] == [16]


@pytest.mark.parametrize("dist", [1, 2, 3, 5, 17])
def test_last_kept_form_equals_the_literal_loop(dist):
    rng = np.random.default_rng(100 + dist)
    for r in range(200):                                     # 5 x 200 = 1,000 rows
        K = int(rng.integers(3, 97))
        m = np.abs(rng.standard_normal(K))
        if r % 4 == 0:
            m = np.round(m * 4) / 4                          # ties and plateaus
        if r % 7 == 0:
            m[rng.integers(0, K)] = np.nan
        mp = int(rng.integers(0, 40))
        a = R.detect_peaks(m, 64, 64, 0.3, dist + 0.5, mp)
        b = R.detect_peaks_last_kept(m, 64, 64, 0.3, dist + 0.5, mp)
        assert a == b, (dist, r)


def test_equal_magnitudes_come_in_bin_order():
    comb = np.tile([0.0, 1.0], 200)
    got = R.detect_peaks_last_kept(np.append(comb, 0.0), 64, 64, 0.5, 1.0, 60)
    assert [p[0] for p in got] == list(range(1, 121, 2))


def test_max_shifted_is_the_identity():
    rng = np.random.default_rng(7)
    for r in range(1000):
        n = int(rng.integers(1, 37))
        h = rng.random(n) * (rng.random(n) < 0.6)
        plain = R.post(h, R.params(size=n, normalized=r % 2))
        shifted = R.post(h, R.params(size=n, normalized=r % 2, max_shifted=1))
        assert np.array_equal(plain[0], shifted[0]) and plain[1:] == shifted[1:]


# ---- the library's host-only side ---------------------------------------------------------------

def _lib_params(p):
    return sonar.hpcp_params(**p)


def _compare_tables(sr, ws, K, p, exact_sets):
    ref = R.table(sr, ws, K, p)
    got = sonar.hpcp_table(sr, ws, K, _lib_params(p))
    if exact_sets:
        print(f"sr={sr} ws={ws} K={K}: least margin {ref['min_margin']:.3g}")
        assert ref["min_margin"] >= 1e-9
    worst = 0.0
    for i in range(K):
        a0, a1 = ref["row_start"][i:i + 2]
        b0, b1 = got["row_start"][i:i + 2]
        a = [(int(ref["wrapped_bin"][e]), float(ref["factor"][e]), float(ref["window_weight"][e])) for e in range(a0, a1)]
        b = [(int(got["wrapped_bin"][e]), float(got["factor"][e]), float(got["window_weight"][e])) for e in range(b0, b1)]
        if not exact_sets and [x[:2] for x in a] != [x[:2] for x in b]:
            a = [x for x in a if x[2] > 1e-12]               # a cosine edge may be on one side only
            b = [x for x in b if x[2] > 1e-12]
        assert [x[:2] for x in a] == [x[:2] for x in b], (i, a, b)
        for x, y in zip(a, b):
            worst = max(worst, abs(x[2] - y[2]))
    print(f"sr={sr} ws={ws} K={K}: {len(got['wrapped_bin'])} entries, worst weight difference {worst:.3g}")
    assert worst <= 1e-12
    return got


TABLE_CASES = {
    "default": (44100, 2048, 1025, R.params()),
    "full_spectrum_8k": (8000, 2048, 2048, R.params()),
    "size36_squared": (44100, 2048, 1025, R.params(size=36, weight_type=2, window_size=1.33)),
    "harmonics16": (44100, 2048, 1025, R.params(size=24, max_harmonics=16, harmonics_strength=0.8)),
    "window12": (22050, 1024, 513, R.params(window_size=12.0, max_harmonics=4)),
    "window0": (44100, 2048, 1025, R.params(window_size=0.0)),
    "size1": (44100, 2048, 1025, R.params(size=1)),
}


@pytest.mark.parametrize("name", sorted(TABLE_CASES))
def test_library_table_matches_checker(name):
    sr, ws, K, p = TABLE_CASES[name]
    got = _compare_tables(sr, ws, K, p, exact_sets=False)
    lo = int(math.ceil(p["min_freq"] / (sr / ws)))
    assert got["row_start"][min(lo, K)] == 0                 # rows below min_freq are empty
    assert got["row_start"][K] == got["row_start"][K - 1]    # bin K - 1 is never a peak


@pytest.mark.parametrize("ws_semitones", [0.0, 1.0, 1.33, 12.0])
def test_library_table_weight_none_identical_sets(ws_semitones):
    p = R.params(weight_type=0, window_size=ws_semitones, max_harmonics=4, size=24)
    got = _compare_tables(44100, 2048, 1025, p, exact_sets=True)
    assert np.all(got["window_weight"] == 1.0)
    assert set(np.unique(got["factor"])) <= {1.0, 2.0, 1.0 / 2, 1.0 / 3, 1.0 / 4}


def test_unknown_weight_type_is_none():
    a = sonar.hpcp_table(44100, 2048, 1025, sonar.hpcp_params(weight_type=7))
    b = sonar.hpcp_table(44100, 2048, 1025, sonar.hpcp_params(weight_type="none"))
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert sonar.hpcp_params(weight_type="hann").weight_type == 0


def test_defaults_are_new_hpcp():
    p = sonar.hpcp_params()
    assert {k: getattr(p, k) for k in R.DEFAULT} == R.DEFAULT


def test_table_errors():
    for kw, code in [(dict(size=-1), sonar.ERR_PANIC), (dict(reference_freq=0.0), sonar.ERR_UNSUPPORTED),
                     (dict(reference_freq=float("nan")), sonar.ERR_UNSUPPORTED),
                     (dict(window_size=-0.5), sonar.ERR_UNSUPPORTED), (dict(window_size=float("inf")), sonar.ERR_UNSUPPORTED),
                     (dict(window_size=12.5), sonar.ERR_UNSUPPORTED), (dict(size=121), sonar.ERR_UNSUPPORTED),
                     (dict(max_harmonics=17), sonar.ERR_UNSUPPORTED)]:
        with pytest.raises(sonar.SonarError) as e:
            sonar.hpcp_table(44100, 2048, 1025, sonar.hpcp_params(**kw))
        assert e.value.code == code, kw
    with pytest.raises(sonar.SonarError) as e:
        sonar.hpcp_table(44100, 2048, 1025, sonar.hpcp_params(size=-1))
    assert "makeslice: len out of range" in e.value.msg
    for sr, ws, K in [(0, 2048, 1025), (44100, 0, 1025), (44100, 2048, 8193)]:
        with pytest.raises(sonar.SonarError) as e:
            sonar.hpcp_table(sr, ws, K, sonar.hpcp_params())
        assert e.value.code == sonar.ERR_UNSUPPORTED
    empty = sonar.hpcp_table(44100, 2048, 1025, sonar.hpcp_params(size=0))
    assert len(empty["wrapped_bin"]) == 0 and not empty["row_start"].any()
    assert len(sonar.hpcp_table(44100, 2048, 8192, sonar.hpcp_params(size=120, max_harmonics=16))["factor"]) > 0


def test_plan_arithmetic():
    p = sonar.hpcp_plan(140_000, 128, 1)
    assert p["frames"] == 139_873 == sonar.stft_frames(140_000, 128, 1)
    assert p["chunk_frames"] == (64 << 20) // (65 * 8) and p["n_chunks"] == 2
    p = sonar.hpcp_plan(26_460_000, 2048, 512)               # 10 minutes at 44.1 kHz
    assert p["frames"] == 51_676 and p["chunk_frames"] == (64 << 20) // (1025 * 8)
    assert p["n_chunks"] == -(-51_676 // p["chunk_frames"])
    assert sonar.hpcp_plan(2048, 2048, 512) == {"frames": 1, "chunk_frames": 8184, "n_chunks": 1}
    # an hour at 44.1 kHz: the scratch stays one chunk whatever the length
    hour = sonar.hpcp_plan(158_760_000, 2048, 512)
    assert hour["chunk_frames"] * 1025 * 8 <= 64 << 20 < hour["frames"] * 1025 * 8
    for n, w, h, code in [(0, 2048, 512, sonar.ERR_EMPTY), (100, 0, 512, sonar.ERR_INVALID),
                          (100, 2048, 0, sonar.ERR_INVALID), (1536, 2048, 512, sonar.ERR_TOO_SHORT),
                          (20000, 9000, 512, sonar.ERR_UNSUPPORTED)]:
        with pytest.raises(sonar.SonarError) as e:
            sonar.hpcp_plan(n, w, h)
        assert e.value.code == code, (n, w, h)


def test_peaks_width_and_abi_version():
    assert [sonar.spectral_peaks_width(K, 60) for K in (0, 1, 2, 3, 4, 5, 121, 122, 123, 8192)] == \
        [0, 0, 0, 1, 1, 2, 60, 60, 60, 60]
    assert sonar.spectral_peaks_width(8192, 10_000) == 4095 and sonar.spectral_peaks_width(100, 0) == 0
    assert sonar.abi_version() == 4
