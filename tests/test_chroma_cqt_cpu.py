"""The parts of the constant-Q chroma (sonar_chroma_cqt) that need no GPU: sonar_chroma_cqt_plan's known
answers, the frame rule, the Python checker (tests/chroma_cqt_ref.py) held to DESIGN.md F24 -- its
literal FFT-domain sums are N times a real dot product with a Gaussian -- and to a closed form, and the
two new symbols in the header and the library.

Configuration A: sr 8000, 200-1600 Hz, 12 bins per octave, Q 5, tuning 440 (N = 512, 36 bins,
L = 201 .. 27).  D: NewChromaCQTDefault(44100)."""
import ctypes
import math
import re

import numpy as np
import pytest

import chroma_cqt_ref as R
import sonar

A = dict(sample_rate=8000, min_freq=200.0, max_freq=1600.0, bins_per_octave=12, q_factor=5.0, tuning_freq=440.0)
CAPPED = dict(sample_rate=8000, min_freq=30.0, max_freq=480.0, bins_per_octave=12, q_factor=25.0, tuning_freq=440.0)
FIVE = dict(sample_rate=8000, min_freq=200.0, max_freq=400.0, bins_per_octave=5, q_factor=5.0, tuning_freq=432.0)


def _noise(n, seed=0):
    return 0.5 + 0.1 * np.random.default_rng(seed).standard_normal(n)


def _both(**kw):
    """The library's plan, after checking that the checker's says the same."""
    got = sonar.chroma_cqt_plan(**kw)
    ref = R.plan(**kw)
    assert got["total_bins"] == ref["total_bins"] and got["fft_size"] == ref["fft_size"]
    assert got["sum_taps"] == ref["sum_taps"]
    assert np.array_equal(got["kernel_len"], ref["kernel_len"]) and np.array_equal(got["chroma_bin"], ref["chroma_bin"])
    assert got["kernel_len"].dtype == np.int32 and got["n_frames"] == 0
    return got


def test_plan_default():
    p = _both(sample_rate=44100)
    assert p["total_bins"] == 60 and p["fft_size"] == 65536 and p["sum_taps"] == 290970
    assert p["kernel_len"][:3].tolist() == [16857, 15911, 15019]
    assert p["kernel_len"][-3:].tolist() == [627, 591, 559]
    assert p["chroma_bin"].tolist() == [k % 12 for k in range(60)]


def test_plan_a():
    p = _both(**A)
    assert p["total_bins"] == 36 and p["fft_size"] == 512 and p["sum_taps"] == 3122
    assert p["kernel_len"][0] == 201 and p["kernel_len"][-1] == 27


def test_plan_capped_lengths():
    p = _both(**CAPPED)
    assert p["total_bins"] == 48 and p["fft_size"] == 8192
    assert p["kernel_len"][:9].tolist() == [4000] * 9 and p["kernel_len"][9] == 3965


def test_plan_five_bins():
    p = _both(**FIVE)
    assert p["total_bins"] == 5
    assert p["kernel_len"].tolist() == [201, 175, 151, 131, 115] and p["chroma_bin"].tolist() == [8, 10, 0, 3, 5]


def test_plan_minimum_length():
    p = _both(**dict(A, q_factor=0.001))
    assert p["kernel_len"].tolist() == [3] * 36 and p["fft_size"] == 8


@pytest.mark.parametrize("n,hop,frames", [(3000, 64, 45), (40000, 512, 77), (3000, 5000, 1), (1, 64, 1), (3000, -5, 1),
                                          (0, 64, 0), (0, 0, 0)])
def test_frame_counts(n, hop, frames):
    assert R.n_frames(n, hop) == frames
    assert sonar.chroma_cqt_plan(n=n, hop=hop, **A)["n_frames"] == frames


def test_plan_errors():
    for kw, code in ((dict(A, max_freq=200.0), sonar.ERR_PANIC), (dict(A, max_freq=100.0), sonar.ERR_PANIC),
                     (dict(A, q_factor=0.0), sonar.ERR_UNSUPPORTED), (dict(A, bins_per_octave=0), sonar.ERR_UNSUPPORTED),
                     (dict(A, sample_rate=5), sonar.ERR_UNSUPPORTED), (dict(A, tuning_freq=math.inf), sonar.ERR_UNSUPPORTED),
                     (dict(A, min_freq=math.nan), sonar.ERR_UNSUPPORTED)):
        with pytest.raises(sonar.SonarError) as e:
            sonar.chroma_cqt_plan(**kw)
        assert e.value.code == code, kw
    with pytest.raises(sonar.SonarError) as e:
        sonar.chroma_cqt_plan(n=100, hop=0, **A)             # the division of :169
    assert e.value.code == sonar.ERR_PANIC
    with pytest.raises(IndexError, match=r"index out of range \[0\] with length 0"):
        R.plan(**dict(A, max_freq=200.0))
    with pytest.raises(ValueError, match="makeslice: len out of range"):
        R.plan(**dict(A, max_freq=100.0))
    with pytest.raises(ZeroDivisionError, match="integer divide by zero"):
        R.n_frames(100, 0)


@pytest.mark.parametrize("cfg,n,hop", [(A, 3000, 64), (CAPPED, 9000, 100)])
def test_checker_sums_are_gaussian_dot_products(cfg, n, hop):
    """F24: sum_n frameFFT[n] conj(K_k[n]) = N sum_t frame[t] g_k[t], g_k real and without phase."""
    x = _noise(n, seed=n)
    ref = R.chroma_cqt(x, hop, **cfg)
    N, lens = ref["plan"]["fft_size"], ref["plan"]["kernel_len"]
    F = R.n_frames(n, hop)
    assert ref["cqt"].shape == (F, len(lens)) and ref["chroma"].shape == (F, 12)
    worst = 0.0
    for f in range(F):
        fr = ref["frames"][f]
        for k, L in enumerate(lens):
            direct = N * abs(math.fsum(fr[:L] * ref["g"][k]))
            worst = max(worst, abs(ref["cqt"][f, k] - direct) / ref["scale"][f, k])
    assert worst <= 1e-12, worst
    for k, L in enumerate(lens):                              # the taps: a Gaussian, not a band-pass
        t = np.arange(L) - L // 2
        sigma = cfg["sample_rate"] / (2 * math.pi * ref["plan"]["freqs"][k] / cfg["q_factor"])
        # values <= 1; an ulp each for exp (twice), cos, sin and hypot, half for each product: < 8 ulp
        assert np.max(np.abs(ref["g"][k] - np.exp(-t * t / (2 * sigma * sigma)))) <= 8 * 1.2e-16


def test_constant_signal_has_a_closed_form():
    """x = c: a frame whose longest kernel ends inside the signal has cqt_k = N c sum(g_k)."""
    c, n, hop = 0.75, 3000, 64
    ref = R.chroma_cqt(np.full(n, c), hop, **A)
    p = ref["plan"]
    gsum = np.array([math.fsum(g) for g in ref["g"]])
    want = p["fft_size"] * c * gsum
    e = np.zeros(12)
    for k, cl in enumerate(p["chroma_bin"]):
        e[cl] += want[k] ** 2
    inside = [f for f in range(45) if f * hop + p["kernel_len"][0] <= n]
    assert len(inside) == 44                                 # the last frame runs past the signal
    for f in inside:
        assert np.max(np.abs(ref["cqt"][f] - want) / ref["scale"][f]) <= 1e-12
        assert np.max(np.abs(ref["chroma"][f] - e / e.sum())) <= 1e-12
    assert np.max(np.abs(ref["chroma"][44] - e / e.sum())) > 1e-6


def test_new_symbols_are_declared_and_exported():
    with open(sonar._abi.HEADER) as f:
        text = f.read()
    lib = ctypes.CDLL(sonar.LIB_PATH)
    for n in ("sonar_chroma_cqt", "sonar_chroma_cqt_plan"):
        assert n in sonar.EXPORTED_SYMBOLS
        assert re.search(r"^int " + n + r"\(", text, re.M)
        assert hasattr(lib, n)
    assert callable(sonar.chroma_cqt_plan) and hasattr(sonar.Context, "chroma_cqt")
    assert hasattr(sonar.Context, "chroma_cqt_device")
    assert sonar.abi_version() == 4
