"""sonar_spectral_peaks, sonar_hpcp_from_spectrum and sonar_hpcp on the GPU against the Python checker
(tests/hpcp_ref.py, held to known answers in test_hpcp_cpu.py).

Peaks are bit-exact: counts, bins, magnitudes, frequencies (comparisons, a selection, one product).
The profile is compared with the checker fed the library's own table (the table is held to the
checker's in test_hpcp_cpu.py), so what is left is comparisons and (magnitude * factor) * weight
sums in the reference's order: hpcp and energy bit-exact whenever NonLinear is off; entropy within
1e-12 absolute (log2); with NonLinear on (log) the unnormalised profile within 1e-12 relative.

Shapes: the kernel takes one row per wave and 64 bins per step, keeps up to (K - 1) / 2 candidates and
ranks them 64 at a time; K runs over 1..4, both sides of 64 and 128, and the largest row the library
takes; F over both sides of 64 and past 256; max_peaks over 0, 1, both sides of 60, and both sides of
the candidate count; min_distance_bins over the inert values (1, 2) and the greedy ones (3, 5, K)."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library loads HIP (one HIP runtime in the process)

import hpcp_ref as R
import sonar

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ---- peaks ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _rows(F, K, seed=0):
    rng = np.random.default_rng(1000 * K + F + seed)
    m = np.abs(rng.standard_normal((F, K)))
    for f in range(F):
        for b in rng.integers(0, K, size=min(4, K)):
            m[f, b] += 5.0 + rng.random()
    assert all(len(np.unique(r)) == K for r in m)            # distinct magnitudes: Go's order is pinned too
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _all_peaks(F, K, dist, min_height=0.3):
    """Every row's kept peaks in output order; window_size = sample_rate, so a bin is 1 Hz wide."""
    mag = _rows(F, K)
    return [R.detect_peaks_last_kept(mag[f], 64, 64, min_height, dist + 0.5, 1 << 30) for f in range(F)]


def _expect(peaks, K, max_peaks):
    P = min(max_peaks, max((K - 1) // 2, 0))
    F = len(peaks)
    count, bins = np.zeros(F, np.int32), np.zeros((F, P), np.int32)
    pm, pf = np.zeros((F, P)), np.zeros((F, P))
    for f, row in enumerate(peaks):
        row = row[:max_peaks]
        count[f] = len(row)
        for r, (b, m, fr) in enumerate(row):
            bins[f, r], pm[f, r], pf[f, r] = b, m, fr
    return count, bins, pm, pf


def _check_peaks(got, want):
    count, bins, pm, pf = want
    assert np.array_equal(got["count"], count)
    assert got["bin"].shape == bins.shape and np.array_equal(got["bin"], bins)
    assert _same(got["magnitude"], pm) and _same(got["frequency"], pf)


PEAK_SHAPES = [(1, 2), (2, 1), (3, 2), (4, 63), (64, 64), (65, 65), (129, 257), (1025, 65), (2048, 63), (4097, 2),
               (8192, 64)]


@pytest.mark.parametrize("K,F", PEAK_SHAPES)
def test_peaks_every_max_peaks(ctx, K, F):
    peaks = _all_peaks(F, K, 1)
    cand = max(len(p) for p in peaks)
    if K >= 64:
        assert K / 4 <= cand <= K / 2                        # about K / 3 candidates above 0.3
    for mp in (0, 1, 60, 61, cand, cand + 1):
        got = ctx.spectral_peaks(_rows(F, K), 64, 64, 0.3, 1.5, mp)
        _check_peaks(got, _expect(peaks, K, mp))


@pytest.mark.parametrize("K,F", [(65, 65), (1025, 63), (8192, 2)])
@pytest.mark.parametrize("dist", [1, 2, 3, 5, "K"])
def test_peaks_every_distance(ctx, K, F, dist):
    d = K if dist == "K" else dist
    peaks = _all_peaks(F, K, d)
    cand = max(len(p) for p in peaks)
    if d >= K:
        assert cand == 1
    for mp in (60, cand + 1):
        got = ctx.spectral_peaks(_rows(F, K), 64, 64, 0.3, d + 0.5, mp)
        _check_peaks(got, _expect(peaks, K, mp))
    if d in (1, 2):                                           # the inert branch: the same peaks as no rule at all
        assert peaks == _all_peaks(F, K, 1)


def test_peaks_two_greedy_outcomes(ctx):
    rows = np.zeros((3, 32))
    rows[0, [10, 13, 17]] = [1.0, 2.0, 1.5]                  # 13 replaces 10 and moves the reference point: 17 stays
    rows[1, [10, 13, 15]] = [1.0, 0.5, 0.7]                  # 13 is dropped, 10 stays the reference: 15 stays
    rows[2, [10, 13, 16]] = [1.0, 2.0, 3.0]                  # a chain of replacements: not a cluster maximum
    got = ctx.spectral_peaks(rows, 64, 64, 0.0, 4.5, 60)
    assert got["count"].tolist() == [2, 2, 1]
    assert got["bin"][0, :2].tolist() == [13, 17] and got["bin"][1, :2].tolist() == [10, 15]
    assert got["bin"][2, 0] == 16
    want = [R.detect_peaks(r, 64, 64, 0.0, 4.5, 60) for r in rows]
    _check_peaks(got, _expect(want, 32, 60))


def test_peaks_equal_magnitudes_in_bin_order(ctx):
    comb = np.append(np.tile([0.0, 1.0], 200), 0.0)
    got = ctx.spectral_peaks(comb, 64, 64, 0.5, 1.0, 60)
    assert got["count"][0] == 60 and got["bin"][0].tolist() == list(range(1, 121, 2))
    assert np.all(got["magnitude"] == 1.0)
    assert _same(got["frequency"][0], np.arange(1, 121, 2, dtype=np.float64))


def test_peaks_nan_and_inf(ctx):
    rows = np.array(_rows(3, 129, seed=5))
    rows[0, 40], rows[0, 90] = np.nan, np.inf                # no peak at 39, 40, 41; the largest at 90
    rows[1, 0], rows[1, 128] = np.inf, np.inf                # the end bins are never peaks
    rows[2, 64] = -np.inf
    got = ctx.spectral_peaks(rows, 2048, 44100, -1.0, 20.0, 30)
    want = [R.detect_peaks(r, 2048, 44100, -1.0, 20.0, 30) for r in rows]
    _check_peaks(got, _expect(want, 129, 30))
    assert got["bin"][0, 0] == 90 and np.isinf(got["magnitude"][0, 0])
    assert not set(got["bin"][0, :got["count"][0]].tolist()) & {39, 40, 41}


def test_peaks_host_and_device_pointers_agree(ctx):
    F, K, P = 65, 1025, 60
    mag = _rows(F, K)
    host = ctx.spectral_peaks(mag, 2048, 8000, 0.3, 20.0, P)  # 20 Hz at 3.9 Hz per bin: 5 bins, the greedy
    d = torch.from_numpy(mag.copy()).cuda()
    count = torch.full((F,), -1, dtype=torch.int32, device="cuda")
    bins = torch.full((F, P), -1, dtype=torch.int32, device="cuda")
    pm, pf = (torch.full((F, P), -1.0, dtype=torch.float64, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    ctx.spectral_peaks_device(d.data_ptr(), F, K, 2048, 8000, count.data_ptr(), bins.data_ptr(), pm.data_ptr(),
                              pf.data_ptr(), 0.3, 20.0, P)
    assert np.array_equal(count.cpu().numpy(), host["count"]) and np.array_equal(bins.cpu().numpy(), host["bin"])
    assert _same(pm.cpu().numpy(), host["magnitude"]) and _same(pf.cpu().numpy(), host["frequency"])
    want = [R.detect_peaks_last_kept(r, 2048, 8000, 0.3, 20.0, P) for r in mag]
    _check_peaks(host, _expect(want, K, P))


def test_peaks_edges_and_errors(ctx):
    got = ctx.spectral_peaks(np.zeros((0, 16)), 2048, 44100)
    assert got["count"].shape == (0,)
    got = ctx.spectral_peaks(np.zeros((3, 0)), 2048, 44100)
    assert got["count"].tolist() == [0, 0, 0] and got["bin"].shape == (3, 0)
    with pytest.raises(sonar.SonarError) as e:
        ctx.spectral_peaks(np.zeros((2, 16)), 2048, 44100, max_peaks=-1)
    assert e.value.code == sonar.ERR_PANIC and e.value.msg == "runtime error: slice bounds out of range [:-1]"
    for ws, sr, K in [(0, 44100, 16), (2048, 0, 16), (2048, 44100, 8193)]:
        with pytest.raises(sonar.SonarError) as e:
            ctx.spectral_peaks(np.zeros((1, K)), ws, sr)
        assert e.value.code == sonar.ERR_UNSUPPORTED


# ---- the profile ---------------------------------------------------------------------------------

PROFILE_CASES = {
    "default": (44100, 2048, 1025, {}),
    "chord_44100": (44100, 2048, 2048, {}),
    "chord_8000": (8000, 2048, 2048, {}),                    # mirror bins inside max_freq; 5-bin distance rule
    "size24": (44100, 2048, 1025, dict(size=24)),
    "size36": (44100, 2048, 1025, dict(size=36, weight_type=2)),
    "size120": (44100, 2048, 1025, dict(size=120, window_size=2.0)),
    "window0": (44100, 2048, 1025, dict(window_size=0.0)),
    "window1.33": (44100, 2048, 1025, dict(window_size=1.33, weight_type=2)),
    "window12": (44100, 2048, 1025, dict(window_size=12.0)),
    "order_none_raw": (44100, 2048, 1025, dict(weight_type=0, normalized=0, window_size=12.0, max_harmonics=4)),
    "none": (44100, 2048, 1025, dict(weight_type=0, window_size=1.33)),
    "harmonics4": (44100, 2048, 1025, dict(max_harmonics=4, harmonics_strength=0.7)),
    "harmonics16": (44100, 2048, 1025, dict(max_harmonics=16, size=24)),
    "harmonics16_removal": (44100, 2048, 1025, dict(max_harmonics=16, harmonics_removal=1)),
    "harmonics4_removal": (44100, 2048, 1025, dict(max_harmonics=4, harmonics_removal=1)),
    "raw": (44100, 2048, 1025, dict(normalized=0)),
    "max_shifted": (44100, 2048, 1025, dict(max_shifted=1, size=36)),
    "max_shifted_raw": (44100, 2048, 1025, dict(max_shifted=1, normalized=0, max_harmonics=4)),
    "no_band_preset": (22050, 1024, 513, dict(band_preset=0)),
}
PROFILE_F = 34


@functools.lru_cache(maxsize=None)
def _profile_rows(K, sr, ws):
    """32 noise rows with spikes, a row of zeros and a quiet row (one peak whose square stays below the
    normaliser's 1e-10)."""
    rng = np.random.default_rng(K + sr)
    m = 0.05 * np.abs(rng.standard_normal((PROFILE_F, K))) / (1.0 + np.arange(K) / 200.0)
    for f in range(PROFILE_F):
        for b in rng.integers(2, K - 2, size=6):
            m[f, b] += rng.random()
    m[PROFILE_F - 2] = 0.0
    m[PROFILE_F - 1] = 0.0
    m[PROFILE_F - 1, int(1000.0 / (sr / ws))] = 9e-6 + 1.1e-6   # 1.01e-5: a peak, its square is 1.02e-10 at weight 1
    m.setflags(write=False)
    return m


def _run_profile(ctx, name, extra=None):
    sr, ws, K, kw = PROFILE_CASES[name]
    kw = dict(kw, **(extra or {}))
    p = R.params(**kw)
    lp = sonar.hpcp_params(**kw)
    mag = _profile_rows(K, sr, ws)
    tab = sonar.hpcp_table(sr, ws, K, lp)
    got = ctx.hpcp_from_spectrum(mag, ws, sr, lp)
    want = [R.hpcp_with_table(row, tab, ws, sr, p) for row in mag]
    return p, got, want


@pytest.mark.parametrize("name", sorted(PROFILE_CASES))
def test_profile_bit_exact(ctx, name):
    p, got, want = _run_profile(ctx, name)
    wh = np.array([w[0] for w in want])
    assert got["hpcp"].shape == (PROFILE_F, p["size"])
    if p["window_size"] > 0:
        assert np.count_nonzero(wh[:PROFILE_F - 2].sum(axis=1)) == PROFILE_F - 2   # every noise row has a profile
    else:
        assert not wh.any()        # a zero-width window passes only a pitch class that is a whole number
    diff = np.flatnonzero(~np.all(_bits(got["hpcp"]) == _bits(wh), axis=1))
    assert diff.size == 0, (diff, got["hpcp"][diff[:1]], wh[diff[:1]])
    assert _same(got["energy"], np.array([w[1] for w in want]))
    err = np.max(np.abs(got["entropy"] - np.array([w[2] for w in want])))
    print(f"{name}: entropy error {err:.3g}")
    assert err <= 1e-12
    assert not got["hpcp"][PROFILE_F - 2].any() and got["energy"][PROFILE_F - 2] == 0 and got["entropy"][PROFILE_F - 2] == 0


def test_profile_quiet_frame_is_left_unnormalised(ctx):
    _, got, want = _run_profile(ctx, "no_band_preset")
    _, raw, _ = _run_profile(ctx, "no_band_preset", dict(normalized=0))
    q = PROFILE_F - 1
    assert 0 < np.sum(want[q][0] ** 2) < 1e-10               # on the checker: below the normaliser's threshold
    assert _same(got["hpcp"][q], raw["hpcp"][q]) and got["energy"][q] < 1.1e-5
    assert abs(got["energy"][0] - 1.0) < 1e-14 and raw["energy"][0] != got["energy"][0]


@pytest.mark.parametrize("name", ["default", "harmonics4", "window12"])
def test_profile_non_linear(ctx, name):
    p, got, want = _run_profile(ctx, name, dict(non_linear=1, normalized=0))
    wh = np.array([w[0] for w in want])
    assert np.array_equal(got["hpcp"] == 0, wh == 0)
    nz = wh != 0
    err = np.max(np.abs(got["hpcp"][nz] - wh[nz]) / np.abs(wh[nz]))
    print(f"{name}: non-linear relative error {err:.3g}")
    assert err <= 1e-12
    _, lin, _ = _run_profile(ctx, name, dict(normalized=0))
    assert np.all(got["hpcp"][nz] < lin["hpcp"][nz])


def test_profile_against_independent_checker(ctx):
    sr, ws, K, _ = PROFILE_CASES["default"]
    mag = _profile_rows(K, sr, ws)[:16]
    got = ctx.hpcp_from_spectrum(mag, ws, sr)
    want = np.array([R.hpcp_from_spectrum(row, ws, sr, R.params())[0] for row in mag])
    err = np.max(np.abs(got["hpcp"] - want))
    print(f"default against hpcp_from_peaks: {err:.3g}")
    assert err <= 1e-12


def test_profile_edges_and_errors(ctx):
    mag = _profile_rows(1025, 44100, 2048)[:3]
    got = ctx.hpcp_from_spectrum(mag, 2048, 44100, sonar.hpcp_params(size=0))
    assert got["hpcp"].shape == (3, 0) and not got["energy"].any() and not got["entropy"].any()
    got = ctx.hpcp_from_spectrum(np.zeros((2, 0)), 2048, 44100)
    assert got["hpcp"].shape == (2, 12) and not got["hpcp"].any()
    assert ctx.hpcp_from_spectrum(np.zeros((0, 1025)), 2048, 44100)["hpcp"].shape == (0, 12)
    for K in (1, 2, 3):
        assert not ctx.hpcp_from_spectrum(np.ones((2, K)), 2048, 44100)["hpcp"].any()
    with pytest.raises(sonar.SonarError) as e:
        ctx.hpcp_from_spectrum(mag, 2048, 44100, sonar.hpcp_params(size=-3))
    assert e.value.code == sonar.ERR_PANIC and e.value.msg == "runtime error: makeslice: len out of range"
    for kw, word in [(dict(reference_freq=-1.0), "reference_freq"), (dict(window_size=float("nan")), "window_size"),
                     (dict(size=121), "size"), (dict(max_harmonics=17), "max_harmonics"),
                     (dict(window_size=13.0), "12 semitones")]:
        with pytest.raises(sonar.SonarError) as e:
            ctx.hpcp_from_spectrum(mag, 2048, 44100, sonar.hpcp_params(**kw))
        assert e.value.code == sonar.ERR_UNSUPPORTED and word in e.value.msg, (kw, e.value.msg)
    with pytest.raises(sonar.SonarError) as e:
        ctx.hpcp_from_spectrum(mag, 0, 44100)
    assert e.value.code == sonar.ERR_UNSUPPORTED
    # a table survives sonar_trim by being rebuilt
    a = ctx.hpcp_from_spectrum(mag, 2048, 44100)
    ctx.trim()
    assert _same(ctx.hpcp_from_spectrum(mag, 2048, 44100)["hpcp"], a["hpcp"])


# ---- the PCM entry -------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _pcm(n):
    rng = np.random.default_rng(n)
    t = np.arange(n) / 44100.0
    x = sum(a * np.sin(2 * np.pi * f * t) for a, f in [(0.5, 220.0), (0.3, 554.37), (0.2, 1318.5), (0.1, 3520.0)])
    x = x + 0.01 * rng.standard_normal(n)
    x.setflags(write=False)
    return x


def _two_step(ctx, x, W, H, window, params=None):
    cfg = ctx.config(window_size=W, hop_size=H, window_type=window, sample_rate=44100, flags=sonar.FP_MAGNITUDE,
                     precision=sonar.F64, pcm_dtype=sonar.F64, out_dtype=sonar.F64)
    mag = ctx.fingerprint(x, cfg)["magnitude"]
    return mag, ctx.hpcp_from_spectrum(mag, W, 44100, params)


@pytest.mark.parametrize("W,H,frames,tail", [(128, 32, 70, 5), (1024, 256, 37, 100), (2048, 512, 33, 511),
                                             (1000, 250, 21, 7), (2048, 512, 1, 0), (1000, 250, 1, 0)])
@pytest.mark.parametrize("window", ["rectangular", "hann"])
def test_hpcp_equals_fingerprint_then_from_spectrum(ctx, W, H, frames, tail, window):
    n = W + H * (frames - 1) + tail
    x = _pcm(n)
    assert sonar.hpcp_plan(n, W, H)["frames"] == frames
    cfg = ctx.config(window_size=W, hop_size=H, precision=sonar.F64, pcm_dtype=sonar.F64, out_dtype=sonar.F64,
                     flags=sonar.FP_MAGNITUDE)
    assert sonar.fp_kernel_plan(cfg, n) == (sonar.PLAN_DFT if W == 1000 else sonar.PLAN_WAVE)
    mag, want = _two_step(ctx, x, W, H, window)
    got = ctx.hpcp(x, 44100, W, H, window)
    assert got["hpcp"].shape == (frames, 12) and got["hpcp"].any()
    for k in ("hpcp", "energy", "entropy"):
        assert _same(got[k], want[k]), k


def test_hpcp_chunk_seam(ctx):
    n, W, H = 140_000, 128, 1
    plan = sonar.hpcp_plan(n, W, H)
    assert plan["frames"] == 139_873 and plan["n_chunks"] >= 2
    x = _pcm(n)
    params = sonar.hpcp_params(min_freq=300.0, max_harmonics=2)
    _, want = _two_step(ctx, x, W, H, "hann", params)
    got = ctx.hpcp(x, 44100, W, H, "hann", params)
    seam = plan["chunk_frames"]
    assert got["hpcp"][seam - 1].any() and got["hpcp"][seam].any()
    for k in ("hpcp", "energy", "entropy"):
        assert _same(got[k], want[k]), k


def test_hpcp_device_pointers_and_errors(ctx):
    W, H, n = 1024, 256, 1024 + 256 * 20
    x = _pcm(n)
    host = ctx.hpcp(x, 44100, W, H)
    d = torch.from_numpy(x.copy()).cuda()
    out = torch.zeros(21, 12, dtype=torch.float64, device="cuda")
    e, h = (torch.zeros(21, dtype=torch.float64, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    ctx.hpcp_device(d.data_ptr(), n, 44100, out.data_ptr(), W, H, energy_ptr=e.data_ptr(), entropy_ptr=h.data_ptr())
    assert _same(out.cpu().numpy(), host["hpcp"]) and _same(e.cpu().numpy(), host["energy"])
    assert _same(h.cpu().numpy(), host["entropy"])
    with pytest.raises(sonar.SonarError) as err:
        ctx.hpcp(x[:512], 44100, 2048, 512)
    assert err.value.code == sonar.ERR_TOO_SHORT
    assert err.value.msg == "signal too short for given window size and hop size"
    with pytest.raises(sonar.SonarError) as err:
        ctx.hpcp(np.zeros(0), 44100)
    assert err.value.code == sonar.ERR_EMPTY
    with pytest.raises(sonar.SonarError) as err:
        ctx.hpcp(x, 44100, 1024, 0)
    assert err.value.code == sonar.ERR_INVALID
    with pytest.raises(sonar.SonarError) as err:
        ctx.hpcp(x, 44100, W, H, params=sonar.hpcp_params(size=-1))
    assert err.value.code == sonar.ERR_PANIC
    with pytest.raises(sonar.SonarError) as err:
        ctx.hpcp(x, 0, W, H)
    assert err.value.code == sonar.ERR_UNSUPPORTED
    empty = ctx.hpcp(x, 44100, W, H, params=sonar.hpcp_params(size=0))
    assert empty["hpcp"].shape == (21, 0) and not empty["energy"].any()


# ---- the hand-off to the similarity kernels ----------------------------------------------------

def test_device_hpcp_feeds_chroma_similarity(ctx):
    sr, ws, K, F = 44100, 2048, 1025, 48
    rng = np.random.default_rng(3)
    res = sr / ws

    def spectra(semitones):
        m = np.zeros((F, K))
        for f in range(F):
            for note, amp in zip(notes[f], (1.0, 0.6, 0.4)):
                m[f, int(round(440.0 * 2.0 ** ((note + semitones) / 12.0) / res))] += amp
        return m
    notes = [rng.choice(np.arange(8, 30), size=3, replace=False) for _ in range(F)]   # 700 Hz .. 2.3 kHz
    orig, up3 = spectra(0), spectra(3)
    d_orig, d_up = torch.from_numpy(orig).cuda(), torch.from_numpy(up3).cuda()
    h_orig, h_up = (torch.zeros(F, 12, dtype=torch.float64, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    ctx.hpcp_from_spectrum_device(d_orig.data_ptr(), F, K, ws, sr, h_orig.data_ptr())
    ctx.hpcp_from_spectrum_device(d_up.data_ptr(), F, K, ws, sr, h_up.data_ptr())
    got = ctx.chroma_similarity_device(h_up.data_ptr(), F, h_orig.data_ptr(), F, 12, "direct", "cosine",
                                       transposition_invariant=True)
    assert got["best_transposition"] == 3
    plain = ctx.chroma_similarity_device(h_up.data_ptr(), F, h_orig.data_ptr(), F, 12, "direct", "cosine")
    assert got["overall"] > plain["overall"]
    assert _same(h_orig.cpu().numpy(), ctx.hpcp_from_spectrum(orig, ws, sr)["hpcp"])
