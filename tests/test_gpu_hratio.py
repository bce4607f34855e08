"""sonar_hratio_from_spectrum / sonar_hratio_frames / sonar_hratio on the GPU against the Python checker
(tests/hratio_ref.py, pinned to hand-worked answers in test_hratio_cpu.py; the cases are hratio_cases.py's).

From spectrum the inputs are the same bits on both sides, so every discrete output, the energies, the
periodicity, the roughness, the noise floor, h_freq, h_amp and f0 are compared bit for bit; the four outputs
that pass through log10 or exp within 16 x 2^-52 x max(1, |expected|) (two libraries of <= 2 ulp each over at
most three chained operations), +-Inf and NaN matching as such.

From PCM the reference's transform is go-dsp's: the tolerance is FACTOR (test_gpu_pitch.py's) x the measured
numpy-vs-go difference of the checker's own |X|, relative to the row's peak and scaled per output by
hratio_cases.scales; each case prints it.  Frames the checker leaves undecided under either transform are
skipped (test_hratio_cpu.py holds them to 10 % per case; on these signals there is none).  Measured on these
cases: numpy vs go_fft at most 4.33e-16 of the row's peak, so tolerances of at most 6.92e-15; the library's own
difference from the checker at most 4.6e-16 in the same scaled units.  The library's
transform is correlation.go's radix-2 order, which xcorr_params_ref.go_fft restates, so the PCM entry is also
held, bit for bit, to the spectrum entry on the checker's go_fft |X|: the library does not expose its own |X|
rows, and this is the nearest check that needs none.

One frame per block: there is no frames-per-block or frames-per-lane boundary; F = 1, 5, 65, 66 and 130 are
covered."""
import math

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library loads HIP (one HIP runtime in the process)

import hratio_cases as HC
import hratio_ref as R
import sonar
import test_gpu_pitch

pytestmark = pytest.mark.gpu

SR = HC.SR
FIELDS = sonar.HRATIO_FRAME_FIELDS


def _close(got, want, tol):
    """|got - want| <= tol elementwise; NaN and the infinities must match as such"""
    got, want, tol = np.broadcast_arrays(np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), tol)
    fin = np.isfinite(want)
    return bool(np.array_equal(got[~fin], want[~fin], equal_nan=True) and np.all(np.abs(got[fin] - want[fin]) <= tol[fin]))


def _ulp_tol(want):
    return HC.ULP16 * np.maximum(1.0, np.abs(np.where(np.isfinite(want), want, 1.0)))


def _assert_exact(got, ref, skip=()):
    for k in HC.EXACT_KEYS:
        if k not in skip:
            assert np.array_equal(got[k], ref[k], equal_nan=True), k
    for k in HC.LOG_KEYS:
        if k not in skip:
            assert _close(got[k], ref[k], _ulp_tol(ref[k])), (k, got[k], ref[k])


def test_factor_is_the_pitch_tests():
    assert HC.FACTOR == test_gpu_pitch.FACTOR


# ---------------------------------------------------------- from spectrum ----
@pytest.mark.parametrize("method,W,F,nf", HC.SPECTRUM_CASES)
def test_from_spectrum_matches_checker(ctx, method, W, F, nf):
    """F86-F93 at K = 32, 128 and 1024, every method and noise floor"""
    mag, ph = HC.spectrum_rows(W, F)
    ref = HC.spectrum_ref(method, W, F, nf)
    p = HC.lib_params(sonar, method, W, W // 2, noise_floor_method=nf)
    got = ctx.hratio_from_spectrum(mag, p, phase=ph)
    assert got["harmonic_ratio"].shape == (F,) and got["h_bin"].shape == (F, 20) and got["noise_floor"].shape == (F, W // 2)
    _assert_exact(got, ref)
    assert np.array_equal(got["h_phase"], ref["h_phase"])            # the caller's own values at the reported bins
    none = ctx.hratio_from_spectrum(mag, p, want=("h_phase", "num_harmonics"))
    assert not none["h_phase"].any() and np.array_equal(none["num_harmonics"], ref["num_harmonics"])


@pytest.mark.parametrize("kw", [dict(spectral_smoothing_len=1, noise_floor_smoothing_len=0), dict(spectral_smoothing_len=40),
                                dict(spectral_smoothing_len=32, noise_floor_smoothing_len=32),
                                dict(noise_floor_percentile=0.0), dict(noise_floor_percentile=1.0),
                                dict(noise_floor_percentile=1.5), dict(noise_floor_percentile=0.55),
                                dict(peak_detection_width=0), dict(peak_detection_width=-2), dict(peak_detection_width=40),
                                dict(max_harmonics=64, max_freq=7900.0, harmonic_tolerance=0.5), dict(max_harmonics=1),
                                dict(max_harmonics=0), dict(max_harmonics=-1), dict(min_freq=4000.0),
                                dict(min_freq=7990.0), dict(min_peak_height=50.0), dict(min_peak_height=1e9),
                                dict(harmonic_tolerance=-0.1), dict(min_freq=3000.0, max_freq=200.0)],
                         ids=lambda v: ",".join(f"{k}={x}" for k, x in v.items()))
@pytest.mark.parametrize("method", ["hnr", "hps", "spectral"])
def test_from_spectrum_parameter_edges(ctx, method, kw):
    """F88: L = 1, L = K and L > K at K = 32; F89: p = 0, 1, outside [0, 1]; widths 0, negative and wider than
    the row; as many harmonics as fit under max_freq, one, none; a min_freq above
    every peak (F86's fallback) and a height above every magnitude (no peak at all)"""
    W, F = 64, 5
    mag, ph = HC.spectrum_rows(W, F)
    ref = R.from_spectrum(mag, ph, HC.ref_params(method, W, W // 2, **kw))
    got = ctx.hratio_from_spectrum(mag, HC.lib_params(sonar, method, W, W // 2, **kw), phase=ph)
    _assert_exact(got, ref)
    assert np.array_equal(got["h_phase"], ref["h_phase"])
    if kw.get("min_peak_height") == 1e9 and method == "hnr":
        assert not ref["f0"].any() and np.all(ref["harmonic_ratio"] == -math.inf) and not got["voicing"].any()
    if kw.get("noise_floor_percentile") == 1.5 and method == "hnr":
        assert np.all(got["snr"] == 60.0) and not got["noise_floor"].any()


def test_f87_peak_distance_rule_and_more_than_100_peaks(ctx):
    """at 8 kHz and W 2048 the detector's distance is int(20 / 3.90625) = 5 bins (the greedy runs); at 44.1 kHz it
    is 1 and a noisy row keeps more than 100 peaks, of which f0 may only be one of the 100 strongest"""
    rng = np.random.default_rng(3)
    K = 1024
    mag = rng.uniform(0.5, 1.0, (3, K))
    for sr in (8000, 44100):
        for method in ("hnr", "spectral"):
            kw = dict(spectral_smoothing_len=1, min_freq=0.45 * sr, max_freq=0.5 * sr)
            rp = R.Params(sr, method=HC.METHODS[method], window_size=2048, **kw)
            ref = R.from_spectrum(mag, None, rp)
            got = ctx.hratio_from_spectrum(mag, sonar.hratio_params_default(sr, method=method, window_size=2048, **kw))
            _assert_exact(got, ref)
    assert len(R.HP.candidates(mag[0], 0.001)) > 300


def test_f90_the_same_bin_listed_twice_and_64_harmonics(ctx):
    """Row 0: one peak at bin 20, width 30, tolerance 0.6: the windows of both harmonics hold bin 20 as their
    maximum and 1250 Hz is within 0.6 x 2500 Hz of the second target.  Row 1 at W 2048: partials 1 / h at bins
    12 h, h <= 64: every lane of findHarmonicPeaks finds its own, 2016 roughness pairs (two chunks of K)."""
    mag = np.zeros((1, 128))
    mag[0, 19:22] = 1.0, 3.0, 1.0
    kw = dict(window_size=256, spectral_smoothing_len=1, peak_detection_width=30, harmonic_tolerance=0.6, max_harmonics=2)
    got = ctx.hratio_from_spectrum(mag, sonar.hratio_params_default(SR, **kw))
    assert got["h_bin"].tolist() == [[20, 20]] and got["h_freq"].tolist() == [[1250.0, 1250.0]] and got["num_harmonics"][0] == 2
    _assert_exact(got, R.from_spectrum(mag, None, R.Params(SR, **kw)))
    mag = np.zeros((1, 1024))
    for h in range(1, 65):
        mag[0, 12 * h] = 1.0 / h
    kw = dict(window_size=2048, spectral_smoothing_len=1, max_harmonics=64)
    for method in ("hnr", "hps", "spectral"):
        got = ctx.hratio_from_spectrum(mag, sonar.hratio_params_default(SR, method=method, **kw))
        _assert_exact(got, R.from_spectrum(mag, None, R.Params(SR, method=HC.METHODS[method], **kw)))
        if method == "hps":                                            # bins from K / 2 on keep their own magnitude:
            assert got["f0"][0] == 516 * 7.8125                        # 1 / 43 at bin 516 beats 1 / 120 at bin 12
            continue
        assert got["num_harmonics"][0] == 64 and got["h_bin"][0].tolist() == [12 * h for h in range(1, 65)], method
        assert got["harmonic_ratio"][0] == 60.0                        # every peak is a harmonic: no noise energy


def test_f93_hps_scan_starts_at_bin_0(ctx):
    mag = np.full((2, 128), 0.5)
    mag[:, 0] = 4.0
    p = sonar.hratio_params_default(SR, method="hps", window_size=256, spectral_smoothing_len=1)
    got = ctx.hratio_from_spectrum(mag, p)
    assert not got["f0"].any() and not got["num_harmonics"].any() and (got["h_bin"] == -1).all()
    assert _close(got["harmonic_ratio"], np.full(2, 20.0 * math.log10(4.0 ** 5 + 1e-10)), HC.ULP16 * 61)


def test_f92_negative_infinity_and_60_db(ctx):
    mag = np.stack((np.linspace(1.0, 2.0, 128), np.zeros(128)))
    got = ctx.hratio_from_spectrum(mag, sonar.hratio_params_default(SR, window_size=256, spectral_smoothing_len=1))
    assert got["harmonic_ratio"].tolist() == [-math.inf, 60.0] and got["voicing"][0] == 0.0 and got["snr"][1] == 60.0
    assert not got["f0"].any() and not got["harmonic_energy"].any() and got["noise_energy"][0] > 0


# --------------------------------------------------------------- from PCM ----
@pytest.mark.parametrize("method,W,H,F", HC.PCM_CASES)
def test_frames_match_checker_at_measured_tolerance(ctx, method, W, H, F):
    x = HC.signal(W, H, F)
    assert len(x) == (F - 1) * H + W
    tol, measured, decided = HC.pcm_tolerance(method, W, H, F)
    a = HC.pcm_ref(method, W, H, F)
    rp = HC.ref_params(method, W, H)
    got = ctx.hratio_frames(x, HC.lib_params(sonar, method, W, H))
    print(f"{method} W {W} H {H} F {F}: numpy vs go_fft {measured:.3g}, tolerance {tol:.3g}, undecided "
          f"{np.count_nonzero(~decided)}")
    assert 0.0 < tol < 1e-11 and got["f0"].shape == (F,)
    worst = 0.0
    for f in np.nonzero(decided)[0]:
        for k in ("num_harmonics", "h_bin", "f0", "h_freq"):
            assert np.array_equal(got[k][f], a[k][f]), (k, f)
        assert _close(got["harmonicity"][f], a["harmonicity"][f], _ulp_tol(a["harmonicity"][f])), f
        s = HC.scales(a, f, rp)
        unset = {"hps": ("harmonic_energy", "noise_energy", "total_energy", "f0_confidence", "snr", "periodicity", "voicing",
                         "roughness", "noise_floor"),
                 "spectral": ("f0_confidence", "snr", "periodicity", "voicing", "roughness", "noise_floor")}.get(method, ())
        for k in ("h_amp", "f0_confidence", "noise_floor", "harmonic_energy", "noise_energy", "total_energy",
                  "harmonic_ratio", "voicing", "periodicity", "roughness", "snr"):
            if k in unset:
                assert not np.any(got[k][f]), (k, f)
                continue
            extra = _ulp_tol(a[k][f]) if k in HC.LOG_KEYS else 0.0
            assert _close(got[k][f], a[k][f], tol * s[k] + extra), (k, f, got[k][f], a[k][f], tol * s[k])
            if np.all(np.isfinite(a[k][f])) and s[k] < math.inf:
                worst = max(worst, float(np.max(np.abs(got[k][f] - a[k][f])) / s[k]))
        n = int(a["num_harmonics"][f])                               # the phase, modulo 2 pi, scaled by peak / |X| there
        raw = a["raw_magnitude"][f][a["h_bin"][f, :n]]
        d = np.abs(np.angle(np.exp(1j * (got["h_phase"][f, :n] - a["h_phase"][f, :n]))))
        assert np.all(d <= tol * a["raw_magnitude"][f].max() / raw + 4 * 2.0 ** -52 * math.pi), (f, d)
        assert not got["h_phase"][f, n:].any()
    print(f"  library vs checker, in units of the scaled tolerance's base: {worst:.3g}")
    # one sample fewer: the last frame is no longer whole
    assert ctx.hratio_frames(x[:-1], HC.lib_params(sonar, method, W, H), want=("f0",))["f0"].shape == (F - 1,)


@pytest.mark.parametrize("method,W,H,F", [c for c in HC.PCM_CASES if c[3] == 5 and c[2] != c[1]])
def test_frames_equal_from_spectrum_on_the_same_transform(ctx, method, W, H, F):
    """the PCM entry against the spectrum entry on the checker's |X| and atan2 through go_fft, the transform
    order the library runs: bit for bit (the phase within 4 ulp of pi: two atan2)"""
    x, win = HC.signal(W, H, F), R.window(W)
    rows = [R.spectrum(x[f * H:f * H + W] * win, "go") for f in range(F)]
    mag, ph = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    p = HC.lib_params(sonar, method, W, H)
    a, b = ctx.hratio_frames(x, p), ctx.hratio_from_spectrum(mag, p, phase=ph)
    for k in FIELDS:
        if k != "h_phase":
            assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert np.all(np.abs(a["h_phase"] - b["h_phase"]) <= 4 * 2.0 ** -52 * math.pi)


# ------------------------------------------------------------- ACF and YIN ----
@pytest.mark.parametrize("W,H,F", [(256, 64, 5), (2048, 512, 5), (64, 140, 3)])
def test_f94_acf_equals_autocorr_of_the_windowed_frames(ctx, W, H, F):
    """Pearson per lag at W <= 512 (lag 0 is 1: 200 dB), the frequency-domain sums at 2048 (lag 0 about W: NaN)"""
    x, win = HC.signal(W, H, F), R.window(W)
    got = ctx.hratio_frames(x, HC.lib_params(sonar, "acf", W, H))
    for f in range(F):
        corr, lags, _ = ctx.autocorr(x[f * H:f * H + W] * win, max(W, 2048))
        assert len(lags) == 2 * W - 1
        mx, mx1 = float(np.max(np.abs(corr))), float(np.max(np.abs(corr[1:])))
        assert got["voicing"][f] == mx and got["periodicity"][f] == mx1 and mx == mx1
        with np.errstate(all="ignore"):
            want = 20.0 * np.log10(np.float64(mx) / np.float64(1.0 - mx + 1e-10))
        assert _close(got["harmonic_ratio"][f], want, _ulp_tol(want)), (f, got["harmonic_ratio"][f], want)
    if W > 1000:
        assert np.isnan(got["harmonic_ratio"]).all() and got["voicing"].min() > 0.5 * W
    else:
        assert np.all(got["voicing"] == 1.0) and _close(got["harmonic_ratio"], np.full(F, 200.0), HC.ULP16 * 200)
    for k in FIELDS:
        if k not in ("harmonic_ratio", "periodicity", "voicing", "h_bin"):
            assert not got[k].any(), k
    assert (got["h_bin"] == -1).all()
    ref = R.frames(x, HC.ref_params("acf", W, H))
    assert np.array_equal(got["voicing"], ref["voicing"]) and np.array_equal(got["periodicity"], ref["periodicity"])


@pytest.mark.parametrize("W,H,F", [(256, 64, 5), (1024, 1100, 5)])
def test_f95_yin_equals_the_pitch_entries_on_the_windowed_frames(ctx, W, H, F):
    """sonar_pitch_frames_raw + sonar_pitch_track on the windowed frames laid out with hop = W, with the temporary
    detector's parameters (it windows them again): bit for bit.  Its threshold is 0, so no frame has a pitch."""
    x, win = HC.signal(W, H, F), R.window(W)
    got = ctx.hratio_frames(x, HC.lib_params(sonar, "yin", W, H))
    laid = np.concatenate([x[f * H:f * H + W] * win for f in range(F)])
    tp = sonar.pitch_params_default(SR, method="yin", window_size=W, hop_size=W, min_freq=80.0, max_freq=8000.0,
                                    yin_threshold=0.0, autocorr_threshold=0.0, min_confidence=0.0, pre_emphasis=0,
                                    window_function="hann", zero_padding=0, median_filter=0, temporal_smoothing=0,
                                    octave_correction=0)
    raw = ctx.pitch_frames_raw(laid, tp, 1, want_curve=False)
    tr = sonar.pitch_track(tp, raw["pitch"], raw["confidence"], raw["n_candidates"], raw["second_confidence"])
    assert np.array_equal(got["f0"], tr["pitch"]) and np.array_equal(got["f0_confidence"], tr["confidence"])
    assert np.array_equal(got["periodicity"], tr["periodicity"]) and np.array_equal(got["voicing"], tr["voicing"])
    want = 20.0 * np.log10(tr["confidence"] + 1e-10)
    assert _close(got["harmonic_ratio"], want, _ulp_tol(want))
    assert not got["f0"].any() and _close(got["harmonic_ratio"], np.full(F, -200.0), HC.ULP16 * 200)
    ref = R.frames(x, HC.ref_params("yin", W, H))
    assert np.array_equal(got["f0"], ref["f0"]) and np.array_equal(got["f0_confidence"], ref["f0_confidence"])
    for k in ("harmonic_energy", "noise_energy", "total_energy", "snr", "harmonicity", "roughness", "num_harmonics",
              "h_freq", "h_amp", "h_phase", "noise_floor"):
        assert not got[k].any(), k


# ---------------------------------------------------------- the whole call ----
@pytest.mark.parametrize("method", ["hnr", "acf", "hps", "comb", "spectral", "yin"])
def test_sequence_is_frames_then_track(ctx, method):
    W, H, F = 256, 64, 66
    x = HC.signal(W, H, F)
    p = HC.lib_params(sonar, method, W, H)
    fr = ctx.hratio_frames(x, p)
    want = dict(fr)
    want.update(sonar.hratio_track(p, fr["harmonic_ratio"], fr["f0"]))
    got = ctx.hratio(x, p)
    for k in sonar.HRATIO_FIELDS:
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    if method not in ("acf", "yin"):
        assert not np.array_equal(got["harmonic_ratio"], fr["harmonic_ratio"]) and got["temporal_coherence"][2:].min() > 0
    # device pointers: the PCM and every output live on the device
    xd = torch.from_numpy(x.copy()).cuda()
    outs = {k: torch.full(want[k].shape, -7, dtype=torch.from_numpy(want[k]).dtype, device="cuda") for k in sonar.HRATIO_FIELDS}
    assert ctx.hratio_device("sequence", xd.data_ptr(), len(x), p, {k: v.data_ptr() for k, v in outs.items()}) == F
    torch.cuda.synchronize()
    for k in sonar.HRATIO_FIELDS:
        assert np.array_equal(outs[k].cpu().numpy(), want[k], equal_nan=True), k
    outs = {k: torch.full(fr[k].shape, -7, dtype=torch.from_numpy(fr[k]).dtype, device="cuda") for k in FIELDS}
    assert ctx.hratio_device("frames", xd.data_ptr(), len(x), p, {k: v.data_ptr() for k, v in outs.items()}) == F
    torch.cuda.synchronize()
    for k in FIELDS:
        assert np.array_equal(outs[k].cpu().numpy(), fr[k], equal_nan=True), k


def test_from_spectrum_with_device_pointers(ctx):
    W, F = 256, 5
    mag, ph = HC.spectrum_rows(W, F)
    p = HC.lib_params(sonar, "hnr", W, W // 2)
    host = ctx.hratio_from_spectrum(mag, p, phase=ph)
    md, pd = torch.from_numpy(mag.copy()).cuda(), torch.from_numpy(ph.copy()).cuda()
    outs = {k: torch.full(host[k].shape, -7, dtype=torch.from_numpy(host[k]).dtype, device="cuda") for k in FIELDS}
    ctx.hratio_from_spectrum_device(md.data_ptr(), pd.data_ptr(), F, W // 2, p, {k: v.data_ptr() for k, v in outs.items()})
    torch.cuda.synchronize()
    for k in FIELDS:
        assert np.array_equal(outs[k].cpu().numpy(), host[k], equal_nan=True), k


@pytest.mark.parametrize("method", ["hnr", "spectral", "acf"])
def test_every_null_output_combination_leaves_the_rest_unchanged(ctx, method):
    """each output alone, and all but each: the values do not depend on which others are asked for"""
    W, H, F = 64, 16, 3
    x = HC.signal(W, H, F)
    p = HC.lib_params(sonar, method, W, H)
    full = ctx.hratio(x, p)
    names = sonar.HRATIO_FIELDS
    for k in names:
        for want in ((k,), tuple(n for n in names if n != k)):
            got = ctx.hratio(x, p, want=want)
            for n in names:
                if n in want:
                    assert np.array_equal(got[n], full[n], equal_nan=True), (want, n)
                else:
                    assert got[n] is None
    assert ctx.hratio(x, p, want=())["harmonic_ratio"] is None


def test_no_frames_succeeds_and_writes_nothing(ctx):
    for method in ("hnr", "acf", "yin"):
        p = sonar.hratio_params_default(SR, method=method)
        assert ctx.hratio_frames(np.zeros(2047), p)["f0"].shape == (0,)
        assert ctx.hratio(np.zeros(0), p)["harmonic_ratio"].shape == (0,)
    p = sonar.hratio_params_default(SR)
    assert ctx.hratio_from_spectrum(np.zeros((0, 1024)), p)["noise_floor"].shape == (0, 1024)


ERRORS = [(dict(sample_rate=0), sonar.ERR_INVALID, "harmonic ratio: hop_size and sample_rate must be at least 1"),
          (dict(hop_size=0), sonar.ERR_INVALID, "harmonic ratio: hop_size and sample_rate must be at least 1"),
          (dict(max_freq=math.inf), sonar.ERR_INVALID, None), (dict(harmonic_tolerance=math.nan), sonar.ERR_INVALID, None),
          (dict(noise_floor_percentile=math.nan), sonar.ERR_PANIC, "stat: percentile out of bounds"),
          (dict(method="hps", min_freq=-100.0), sonar.ERR_PANIC, "runtime error: index out of range [-12]"),
          (dict(window_size=1000), sonar.ERR_UNSUPPORTED, "harmonic ratio: window_size must be a power of two in [64, 2048]"),
          (dict(window_size=4096, autocorr_max_lag=4096), sonar.ERR_UNSUPPORTED, None),
          (dict(max_harmonics=65), sonar.ERR_UNSUPPORTED, "harmonic ratio: max_harmonics above 64"),
          (dict(autocorr_max_lag=2046), sonar.ERR_UNSUPPORTED, "harmonic ratio: autocorr_max_lag below window_size - 1"),
          (dict(max_freq=1e300), sonar.ERR_UNSUPPORTED, None)]


@pytest.mark.parametrize("kw,code,msg", ERRORS, ids=lambda v: str(v))
def test_errors_through_the_entries(ctx, kw, code, msg):
    p = sonar.hratio_params_default(kw.get("sample_rate", SR), **{k: v for k, v in kw.items() if k != "sample_rate"})
    K = max(p.window_size // 2, 1)
    for call in (lambda: ctx.hratio_frames(np.zeros(5000), p), lambda: ctx.hratio(np.zeros(5000), p),
                 lambda: ctx.hratio_from_spectrum(np.zeros((2, K)), p)):
        with pytest.raises(sonar.SonarError) as e:
            call()
        assert e.value.code == code
        if msg:
            assert e.value.msg == msg


def test_errors_of_single_entries(ctx):
    p = sonar.hratio_params_default(SR, window_size=256)
    for method in ("acf", "yin"):
        with pytest.raises(sonar.SonarError) as e:
            ctx.hratio_from_spectrum(np.zeros((2, 128)), sonar.hratio_params_default(SR, window_size=256, method=method))
        assert e.value.code == sonar.ERR_INVALID and "need the samples" in e.value.msg
    with pytest.raises(sonar.SonarError) as e:
        ctx.hratio_from_spectrum(np.zeros((2, 129)), p)
    assert e.value.code == sonar.ERR_INVALID and e.value.msg == "harmonic ratio: K must be window_size / 2"
    with pytest.raises(sonar.SonarError) as e:                          # F97: AnalyzeSequence panics at its first frame
        ctx.hratio(np.zeros(5000), sonar.hratio_params_default(SR, temporal_smoothing_len=-1))
    assert e.value.code == sonar.ERR_PANIC and e.value.msg == "runtime error: slice bounds out of range [3:1]"
    assert ctx.hratio(np.zeros(100), sonar.hratio_params_default(SR, temporal_smoothing_len=-1))["f0"].shape == (0,)
    assert ctx.hratio_frames(np.zeros(5000), sonar.hratio_params_default(SR, temporal_smoothing_len=-1))["f0"].shape == (6,)
