"""sonar_pitch_frames_raw / sonar_pitch_detect on the GPU against the Python checker (tests/pitch_ref.py,
pinned to the C oracle and to hand-worked answers in test_pitch_cpu.py).

YIN, NSDF, ACF and the zero-crossing count are compared bit for bit (a NaN equals a NaN) in every output
and in the curve.  The HPS and the cepstrum go through go-dsp's FFT in the reference, so their curves are
held to a tolerance that is measured, not chosen: the largest difference, on the test's own frames, between
the checker on numpy's FFT and on xcorr_params_ref.go_fft (two independent float64 orderings, on the CPU),
relative to the row's peak for the HPS and absolute for the cepstrum, times FACTOR = 16 for a third
ordering and the ln.  On 200 frames at W 1024, ZP 2 that difference measured 1.1e-15 (HPS) and 1.1e-14
(cepstrum); the test recomputes it on the frames it uses and prints it (on these frames at most 1.6e-15 for
the HPS and 2.0e-15 for the cepstrum, so tolerances of at most 2.6e-14 and 3.2e-14; the library's own
difference from the checker measured at most 1.6e-15 and 2.0e-15).  Their picks are compared exactly, after the
test has asserted that on every frame the best value leads the runner-up by more than 1000 x the tolerance.

Shapes.  W 64 (the lag range is half a wave), 128 (exactly one wave), 512 and 1024 (either side of the ACF
regime switch at 1000 samples), 2048 (the LDS ceiling); zero padding 1, 2, and 4 at W <= 1024; hop 1, W / 2,
W and one above W.  Frame counts 1 and both sides of the kernels' constants: PITCH_FRAMES_PER_BLOCK = 4
frames per block of the wave-per-frame kernels (4, 5), PITCH_STATS_FRAMES_PER_WAVE = 64 frames per wave of
the z-score pass (64, 65) and its 256 frames per block (257).  n is chosen so that the last frame ends exactly
at n; with n - 1 the count drops by one.  The signal is pitch_ref.make_signal: a fixed seed, six partials
at 0.7^h plus 0.05 noise, f0 drawn per hop from 90-900 Hz at 16 kHz."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library loads HIP (one HIP runtime in the process)

import pitch_ref as R
import sonar

pytestmark = pytest.mark.gpu

SR = 16000
FACTOR = 16
RAW_KEYS = ("pitch", "confidence", "index", "n_candidates", "second_confidence", "cand_index", "cand_conf", "curve")
# (W, hop, F)
GEOMETRY = [(64, 1, 257), (64, 70, 5), (128, 64, 65), (128, 128, 64), (512, 256, 5), (512, 512, 4),
            (1024, 512, 5), (1024, 1100, 2), (2048, 1024, 1), (2048, 1, 4)]
EXACT = ["yin", "nsdf", "acf", "zero_crossing"]


@functools.lru_cache(maxsize=None)
def _signal(W, H, F):
    x = R.make_signal(F, W, H, seed=W * 7 + H + F)
    x.setflags(write=False)
    return x


def _params(method, W, H, **kw):
    ref = R.Params(SR, method=sonar.PITCH_METHODS[method], window_size=W, hop_size=H, **kw)
    lib = sonar.pitch_params_default(SR, method=method, window_size=W, hop_size=H,
                                     **{k: (int(v) if isinstance(v, bool) else v) for k, v in kw.items()})
    return ref, lib


@functools.lru_cache(maxsize=None)
def _ref(method, W, H, F, fft="numpy", zp=2, min_freq=80.0):
    ref, _ = _params(method, W, H, zero_padding=zp, min_freq=min_freq)
    return R.frames_raw(_signal(W, H, F), ref, 8, fft)


def _same(got, ref, keys=RAW_KEYS):
    return [k for k in keys if not np.array_equal(got[k], ref[k], equal_nan=True)]


@pytest.mark.parametrize("method", EXACT)
@pytest.mark.parametrize("W,H,F", GEOMETRY)
def test_exact_methods_match_checker(ctx, method, W, H, F):
    x = _signal(W, H, F)
    assert len(x) == (F - 1) * H + W
    ref = _ref(method, W, H, F)
    assert not ref["ties"].any()                    # Go's order would be unspecified: change the seed
    _, p = _params(method, W, H)
    got = ctx.pitch_frames_raw(x, p, 8)
    assert got["pitch"].shape == (F,) and got["curve"].shape == ref["curve"].shape
    assert _same(got, ref) == []
    # one sample fewer: the last frame is no longer whole
    short = ctx.pitch_frames_raw(x[:-1], p, 8)
    assert short["pitch"].shape == (F - 1,)
    assert _same(short, {k: ref[k][:F - 1] for k in RAW_KEYS}) == []


@pytest.mark.parametrize("alias,method", [("yin_fft", "yin"), ("mpm", "nsdf")])
def test_hybrid_methods_are_their_targets(ctx, alias, method):
    W, H, F = 512, 256, 5
    _, p = _params(alias, W, H)
    assert _same(ctx.pitch_frames_raw(_signal(W, H, F), p, 8), _ref(method, W, H, F)) == []


def test_yin_at_the_defaults_equals_pitch_yin(ctx):
    W, H, F = 1024, 512, 5
    x = _signal(W, H, F)
    got = ctx.pitch_frames_raw(x, sonar.pitch_params_default(SR), 1)
    p, c, t = ctx.pitch_yin(x, SR)
    assert np.array_equal(got["pitch"], p[:F]) and np.array_equal(got["confidence"], c[:F])
    assert np.array_equal(got["index"], t[:F]) and np.count_nonzero(p[:F]) > 0


@pytest.mark.parametrize("W,H,F", [(512, 256, 5), (1024, 512, 5), (2048, 1024, 1)])
def test_acf_curve_equals_autocorr_of_the_frame(ctx, W, H, F):
    """both regimes: Pearson per lag at W 512, the frequency-domain sums at 1024 and 2048"""
    x = _signal(W, H, F)
    ref, p = _params("acf", W, H)
    got = ctx.pitch_frames_raw(x, p, 0)
    for f in range(F):
        corr, lags, _ = ctx.autocorr(R.preprocess(x[f * H:f * H + W], ref), 2 * W)
        assert len(lags) == 2 * W - 1 and np.array_equal(got["curve"][f], corr)
    if W > 1000:
        assert got["curve"][:, W - 1].min() > 0.9 * W          # lag 0 of the un-normalised sums is W
    else:
        assert np.all(got["curve"][:, W - 1] == 1.0)


@pytest.mark.parametrize("max_candidates", [0, 1, 3])
def test_fewer_reported_candidates(ctx, max_candidates):
    W, H, F = 1024, 512, 5
    ref = _ref("acf", W, H, F)
    _, p = _params("acf", W, H)
    got = ctx.pitch_frames_raw(_signal(W, H, F), p, max_candidates, want_curve=False)
    assert got["curve"] is None and got["cand_index"].shape == (F, max_candidates)
    assert _same(got, ref, ("pitch", "confidence", "index", "n_candidates", "second_confidence")) == []
    assert np.array_equal(got["cand_index"], ref["cand_index"][:, :max_candidates])
    assert np.array_equal(got["cand_conf"], ref["cand_conf"][:, :max_candidates])
    assert ref["n_candidates"].max() > 3


def test_equal_peaks_are_ordered_by_ascending_lag(ctx):
    """Ones at samples 0, 10 and 30 of a 64-sample frame (no pre-emphasis, rectangular window): over j < 32 the
    products give acf[10] = acf[20] = acf[30] = 1, m1 = 3, m2 = 2, 1, 1, so the NSDF is 0.4, 0.5, 0.5 there
    and 0 elsewhere, all in exact arithmetic.  Lag 10 is 1600 Hz, out of range; lags 20 and 30 tie at 0.5."""
    x = np.zeros(64)
    x[[0, 10, 30]] = 1.0
    ref, p = _params("nsdf", 64, 64, pre_emphasis=False, window_function="rectangular")
    r = R.frames_raw(x, ref, 8)
    assert r["ties"].all() and list(r["cand_index"][0, :3]) == [20, 30, -1]
    got = ctx.pitch_frames_raw(x, p, 8)
    assert _same(got, r) == []
    assert got["curve"][0, 10] == 0.4 and got["curve"][0, 20] == 0.5 and got["curve"][0, 30] == 0.5
    assert got["index"][0] == 20 and got["pitch"][0] == 800.0 and got["second_confidence"][0] == 0.5


SPECIAL = [("nan", True), ("inf", True), ("zero", True), ("constant", False)]


@pytest.mark.parametrize("method", EXACT)
@pytest.mark.parametrize("kind,pre", SPECIAL)
@pytest.mark.parametrize("W", [512, 1024])
def test_special_frames_match_checker(ctx, method, kind, pre, W):
    """Non-finite PCM; an all-zero frame (NSDF: m1 + m2 = 0, YIN: 0 / 0 and no minimum); a constant frame under
    the rectangular window without pre-emphasis (z-score: stdDev < minStdDev, only centred)."""
    H, F = W // 2, 3
    x = _signal(W, H, F).copy()
    if kind == "nan":
        x[H + 7] = np.nan
    elif kind == "inf":
        x[H + 7] = np.inf
    elif kind == "zero":
        x[:W] = 0.0
    else:
        x[:W] = 2.5
    kw = {} if pre else dict(pre_emphasis=False, window_function="rectangular")
    ref, p = _params(method, W, H, **kw)
    r = R.frames_raw(x, ref, 8)
    got = ctx.pitch_frames_raw(x, p, 8)
    assert _same(got, r) == []
    if kind in ("zero", "constant") and method != "zero_crossing":
        assert r["n_candidates"][0] == 0 and r["index"][0] == -1 and r["pitch"][0] == 0.0


# ------------------------------------------------------ HPS and the cepstrum ----
# (method, W, hop, F, zero padding, min_freq).  The real cepstrum of a real frame is symmetric, c[q] = c[W - q] up
# to rounding, so a scan that reaches past W / 2 has no decided pick in the reference itself: at W 64 and 128
# min_freq keeps the last quefrency int(sr / min_freq) below W / 2 (30 < 32, 61 < 64).
SPECTRAL = [("hps", 64, 32, 65, 4, 80.0), ("hps", 128, 128, 5, 2, 80.0), ("hps", 512, 256, 5, 1, 80.0),
            ("hps", 1024, 512, 5, 4, 80.0), ("hps", 1024, 1100, 4, 2, 80.0), ("hps", 2048, 1024, 2, 2, 80.0),
            ("hps", 2048, 1, 1, 1, 80.0), ("peaks", 1024, 512, 4, 2, 80.0),
            ("cepstrum", 64, 1, 257, 2, 520.0), ("cepstrum", 128, 64, 5, 2, 260.0), ("cepstrum", 512, 512, 5, 2, 80.0),
            ("cepstrum", 1024, 512, 5, 2, 80.0), ("cepstrum", 2048, 1024, 4, 2, 80.0)]


def _scan(method, W, zp, min_freq):
    """the values the scan compares: the start value and the range (Go's integers)"""
    if method == "cepstrum":
        lo, hi = int(SR / 1000.0), min(int(SR / min_freq), W)
        return lo, lo, hi
    N = W * zp
    return 0, int(min_freq * N / SR), min(int(1000.0 * N / SR), N // 2)


@pytest.mark.parametrize("method,W,H,F,zp,min_freq", SPECTRAL)
def test_spectral_methods_match_checker_at_measured_tolerance(ctx, method, W, H, F, zp, min_freq):
    base = "hps" if method == "peaks" else method
    a, b = _ref(base, W, H, F, "numpy", zp, min_freq), _ref(base, W, H, F, "go", zp, min_freq)
    peak = np.abs(a["curve"]).max(axis=1, keepdims=True) if base == "hps" else 1.0
    measured = float(np.max(np.abs(a["curve"] - b["curve"]) / peak))
    tol = FACTOR * measured
    assert 0.0 < tol < 1e-11
    # the picks are decided: on every frame the best value leads the runner-up by more than 1000 tol
    i0, lo, hi = _scan(base, W, zp, min_freq)
    for f in range(F):
        vals = a["curve"][f, lo:hi]                 # the cepstrum's start value is the range's first
        if base == "hps":
            assert lo > 0
            vals = np.concatenate(([a["curve"][f, i0]], vals))
        top = np.sort(vals)[::-1]
        scale = float(peak[f, 0]) if base == "hps" else 1.0
        assert (top[0] - top[1]) / scale > 1000 * tol, (f, top[:2])
    assert np.array_equal(a["index"], b["index"])
    _, p = _params(method, W, H, zero_padding=zp, min_freq=min_freq)
    got = ctx.pitch_frames_raw(_signal(W, H, F), p, 2)
    err = float(np.max(np.abs(got["curve"] - a["curve"]) / peak))
    print(f"{method} W {W} ZP {zp}: numpy vs go_fft {measured:.3g}, tolerance {tol:.3g}, library vs checker {err:.3g}")
    assert got["curve"].shape == a["curve"].shape and err <= tol
    assert np.array_equal(got["index"], a["index"]) and np.array_equal(got["pitch"], a["pitch"])
    assert np.array_equal(got["n_candidates"], a["n_candidates"]) and np.all(got["second_confidence"] == 0.0)
    assert np.array_equal(got["cand_index"][:, 0], a["index"]) and np.all(got["cand_index"][:, 1] == -1)
    # the confidence is a clipped multiple of the picked value: the same tolerance, scaled like it
    cscale = peak[:, 0] / 1000.0 if base == "hps" else 10.0
    assert np.all(np.abs(got["confidence"] - a["confidence"]) <= tol * cscale)
    assert np.array_equal(got["cand_conf"][:, 0], got["confidence"])


def test_hps_bin_0_start(ctx):
    """a constant frame: nothing beats hps[0], pitch 0 Hz with a confidence"""
    ref, p = _params("hps", 256, 256, zero_padding=1, pre_emphasis=False, window_function="rectangular")
    got = ctx.pitch_frames_raw(np.ones(256), p, 1)
    assert got["index"][0] == 0 and got["pitch"][0] == 0.0 and got["confidence"][0] == 1.0
    assert got["n_candidates"][0] == 1 and abs(got["curve"][0, 0] / 256.0 ** 5 - 1.0) < 1e-14


# -------------------------------------------------------------- the whole call ----
@pytest.mark.parametrize("method", ["yin", "nsdf", "acf", "hps", "cepstrum", "zero_crossing"])
def test_detect_is_raw_then_track(ctx, method):
    W, H, F = 1024, 512, 5
    x = _signal(W, H, F)
    kw = dict(min_confidence=0.2) if method == "zero_crossing" else {}
    _, p = _params(method, W, H, **kw)
    raw = ctx.pitch_frames_raw(x, p, 2, want_curve=False)
    want = sonar.pitch_track(p, raw["pitch"], raw["confidence"], raw["n_candidates"], raw["second_confidence"])
    got = ctx.pitch_detect(x, p)
    for k in sonar.PITCH_TRACK_FIELDS:
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    assert np.count_nonzero(got["pitch"]) > 0
    # device pointers: the PCM and every output live on the device
    xd = torch.from_numpy(x.copy()).cuda()
    outs = {k: torch.full((F,), -1.0, dtype=torch.float64, device="cuda") for k in sonar.PITCH_TRACK_FIELDS}
    assert ctx.pitch_detect_device(xd.data_ptr(), len(x), p, {k: v.data_ptr() for k, v in outs.items()}) == F
    for k in sonar.PITCH_TRACK_FIELDS:
        assert np.array_equal(outs[k].cpu().numpy(), want[k], equal_nan=True), k


def test_raw_with_device_pointers(ctx):
    W, H, F = 1024, 512, 5
    x = _signal(W, H, F)
    _, p = _params("acf", W, H)
    host = ctx.pitch_frames_raw(x, p, 3)
    xd = torch.from_numpy(x.copy()).cuda()
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")     # noqa: E731
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")       # noqa: E731
    d = {"pitch": f64(F), "confidence": f64(F), "index": i32(F), "n_candidates": i32(F), "second_confidence": f64(F),
         "cand_index": i32(F, 3), "cand_conf": f64(F, 3), "curve": f64(F, 2 * W - 1)}
    ctx.pitch_frames_raw_device(xd.data_ptr(), len(x), p, d["pitch"].data_ptr(), d["confidence"].data_ptr(), 3,
                                d["index"].data_ptr(), d["n_candidates"].data_ptr(),
                                d["second_confidence"].data_ptr(), d["cand_index"].data_ptr(),
                                d["cand_conf"].data_ptr(), d["curve"].data_ptr())
    torch.cuda.synchronize()
    assert _same({k: v.cpu().numpy() for k, v in d.items()}, host) == []


def test_no_frames_succeeds_and_writes_nothing(ctx):
    p = sonar.pitch_params_default(SR, method="acf")
    got = ctx.pitch_frames_raw(np.zeros(1023), p, 8)
    assert got["pitch"].shape == (0,) and got["curve"].shape == (0, 2047)
    assert ctx.pitch_detect(np.zeros(0), p)["pitch"].shape == (0,)


ERRORS = [(dict(method=7), sonar.ERR_INVALID, "unsupported pitch detection method: 7"),
          (dict(method=10), sonar.ERR_INVALID, "unsupported pitch detection method: 10"),
          (dict(method=99), sonar.ERR_INVALID, "unsupported pitch detection method: 99"),
          (dict(hop_size=0), sonar.ERR_INVALID, None), (dict(min_freq=1000.0), sonar.ERR_INVALID, None),
          (dict(max_freq=float("inf")), sonar.ERR_INVALID, None),
          (dict(method="hps", zero_padding=0), sonar.ERR_PANIC, "runtime error: index out of range [0] with length 0"),
          (dict(method="cepstrum", window_size=128, max_freq=125.0), sonar.ERR_PANIC,
           "runtime error: index out of range [128] with length 128"),
          (dict(window_size=1000), sonar.ERR_UNSUPPORTED, None), (dict(window_size=4096), sonar.ERR_UNSUPPORTED, None),
          (dict(method="hps", zero_padding=3), sonar.ERR_UNSUPPORTED, None),
          (dict(method="hps", window_size=2048, zero_padding=4), sonar.ERR_UNSUPPORTED, None)]


@pytest.mark.parametrize("kw,code,msg", ERRORS, ids=lambda v: str(v))
def test_errors_through_the_entries(ctx, kw, code, msg):
    p = sonar.pitch_params_default(SR, **kw)
    for call in (lambda: ctx.pitch_frames_raw(np.zeros(5000), p, 8), lambda: ctx.pitch_detect(np.zeros(5000), p)):
        with pytest.raises(sonar.SonarError) as e:
            call()
        assert e.value.code == code
        if msg:
            assert e.value.msg == msg


def test_max_candidates_outside_0_to_8(ctx):
    p = sonar.pitch_params_default(SR)
    for k in (-1, 9):
        with pytest.raises(sonar.SonarError) as e:
            ctx.pitch_frames_raw(np.zeros(5000), p, k)
        assert e.value.code == sonar.ERR_INVALID
