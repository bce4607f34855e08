"""sonar_inharm_from_spectrum / sonar_inharm_frames / sonar_inharm on the GPU against the Python checker
(tests/inharm_ref.py, pinned to hand-worked answers in test_inharm_cpu.py; the cases are inharm_cases.py's).

From spectrum the inputs are the same bits on both sides, so every discrete output, every frequency, deviation
and sum is compared bit for bit (inharm_cases.EXACT_KEYS); the outputs that pass through log10 or exp (the
clarity, the purity, the String model's fit, the chi-squared statistic and its p-value; with FletcherMunson
above 4 kHz also its weights and what is made of them) within 16 x 2^-52 x max(1, |expected|), hratio_cases.ULP16
as test_gpu_hratio.py scales it; +-Inf and NaN match as such.

From PCM the f0 is sonar_pitch_detect's, bit for bit, and every output equals the spectrum entry on the checker's
go_fft |X| with that f0, bit for bit: the library's transform is correlation.go's radix-2 order, which
xcorr_params_ref.go_fft restates.  The reference's own transform is go-dsp's, so against the checker on numpy's
transform the discrete outputs, frequencies and deviations are equal on decided frames (test_inharm_cpu.py shows
every frame of every case is decided; the cap of 10 % is asserted here all the same) and the amplitude-borne
outputs are held to FACTOR (test_gpu_pitch.py's) x the measured numpy-vs-go_fft difference of the case's rows,
relative to the row's peak and scaled per output (_amp_scales); each case prints it.

One frame per block: there is no frames-per-block boundary; F = 1, 5, 65, 66 and 130 are covered."""
import math

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library loads HIP (one HIP runtime in the process)

import hratio_cases as HC
import inharm_cases as IC
import inharm_ref as R
import sonar
import test_gpu_pitch

pytestmark = pytest.mark.gpu

FIELDS = sonar.INHARM_FRAME_FIELDS
MODELS = ("string", "pipe", "membrane", "general")


def _close(got, want, tol):
    """|got - want| <= tol elementwise; NaN and the infinities must match as such"""
    got, want, tol = np.broadcast_arrays(np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), tol)
    fin = np.isfinite(want)
    return bool(np.array_equal(got[~fin], want[~fin], equal_nan=True) and np.all(np.abs(got[fin] - want[fin]) <= tol[fin]))


def _ulp_tol(want):
    return HC.ULP16 * np.maximum(1.0, np.abs(np.where(np.isfinite(want), want, 1.0)))


def _log_keys(method, model, fm_log=False):
    """the outputs of a case that pass through log10 or exp"""
    keys = ["harmonic_clarity", "spectral_purity"]
    if model == "string":
        keys.append("model_fit_quality")
    if method == "statistical":
        keys += ["chi_squared", "p_value"]
    if method == "fletcher_munson" and fm_log:                     # its weight above 4 kHz is 1 - 0.3 log10(f / 4000)
        keys += ["h_deviation", "inharmonicity", "std_dev"]
        if model == "string":
            keys.append("estimated_stiffness")
    return keys


def _assert_rows(got, ref, method, model, fm_log=False, rows=slice(None)):
    logs = _log_keys(method, model, fm_log)
    for k in FIELDS:
        g, r = got[k][rows], ref[k][rows]
        assert g.shape == r.shape and g.dtype == r.dtype, k
        if k in logs:
            assert _close(g, r, _ulp_tol(r)), (k, g, r)
        else:
            assert np.array_equal(g, r, equal_nan=True), (k, np.argwhere(g != r)[:3])


# ---------------------------------------------------------- from spectrum ----
@pytest.mark.parametrize("F", IC.SPECTRUM_F)
@pytest.mark.parametrize("K", sorted(IC.SPECTRUM_K))
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("method", IC.SPECTRUM_METHODS)
def test_from_spectrum_matches_checker(ctx, method, model, K, F):
    """F101-F105 at K = 32 and 512, every method but BeatPattern and every model"""
    mag, f0, fc = IC.spectrum_rows(K)
    ref = IC.spectrum_ref(K, method, model)
    p = IC.lib_params(sonar, IC.SPECTRUM_K[K], method, model, window_size=2 * K, **dict(IC.SPECTRUM_EXTRA[K]))
    got = ctx.inharm_from_spectrum(mag[:F], f0[:F], fc[:F], p)
    assert got["status"].shape == (F,) and got["h_number"].shape == (F, 20)
    _assert_rows(got, ref, method, model, fm_log=K == 32, rows=slice(0, F))
    assert np.array_equal(got["f0"], f0[:F]) and np.array_equal(got["f0_confidence"], fc[:F])
    bad = got["status"] != R.OK
    for k in FIELDS:
        if k not in ("status", "f0", "f0_confidence", "num_harmonics", "quality", "h_number"):
            assert not got[k][bad].any(), k
    assert (got["h_number"][bad] == -1).all()
    assert (got["quality"][got["status"] == R.INVALID_F0] == 5).all() and (got["quality"][got["status"] == R.INSUFFICIENT] == -1).all()


EDGES = [dict(max_harmonics=64), dict(max_harmonics=1, min_harmonics=1), dict(max_harmonics=0, min_harmonics=0),
         dict(max_harmonics=-1, min_harmonics=0), dict(min_harmonics=0), dict(min_harmonics=25),
         dict(harmonic_tolerance=0.0, min_harmonics=0), dict(harmonic_tolerance=-0.1, min_harmonics=0),
         dict(harmonic_tolerance=40.0, max_harmonics=64), dict(min_harmonic_strength=1e9, min_harmonics=0),
         dict(weight_by_amplitude=False), dict(use_robust_estimation=False), dict(outlier_threshold=0.0),
         dict(outlier_threshold=math.nan), dict(max_freq=500.0, min_harmonics=1), dict(min_harmonics=2),
         dict(string_tension=2.5, string_length=0.65)]


@pytest.mark.parametrize("K", sorted(IC.SPECTRUM_K))
@pytest.mark.parametrize("kw", EDGES, ids=lambda v: str(v))
@pytest.mark.parametrize("method", ("railsback", "fletcher_munson", "spectral_deviation", "statistical"))
def test_from_spectrum_parameter_edges(ctx, method, kw, K):
    """the String model throughout (it also reads the Railsback fit and every method's B); 24 frames"""
    F = 24
    mag, f0, fc = IC.spectrum_rows(K)
    extra = tuple(sorted({**dict(IC.SPECTRUM_EXTRA[K]), **kw}.items()))
    ref = IC.spectrum_ref(K, method, "string", extra)
    p = IC.lib_params(sonar, IC.SPECTRUM_K[K], method, "string", window_size=2 * K, **dict(extra))
    got = ctx.inharm_from_spectrum(mag[:F], f0[:F], fc[:F], p)
    assert got["h_number"].shape == (F, max(kw.get("max_harmonics", 20), 0))
    fm_log = K == 32 or kw.get("harmonic_tolerance", 0) > 1
    _assert_rows(got, ref, method, "string", fm_log=fm_log, rows=slice(0, F))
    if kw.get("min_harmonics") == 25 or "min_harmonic_strength" in kw and kw.get("min_harmonics") != 0:
        assert (got["status"] != R.OK).all()
    if "max_freq" in kw:                                              # the edge is max_freq below 2 f0: one harmonic
        one = (got["status"] == R.OK) & (2.0 * f0[:F] > kw["max_freq"])
        assert one.any() and (got["num_harmonics"][one] == 1).all() and (got["h_number"][one, 1:] == -1).all()
    if kw.get("max_harmonics", 20) <= 0:
        assert not got["num_harmonics"].any()
    if kw.get("max_harmonics", 20) == 0:
        assert (got["quality"][got["status"] == R.OK] == 0).all()           # 0 / 0 harmonics: a NaN score is Very Poor


def test_f102_the_scan_clamps_at_both_ends_of_the_row(ctx):
    """a tolerance wide enough that every harmonic's window is the whole row: each returns the row's maximum, when
    that is a strict local maximum inside 1 .. K - 2, and nothing when it sits at an end"""
    K, sr = 32, 16000
    mag = np.zeros((3, K))
    mag[0, 5], mag[1, 0], mag[2, K - 1] = 2.0, 2.0, 2.0
    mag[:, 9] = 1.0
    p = IC.lib_params(sonar, sr, "spectral_deviation", harmonic_tolerance=500.0, max_freq=8000.0, min_harmonics=0,
                      window_size=64)
    got = ctx.inharm_from_spectrum(mag, [1250.0] * 3, [0.9] * 3, p)
    ref = R.from_spectrum(mag, [1250.0] * 3, [0.9] * 3, IC.ref_params(sr, "spectral_deviation", harmonic_tolerance=500.0,
                                                                       max_freq=8000.0, min_harmonics=0, window_size=64))
    _assert_rows(got, ref, "spectral_deviation", "general")
    assert got["num_harmonics"].tolist() == [6, 0, 0] and (got["h_freq"][0, :6] == 1250.0).all()


@pytest.mark.parametrize("K", [5, 33, 511])
@pytest.mark.parametrize("method", ("railsback", "statistical"))
def test_from_spectrum_takes_an_odd_k(ctx, method, K):
    """K = W / 2 for any even W: an odd K is a row like any other (W = 2 K); the first K bins of the K = 512 rows"""
    F = 24
    mag, f0, fc = IC.spectrum_rows(512)
    rows = np.ascontiguousarray(mag[:F, :K])
    kw = dict(window_size=2 * K, min_harmonics=1, max_freq=20000.0, harmonic_tolerance=0.2)
    sr = 44100 * 2 * K // 1024                                         # bins as wide as the K = 512 rows'
    ref = R.from_spectrum(rows, f0[:F], fc[:F], IC.ref_params(sr, method, "string", **kw))
    got = ctx.inharm_from_spectrum(rows, f0[:F], fc[:F], IC.lib_params(sonar, sr, method, "string", **kw))
    _assert_rows(got, ref, method, "string")
    assert (got["status"] == R.OK).any() or K == 5


def test_f104_railsback_reaches_the_nan_grid_points(ctx):
    """frames with a harmonic number >= 11 skip grid points; the fit still equals the checker's, and with an
    observed NaN every error is NaN and B stays 0"""
    mag, f0, fc = IC.spectrum_rows(512)
    ref = IC.spectrum_ref(512, "railsback", "general")
    rows = np.flatnonzero((ref["h_number"].max(axis=1) >= 11) & (ref["status"] == R.OK))
    assert len(rows) >= 3
    p = IC.lib_params(sonar, 44100, "railsback", window_size=1024)
    got = ctx.inharm_from_spectrum(mag[rows], f0[rows], fc[rows], p)
    assert np.array_equal(got["inharmonicity"], ref["inharmonicity"][rows]) and np.array_equal(got["r_squared"], ref["r_squared"][rows])
    assert set(got["inharmonicity"].tolist()) <= set(R.GRID)


# ---------------------------------------------------------------- from PCM ----
def _amp_scales(ref, f, method, max_h):
    """What one unit of relative |X| error (in units of the row's peak) can move each amplitude-borne output of
    frame f by, absolutely, from the reference's own values.  One amplitude moves by peak.  The confidence of
    SpectralDeviation and FletcherMunson is (n / max_harmonics) mean(amplitude): (n / max_harmonics) peak.  The
    clarity is (20 / 60) log10(max / min): (1 / (3 ln 10)) (peak / max + peak / min).  SpectralDeviation's
    coefficient is num / den with num = sum w d n^2 and den = sum w n^4: (sum |d| n^2 + |B| sum n^4) peak / den."""
    peak = float(ref["magnitude"][f].max())
    n = int(ref["num_harmonics"][f])
    s = {"h_amp": peak, "confidence": 0.0, "harmonic_clarity": 0.0, "inharmonicity": 0.0}
    if n == 0 or ref["status"][f] != R.OK:
        return s
    amp, num = ref["h_amp"][f, :n], ref["h_number"][f, :n].astype(np.float64)
    s["harmonic_clarity"] = (peak / amp.max() + peak / amp.min()) / (3.0 * math.log(10.0))
    if method in ("spectral_deviation", "partial_tracking", "fletcher_munson"):
        s["confidence"] = n / float(max_h) * peak
    if method in ("spectral_deviation", "partial_tracking"):
        den = float(np.sum(amp * num ** 4))
        dev = np.abs(ref["h_deviation"][f, :n])
        s["inharmonicity"] = (float(np.sum(dev * num ** 2)) + abs(float(ref["inharmonicity"][f])) * float(np.sum(num ** 4))) * peak / den
    return s


PCM_CASES = [("tone", sr, F, hop, m) for sr in (16000, 44100) for hop in IC.PCM_HOPS for F in IC.PCM_F
             for m in ("spectral_deviation", "railsback")] + \
            [("step", 44100, 66, 512, m) for m in ("fletcher_munson", "statistical", "partial_tracking")] + \
            [("sine", 16000, 5, 512, "spectral_deviation"), ("noise", 44100, 5, 1024, "statistical"),
             ("silence", 16000, 5, 512, "railsback")]


@pytest.mark.parametrize("kind,sr,F,hop,method", PCM_CASES)
def test_frames_match_pitch_detect_spectrum_entry_and_checker(ctx, kind, sr, F, hop, method):
    x = IC.signal(kind, sr, F, hop)
    assert len(x) == (F - 1) * hop + 1024
    p = IC.lib_params(sonar, sr, method, window_size=1024)
    got = ctx.inharm_frames(x, hop, p)
    # F101: the default detector's tracked pitch and confidence
    pd = ctx.pitch_detect(x, sonar.pitch_params_default(sr, hop_size=hop))
    assert np.array_equal(got["f0"], pd["pitch"]) and np.array_equal(got["f0_confidence"], pd["confidence"])
    # the spectrum entry on the checker's radix-2 |X| with that f0: bit for bit
    go = IC.pcm_ref(kind, sr, F, hop, method, fft="go")
    again = ctx.inharm_from_spectrum(go["magnitude"], got["f0"], got["f0_confidence"], p)
    for k in FIELDS:
        assert np.array_equal(got[k], again[k], equal_nan=True), k
    # the checker on numpy's transform
    a = IC.pcm_ref(kind, sr, F, hop, method, fft="numpy")
    assert np.array_equal(got["f0"], a["f0"]) and np.array_equal(got["f0_confidence"], a["f0_confidence"])
    decided = a["decided"]
    peak = np.maximum(a["magnitude"].max(axis=1, keepdims=True), 1e-300)
    measured = float(np.max(np.abs(a["magnitude"] - a["magnitude_other"]) / peak))
    tol = test_gpu_pitch.FACTOR * measured
    print(f"{kind} {sr} F {F} hop {hop} {method}: numpy vs go_fft {measured:.3g}, tolerance {tol:.3g}, undecided "
          f"{np.count_nonzero(~decided)}")
    assert np.count_nonzero(~decided) <= 0.1 * F and tol < 1e-11
    amp_keys = ("h_amp", "confidence", "harmonic_clarity", "inharmonicity")
    logs = _log_keys(method, "general")
    worst = 0.0
    for f in np.flatnonzero(decided):
        s = _amp_scales(a, f, method, 20)
        for k in FIELDS:
            if k in amp_keys:
                extra = _ulp_tol(a[k][f]) if (k in logs or s[k] > 0) else 0.0
                assert _close(got[k][f], a[k][f], tol * s[k] + extra), (k, f, got[k][f], a[k][f], tol * s[k])
                if s[k] > 0 and np.all(np.isfinite(a[k][f])):
                    worst = max(worst, float(np.max(np.abs(got[k][f] - a[k][f])) / s[k]))
            elif k in logs:
                assert _close(got[k][f], a[k][f], _ulp_tol(a[k][f])), (k, f)
            else:
                assert np.array_equal(got[k][f], a[k][f], equal_nan=True), (k, f, got[k][f], a[k][f])
    print(f"  library vs checker, in units of the row's peak: {worst:.3g}")
    # one sample fewer: the last frame is no longer whole
    assert ctx.inharm_frames(x[:-1], hop, p, want=("f0",))["f0"].shape == (F - 1,)


@pytest.mark.parametrize("kind,sr,F,hop", [("tone", 44100, 5, 512), ("step", 44100, 66, 1024), ("tone", 16000, 1, 512)])
def test_f106_beat_pattern(ctx, kind, sr, F, hop):
    """inharmonicity from the library's own correlation of the raw frame, bit for bit; the harmonic search, the
    count and the metrics are SpectralDeviation's; no confidence and no arrays"""
    x = IC.signal(kind, sr, F, hop)
    kw = dict(window_size=1024, min_harmonics=1, model="string")
    got = ctx.inharm_frames(x, hop, IC.lib_params(sonar, sr, "beat_pattern", **kw))
    sd = ctx.inharm_frames(x, hop, IC.lib_params(sonar, sr, "spectral_deviation", **kw))
    ok = got["status"] == R.OK
    assert ok.any() and np.array_equal(got["status"], sd["status"]) and np.array_equal(got["num_harmonics"], sd["num_harmonics"])
    for f in range(F):
        corr, lags, _ = ctx.autocorr(x[f * hop:f * hop + 1024], 1024)
        assert len(corr) == 2047
        want = R.beat_value(corr.tolist(), lags.tolist()) if ok[f] else 0.0
        assert got["inharmonicity"][f] == want, f
    for k in ("harmonic_clarity", "spectral_purity", "partial_coherence", "f0", "f0_confidence"):
        assert np.array_equal(got[k], sd[k]), k
    for k in ("std_dev", "confidence", "n_deviations", "h_freq", "h_ideal", "h_amp", "h_deviation", "r_squared", "chi_squared",
              "p_value"):
        assert not got[k].any(), k
    assert (got["h_number"] == -1).all()
    assert np.array_equal(got["estimated_stiffness"], got["inharmonicity"] * 1.0 * 1.0 * 1.0)
    with pytest.raises(sonar.SonarError) as e:
        ctx.inharm_from_spectrum(np.zeros((2, 512)), [100.0, 100.0], [1.0, 1.0], IC.lib_params(sonar, sr, "beat_pattern"))
    assert e.value.code == sonar.ERR_INVALID and "needs the samples" in e.value.msg


# ------------------------------------------------------------ the sequence ----
SEQ = [("tone", "spectral_deviation", dict(use_temporal_tracking=True)),
       ("step", "railsback", dict(use_temporal_tracking=True, temporal_window=3, min_harmonics=1)),
       ("step", "statistical", dict(use_temporal_tracking=True, temporal_window=0, min_harmonics=1)),
       ("step", "fletcher_munson", dict(min_harmonics=1)), ("noise", "spectral_deviation", dict(use_temporal_tracking=True))]


@pytest.mark.parametrize("kind,method,kw", SEQ, ids=lambda v: str(v))
def test_f107_sequence_is_frames_then_track(ctx, kind, method, kw):
    sr, F, hop = 44100, 66, 512
    x = IC.signal(kind, sr, F, hop)
    p = IC.lib_params(sonar, sr, method, window_size=1024, **kw)
    fr = ctx.inharm_frames(x, hop, p)
    want = dict(fr)
    want.update(sonar.inharm_track(p, fr["inharmonicity"], fr["f0"], fr["status"]))
    ref = R.track(IC.ref_params(sr, method, window_size=1024, **kw), fr["inharmonicity"], fr["f0"], fr["status"])
    for k in ref:
        assert np.array_equal(want[k], ref[k], equal_nan=True), k
    got = ctx.inharm(x, hop, p)
    assert set(got) == set(sonar.INHARM_FIELDS)
    for k in sonar.INHARM_FIELDS:
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    if kw.get("use_temporal_tracking") and kw.get("temporal_window", 10) > 2 and kind != "noise":
        assert got["temporal_stability"].any() and got["f0_stability"].any() and got["inharmonicity_trend"].any()
        assert not np.array_equal(got["inharmonicity"], fr["inharmonicity"])
    else:
        assert not got["temporal_stability"].any() and np.array_equal(got["inharmonicity"], fr["inharmonicity"])
    # device pointers: the same bits
    xd = torch.from_numpy(x.copy()).cuda()
    outs = {k: torch.full(want[k].shape, -7, dtype=torch.from_numpy(want[k]).dtype, device="cuda") for k in sonar.INHARM_FIELDS}
    assert ctx.inharm_device("sequence", xd.data_ptr(), len(x), hop, p, {k: v.data_ptr() for k, v in outs.items()}) == F
    torch.cuda.synchronize()
    for k in sonar.INHARM_FIELDS:
        assert np.array_equal(outs[k].cpu().numpy(), want[k], equal_nan=True), k
    outs = {k: torch.full(fr[k].shape, -7, dtype=torch.from_numpy(fr[k]).dtype, device="cuda") for k in FIELDS}
    assert ctx.inharm_device("frames", xd.data_ptr(), len(x), hop, p, {k: v.data_ptr() for k, v in outs.items()}) == F
    torch.cuda.synchronize()
    for k in FIELDS:
        assert np.array_equal(outs[k].cpu().numpy(), fr[k], equal_nan=True), k


def test_f103_first_insufficient_frame_is_the_sequence_error(ctx):
    """AnalyzeSequence returns nil and the error (:1186-1188): Go's message, the frame, and the rows before it"""
    sr, F, hop = 44100, 66, 512
    x = IC.signal("step", sr, F, hop)
    p = IC.lib_params(sonar, sr, "spectral_deviation", window_size=1024, use_temporal_tracking=True)
    fr = ctx.inharm_frames(x, hop, p)
    bad = int(np.flatnonzero(fr["status"] == R.INSUFFICIENT)[0])
    assert bad > 3
    with pytest.raises(sonar.SonarError) as e:
        ctx.inharm(x, hop, p)
    assert e.value.code == sonar.ERR_INVALID and e.value.frame == bad
    assert e.value.msg == "insufficient harmonics found: %d < 3" % fr["num_harmonics"][bad]
    tr = sonar.inharm_track(p, fr["inharmonicity"][:bad], fr["f0"][:bad], fr["status"][:bad])
    for k in sonar.INHARM_FIELDS:
        want = tr[k] if k in tr else fr[k][:bad]
        assert np.array_equal(e.value.rows[k][:bad], want, equal_nan=True), k
    ref = IC.pcm_ref("step", sr, F, hop, "spectral_deviation")
    assert int(np.flatnonzero(ref["status"] == R.INSUFFICIENT)[0]) == bad
    with pytest.raises(R.InsufficientHarmonics) as g:
        R.sequence(x, hop, IC.ref_params(sr, "spectral_deviation", window_size=1024))
    assert str(g.value) == e.value.msg and g.value.frame == bad
    # the pure sine fails at its first frame
    with pytest.raises(sonar.SonarError) as e:
        ctx.inharm(IC.signal("sine", sr, 5, hop), hop, p)
    assert e.value.frame == 0 and e.value.msg == "insufficient harmonics found: 1 < 3"


def test_f107_negative_window_panics_at_the_first_tracked_frame(ctx):
    sr, hop = 44100, 512
    p = IC.lib_params(sonar, sr, "spectral_deviation", window_size=1024, use_temporal_tracking=True, temporal_window=-1)
    with pytest.raises(sonar.SonarError) as e:
        ctx.inharm(IC.signal("tone", sr, 5, hop), hop, p)
    assert e.value.code == sonar.ERR_PANIC and e.value.msg == "runtime error: slice bounds out of range [2:1]"
    got = ctx.inharm(IC.signal("noise", sr, 5, hop), hop, p)             # no frame reaches the history
    assert (got["status"] == R.INVALID_F0).all()
    assert ctx.inharm_frames(IC.signal("tone", sr, 5, hop), hop, p)["status"].tolist() == [0] * 5


def test_f100_only_window_1024_analyses_anything(ctx):
    """with a frame due, the defaults' 4096 (or 512) gives Go's message; n < W succeeds with no frames"""
    x = IC.signal("tone", 44100, 5, 1024)
    for W in (4096, 512):
        p = sonar.inharm_params_default(44100, window_size=W)
        for call in (lambda: ctx.inharm_frames(x, 512, p), lambda: ctx.inharm(x, 512, p)):
            with pytest.raises(sonar.SonarError) as e:
                call()
            assert e.value.code == sonar.ERR_INVALID
            assert e.value.msg == "audio frame size (%d) doesn't match window size (1024)" % W
    assert sonar.inharm_params_default(44100).window_size == 4096
    assert ctx.inharm_frames(x[:4095], 512, sonar.inharm_params_default(44100))["status"].shape == (0,)
    assert ctx.inharm(x[:1023], 512, sonar.inharm_params_default(44100, window_size=1024))["inharmonicity"].shape == (0,)
    assert ctx.inharm(np.zeros(0), 512, sonar.inharm_params_default(44100))["h_number"].shape == (0, 20)
    p = sonar.inharm_params_default(44100, window_size=1024)
    assert ctx.inharm_from_spectrum(np.zeros((0, 512)), [], [], p)["h_freq"].shape == (0, 20)


# ------------------------------------------------ pointers and NULL outputs ----
def test_from_spectrum_with_device_pointers(ctx):
    K, F = 512, 66
    mag, f0, fc = IC.spectrum_rows(K)
    for method in ("railsback", "statistical"):
        p = IC.lib_params(sonar, 44100, method, "string", window_size=1024)
        host = ctx.inharm_from_spectrum(mag[:F], f0[:F], fc[:F], p)
        md, fd, cd = (torch.from_numpy(np.ascontiguousarray(a[:F]).copy()).cuda() for a in (mag, f0, fc))
        outs = {k: torch.full(host[k].shape, -7, dtype=torch.from_numpy(host[k]).dtype, device="cuda") for k in FIELDS}
        ctx.inharm_from_spectrum_device(md.data_ptr(), fd.data_ptr(), cd.data_ptr(), F, K, p, {k: v.data_ptr() for k, v in outs.items()})
        torch.cuda.synchronize()
        for k in FIELDS:
            assert np.array_equal(outs[k].cpu().numpy(), host[k], equal_nan=True), k
    # a non-finite f0: refused where the host can read it, an INVALID_F0 row where it cannot
    bad = np.array([200.0, math.nan, math.inf])
    with pytest.raises(sonar.SonarError) as e:
        ctx.inharm_from_spectrum(mag[:3], bad, fc[:3], p)
    assert e.value.code == sonar.ERR_INVALID and e.value.msg == "inharmonicity: non-finite f0"
    bd = torch.from_numpy(bad).cuda()
    st = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    ctx.inharm_from_spectrum_device(md.data_ptr(), bd.data_ptr(), cd.data_ptr(), 3, K, p, {"status": st.data_ptr()})
    torch.cuda.synchronize()
    assert st.cpu().tolist()[1:] == [R.INVALID_F0, R.INVALID_F0]


@pytest.mark.parametrize("method", ["railsback", "statistical"])
def test_every_null_output_combination_leaves_the_rest_unchanged(ctx, method):
    """each output alone, and all but each: the values do not depend on which others are asked for"""
    sr, F, hop = 44100, 5, 512
    x = IC.signal("step", sr, F, hop)
    p = IC.lib_params(sonar, sr, method, "string", window_size=1024, min_harmonics=1, use_temporal_tracking=True)
    full = ctx.inharm(x, hop, p)
    names = sonar.INHARM_FIELDS
    for k in names:
        for want in ((k,), tuple(n for n in names if n != k)):
            got = ctx.inharm(x, hop, p, want=want)
            for n in names:
                if n in want:
                    assert np.array_equal(got[n], full[n], equal_nan=True), (want, n)
                else:
                    assert got[n] is None
    assert ctx.inharm(x, hop, p, want=())["inharmonicity"] is None
    mag, f0, fc = IC.spectrum_rows(512)
    full = ctx.inharm_from_spectrum(mag[:9], f0[:9], fc[:9], p)
    for k in FIELDS:
        got = ctx.inharm_from_spectrum(mag[:9], f0[:9], fc[:9], p, want=(k,))
        assert np.array_equal(got[k], full[k], equal_nan=True) and all(got[n] is None for n in FIELDS if n != k), k


ERRORS = [(dict(sample_rate=0), sonar.ERR_INVALID, "inharmonicity: sample_rate must be at least 1"),
          (dict(max_freq=math.inf), sonar.ERR_INVALID, None), (dict(harmonic_tolerance=math.nan), sonar.ERR_INVALID, None),
          (dict(min_harmonic_strength=math.nan), sonar.ERR_INVALID, None),
          (dict(max_harmonics=65), sonar.ERR_UNSUPPORTED, "inharmonicity: max_harmonics above 64"),
          (dict(max_freq=1e300), sonar.ERR_UNSUPPORTED, "inharmonicity: the search window does not fit an int32 of bins")]


@pytest.mark.parametrize("kw,code,msg", ERRORS, ids=lambda v: str(v))
def test_errors_through_the_entries(ctx, kw, code, msg):
    p = sonar.inharm_params_default(kw.get("sample_rate", 44100), window_size=1024,
                                    **{k: v for k, v in kw.items() if k != "sample_rate"})
    for call in (lambda: ctx.inharm_frames(np.zeros(5000), 512, p), lambda: ctx.inharm(np.zeros(5000), 512, p),
                 lambda: ctx.inharm_from_spectrum(np.zeros((2, 512)), [100.0, 100.0], [1.0, 1.0], p)):
        with pytest.raises(sonar.SonarError) as e:
            call()
        assert e.value.code == code
        if msg:
            assert e.value.msg == msg


def test_errors_of_single_entries(ctx):
    p = sonar.inharm_params_default(44100, window_size=1024)
    for K in (2, 3, 4097):
        with pytest.raises(sonar.SonarError) as e:
            ctx.inharm_from_spectrum(np.zeros((2, K)), [100.0, 100.0], [1.0, 1.0], p)
        assert e.value.code == sonar.ERR_INVALID and e.value.msg == "inharmonicity: K must be in [4, 4096]"
    with pytest.raises(sonar.SonarError) as e:
        ctx.inharm_frames(np.zeros(5000), 0, p)
    assert e.value.code == sonar.ERR_INVALID and e.value.msg == "inharmonicity: hop_size must be at least 1"
    got = ctx.inharm_from_spectrum(np.ones((2, 4096)), [100.0, 100.0], [1.0, 1.0], sonar.inharm_params_default(44100))
    assert got["status"].tolist() == [R.INSUFFICIENT] * 2 and got["num_harmonics"].tolist() == [0, 0]    # a flat row has no peak
