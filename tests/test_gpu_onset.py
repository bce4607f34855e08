"""The onset and tempo entries on the GPU against the Python checker (tests/onset_ref.py, held to known
answers in test_onset_cpu.py).

Everything that starts from a spectrum, a curve or an envelope is bit-exact: the flux, the RMS envelope,
the energy difference, the adaptive threshold and the autocorrelation are ordered IEEE sums, products,
quotients and square roots, and the peaks, the combined onsets and the tempo votes are comparisons on
them.  One thing is not compared: which NaN an invalid operation makes, so a NaN equals a NaN (_same, as
in test_gpu_hps).  The only tolerance is the transform's: the rows sonar_onsets_flux returns are held to
numpy's rfft of the unwindowed frames at 1e-11 of the frame's peak on the fused transform and 1e-10 on
the DFT path (parity.assert_rel), the bounds of the existing float64 magnitude tests, and the flux and
the onsets of that call are then held bit for bit to sonar_spectral_flux and sonar_onset_peaks on those
same rows.

Shapes: the flux and envelope kernels give a wave 64 outputs and walk 32 columns per tile, so rows and
frames run over both sides of 64 and row lengths over 1..4, both sides of 64, 513 and the largest row;
the peak kernels keep a bit per frame in 64-bit words, 4,096 words per LDS tile, so curve lengths run
over 0..4, both sides of 64, 4097 and one length past a tile; minIntervalFrames over the values at which
the greedy starts to act (3) and both sides of it."""
import functools
import math

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library loads HIP (one HIP runtime in the process)

import onset_ref as R
import sonar
from parity import assert_rel

pytestmark = pytest.mark.gpu


def _same(a, b):
    """Equal bits, except that any NaN equals any NaN."""
    a, b = (np.atleast_1d(np.ascontiguousarray(v, dtype=np.float64)) for v in (a, b))
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    if not np.array_equal(nan, np.isnan(b)):
        return False
    return np.array_equal(a.view(np.uint64)[~nan], b.view(np.uint64)[~nan])


def _dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
    torch.cuda.synchronize()
    return t


# ---- sonar_spectral_flux -------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _rows(F, K):
    rng = np.random.default_rng(100 * K + F)
    m = np.abs(rng.standard_normal((F, K)))
    if F >= 3 and K >= 2:
        m[1, : K // 2] = m[0, : K // 2]                      # equal neighbours: d = 0
    m.setflags(write=False)
    return m


FLUX_SHAPES = [(F, K) for K in (1, 2, 3, 4, 63, 64, 65) for F in (2, 3, 65)] + \
              [(0, 5), (1, 5), (63, 33), (64, 33), (257, 513), (3, 8192), (66, 0)]


@pytest.mark.parametrize("F,K", FLUX_SHAPES, ids=[f"F{f}-K{k}" for f, k in FLUX_SHAPES])
def test_flux_bit_exact(ctx, F, K):
    mag = _rows(F, K)
    for all_changes in (False, True):
        want = np.array(R.spectral_flux(mag.tolist(), all_changes))
        got = ctx.spectral_flux(mag, all_changes)
        assert got.shape == (max(F - 1, 0),) and _same(got, want), (all_changes, np.argwhere(got != want)[:3].tolist())
        if F >= 2 and K > 0:
            d = _dev(mag)
            out = torch.full((F - 1,), -1.0, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            ctx.spectral_flux_device(d.data_ptr(), F, K, out.data_ptr(), all_changes)
            ctx.synchronize()
            assert _same(out.cpu().numpy(), want)


def test_flux_special_rows(ctx):
    rng = np.random.default_rng(3)
    m = rng.random((9, 70))
    m[2, 5] = math.nan
    m[4, 7] = math.inf
    m[5, 7] = math.inf                                       # Inf - Inf
    m[6, 69] = -math.inf
    m[7] = m[8]                                              # a zero flux
    for all_changes in (False, True):
        want = np.array(R.spectral_flux(m.tolist(), all_changes))
        got = ctx.spectral_flux(m, all_changes)
        assert _same(got, want), (got, want)
    plain = ctx.spectral_flux(m)
    assert not np.isnan(plain[1]) and not np.isnan(plain[2]) and plain[7] == 0.0   # a NaN difference adds nothing
    assert np.isnan(ctx.spectral_flux(m, True)[[1, 2, 4]]).all() and np.isinf(plain[3])


def test_flux_errors(ctx):
    with pytest.raises(sonar.SonarError) as e:
        ctx.spectral_flux(np.zeros((2, 8193)))
    assert e.value.code == sonar.ERR_UNSUPPORTED and "8192" in e.value.msg


# ---- sonar_rms_envelope ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _noise(n, seed=0):
    x = np.random.default_rng(n + seed).standard_normal(n) * 0.3
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("frame,hop,frames", [(512, 256, 66), (800, 200, 65), (4410, 1102, 5), (4800, 1200, 4),
                                              (1, 1, 130), (33, 7, 64)])
def test_rms_bit_exact(ctx, frame, hop, frames):
    for extra in (-1, 0, 1):                                 # both sides of a frame boundary
        n = frame + hop * (frames - 1) + extra
        x = _noise(n)
        want = np.array(R.rms_envelope(x.tolist(), frame, hop))
        got = ctx.rms_envelope(x, frame, hop)
        assert len(want) == sonar.rms_envelope_frames(n, frame, hop) == frames + (extra if hop == 1 else -(extra < 0))
        assert _same(got, want), np.argwhere(got != want)[:3].tolist()


def test_rms_edges_and_device(ctx):
    x = _noise(1000)
    assert ctx.rms_envelope(x, 1001, 10).shape == (0,)       # frame > n
    assert ctx.rms_envelope(x, 0, 10).shape == (0,) and ctx.rms_envelope(x, 10, 0).shape == (0,)
    assert ctx.rms_envelope(np.zeros(0), 512, 256).shape == (0,)
    y = x.copy()
    y[[100, 700]] = [math.nan, math.inf]
    assert _same(ctx.rms_envelope(y, 64, 16), R.rms_envelope(y.tolist(), 64, 16))
    d = _dev(x)
    out = torch.full((59,), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert ctx.rms_envelope_device(d.data_ptr(), 1000, 64, 16, out.data_ptr()) == 59
    ctx.synchronize()
    assert _same(out.cpu().numpy(), R.rms_envelope(x.tolist(), 64, 16))


# ---- sonar_onset_peaks -----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _curve(n, kind):
    rng = np.random.default_rng(n)
    if kind == "steps":                                      # few distinct values: ties, plateaux, values equal to 3.0
        v = rng.integers(0, 6, n).astype(np.float64)
    elif kind == "sawtooth":                                 # every second sample is a candidate
        v = (np.arange(n) % 2).astype(np.float64) * (1.0 + rng.random(n))
    else:                                                    # NaN and Inf among noise
        v = rng.random(n) * 6.0
        if n > 8:
            v[rng.integers(0, n, n // 8)] = math.nan
            v[rng.integers(0, n, max(n // 16, 1))] = math.inf
            v[rng.integers(0, n, max(n // 16, 1))] = -math.inf
    v.setflags(write=False)
    return v


def _peaks(ctx, v, thr, mif):
    """min_interval in seconds at hop 1 and 1 Hz is minIntervalFrames itself."""
    assert sonar.onset_min_interval_frames(float(mif), 1, 1) == mif
    index, count = ctx.onset_peaks(v, thr, float(mif), 1, 1, padded=True)
    assert len(index) == sonar.onset_peaks_width(len(v)) == max((len(v) - 1) // 2, 0)
    assert 0 <= count <= len(index) and not index[count:].any()   # the slots past count are 0
    return index[:count].tolist()


@pytest.mark.parametrize("kind", ["steps", "sawtooth", "special"])
@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 63, 64, 65, 4097])
def test_peaks_exact(ctx, n, kind):
    v = _curve(n, kind)
    some = 0
    for mif in (0, 1, 2, 3, 4, 64, n + 1, -3):
        for thr in (3.0, 0.0, math.nan, math.inf, -math.inf):
            want = R.find_peaks_frames(v.tolist(), thr, mif)
            assert _peaks(ctx, v, thr, mif) == want, (mif, thr)
            some += len(want)
    if n >= 63:
        assert some > 0
    if n >= 63 and kind == "sawtooth":
        assert _peaks(ctx, v, 0.0, 2) == list(range(1, n - 1, 2))        # the most a curve can hold
        assert _peaks(ctx, v, 0.0, 3) == list(range(1, n - 1, 4))        # ... and the chain at its densest
    if n >= 63 and kind == "steps":
        assert any(v[i] == 3.0 for i in _peaks(ctx, v, 3.0, 0))          # a value equal to the threshold is a peak


@pytest.mark.parametrize("kind", ["steps", "sawtooth"])
def test_peaks_beyond_one_tile(ctx, kind):
    n = 4096 * 64 + 64 * 3 + 7                               # a second tile of four words
    v = _curve(n, kind)
    for mif, thr in ((2, 0.0), (4, 3.0 if kind == "steps" else 0.0), (131100, 0.0)):
        want = R.find_peaks_frames(v.tolist(), thr, mif)
        assert _peaks(ctx, v, thr, mif) == want and want[-1] > 4096 * 64, mif
    d = _dev(v)
    idx = torch.full((sonar.onset_peaks_width(n),), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    count = ctx.onset_peaks_device(d.data_ptr(), n, 0.0, 4.0, 1, 1, idx.data_ptr())
    ctx.synchronize()
    want = R.find_peaks_frames(v.tolist(), 0.0, 4)
    got = idx.cpu().numpy()
    assert count == len(want) and got[:count].tolist() == want and not got[count:].any()


def test_peaks_errors(ctx):
    v = _curve(65, "steps")
    for mi, sr, hop, word in [(math.nan, 44100, 512, "NaN"), (1e300, 44100, 512, "int32"), (-1e300, 44100, 512, "int32"),
                              (0.05, 0, 512, "sample_rate"), (0.05, 44100, 0, "hop_size")]:
        with pytest.raises(sonar.SonarError) as e:
            ctx.onset_peaks(v, 0.0, mi, hop, sr)
        assert e.value.code == sonar.ERR_UNSUPPORTED and word in e.value.msg
    assert ctx.onset_peaks(v[:2], 0.0, math.nan, 0, 0).shape == (0,)   # fewer than 3 values return first


# ---- sonar_onset_adaptive_threshold ------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 2, 65, 2048, 2049, 4097])
def test_adaptive_threshold_bit_exact(ctx, n):
    v = _noise(n, 5) + 1.0
    got, want = ctx.onset_adaptive_threshold(v), R.adaptive_threshold(v.tolist())
    assert _same(got, want), (got, want)
    if n == 65:
        w = v.copy()
        w[7] = math.nan
        assert math.isnan(ctx.onset_adaptive_threshold(w))
        d = _dev(v)
        out = torch.full((1,), -1.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ctx.onset_adaptive_threshold_device(d.data_ptr(), n, out.data_ptr())
        ctx.synchronize()
        assert _same(out.cpu().numpy()[0], want)


# ---- sonar_onsets_flux -------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _bursts(n, sr, period=0.25):
    """Decaying noise bursts every `period` seconds over a quiet floor."""
    rng = np.random.default_rng(n + sr)
    x = 1e-3 * rng.standard_normal(n)
    step, length = int(period * sr), int(0.03 * sr)
    for k, s in enumerate(range(step // 2, n - length, step)):
        x[s:s + length] += (0.4 + 0.1 * (k % 4)) * rng.standard_normal(length) * np.exp(-np.arange(length) / (0.01 * sr))
    x.setflags(write=False)
    return x


def _check_flux_call(ctx, got, sr, thr, mi, H, checker=True):
    """flux and onsets of one call against the spectrum and curve entries on the call's own rows, and
    the onsets against the checker on those rows."""
    want_flux = ctx.spectral_flux(got["magnitude"])
    assert _same(got["flux"], want_flux)
    want = ctx.onset_peaks(want_flux, thr, mi, H, sr) * H
    assert got["onsets"].tolist() == want.tolist()
    if checker:
        assert want.tolist() == R.detect_onsets_from_rows(got["magnitude"].tolist(), sr, thr, mi, H)


@pytest.mark.parametrize("W,H,frames,tol", [(1024, 512, 1, 1e-11), (1024, 512, 2, 1e-11), (1024, 512, 3, 1e-11),
                                            (1024, 512, 66, 1e-11), (256, 64, 70, 1e-11), (1000, 250, 21, 1e-10)])
def test_onsets_flux(ctx, W, H, frames, tol):
    sr = 44100
    n = W + H * (frames - 1) + 5
    x = _bursts(n, sr, 0.1)
    default = (W, H) == (1024, 512)
    got = ctx.onsets_flux(x, sr, 0.3, 0.05, 0 if default else W, 0 if default else H, skip=())
    assert got["frames"] == frames and got["magnitude"].shape == (frames, W // 2 + 1) and got["flux"].shape == (frames - 1,)
    fr = np.stack([x[i * H:i * H + W] for i in range(frames)])
    ref = np.abs(np.fft.rfft(fr, axis=1))                    # no window at all
    worst = max(assert_rel(g, r, tol, float(r.max()), f"frame {i}") for i, (g, r) in enumerate(zip(got["magnitude"], ref)))
    print(f"W {W}: worst |X| error {worst:.3g} of the frame's peak (bound {tol:g})")
    _check_flux_call(ctx, got, sr, 0.3, 0.05, H)
    if frames == 1:
        assert got["onsets"].shape == (0,)                   # one frame: no flux, no onsets, no error
    if frames >= 21:
        assert len(got["onsets"]) > 0 and np.all(got["onsets"] % H == 0)
        lean = ctx.onsets_flux(x, sr, 0.3, 0.05, W, H, skip=("flux", "magnitude"))
        assert lean["flux"] is None and lean["onsets"].tolist() == got["onsets"].tolist()


def test_onsets_flux_chunk_seam(ctx):
    n, W, H = 140_000, 128, 1
    plan = sonar.hpcp_plan(n, W, H)
    assert plan["frames"] == 139_873 and plan["n_chunks"] >= 2
    got = ctx.onsets_flux(_bursts(n, 44100, 0.05), 44100, 0.05, 0.001, W, H, skip=())
    seam = plan["chunk_frames"]
    assert got["flux"][seam - 1] != 0.0 and got["flux"][seam] != 0.0 and got["magnitude"][seam].any()
    _check_flux_call(ctx, got, 44100, 0.05, 0.001, H, checker=False)   # 9 M differences: the entries suffice
    assert np.any(got["onsets"] > seam) and np.any(got["onsets"] < seam)


def test_onsets_flux_device_and_errors(ctx):
    sr, n = 44100, 1024 + 512 * 40
    x = _bursts(n, sr, 0.1)
    host = ctx.onsets_flux(x, sr, 0.3, 0.05, skip=())
    d = _dev(x)
    on = torch.full((sonar.onset_peaks_width(40),), -1, dtype=torch.int64, device="cuda")
    fl = torch.full((40,), -1.0, dtype=torch.float64, device="cuda")
    mg = torch.full((41, 513), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    count, frames = ctx.onsets_flux_device(d.data_ptr(), n, sr, 0.3, 0.05, on.data_ptr(), flux_ptr=fl.data_ptr(),
                                           magnitude_ptr=mg.data_ptr())
    ctx.synchronize()
    assert frames == 41 and on.cpu().numpy()[:count].tolist() == host["onsets"].tolist() and count > 0
    assert not on.cpu().numpy()[count:].any()
    assert _same(fl.cpu().numpy(), host["flux"]) and _same(mg.cpu().numpy(), host["magnitude"])
    assert ctx.onsets_flux(np.zeros(0), sr, 0.3, 0.05)["onsets"].shape == (0,)   # empty: no error
    one = ctx.onsets_flux(x[:1023], sr, 0.3, 0.05, skip=())   # Go's truncating count: one frame, left all zero
    assert one["frames"] == 1 and not one["magnitude"].any() and one["onsets"].shape == (0,)
    for args, code, text in [((x[:512], sr, 0.3, 0.05), sonar.ERR_TOO_SHORT, "signal too short for given window size and hop size"),
                             ((x[:1], sr, 0.3, 0.05), sonar.ERR_TOO_SHORT, "signal too short for given window size and hop size"),
                             ((x, 0, 0.3, 0.05), sonar.ERR_UNSUPPORTED, "sample_rate"),
                             ((x, sr, 0.3, math.nan), sonar.ERR_UNSUPPORTED, "NaN"),
                             ((x, sr, 0.3, 1e300), sonar.ERR_UNSUPPORTED, "int32"),
                             ((np.zeros(10000), sr, 0.3, 0.05, 8193, 256), sonar.ERR_UNSUPPORTED, "above 8192")]:
        with pytest.raises(sonar.SonarError) as e:
            ctx.onsets_flux(*args)
        assert e.value.code == code and text in e.value.msg, e.value.msg


# ---- sonar_onsets_energy -----------------------------------------------------------------------------

@pytest.mark.parametrize("sr,n", [(8000, 16000), (44100, 30000), (8000, 512 + 256 * 2)])
def test_onsets_energy(ctx, sr, n):
    x = _bursts(n, sr, 0.2)
    for thr, mi in ((0.1, 0.05), (0.01, 0.0), (0.01, 0.5)):
        want_onsets, want_curve = R.detect_onsets_energy(x.tolist(), sr, thr, mi)
        got = ctx.onsets_energy(x, sr, thr, mi)
        assert _same(got["curve"], want_curve) and got["onsets"].tolist() == want_onsets, (thr, mi)
    if n >= 16000:
        assert len(ctx.onsets_energy(x, sr, 0.01, 0.0)["onsets"]) > 2
    other = ctx.onsets_energy(x, sr, 0.01, 0.05, 300, 100)    # another grid
    want_onsets, want_curve = R.detect_onsets_energy(x.tolist(), sr, 0.01, 0.05, 300, 100)
    assert _same(other["curve"], want_curve) and other["onsets"].tolist() == want_onsets


def test_onsets_energy_edges(ctx):
    for n in (0, 1, 511):
        got = ctx.onsets_energy(_noise(n), 44100, 0.1, 0.05)
        assert got["onsets"].shape == (0,) and got["curve"].shape == (0,)
    x = _bursts(16000, 8000, 0.2).copy()
    x[3000] = math.nan                                        # a NaN difference gives 0
    want_onsets, want_curve = R.detect_onsets_energy(x.tolist(), 8000, 0.01, 0.0)
    got = ctx.onsets_energy(x, 8000, 0.01, 0.0)
    assert _same(got["curve"], want_curve) and got["onsets"].tolist() == want_onsets and 0.0 in got["curve"]
    d = _dev(x)
    on = torch.full((sonar.onset_peaks_width(60),), -1, dtype=torch.int64, device="cuda")
    cv = torch.full((60,), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    count, nc = ctx.onsets_energy_device(d.data_ptr(), 16000, 8000, 0.01, 0.0, on.data_ptr(), curve_ptr=cv.data_ptr())
    ctx.synchronize()
    assert nc == 60 and on.cpu().numpy()[:count].tolist() == want_onsets and _same(cv.cpu().numpy(), want_curve)


# ---- sonar_onsets_complex ----------------------------------------------------------------------------

@pytest.mark.parametrize("sr", [8000, 44100])
def test_onsets_complex(ctx, sr):
    """The tolerance, int(0.05 * sr), is 400 samples at 8 kHz, below one flux hop of 512, and 2,205 at
    44.1 kHz, above it."""
    n = 3 * sr + 77
    x = _bursts(n, sr, 0.3)
    f = ctx.onsets_flux(x, sr, R.FLUX_THRESHOLD, R.MIN_INTERVAL)["onsets"].tolist()
    e = ctx.onsets_energy(x, sr, R.ENERGY_THRESHOLD, R.MIN_INTERVAL)["onsets"].tolist()
    tol = R.complex_tolerance(sr)
    assert tol == (400 if sr == 8000 else 2205) and len(f) > 2 and len(e) > 2
    want = R.combine_onsets(f, e, tol)
    got = ctx.onsets_complex(x, sr)
    print(f"sr {sr}: {len(f)} flux + {len(e)} energy onsets -> {len(want)} combined, density {got['density']}")
    assert got["onsets"].tolist() == want
    assert _same(got["density"], R.onset_density(len(want), n, sr)) and got["density"] > 0
    merged = sorted(f + e)
    gaps = [b - a for a, b in zip(merged, merged[1:])]
    assert any(g > tol for g in gaps)
    if sr == 44100:                                           # the two detectors meet inside the tolerance
        assert any(g <= tol for g in gaps) and len(want) < len(f) + len(e)
    else:                                                     # ... and at 8 kHz they never do on this signal
        assert len(want) == len(f) + len(e)
    d = _dev(x)
    on = torch.full((sonar.onsets_complex_width(n),), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    count, density = ctx.onsets_complex_device(d.data_ptr(), n, sr, on.data_ptr())
    ctx.synchronize()
    assert on.cpu().numpy()[:count].tolist() == want and not on.cpu().numpy()[count:].any() and density == got["density"]


def test_onsets_complex_edges(ctx):
    got = ctx.onsets_complex(np.zeros(0), 44100)
    assert got["onsets"].shape == (0,) and got["density"] == 0.0
    with pytest.raises(sonar.SonarError) as e:                # the flux detector's error ends the call
        ctx.onsets_complex(_noise(512), 44100)
    assert e.value.code == sonar.ERR_TOO_SHORT and "signal too short for given window size and hop size" in e.value.msg
    assert ctx.onsets_energy(_noise(512), 44100, 0.0, 0.0)["curve"].shape == (0,)   # ... which would have run
    got = ctx.onsets_complex(_noise(1000), 44100)             # 513..1023 samples: one all-zero frame, no error
    assert got["onsets"].shape == (0,) and got["density"] == 0.0


# ---- sonar_tempo_autocorrelation ---------------------------------------------------------------------

def _beat(n, sr, bpm):
    t = np.arange(n) / sr
    return (0.5 + 0.5 * np.cos(2 * np.pi * (bpm / 60.0) * t)) * _noise(n, 9)


@pytest.mark.parametrize("L", [9, 10, 19, 20, 21, 50, 397])
def test_tempo_autocorrelation(ctx, L):
    """The envelope at 8 kHz has frames of 800 at hop 200.  9 | 10 and 19 | 20 are the two length gates;
    at 50 values the curve has 25 lags and the search's upper lag, 40, clamps to 24."""
    sr = 8000
    n = 800 + 200 * (L - 1) + 3
    x = _beat(n, sr, 100.0)
    plan = sonar.tempo_autocorr_plan(n, sr)
    assert (plan["frame_size"], plan["hop_size"], plan["envelope_len"]) == (800, 200, L)
    assert plan["n_autocorr"] == (L // 2 if L >= 10 else 0)
    env = ctx.rms_envelope(x, 800, 200)
    tempo, lag, curve = R.tempo_autocorrelation_from_envelope(env.tolist(), 200, sr)
    full = ctx.tempo_autocorrelation(x, sr, full=True)
    narrow = ctx.tempo_autocorrelation(x, sr)
    assert _same(full["autocorr"], curve), np.argwhere(full["autocorr"] != np.array(curve))[:3].tolist()
    assert narrow["autocorr"] is None
    for got in (full, narrow):
        assert _same(got["tempo"], tempo) and got["best_lag"] == lag, (got, tempo, lag)
    if L < 20:
        assert tempo == 0.0
    if L >= 10:
        assert curve[0] == 1.0 and curve[1] != 1.0 and curve[1] < 0.9   # only lag 0 is normalised
    if L == 50:
        assert (plan["min_lag"], plan["max_lag"]) == (13, 24)
    if L == 397:
        assert (plan["min_lag"], plan["max_lag"]) == (13, 40) and lag > 0 and tempo == 60.0 / (float(lag) * (200.0 / 8000.0))


def test_tempo_autocorrelation_flat_curves(ctx):
    sr, n = 8000, 800 + 200 * 99
    const = ctx.tempo_autocorrelation(np.full(n, 0.5), sr, full=True)      # every lag is exactly 0.25
    assert const["tempo"] == 120.0 and const["best_lag"] == 0
    assert const["autocorr"][0] == 1.0 and np.all(const["autocorr"][1:] == 0.25)
    silent = ctx.tempo_autocorrelation(np.zeros(n), sr, full=True)         # ac[0] is not > 0: no division
    assert silent["tempo"] == 120.0 and not silent["autocorr"].any()
    assert ctx.tempo_autocorrelation(np.zeros(0), sr)["tempo"] == 0.0
    x = _beat(n, sr, 100.0)
    host = ctx.tempo_autocorrelation(x, sr, full=True)
    d = _dev(x)
    t = torch.full((1,), -1.0, dtype=torch.float64, device="cuda")
    lg = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    ac = torch.full((50,), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert ctx.tempo_autocorrelation_device(d.data_ptr(), n, sr, t.data_ptr(), lg.data_ptr(), ac.data_ptr()) == 50
    ctx.synchronize()
    assert t.item() == host["tempo"] and lg.item() == host["best_lag"] and _same(ac.cpu().numpy(), host["autocorr"])
    with pytest.raises(sonar.SonarError) as e:
        ctx.tempo_autocorrelation(x, 0)
    assert e.value.code == sonar.ERR_UNSUPPORTED


# ---- sonar_tempo -------------------------------------------------------------------------------------

def _want_tempo(ctx, x, sr):
    """The checker composed from the GPU's own onset list and envelope."""
    onsets = None if len(x) <= 512 else ctx.onsets_complex(x, sr)["onsets"].tolist()   # the STFT's error (n <= W - H)
    frame, hop = R.autocorr_frame_hop(sr)
    env = ctx.rms_envelope(x, frame, hop).tolist()
    onset_tempo = 0.0 if onsets is None else R.tempo_from_onsets(onsets, sr)[0]
    ac_tempo, lag, _ = R.tempo_autocorrelation_from_envelope(env, hop, sr) if len(x) else (0.0, 0, [])
    avg, conf, diff = R.tempo_range(onset_tempo, ac_tempo)
    return dict(onset_tempo=onset_tempo, autocorr_tempo=ac_tempo, tempo=avg, confidence=conf, difference=diff,
                onset_count=0 if onsets is None else len(onsets), best_lag=lag, category=R.classify(avg),
                onset_error=sonar.ERR_TOO_SHORT if onsets is None and len(x) else 0, category_name=R.CATEGORIES[R.classify(avg)])


def _check_tempo(got, want):
    for k, v in want.items():
        assert _same(got[k], v) if isinstance(v, float) else got[k] == v, (k, got[k], v)


@pytest.mark.parametrize("sr,seconds", [(8000, 6.0), (44100, 3.0)])
def test_tempo_fields(ctx, sr, seconds):
    x = _bursts(int(seconds * sr), sr, 0.5)
    want = _want_tempo(ctx, x, sr)
    got = ctx.tempo(x, sr)
    print(want)
    _check_tempo(got, want)
    assert want["onset_count"] >= 2 and want["onset_tempo"] > 0
    d = _dev(x)
    _check_tempo(ctx.tempo(d.data_ptr(), sr, device_n=len(x)), want)


def test_tempo_short_signal_swallows_the_error(ctx):
    for n, code in ((1000, 0), (500, sonar.ERR_TOO_SHORT)):   # one all-zero frame | the STFT's error, dropped
        x = _noise(n)
        got = ctx.tempo(x, 8000)
        _check_tempo(got, _want_tempo(ctx, x, 8000))
        assert got["onset_tempo"] == 0.0 and got["onset_error"] == code and got["autocorr_tempo"] == 0.0
        assert got["confidence"] == 1.0 and got["category_name"] == "very_slow"
    empty = ctx.tempo(np.zeros(0), 8000)
    assert empty["tempo"] == 0.0 and empty["confidence"] == 1.0 and empty["onset_error"] == 0


def test_tempo_click_track(ctx):
    """8 s at 8 kHz, a click every half second and silence between.  The reference's fixed thresholds act
    on unnormalised magnitudes, so the values are the checker's, not a musical expectation."""
    sr = 8000
    x = np.zeros(8 * sr)
    for s in range(1000, len(x) - 64, sr // 2):
        x[s:s + 32] = 0.9 * np.hanning(32) * np.where(np.arange(32) % 2, -1.0, 1.0)
    want = _want_tempo(ctx, x, sr)
    got = ctx.tempo(x, sr)
    print({k: got[k] for k in want})
    _check_tempo(got, want)
    assert got["onset_count"] >= 2 and 0.0 <= got["confidence"] <= 1.0
