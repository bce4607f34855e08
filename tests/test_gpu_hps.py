"""sonar_hps_from_spectrum and sonar_hps on the GPU against the Python checker (tests/hps_ref.py, held to
known answers in test_hps_cpu.py).

The spectrum entry is bit-exact in every output: f0_bin, f0, confidence, strengths and the HPS rows, in
both modes.  Its arithmetic is products, comparisons, a two-point interpolation and two quotients, all
IEEE operations that Python performs identically.  One thing is not compared: which NaN an invalid
operation makes (Inf * 0.0 is a NaN of either sign, the processor's choice), so a NaN equals a NaN.

Shapes: one row per wave, 64 bins per step and one lane per harmonic strength, so K runs over 1..4,
both sides of 64 and 128, the music extractor's 1025 and the largest row; F over both sides of 64 and
past 256; num_harmonics over 0, 1, the first few, the extractor's 10 and one value above K where K
allows it (10 at K <= 4, 64 at K = 63).  The frequency resolution is 44.1 Hz, which is not exact in
binary, so the strengths' (f0 * h) / resolution lands below bin * h on some rows (asserted).

The PCM entry is held to the spectrum entry on the magnitude rows the same call returned, bit for
bit, and its rows to numpy's rfft of the frames under the unnormalised symmetric Hann at the
tolerance of the existing float64 magnitude tests: 1e-11 of the frame's peak on the fused transform
(test_gpu_stft_mfcc.test_magnitude_matches_oracle) and 1e-10 on the DFT path
(test_gpu_stft_generic), applied with parity.assert_rel."""
import functools
import itertools
import math

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library loads HIP (one HIP runtime in the process)

import hps_ref as R
import sonar
from parity import assert_rel

pytestmark = pytest.mark.gpu

SR, WS = 44100, 1000             # 44.1 Hz per bin whatever K is
RES = SR / WS
FLOAT_OUTPUTS = ("f0", "confidence", "strengths", "hps")


def _same(a, b):
    """Equal bits, except that any NaN equals any NaN."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    if not np.array_equal(nan, np.isnan(b)):
        return False
    return np.array_equal(a.view(np.uint64)[~nan], b.view(np.uint64)[~nan])


def _check(got, want, names=FLOAT_OUTPUTS):
    assert np.array_equal(got["f0_bin"], want["f0_bin"]), (got["f0_bin"], want["f0_bin"])
    for k in names:
        bad = [] if _same(got[k], want[k]) else np.argwhere(np.atleast_1d(got[k] != want[k]))[:3].tolist()
        assert not bad, (k, bad)


# ---- rows and the checker's answers, computed once --------------------------------------------

@functools.lru_cache(maxsize=None)
def _rows(F, K):
    """Noise with distinct magnitudes plus, per row, a harmonic comb and a few spikes."""
    rng = np.random.default_rng(1000 * K + F)
    m = np.abs(rng.standard_normal((F, K)))
    for f in range(F):
        base = int(rng.integers(1, max(K // 8, 2)))
        for k in range(1, 11):
            if base * k < K:
                m[f, base * k] += 6.0 * 0.8 ** k + rng.random()
        for b in rng.integers(0, K, size=min(3, K)):
            m[f, b] += 3.0 + rng.random()
    assert all(len(np.unique(r)) == K for r in m)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _hps(F, K, nh, interpolated):
    fn = R.compute_hps_interpolated if interpolated else R.compute_hps
    return [fn(R.analyzer(SR, nh), row) for row in _rows(F, K)]


def _want(F, K, nh, interpolated, lo, hi):
    """The checker per row, with the HPS rows shared between the ranges."""
    hp = R.analyzer(SR, nh, lo, hi)
    out = dict(f0_bin=np.zeros(F, np.int32), f0=np.zeros(F), confidence=np.zeros(F), strengths=np.zeros((F, max(nh, 0))),
               hps=np.array(_hps(F, K, nh, interpolated), dtype=np.float64).reshape(F, K))
    for f, row in enumerate(_rows(F, K)):
        b = R.find_f0_peak(hp, _hps(F, K, nh, interpolated)[f], WS)
        if b == 0:
            continue
        out["f0_bin"][f], out["f0"][f] = b, float(b) * RES
        out["confidence"][f] = R.compute_harmonicity(hp, row, out["f0"][f], WS)
        if nh > 0:
            out["strengths"][f] = R.compute_harmonic_strength(hp, row, out["f0"][f], WS)
    return out


def _ranges(K):
    return {"music": (80.0, 2000.0),                         # bins 1..45
            "min_clamps": (0.0, RES * (K // 2) + 1.0),       # min_bin 0 -> 1
            "max_clamps": (RES * 1.5, 1e7),                  # max_bin -> K - 1, through the K / h zero region
            "empty": (500.0, 100.0)}


SHAPES = [(1, 65, (0, 1, 2, 10)), (2, 65, (0, 1, 2, 3, 10)), (3, 64, (1, 2, 3, 5, 10)), (4, 63, (0, 1, 2, 3, 5, 10)),
          (63, 65, (0, 1, 2, 3, 5, 10, 64)), (64, 63, (2, 10)), (65, 64, (1, 3, 10)), (128, 257, (2, 5, 10)),
          (129, 1, (0, 1, 2, 3, 5, 10)), (1025, 64, (5, 10)), (8192, 3, (10, 64))]


@pytest.mark.parametrize("interpolated", [False, True], ids=["plain", "interpolated"])
@pytest.mark.parametrize("K,F,harmonics", SHAPES, ids=[f"K{s[0]}-F{s[1]}" for s in SHAPES])
def test_rows_bit_exact(ctx, K, F, harmonics, interpolated):
    mag = _rows(F, K)
    voiced = below = 0
    for nh in harmonics:
        for name, (lo, hi) in _ranges(K).items():
            want = _want(F, K, nh, interpolated, lo, hi)
            assert sonar.hps_bins(SR, WS, K, lo, hi) == R.scan_bins(R.analyzer(SR, nh, lo, hi), K, WS)
            got = ctx.hps_from_spectrum(mag, WS, SR, nh, lo, hi, interpolated, skip=())
            _check(got, want)
            if name == "empty":
                assert not got["f0_bin"].any() and not got["f0"].any() and not got["strengths"].any()
            voiced += int(np.count_nonzero(want["f0_bin"]))
            below += sum(int((float(b) * RES * h) / RES) < b * h for b in want["f0_bin"] for h in range(1, nh + 1))
    if K >= 63:
        assert voiced > 0                                    # peaks were found
    if K >= 63 and F >= 63:
        assert below > 0                                     # and on some of them the literal index matters


def test_harmonic_above_K_changes_nothing_in_plain_mode(ctx):
    mag = _rows(63, 4)
    a = ctx.hps_from_spectrum(mag, WS, SR, 4, 0.0, 1e7, skip=("confidence", "strengths"))
    b = ctx.hps_from_spectrum(mag, WS, SR, 10, 0.0, 1e7, skip=("confidence", "strengths"))
    assert _same(a["hps"], b["hps"]) and np.array_equal(a["f0_bin"], b["f0_bin"]) and a["hps"][:, 0].all()


# ---- special rows ------------------------------------------------------------------------------

def _special_rows():
    K = 65
    rng = np.random.default_rng(7)
    base = 0.5 + rng.random(K)
    rows = {"zeros": np.zeros(K)}
    for name, bin_, v in [("nan_inside", 3, math.nan), ("nan_beyond", 50, math.nan), ("inf_inside", 4, math.inf),
                          ("inf_beyond", 40, math.inf), ("neg_inf_inside", 5, -math.inf),
                          ("neg_inf_beyond", 60, -math.inf)]:
        r = base.copy()
        r[bin_] = v                                          # K / 10 = 6: bins 0..5 are inside every harmonic's range
        rows[name] = r
    sub = np.full(K, 1e-16)
    sub[5] = 3e-16
    rows["subnormal"] = sub
    rows["overflow"] = base * 1e40                           # p = 1e80: the fourth product is Inf
    tie = np.full(K, 0.5)
    tie[[7, 19]] = 2.0
    rows["tie"] = tie
    return rows


@pytest.mark.parametrize("interpolated", [False, True], ids=["plain", "interpolated"])
@pytest.mark.parametrize("nh", [1, 2, 10])
def test_special_rows(ctx, nh, interpolated):
    rows = _special_rows()
    mag = np.array(list(rows.values()))
    hp = R.analyzer(64, nh, 1.0, 40.0)                       # window_size = sample_rate = 64: a bin is 1 Hz
    want = R.estimate_rows(hp, mag, 64, interpolated)
    got = ctx.hps_from_spectrum(mag, 64, 64, nh, 1.0, 40.0, interpolated, skip=())
    _check(got, want)
    at = {name: i for i, name in enumerate(rows)}
    assert got["f0_bin"][at["zeros"]] == 0 and not got["hps"][at["zeros"]].any()
    if not interpolated:
        if nh == 10:
            sub = got["hps"][at["subnormal"]]
            assert sub[1] == 9e-320 and sub[2] == 1e-320 and got["f0_bin"][at["subnormal"]] == 1
            assert np.isinf(got["hps"][at["overflow"]][1:6]).all() and got["f0_bin"][at["overflow"]] == 1
        if nh >= 2:
            assert np.isnan(got["hps"][at["inf_beyond"]][40]) and np.isnan(got["hps"][at["neg_inf_beyond"]][60])
            assert np.isinf(got["hps"][at["inf_inside"]][4]) and got["f0_bin"][at["inf_inside"]] in (1, 2, 4)
        if nh == 1:
            assert got["f0_bin"][at["tie"]] == 7 and got["hps"][at["tie"]][7] == got["hps"][at["tie"]][19] == 4.0
    assert got["f0_bin"][at["nan_inside"]] != 3              # a NaN is never the peak


# ---- the two layouts of the total-energy chain ---------------------------------------------------

@pytest.mark.parametrize("K", [1, 33, 65])
def test_both_chain_layouts_give_the_same_bits(ctx, K):
    """From 32,768 rows on, the sum of mag^2 behind the confidence comes from a kernel of its own (a row
    per lane, 64 rows per wave, tiles of 32 columns); below, lane 0 walks the row.  32,768 + 65 rows take
    the first path with a last wave of one row; the same rows in two calls take the second.  K runs
    over one column, one past a tile and one past two.  64 rows are also held to the checker."""
    F = 32768 + 65
    rng = np.random.default_rng(K)
    mag = np.abs(rng.standard_normal((F, K))) + 0.01
    whole = ctx.hps_from_spectrum(mag, WS, SR, 3, 0.0, 1e7, skip=("hps",))
    halves = [ctx.hps_from_spectrum(m, WS, SR, 3, 0.0, 1e7, skip=("hps",)) for m in (mag[:20000], mag[20000:])]
    for k in ("f0_bin", "f0", "confidence", "strengths"):
        assert _same(whole[k], np.concatenate([h[k] for h in halves])), k
    tail = R.estimate_rows(R.analyzer(SR, 3, 0.0, 1e7), mag[-64:], WS)
    assert _same(whole["confidence"][-64:], tail["confidence"]) and np.array_equal(whole["f0_bin"][-64:], tail["f0_bin"])
    if K > 1:
        assert whole["confidence"].all()
    below = ctx.hps_from_spectrum(mag[:32767], WS, SR, 3, 0.0, 1e7, skip=("hps", "strengths"))
    at = ctx.hps_from_spectrum(mag[:32768], WS, SR, 3, 0.0, 1e7, skip=("hps", "strengths"))
    assert _same(at["confidence"][:32767], below["confidence"]) and _same(at["confidence"], whole["confidence"][:32768])


# ---- optional outputs, host and device pointers -------------------------------------------------

def test_every_combination_of_null_outputs(ctx):
    F, K, nh = 65, 129, 5
    mag = _rows(F, K)
    for interpolated in (False, True):
        full = ctx.hps_from_spectrum(mag, WS, SR, nh, 80.0, 2000.0, interpolated, skip=())
        _check(full, _want(F, K, nh, interpolated, 80.0, 2000.0))
        for r in range(1, 4):
            for skip in itertools.combinations(("confidence", "strengths", "hps"), r):
                got = ctx.hps_from_spectrum(mag, WS, SR, nh, 80.0, 2000.0, interpolated, skip=skip)
                assert all(got[k] is None for k in skip)
                _check(got, full, [k for k in FLOAT_OUTPUTS if k not in skip])


def test_host_and_device_pointers_agree(ctx):
    F, K, nh = 257, 128, 10
    mag = _rows(F, K)
    host = ctx.hps_from_spectrum(mag, WS, SR, nh, 80.0, 2000.0, skip=())
    d = torch.from_numpy(mag.copy()).cuda()
    b = torch.full((F,), -1, dtype=torch.int32, device="cuda")
    f0, conf = (torch.full((F,), -1.0, dtype=torch.float64, device="cuda") for _ in range(2))
    st = torch.full((F, nh), -1.0, dtype=torch.float64, device="cuda")
    hps = torch.full((F, K), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.hps_from_spectrum_device(d.data_ptr(), F, K, WS, SR, b.data_ptr(), f0.data_ptr(), nh, 80.0, 2000.0, False,
                                 conf.data_ptr(), st.data_ptr(), hps.data_ptr())
    ctx.synchronize()
    dev = dict(f0_bin=b.cpu().numpy(), f0=f0.cpu().numpy(), confidence=conf.cpu().numpy(), strengths=st.cpu().numpy(),
               hps=hps.cpu().numpy())
    _check(dev, host)
    # only the required outputs
    b.fill_(-1)
    f0.fill_(-1.0)
    torch.cuda.synchronize()
    ctx.hps_from_spectrum_device(d.data_ptr(), F, K, WS, SR, b.data_ptr(), f0.data_ptr(), nh)
    ctx.synchronize()
    assert np.array_equal(b.cpu().numpy(), host["f0_bin"]) and _same(f0.cpu().numpy(), host["f0"])


# ---- the PCM entry -----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _pcm(n):
    rng = np.random.default_rng(n)
    t = np.arange(n) / 44100.0
    x = sum(a * np.sin(2 * np.pi * f * t) for a, f in [(0.5, 220.0), (0.3, 440.0), (0.2, 660.0), (0.1, 3520.0)])
    x = x + 0.01 * rng.standard_normal(n)
    x.setflags(write=False)
    return x


def _check_against_own_rows(ctx, got, W, nh, interpolated):
    want = ctx.hps_from_spectrum(got["magnitude"], W, 44100, nh, 80.0, 2000.0, interpolated, skip=("hps",))
    _check(got, want, ("f0", "confidence", "strengths"))


@pytest.mark.parametrize("interpolated", [False, True], ids=["plain", "interpolated"])
@pytest.mark.parametrize("W,H,frames,tail", [(128, 32, 70, 5), (1024, 256, 37, 100), (2048, 512, 33, 511),
                                             (1000, 250, 21, 7), (2048, 512, 1, 0)])
def test_hps_equals_from_spectrum_on_its_own_rows(ctx, W, H, frames, tail, interpolated):
    n = W + H * (frames - 1) + tail
    assert sonar.hps_plan(n, W, H)["frames"] == frames
    got = ctx.hps(_pcm(n), 44100, W, H, 10, 80.0, 2000.0, interpolated, skip=())
    assert got["magnitude"].shape == (frames, W // 2 + 1) and got["magnitude"].any()
    _check_against_own_rows(ctx, got, W, 10, interpolated)
    if W >= 1000:
        assert got["f0_bin"].all() and got["confidence"].all()   # 220 Hz and its partials are inside 80..2000


def test_hps_chunk_seam(ctx):
    n, W, H = 140_000, 128, 1
    plan = sonar.hps_plan(n, W, H)
    assert plan["frames"] == 139_873 and plan["n_chunks"] >= 2
    got = ctx.hps(_pcm(n), 44100, W, H, 3, 300.0, 5000.0, skip=())
    want = ctx.hps_from_spectrum(got["magnitude"], W, 44100, 3, 300.0, 5000.0, skip=("hps",))
    seam = plan["chunk_frames"]
    assert got["f0_bin"][seam - 1] and got["f0_bin"][seam] and got["magnitude"][seam].any()
    _check(got, want, ("f0", "confidence", "strengths"))


@pytest.mark.parametrize("W,H,tol", [(128, 32, 1e-11), (1024, 256, 1e-11), (2048, 512, 1e-11), (1000, 250, 1e-10)])
def test_rows_are_the_unnormalised_symmetric_hann(ctx, W, H, tol):
    n = W + H * 8 + 3
    x = _pcm(n)
    got = ctx.hps(x, 44100, W, H, skip=("confidence", "strengths"))["magnitude"]
    frames = np.stack([x[i * H:i * H + W] for i in range(9)])
    ref = np.abs(np.fft.rfft(frames * np.hanning(W), axis=1))   # numpy's hanning: 0.5 - 0.5 cos(2 pi i / (W - 1))
    assert np.hanning(W)[0] == 0.0 and abs(np.mean(np.hanning(W) ** 2) - 0.375) < 1e-2   # not energy-normalised
    assert got.shape == ref.shape
    worst = max(assert_rel(g, r, tol, float(r.max()), f"frame {i}") for i, (g, r) in enumerate(zip(got, ref)))
    print(f"W {W}: worst |X| error {worst:.3g} of the frame's peak (bound {tol:g})")


@pytest.mark.parametrize("nh", [5, 10])
@pytest.mark.parametrize("W", [1000, 1024, 2048])
def test_known_tone(ctx, W, nh):
    sr, H = 44100, W // 4
    n = W + H * 7
    f = 10.0 * sr / W
    t = np.arange(n) / sr
    x = sum(0.8 ** k * np.sin(2 * np.pi * k * f * t) for k in range(1, 11))
    x = x + 1e-3 * np.random.default_rng(W + nh).standard_normal(n)
    got = ctx.hps(x, sr, W, H, nh, 80.0, 2000.0)
    assert got["f0_bin"].tolist() == [10] * 8
    assert got["f0"].tolist() == [10.0 * (float(sr) / float(W))] * 8
    assert np.all(got["confidence"] > 0.5) and np.all(got["strengths"][:, 0] > got["strengths"][:, 1])


def test_hps_device_pointers(ctx):
    W, H, n, nh = 1024, 256, 1024 + 256 * 20, 10
    x = _pcm(n)
    host = ctx.hps(x, 44100, W, H, nh, skip=())
    d = torch.from_numpy(x.copy()).cuda()
    b = torch.full((21,), -1, dtype=torch.int32, device="cuda")
    f0, conf = (torch.full((21,), -1.0, dtype=torch.float64, device="cuda") for _ in range(2))
    st = torch.full((21, nh), -1.0, dtype=torch.float64, device="cuda")
    mag = torch.full((21, 513), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    frames = ctx.hps_device(d.data_ptr(), n, 44100, b.data_ptr(), f0.data_ptr(), W, H, nh, confidence_ptr=conf.data_ptr(),
                            strengths_ptr=st.data_ptr(), magnitude_ptr=mag.data_ptr())
    ctx.synchronize()
    assert frames == 21
    dev = dict(f0_bin=b.cpu().numpy(), f0=f0.cpu().numpy(), confidence=conf.cpu().numpy(), strengths=st.cpu().numpy())
    _check(dev, host, ("f0", "confidence", "strengths"))
    assert _same(mag.cpu().numpy(), host["magnitude"])
    # a table survives sonar_trim by being rebuilt
    ctx.trim()
    _check(ctx.hps(x, 44100, W, H, nh, skip=()), host, ("f0", "confidence", "strengths"))


# ---- edges and errors ---------------------------------------------------------------------------

def test_from_spectrum_edges(ctx):
    got = ctx.hps_from_spectrum(np.zeros((0, 16)), 2048, 44100, skip=())
    assert got["f0_bin"].shape == (0,) and got["hps"].shape == (0, 16)
    got = ctx.hps_from_spectrum(np.ones((3, 0)), 2048, 44100, skip=())
    assert got["f0_bin"].tolist() == [0, 0, 0] and not got["f0"].any() and not got["confidence"].any()
    assert got["strengths"].shape == (3, 10) and not got["strengths"].any() and got["hps"].shape == (3, 0)
    # K == 0 returns before the parameters are looked at, as the reference does
    assert ctx.hps_from_spectrum(np.ones((2, 0)), 0, 0, -3, math.nan, -1.0)["f0_bin"].tolist() == [0, 0]
    # a negative num_harmonics is the power spectrum as long as no strengths are asked for
    mag = _rows(65, 65)
    a = ctx.hps_from_spectrum(mag, WS, SR, -3, 80.0, 2000.0, skip=("confidence", "strengths"))
    b = ctx.hps_from_spectrum(mag, WS, SR, 1, 80.0, 2000.0, skip=("confidence", "strengths"))
    assert _same(a["hps"], b["hps"]) and _same(a["hps"], mag * mag) and np.array_equal(a["f0_bin"], b["f0_bin"])
    # zero harmonics: strengths are empty and the confidence is 0 on voiced rows
    z = ctx.hps_from_spectrum(mag, WS, SR, 0, 80.0, 2000.0, skip=())
    assert z["strengths"].shape == (65, 0) and z["f0_bin"].all() and not z["confidence"].any()


@pytest.mark.parametrize("kw,word", [
    (dict(sample_rate=0), "sample_rate"), (dict(window_size=0), "window_size"), (dict(window_size=-5), "window_size"),
    (dict(min_f0=math.nan), "min_f0"), (dict(max_f0=math.inf), "max_f0"), (dict(min_f0=-1.0), "negative"),
    (dict(max_f0=-1.0), "negative"), (dict(max_f0=1e300), "int32"), (dict(K=8193), "8192"),
    (dict(num_harmonics=65), "64"), (dict(num_harmonics=-1), "negative num_harmonics"),
    (dict(num_harmonics=-1, skip=("confidence", "hps")), "negative num_harmonics"),
    (dict(num_harmonics=-1, skip=("strengths", "hps")), "negative num_harmonics")])
def test_from_spectrum_unsupported(ctx, kw, word):
    a = dict(K=16, window_size=2048, sample_rate=44100, num_harmonics=10, min_f0=80.0, max_f0=2000.0, skip=())
    a.update(kw)
    with pytest.raises(sonar.SonarError) as e:
        ctx.hps_from_spectrum(np.ones((2, a["K"])), a["window_size"], a["sample_rate"], a["num_harmonics"], a["min_f0"],
                              a["max_f0"], skip=a["skip"])
    assert e.value.code == sonar.ERR_UNSUPPORTED and e.value.msg.startswith("harmonic product: ") and word in e.value.msg


def test_from_spectrum_invalid(ctx):
    d = torch.ones(2, 16, dtype=torch.float64, device="cuda")
    b = torch.zeros(2, dtype=torch.int32, device="cuda")
    f0 = torch.zeros(2, dtype=torch.float64, device="cuda")
    for args, text in [((d.data_ptr(), -1, 16, 2048, 44100, b.data_ptr(), f0.data_ptr()), "negative row count"),
                       ((d.data_ptr(), 2, -1, 2048, 44100, b.data_ptr(), f0.data_ptr()), "negative row count"),
                       ((d.data_ptr(), 2, 16, 2048, 44100, None, f0.data_ptr()), "null f0_bin or f0"),
                       ((d.data_ptr(), 2, 16, 2048, 44100, b.data_ptr(), None), "null f0_bin or f0"),
                       ((None, 2, 16, 2048, 44100, b.data_ptr(), f0.data_ptr()), "null magnitude")]:
        with pytest.raises(sonar.SonarError) as e:
            ctx.hps_from_spectrum_device(*args)
        assert e.value.code == sonar.ERR_INVALID and text in e.value.msg


def test_hps_errors(ctx):
    x = _pcm(1024 + 256 * 20)
    for args, code, text in [
            ((np.zeros(0), 44100), sonar.ERR_EMPTY, "empty signal"),
            ((x, 44100, 0, 256), sonar.ERR_INVALID, "window size must be positive"),
            ((x, 44100, 1024, 0), sonar.ERR_INVALID, "hop size must be positive"),
            ((x[:512], 44100, 2048, 512), sonar.ERR_TOO_SHORT, "signal too short for given window size and hop size"),
            ((np.zeros(10000), 44100, 8193, 256), sonar.ERR_UNSUPPORTED, "above 8192"),
            ((x, 44100, 1, 1), sonar.ERR_UNSUPPORTED, "fewer than 2 samples"),
            ((x, 0, 1024, 256), sonar.ERR_UNSUPPORTED, "sample_rate"),
            ((x, 44100, 1024, 256, 10, math.nan, 2000.0), sonar.ERR_UNSUPPORTED, "min_f0"),
            ((x, 44100, 1024, 256, 10, 80.0, -2.0), sonar.ERR_UNSUPPORTED, "negative"),
            ((x, 44100, 1024, 256, 10, 80.0, 1e300), sonar.ERR_UNSUPPORTED, "int32"),
            ((x, 44100, 1024, 256, 65), sonar.ERR_UNSUPPORTED, "64"),
            ((x, 44100, 1024, 256, -1), sonar.ERR_UNSUPPORTED, "negative num_harmonics")]:
        with pytest.raises(sonar.SonarError) as e:
            ctx.hps(*args)
        assert e.value.code == code and text in e.value.msg, (args[1:], e.value.msg)
    ok = ctx.hps(x, 44100, 1024, 256, -1, skip=("confidence", "strengths", "magnitude"))
    assert ok["f0_bin"].shape == (21,) and ok["f0_bin"].all()
    d = torch.from_numpy(x.copy()).cuda()
    with pytest.raises(sonar.SonarError) as e:
        ctx.hps_device(d.data_ptr(), len(x), 44100, None, None, 1024, 256)
    assert e.value.code == sonar.ERR_INVALID and "null f0_bin or f0" in e.value.msg
