"""Row a13: LPC formant analysis (FormantAnalyzer.AnalyzeMultipleFrames / AnalyzeFormants,
algorithms/speech/format.go:85-449; LPCAnalyzer, lpc.go:44-265) on the GPU vs the oracle.

The reference obtains R through an FFT cross-correlation; the device sums the same lags
directly, so R agrees to ~1e-13 relative and every downstream value to a tolerance:
frame status, formant count and formant frequencies (bin index x sr/1024) must match
exactly; LPC coefficients, amplitudes, confidences, gain and quality to 1e-6 relative."""
import numpy as np
import pytest
import torch  # noqa: F401 -- before the library loads HIP (one HIP runtime in the process)

import oracle as O
from sonar import synth

pytestmark = pytest.mark.gpu


def _cmp(got, ref):
    assert np.array_equal(got["status"], ref["status"])
    ok = ref["status"] == 0
    assert np.array_equal(got["n_formants"][ok], ref["n_formants"][ok])
    assert np.array_equal(got["frequency"][ok], ref["frequency"][ok])
    assert np.array_equal(got["bandwidth"][ok], ref["bandwidth"][ok])
    assert np.array_equal(got["stable"][ok], ref["stable"][ok])
    for k in ("amplitude", "confidence", "vocal_tract_length", "quality", "gain", "residual_energy"):
        a, b = got[k][ok], ref[k][ok]
        assert np.allclose(a, b, rtol=1e-6, atol=1e-9, equal_nan=True), k


@pytest.mark.parametrize("sr,seconds", [(16000, 30.0), (8000, 10.0), (44100, 5.0)])
def test_formant_frames_match_oracle(ctx, sr, seconds):
    x = synth.c4_speech(seconds=seconds, sr=sr)
    got = ctx.formants(x, sr, want_lpc=True)
    ref = O.formant_frames(x, sr, want_lpc=True)
    assert len(got["status"]) == len(ref["status"]) > 0
    _cmp(got, ref)
    ok = ref["status"] == 0
    scale = np.max(np.abs(ref["lpc_coeffs"][ok]), axis=1, keepdims=True)
    assert np.max(np.abs(got["lpc_coeffs"][ok] - ref["lpc_coeffs"][ok]) / scale) < 1e-6


def test_formant_frames_full_c4_30min(ctx):
    """BASELINE configs[3] at its own size: AnalyzeMultipleFrames (format.go:427-449) over the whole
    30-min 16 kHz C4 signal (28,123 frames of 2,048 at hop 1,024), the bench's c4_formants call,
    against the oracle frame by frame with the rules above (status, counts and frequencies exact)."""
    x = synth.c4_speech(seconds=1800.0, sr=16000)
    got = ctx.formants(x, 16000, want_lpc=True)
    ref = O.formant_frames(x, 16000, want_lpc=True)
    assert len(got["status"]) == len(ref["status"]) == 28123
    _cmp(got, ref)
    ok = ref["status"] == 0
    assert np.count_nonzero(ok) > 0
    # the order-28 Levinson recursion amplifies R's ~1e-13 difference (direct sums vs Go's FFT
    # autocorrelation) by the frame's conditioning: over the 28,123 frames the worst coefficient is
    # 1.5e-6 of the frame's largest (round 5, GPU), so the full-size bound is 1e-5 -- the returned
    # features above stay exact / 1e-6, and the 30 s cases keep 1e-6 on the coefficients
    scale = np.max(np.abs(ref["lpc_coeffs"][ok]), axis=1, keepdims=True)
    e = np.abs(got["lpc_coeffs"][ok] - ref["lpc_coeffs"][ok]) / scale
    assert np.max(e) < 1e-5
    assert np.count_nonzero(np.max(e, axis=1) > 1e-6) <= 10


def test_formant_frames_custom_geometry_and_edges(ctx):
    x = synth.c4_speech(seconds=6.0, sr=16000)
    for fs, hop in [(4096, 1000), (2048, 512), (1500, 700)]:          # 1500 < W: every frame rejected
        got = ctx.formants(x, 16000, frame_size=fs, hop_size=hop)
        ref = O.formant_frames(x, 16000, frame_size=fs, hop_size=hop)
        _cmp(got, ref)
    z = np.zeros(3 * 2048)
    got = ctx.formants(z, 16000)
    assert np.all(got["status"] == 3)                                  # zero energy signal
    assert len(ctx.formants(x[:2048], 16000)["status"]) == 0           # i < n - frameSize: no frame


# ---- full-order frames, every rate class and every output (formant_cases.py, formant_ref.py) ----
# The inputs above end the Levinson recursion within four steps (F11), so their E is negative, their
# gain NaN and a[5..p] zero.  The cases below run it to order p at every (W, p) class; the checker
# splits the comparison in two: the front end (lags and recursion) against exact lags within the
# measured disagreement of two references, and the tail (envelope recurrence, ballot searches) fed
# the device's own coefficients, exact on every frame no admissible envelope error can flip.
import ctypes  # noqa: E402

import formant_cases as FC  # noqa: E402
import formant_ref as FR  # noqa: E402
from sonar import _abi  # noqa: E402

_GOT = {}


def _got(ctx, cid):
    if cid not in _GOT:
        pcm, sr, fs, hp = FC.case(cid)
        _GOT[cid] = ctx.formants(pcm, sr, frame_size=fs, hop_size=hp, want_lpc=True)
    return _GOT[cid]


def _order(k_row):
    nz = np.nonzero(k_row)[0]
    return int(nz[-1]) + 1 if len(nz) else 0


@pytest.mark.parametrize("cid", FC.CASE_IDS)
def test_formant_front_end_matches_checker(ctx, cid):
    """lpc_coeffs, reflection, residual_energy and gain against the checker's exact lags: status, the
    order reached, the zeros beyond it and the sign of E exactly, the floats within max(1e-12, 16 d)."""
    got, ref = _got(ctx, cid), FC.reference(cid)
    sr = FC.CASES[cid][1]
    p = FC.RATES[sr][1]
    bound = FC.front_end_bound(cid)
    assert len(got["status"]) == len(ref) and got["lpc_coeffs"].shape == (len(ref), p + 1)
    assert got["reflection"].shape == (len(ref), p)
    full, worst = 0, 0.0
    for i, f in enumerate(ref):
        a, k, E = got["lpc_coeffs"][i], got["reflection"][i], got["residual_energy"][i]
        assert got["status"][i] == f["status"] == 0 and got["lpc_order"][i] == p
        assert _order(k) == f["order"]
        assert not np.any(a[f["order"] + 1:]) and not np.any(k[f["order"]:]) and a[0] == 1.0
        assert (E > 0) == (f["residual_energy"] > 0)
        ea = np.max(np.abs(a - f["lpc_coeffs"])) / np.max(np.abs(f["lpc_coeffs"]))
        ek = np.max(np.abs(k - f["reflection"])) / np.max(np.abs(f["reflection"]))
        eE = abs(E - f["residual_energy"]) / abs(f["residual_energy"])
        worst = max(worst, ea, ek, eE)
        assert ea <= bound and ek <= bound and eE <= bound, (i, ea, ek, eE, bound)
        if E > 0:
            assert np.isfinite(got["gain"][i]) and abs(got["gain"][i] - f["gain"]) <= bound * f["gain"]
        else:
            assert np.isnan(got["gain"][i]) or got["gain"][i] == 0.0
        full += FC.full_order(f, p)
    print("%s: worst front-end error %.3g, bound %.3g" % (cid, worst, bound))
    assert full >= 8                                                   # gain is a number where it matters


@pytest.mark.parametrize("cid", FC.CASE_IDS)
def test_formant_reflection_coefficients(ctx, cid):
    """The `reflection` output by itself: within the front-end bound of the checker's, its last entry
    the coefficient the recursion stored last (a[i] = k[i-1], lpc.go:117), |k| < 1 while E stays positive."""
    got, ref = _got(ctx, cid), FC.reference(cid)
    bound = FC.front_end_bound(cid)
    for i, f in enumerate(ref):
        k, n = got["reflection"][i], f["order"]
        assert np.max(np.abs(k - f["reflection"])) <= bound * np.max(np.abs(f["reflection"]))
        assert k[n - 1] == got["lpc_coeffs"][i][n]
        assert np.all(np.abs(k[:n - 1]) < 1.0)
        assert (abs(k[n - 1]) < 1.0) == (got["residual_energy"][i] > 0)


@pytest.mark.parametrize("cid", FC.CASE_IDS)
def test_formant_tail_in_isolation(ctx, cid):
    """The device's own lpc_coeffs and residual_energy through formant_ref.tail: on decided frames
    n_formants, frequency, bandwidth and stable are exact and amplitude, confidence, VTL and quality lie
    within the derived envelope bound.  No Levinson conditioning is left in this comparison: the
    rotation recurrence (i up to 64) and every ballot search answer for themselves."""
    got = _got(ctx, cid)
    sr = FC.CASES[cid][1]
    decided = 0
    for i in range(len(got["status"])):
        t = FR.tail([float(v) for v in got["lpc_coeffs"][i]], float(got["residual_energy"][i]), sr)
        if not t["decided"]:
            continue
        decided += 1
        assert got["n_formants"][i] == t["n_formants"] and got["stable"][i] == t["stable"], i
        assert np.array_equal(got["frequency"][i], t["frequency"]), i
        assert np.array_equal(got["bandwidth"][i], t["bandwidth"]), i
        for k in ("amplitude", "confidence"):
            assert np.all(np.abs(got[k][i] - t[k]) <= t["bound"][k]), (i, k, got[k][i], t[k], t["bound"][k])
        for k in ("vocal_tract_length", "quality"):
            assert abs(got[k][i] - t[k]) <= t["bound"][k], (i, k, got[k][i], t[k], t["bound"][k])
    assert decided >= 8 and 10 * (len(got["status"]) - decided) <= len(got["status"])


@pytest.mark.parametrize("cid", FC.CASE_IDS)
def test_formant_cases_match_oracle(ctx, cid):
    """End to end against the oracle with the rules of the tests above."""
    got, ref = _got(ctx, cid), FC.oracle_frames(cid)
    _cmp(got, ref)
    scale = np.max(np.abs(ref["lpc_coeffs"]), axis=1, keepdims=True)
    assert np.max(np.abs(got["lpc_coeffs"] - ref["lpc_coeffs"]) / scale) < 1e-6


def _raw_call(ctx, pcm, sr, fs, hp, device):
    """sonar_formants with every output buffer pre-filled with 0xFF bytes, through host pointers or
    (device_ptrs = 1) torch device tensors -> the bytes of the records, coefficients and reflection."""
    L = ctx._L
    p = 12 + sr // 1000
    F = int(L.sonar_formant_frame_count(len(pcm), sr, fs, hp))
    sizes = (F * ctypes.sizeof(_abi.FormantFrame), F * (p + 1) * 8, F * p * 8)
    if device:
        dev = torch.device("cuda", 0)
        x = torch.from_numpy(np.array(pcm, dtype=np.float64)).to(dev)
        bufs = [torch.full((n,), 0xFF, dtype=torch.uint8, device=dev) for n in sizes]
        ptrs = [ctypes.c_void_p(b.data_ptr()) for b in bufs]
        torch.cuda.synchronize()                                       # the fills ran on torch's stream
        rc = L.sonar_formants(ctx._h, ctypes.c_void_p(x.data_ptr()), len(pcm), sr, fs, hp, *ptrs, 1)
        ctx.synchronize()
        out = [b.cpu().numpy().tobytes() for b in bufs]
    else:
        x = np.ascontiguousarray(pcm, dtype=np.float64)
        bufs = [np.full(n, 0xFF, dtype=np.uint8) for n in sizes]
        rc = L.sonar_formants(ctx._h, x.ctypes.data_as(ctypes.c_void_p), len(pcm), sr, fs, hp,
                              *[b.ctypes.data_as(ctypes.c_void_p) for b in bufs], 0)
        out = [b.tobytes() for b in bufs]
    assert rc == 0
    return F, p, out


def _device_ptr_inputs():
    pcm, sr, fs, hp = FC.case("burst-16000")
    mixed = pcm.copy()
    for f in (0, 3, 4, 15):                                           # silent frames among ok ones: status 3
        mixed[f * 2048:(f + 1) * 2048] = 0.0
    return {"ok": (pcm, sr, fs, hp, {0}), "ok-and-silent": (mixed, sr, fs, hp, {0, 3}),
            "frame-under-W": (pcm[:9000], sr, 1500, 700, {1})}


@pytest.mark.parametrize("name", ["ok", "ok-and-silent", "frame-under-W"])
def test_formant_device_ptrs_equal_host_ptrs_and_write_every_field(ctx, name):
    """device_ptrs = 1 (PCM, records, coefficients and reflection in device memory): every byte equals
    the host-pointer call, and over 0xFF-filled buffers every field of every record is written,
    lpc_order, gain and residual_energy of rejected frames included; a rejected frame's coefficient
    rows are zero."""
    pcm, sr, fs, hp, statuses = _device_ptr_inputs()[name]
    F, p, host = _raw_call(ctx, pcm, sr, fs, hp, device=False)
    F2, _, dev = _raw_call(ctx, pcm, sr, fs, hp, device=True)
    assert F == F2 > 0
    for h, d, what in zip(host, dev, ("records", "lpc_coeffs", "reflection")):
        assert h == d, what
    rec = np.frombuffer(dev[0], dtype=np.dtype(_abi.FormantFrame))
    assert set(rec["status"].tolist()) == statuses
    assert np.all(rec["lpc_order"] == p) and np.all(rec["n_formants"] >= 0) and np.all(rec["n_formants"] <= 4)
    assert np.all((rec["stable"] == 0) | (rec["stable"] == 1))
    words = np.frombuffer(dev[0], dtype=np.uint64).reshape(F, -1)
    assert not np.any(words[:, 1:21] == np.uint64(0xFFFFFFFFFFFFFFFF))     # the 20 doubles of a record
    co = np.frombuffer(dev[1], dtype=np.float64).reshape(F, p + 1)
    rf = np.frombuffer(dev[2], dtype=np.float64).reshape(F, p)
    bad = rec["status"] != 0
    assert not np.any(co[bad]) and not np.any(rf[bad])
    assert np.all(co[~bad][:, 0] == 1.0) and not np.any(np.isnan(co)) and not np.any(np.isnan(rf))
    assert np.all(rec["gain"][bad] == 0.0) and np.all(rec["residual_energy"][bad] == 0.0)
    ref = O.formant_frames(pcm, sr, fs, hp, want_lpc=True)
    got = {k: np.array(rec[k]) for k in O.FORMANT_KEYS}
    _cmp(got, ref)


def test_formant_rate_edges(ctx):
    """The W switch at 15,999 / 16,000 Hz, p = 64 = LPC_MAXP up to 52,999 Hz, SONAR_ERR_UNSUPPORTED from
    53,000 Hz, after which the context serves a 16 kHz call as a fresh one does."""
    import sonar
    x = synth.c4_speech(seconds=1.0, sr=16000)[:12000]
    lo, hi = ctx.formants(x, 15999, want_lpc=True), ctx.formants(x, 16000, want_lpc=True)
    assert len(lo["status"]) == (12000 - 1024 - 1) // 512 + 1 == 22 and len(hi["status"]) == 10
    assert np.all(lo["lpc_order"] == 27) and np.all(hi["lpc_order"] == 28)
    assert lo["lpc_coeffs"].shape == (22, 28) and hi["lpc_coeffs"].shape == (10, 29)
    _cmp(lo, O.formant_frames(x, 15999))
    _cmp(hi, O.formant_frames(x, 16000))
    # a frame of 1,500 samples is long enough for W 1024 and too short for W 2048
    short = ctx.formants(x, 15999, frame_size=1500, hop_size=700)["status"]
    assert np.array_equal(short, O.formant_frames(x, 15999, 1500, 700)["status"]) and np.count_nonzero(short == 0) >= 8
    assert np.all(ctx.formants(x, 16000, frame_size=1500, hop_size=700)["status"] == 1)

    pcm = FC.case("periodic-52000")[0]
    top = ctx.formants(pcm, 52999, hop_size=1030, want_lpc=True)
    ref = O.formant_frames(pcm, 52999, hop_size=1030, want_lpc=True)
    assert np.all(top["lpc_order"] == 64) and top["lpc_coeffs"].shape == (14, 65)
    assert np.all(top["status"] == 0) and min(_order(k) for k in top["reflection"]) == 64
    _cmp(top, ref)
    scale = np.max(np.abs(ref["lpc_coeffs"]), axis=1, keepdims=True)
    assert np.max(np.abs(top["lpc_coeffs"] - ref["lpc_coeffs"]) / scale) < 1e-6

    before = ctx.formants(x, 16000, want_lpc=True)
    for sr in (53000, 96000):
        with pytest.raises(sonar.SonarError, match=r"LPC order above 64 \(sample rate > 52 kHz\)") as e:
            ctx.formants(pcm, sr)
        assert e.value.code == sonar.ERR_UNSUPPORTED
    after = ctx.formants(x, 16000, want_lpc=True)
    fresh_ctx = sonar.Context(0)
    try:
        fresh = fresh_ctx.formants(x, 16000, want_lpc=True)
    finally:
        fresh_ctx.close()
    for k in before:
        assert before[k].tobytes() == after[k].tobytes() == fresh[k].tobytes(), k
