"""sonar_chord_frames, sonar_chord_sequence, sonar_chord_progression and sonar_chord_detect on the GPU
against the Python checker (tests/chord_ref.py, held to known answers in test_chord_cpu.py) on the inputs
of tests/chord_cases.py.

Bounds.  Every step is a fixed sequence of float64 operations in the reference's order and nothing calls
a transcendental function, so every floating output is equal bit for bit and every integer output is
equal.  The inputs are finite, so nothing is NaN.  No case is left out.

Shapes.  See chord_cases.py: the lengths run over both sides of the 63 rows a block reports, of 64 and of
two blocks, and one past the 1024 records the chain kernel stages.  sonar_chord_detect is held to the
explicit composition through the public entries (sonar_fingerprint's magnitudes under the rectangular
window, mirrored in numpy, sonar_hpcp_from_spectrum, sonar_chord_sequence), bit for bit."""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library loads HIP (one HIP runtime in the process)

import chord_cases as K
import chord_ref as R
import sonar
from sonar import SonarError

pytestmark = pytest.mark.gpu

INTS = ("root", "quality", "inversion", "n_found", "extensions", "role")
FLOATS = ("confidence", "strength", "clarity", "ambiguity", "consonance", "tension", "stability")
PAD = {"candidates": -1, "cand_inversion": 0, "cand_confidence": 0.0, "cand_strength": 0.0}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _raises(code, text, fn, *a, **kw):
    with pytest.raises(SonarError) as e:
        fn(*a, **kw)
    assert e.value.code == code and text in str(e.value), str(e.value)


def _lib_params(p):
    return sonar.chord_params(**p)


def _check(got, ref, p, skip=()):
    F, mc = len(ref), max(p["max_candidates"], 0)
    for n in INTS:
        if n not in skip:
            assert got[n].dtype == np.int32 and got[n].tolist() == [f[n] for f in ref], n
    for n in FLOATS:
        if n not in skip:
            assert not np.any(np.isnan(got[n])) and _same(got[n], [f[n] for f in ref]), n
    if "template_scores" not in skip:
        assert _same(got["template_scores"], np.array([f["template_scores"] for f in ref]).reshape(F, 120))
    for n, pad in PAD.items():
        if n not in skip:
            want = np.array([f[n] + [pad] * (mc - len(f[n])) for f in ref], dtype=got[n].dtype).reshape(F, mc)
            assert got[n].shape == (F, mc)
            assert np.array_equal(got[n], want) if got[n].dtype == np.int32 else _same(got[n], want), n
    for n in skip:
        assert got[n] is None


# ---- the inputs are what the tests need them to be (the checker alone) ------------------------------------

def test_inputs_meet_their_conditions():
    a, _ = K.reference("a-F%d" % K.LONG, "frames")
    assert sum(r["cand_confidence"][0] == r["cand_confidence"][1] == 1.0 for r in a) >= 0.95 * len(a)   # the tie regime
    b, _ = K.reference("b-F%d" % K.LONG, "frames")
    assert sum(r["confidence"] < 1.0 for r in b) >= 0.95 * len(b)
    assert sum(r["cand_confidence"][0] == r["cand_confidence"][1] for r in b) <= 0.02 * len(b)
    assert min(r["n_found"] for r in b) >= 2 and sum(r["n_found"] > 5 for r in b) >= 0.99 * len(b)
    note, conf = K.bass()
    assert set(note.tolist()) == set(range(12)) and np.any(conf <= 0.3) and np.any(conf > 0.3)
    bass, _ = K.reference("b-bass-F%d" % K.LONG, "frames")
    assert {v for r in bass for v in r["cand_inversion"]} >= {0, 1, 2}     # inversions are found and not found
    gaps, _ = K.reference("gaps-default", "sequence")
    found = [r["n_found"] for r in gaps]
    assert found[0] == found[-1] == found[K.BLOCK] == 0 and max(found) > 5
    steady, _ = K.reference("steady-w5", "sequence")
    assert all(r["n_found"] == 67 for r in steady)


# ---- every case, per frame and in sequence ---------------------------------------------------------------

@pytest.mark.parametrize("cid", K.CASE_IDS)
def test_frames(ctx, cid):
    rows, p, bn, bc = K.case(cid)
    ref, _ = K.reference(cid, "frames")
    _check(ctx.chord_frames(rows, _lib_params(p), bn, bc), ref, p)


@pytest.mark.parametrize("cid", K.CASE_IDS)
def test_sequence(ctx, cid):
    rows, p, bn, bc = K.case(cid)
    ref, err = K.reference(cid, "sequence")
    if err is not None:                                         # Go panics in the middle of the sequence
        with pytest.raises(SonarError) as e:
            ctx.chord_sequence(rows, _lib_params(p), bn, bc)
        assert e.value.code == sonar.ERR_PANIC and str(err) in str(e.value)
        return
    _check(ctx.chord_sequence(rows, _lib_params(p), bn, bc), ref, p)


def test_steady_row_alternates_exactly(ctx):
    """F52 on the device: C 0.82, C 0.902, then Am7 0.8789 and C 0.902 in turn."""
    got = ctx.chord_sequence(np.array([K.STEADY] * 6), sonar.chord_params(normalize_templates=0))
    names = [sonar.chord_name(r, q, i) for r, q, i in zip(got["root"], got["quality"], got["inversion"])]
    assert names == ["C", "C", "Aminor7", "C", "Aminor7", "C"]
    assert got["confidence"].tolist() == [0.8200000000000001, 0.9020000000000001, 0.8789000000000001,
                                          0.9020000000000001, 0.8789000000000001, 0.9020000000000001]
    assert got["n_found"].tolist() == [67] * 6
    got = ctx.chord_sequence(np.array([K.STEADY] * 6), sonar.chord_params(normalize_templates=0, temporal_window=50))
    assert got["quality"].tolist() == [0, 0, 7, 0, 7, 0]


@pytest.mark.parametrize("window", [67, 68])
def test_steady_row_windows_above_the_limit_are_declined(ctx, window):
    """The windows that stop the alternation on the 67-candidate row (test_chord_cpu.py runs them through the
    checker) are above the 64 the stability pass takes; the library says so instead of computing."""
    _raises(sonar.ERR_UNSUPPORTED, "temporal_window above 64", ctx.chord_sequence, np.array([K.STEADY] * 6),
            sonar.chord_params(normalize_templates=0, temporal_window=window))


def test_window_of_the_candidate_count_stops_the_alternation(ctx):
    """F52: a window >= |C| stops it.  The steady row has 67 candidates, above the 64 the library takes, so
    the threshold is raised until 40 remain and the windows 39, 40 and 41 are run."""
    p = R.params(normalize_templates=0, min_chord_strength=0.3)
    rows = np.array([K.STEADY] * 6)
    n = R.sequence(rows, p)[0]["n_found"]
    assert 5 < n <= 64
    for w in (n - 1, n, n + 1):
        q = dict(p, temporal_window=w)
        ref = R.sequence(rows, q)
        assert (len({r["name"] for r in ref}) == 1) == (w >= n)
        _check(ctx.chord_sequence(rows, _lib_params(q)), ref, q)


def test_sequence_equals_frames_on_frame_0_and_differs_after(ctx):
    rows, p, bn, bc = K.case("b-F129")
    seq, fr = ctx.chord_sequence(rows, _lib_params(p)), ctx.chord_frames(rows, _lib_params(p))
    for n in sonar.CHORD_FIELDS:
        assert np.array_equal(seq[n][0], fr[n][0]), n
    assert np.sum(seq["confidence"][1:] != fr["confidence"][1:]) >= 100
    assert np.sum(seq["stability"][1:] != fr["stability"][1:]) >= 100
    assert np.array_equal(seq["template_scores"], fr["template_scores"]) and np.array_equal(seq["n_found"], fr["n_found"])


@pytest.mark.parametrize("name", sonar.CHORD_FIELDS)
@pytest.mark.parametrize("sequence", [False, True])
def test_every_output_null_in_turn(ctx, name, sequence):
    cid = "b-bass-F65"
    rows, p, bn, bc = K.case(cid)
    ref, _ = K.reference(cid, "sequence" if sequence else "frames")
    fn = ctx.chord_sequence if sequence else ctx.chord_frames
    _check(fn(rows, _lib_params(p), bn, bc, skip=(name,)), ref, p, skip=(name,))


@pytest.mark.parametrize("sequence", [False, True])
def test_only_one_output(ctx, sequence):
    cid = "b-bass-F65"
    rows, p, bn, bc = K.case(cid)
    ref, _ = K.reference(cid, "sequence" if sequence else "frames")
    fn = ctx.chord_sequence if sequence else ctx.chord_frames
    for keep in ("stability", "candidates", "root"):
        skip = tuple(n for n in sonar.CHORD_FIELDS if n != keep)
        _check(fn(rows, _lib_params(p), bn, bc, skip=skip), ref, p, skip=skip)


def _device_outs(F, mc):
    i, d = torch.int32, torch.float64
    out = {}
    for n in sonar.CHORD_FIELDS:
        shape = (F, 120) if n == "template_scores" else (F, mc) if n.startswith("cand") else (F,)
        dt = i if n in INTS + ("candidates", "cand_inversion") else d
        out[n] = torch.full(shape, -7, dtype=dt, device="cuda")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("sequence", [False, True])
def test_device_pointers_equal_host_pointers(ctx, sequence):
    cid = "b-bass-F129"
    rows, p, bn, bc = K.case(cid)
    F = len(rows)
    d = torch.from_numpy(np.array(rows)).cuda()
    dn, dc = torch.from_numpy(np.array(bn)).cuda(), torch.from_numpy(np.array(bc)).cuda()
    out = _device_outs(F, p["max_candidates"])
    ctx.chord_rows_device(d.data_ptr(), F, 12, _lib_params(p), sequence=sequence, bass_note_ptr=dn.data_ptr(),
                          bass_confidence_ptr=dc.data_ptr(), **{n: t.data_ptr() for n, t in out.items()})
    host = (ctx.chord_sequence if sequence else ctx.chord_frames)(rows, _lib_params(p), bn, bc)
    for n in sonar.CHORD_FIELDS:
        got = out[n].cpu().numpy()
        assert np.array_equal(got, host[n]) if got.dtype == np.int32 else _same(got, host[n]), n
    ref, _ = K.reference(cid, "sequence" if sequence else "frames")
    _check({n: out[n].cpu().numpy() for n in sonar.CHORD_FIELDS}, ref, p)


# ---- errors -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sequence", [False, True])
def test_errors(ctx, sequence):
    fn = ctx.chord_sequence if sequence else ctx.chord_frames
    rows = np.array(K.rows_b()[:70])
    bn, bc = (np.array(v[:70]) for v in K.bass())
    P = sonar.chord_params
    for mc in (-1, -7):
        _raises(sonar.ERR_PANIC, "runtime error: slice bounds out of range [:%d]" % mc, fn, rows, P(max_candidates=mc))
        _raises(sonar.ERR_PANIC, "runtime error: slice bounds out of range [:%d]" % mc, fn, np.zeros((3, 12)),
                P(max_candidates=mc))                           # even for rows without candidates
    for dim in (0, 1, 11, 13, 48):
        _raises(sonar.ERR_INVALID, "failed to extract chroma features: unsupported chroma size: %d" % dim, fn,
                np.ones((4, dim)), P())
    # Go's order: extractChromaFeatures fails (:416) before the cut panics (:458)
    _raises(sonar.ERR_INVALID, "unsupported chroma size: 13", fn, np.ones((4, 13)), P(max_candidates=-1))
    for bad in (-1, 12):
        for at in (0, 63, 69):
            notes = bn.copy()
            notes[at] = bad
            _raises(sonar.ERR_INVALID, "bass note", fn, rows, P(), notes, bc)
    for bad in (np.nan, np.inf, -np.inf):
        for at in ((0, 0), (62, 11), (63, 5), (69, 11)):
            x = rows.copy()
            x[at] = bad
            _raises(sonar.ERR_UNSUPPORTED, "non-finite", fn, x, P())
        wide = np.array(K.rows_a(K.PF, 36))
        wide[40, 35] = bad                                      # a bin no score reads
        _raises(sonar.ERR_UNSUPPORTED, "non-finite", fn, wide, P())
        conf = bc.copy()
        conf[64] = bad
        _raises(sonar.ERR_UNSUPPORTED, "non-finite", fn, rows, P(), bn, conf)
        _raises(sonar.ERR_UNSUPPORTED, "non-finite", fn, rows, P(min_chord_strength=bad))
        _raises(sonar.ERR_UNSUPPORTED, "non-finite", fn, rows, P(bass_weight=bad))
    _raises(sonar.ERR_UNSUPPORTED, "temporal_window above 64", fn, rows, P(temporal_window=65))
    # more frames than the library takes: refused before anything is read
    out = sonar.ChordOut()
    p = P()
    entry = ctx._L.sonar_chord_sequence if sequence else ctx._L.sonar_chord_frames
    rc = entry(ctx._h, rows.ctypes.data, 2 ** 31, 12, None, None, ctypes.byref(p), ctypes.byref(out), 0)
    assert rc == sonar.ERR_UNSUPPORTED and "2^31 - 1" in ctx._L.sonar_last_error(ctx._h).decode()


@pytest.mark.parametrize("sequence", [False, True])
def test_no_frames_reads_and_writes_nothing(ctx, sequence):
    entry = ctx._L.sonar_chord_sequence if sequence else ctx._L.sonar_chord_frames
    keep = np.full(4, 9.0)
    out = sonar.ChordOut()
    out.confidence = keep.ctypes.data
    for p in (sonar.chord_params(), sonar.chord_params(max_candidates=-1)):
        assert entry(ctx._h, None, 0, 13, None, None, ctypes.byref(p), ctypes.byref(out), 0) == 0
    assert keep.tolist() == [9.0] * 4
    got = (ctx.chord_sequence if sequence else ctx.chord_frames)(np.zeros((0, 12)))
    assert got["root"].shape == (0,) and got["candidates"].shape == (0, 5)


# ---- sonar_chord_progression --------------------------------------------------------------------------------

@pytest.mark.parametrize("F", [0, 1, 2, 65, 1024, 1025])
def test_progression(ctx, F):
    seq, _ = K.reference("b-F%d" % K.LONG, "sequence")
    q, cf = [r["quality"] for r in seq[:F]], [r["confidence"] for r in seq[:F]]
    ref = R.progression(q, cf)
    got = ctx.chord_progression(q, cf, root=[r["root"] for r in seq[:F]], inversion=[r["inversion"] for r in seq[:F]])
    assert got["num_chords"] == ref["num_chords"] == F and got["insufficient_data"] == ref["insufficient_data"]
    if F < 2:
        assert set(got) == {"num_chords", "insufficient_data"}
        return
    assert got["most_common_quality"] == ref["most_common_quality"]
    assert _same(got["average_confidence"], ref["average_confidence"])
    assert got["most_common_quality_name"] == R.quality_name(ref["most_common_quality"])


def test_progression_quality_tie_and_codes(ctx):
    """Equal counts: the lowest code (the reference iterates a map there).  Every ChordQuality code counts."""
    q = [23, 8, 8, 23, 1, 24, 24, 0]
    cf = [0.1 * (i + 1) for i in range(8)]
    got = ctx.chord_progression(q, cf)
    assert got["most_common_quality"] == 8 == R.progression(q, cf)["most_common_quality"]
    assert _same(got["average_confidence"], R.progression(q, cf)["average_confidence"])
    assert ctx.chord_progression([24, 24, 3], [1.0] * 3)["most_common_quality_name"] == "unknown"
    _raises(sonar.ERR_UNSUPPORTED, "quality code", ctx.chord_progression, [0, 32], [0.5, 0.5])
    _raises(sonar.ERR_UNSUPPORTED, "quality code", ctx.chord_progression, [-1, 0], [0.5, 0.5])
    _raises(sonar.ERR_UNSUPPORTED, "non-finite", ctx.chord_progression, [0, 1], [0.5, np.nan])


def test_progression_device_pointers(ctx):
    seq, _ = K.reference("b-F%d" % K.LONG, "sequence")
    q = torch.tensor([r["quality"] for r in seq], dtype=torch.int32).cuda()
    cf = torch.tensor([r["confidence"] for r in seq], dtype=torch.float64).cuda()
    num = torch.zeros(1, dtype=torch.int64, device="cuda")
    ins, most = (torch.full((1,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
    avg = torch.zeros(1, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.chord_progression_device(q.data_ptr(), cf.data_ptr(), len(seq), num.data_ptr(), ins.data_ptr(),
                                 avg.data_ptr(), most.data_ptr())
    ref = R.progression([r["quality"] for r in seq], [r["confidence"] for r in seq])
    assert (num.item(), ins.item(), most.item()) == (len(seq), 0, ref["most_common_quality"])
    assert _same(avg.cpu().numpy(), [ref["average_confidence"]])
    ctx.chord_progression_device(q.data_ptr(), cf.data_ptr(), 1, num.data_ptr(), ins.data_ptr(), avg.data_ptr(),
                                 most.data_ptr())
    assert (num.item(), ins.item(), most.item()) == (1, 1, ref["most_common_quality"])


# ---- sonar_chord_detect ---------------------------------------------------------------------------------------

def _signal(n, sr, seed=5):
    """Three chords in turn, partials with decaying amplitudes, plus a little noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    x = 0.01 * rng.standard_normal(n)
    third = n // 3 + 1
    for k, notes in enumerate(((60, 64, 67), (57, 60, 64, 67), (55, 59, 62, 65))):
        seg = slice(k * third, min((k + 1) * third, n))
        for m in notes:
            f0 = 440.0 * 2.0 ** ((m - 69) / 12.0)
            for h in (1, 2, 3):
                if f0 * h < sr / 2:
                    x[seg] += 0.2 / h * np.sin(2 * np.pi * f0 * h * t[seg])
    return x


def _composition(ctx, pcm, sr, frame_len, hop, p, bn=None, bc=None):
    """DetectChord through the public entries: the first min(2048, frame_len) samples of every frame under the
    rectangular window (F56), the full-length magnitude spectrum (F37), ComputeFromSpectrum, then the sequence."""
    W = min(2048, frame_len)
    F = (len(pcm) - frame_len) // hop + 1
    cfg = ctx.config(window_size=W, hop_size=hop, window_type="rectangular", sample_rate=sr, flags=sonar.FP_MAGNITUDE,
                     precision=sonar.F64, pcm_dtype=sonar.F64, out_dtype=sonar.F64)
    mag = ctx.fingerprint(pcm, cfg)["magnitude"][:F]
    full = np.concatenate([mag, mag[:, W // 2 - 1:0:-1]], axis=1)
    assert full.shape == (F, W) and np.array_equal(full[:, W - 3], full[:, 3])
    hp = ctx.hpcp_from_spectrum(full, W, sr)["hpcp"]
    return hp, ctx.chord_sequence(hp, p, bn, bc)


@pytest.mark.parametrize("sr", [8000, 44100])
@pytest.mark.parametrize("frame_len", [128, 1024, 2048, 4096])
def test_detect_is_the_composition(ctx, frame_len, sr):
    hop, F = frame_len // 4, 70
    pcm = _signal(frame_len + (F - 1) * hop, sr)
    p = sonar.chord_params(normalize_templates=frame_len % 2048 == 0)
    bn, bc = (np.array(v[:F]) for v in K.bass()) if frame_len == 1024 else (None, None)
    got = ctx.chord_detect(pcm, sr, frame_len, hop, p, bn, bc)
    hp, want = _composition(ctx, pcm, sr, frame_len, hop, p, bn, bc)
    assert _same(got["hpcp"], hp) and hp.shape == (F, 12)
    for n in sonar.CHORD_FIELDS:
        assert np.array_equal(got[n], want[n]) if got[n].dtype == np.int32 else _same(got[n], want[n]), n
    if frame_len >= 1024:
        assert np.any(got["n_found"] > 0) and len(set(got["root"].tolist())) > 1
    # and against the checker on the same profiles
    ref = R.sequence(hp, {n: getattr(p, n) for n, _ in p._fields_}, bn, bc)
    _check({n: got[n] for n in sonar.CHORD_FIELDS}, ref, {"max_candidates": p.max_candidates})


def test_detect_bass_only_at_1024(ctx):
    """F53: DetectPitch takes 1024-sample frames only; at every other length the bass is (0, 0.0)."""
    frame_len, hop, sr, F = 2048, 512, 44100, 40
    pcm = _signal(frame_len + (F - 1) * hop, sr)
    bn, bc = (np.array(v[:F]) for v in K.bass())
    with_arrays, without = ctx.chord_detect(pcm, sr, frame_len, hop, None, bn, bc), ctx.chord_detect(pcm, sr, frame_len, hop)
    for n in sonar.CHORD_FIELDS:
        assert np.array_equal(with_arrays[n], without[n]), n
    assert np.all(without["inversion"] == 0)


def test_detect_unsupported_and_errors(ctx):
    sr = 44100
    pcm = _signal(8192, sr)
    _raises(sonar.ERR_UNSUPPORTED, "power of two", ctx.chord_detect, pcm, sr, 1000, 250)
    _raises(sonar.ERR_UNSUPPORTED, "cqt_based", ctx.chord_detect, pcm, sr, 2048, 512, sonar.chord_params(method="cqt_based"))
    _raises(sonar.ERR_UNSUPPORTED, "bass arrays", ctx.chord_detect, pcm, sr, 1024, 256)
    ctx.chord_detect(pcm, sr, 1024, 256, sonar.chord_params(use_bass_detection=0))      # no bass wanted: fine
    _raises(sonar.ERR_TOO_SHORT, "too short", ctx.chord_detect, pcm[:1000], sr, 2048, 512)
    _raises(sonar.ERR_PANIC, "[:-1]", ctx.chord_detect, pcm, sr, 2048, 512, sonar.chord_params(max_candidates=-1))
    _raises(sonar.ERR_UNSUPPORTED, "temporal_window", ctx.chord_detect, pcm, sr, 2048, 512,
            sonar.chord_params(temporal_window=65))
    _raises(sonar.ERR_INVALID, "positive", ctx.chord_detect, pcm, sr, 2048, 0)


def test_detect_across_its_chunk_seam(ctx):
    """Frames of 2048 samples at hop 1 go through the magnitude scratch 2048 at a time: 2050 frames are a
    chunk of 2048 and one of 2.  The profiles on both sides of the seam are those of a call that sees the same
    frames in one chunk, bit for bit, and the chords are those of the sequence over the returned profiles."""
    frame_len, hop, sr, n = 2048, 1, 44100, 4097
    pcm = _signal(n, sr)
    p = sonar.chord_params()
    got = ctx.chord_detect(pcm, sr, frame_len, hop, p)
    assert got["hpcp"].shape == (2050, 12)
    part = ctx.chord_detect(pcm[2040:2040 + 2057], sr, frame_len, hop, p)
    assert part["hpcp"].shape == (10, 12) and _same(got["hpcp"][2040:2050], part["hpcp"])
    assert np.any(got["hpcp"][2046:2050] != 0.0)
    want = ctx.chord_sequence(got["hpcp"], p)
    for n_ in sonar.CHORD_FIELDS:
        assert np.array_equal(got[n_], want[n_]) if got[n_].dtype == np.int32 else _same(got[n_], want[n_]), n_


def test_flag_word_texts(ctx):
    """What the device's status word means, code and whole text, at one or two rows: the three flags of the row
    entries and the two of the progression."""
    def exact(code, text, fn, *a):
        with pytest.raises(SonarError) as e:
            fn(*a)
        assert (e.value.code, e.value.msg) == (code, text)
    P = sonar.chord_params
    rows = np.array(K.rows_b()[:2])
    nan_row = rows.copy()
    nan_row[1, 3] = np.nan
    nonfinite = ("chord detection: a non-finite chroma value or bass confidence is not reproduced (a NaN confidence "
                 "leaves the order of sort.Slice undefined)")
    for fn in (ctx.chord_frames, ctx.chord_sequence):
        exact(sonar.ERR_INVALID, "chord detection: a bass note outside 0..11", fn, rows, P(), np.array([0, 12]),
              np.array([0.5, 0.5]))
        exact(sonar.ERR_UNSUPPORTED, nonfinite, fn, nan_row, P())
        exact(sonar.ERR_UNSUPPORTED, nonfinite, fn, rows[:1], P(), np.array([3]), np.array([np.inf]))
    # a frame without candidates after one with, under a negative window: history[1:] of an empty history
    gap = np.array([K.rows_b()[0], [0.0] * 12])
    p = P(temporal_window=-1)
    with pytest.raises(IndexError, match=r"slice bounds out of range \[1:0\]"):
        R.sequence(gap, {n: getattr(p, n) for n, _ in p._fields_}, None, None)
    exact(sonar.ERR_PANIC, "runtime error: slice bounds out of range [1:0]", ctx.chord_sequence, gap, p)
    exact(sonar.ERR_UNSUPPORTED, "chord progression: a quality code outside 0..31", ctx.chord_progression, [0, 32], [0.5, 0.5])
    exact(sonar.ERR_UNSUPPORTED, "chord progression: a non-finite confidence", ctx.chord_progression, [0, 1], [0.5, np.nan])
