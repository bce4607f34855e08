"""sonar_key_frames, sonar_key_sequence and sonar_key_batch on the GPU against the Python checker
(tests/key_ref.py, held to known answers in test_key_cpu.py).

Bounds.  Everything per frame is a fixed sequence of float64 operations in the reference's order, so
scores, confidence, strength, clarity, tonality, the processed rows, the averages behind the sequence
result, stability, the votes, the global confidence and strength and the transition confidences are
bit-exact, and every integer output is equal.  ambiguity goes through log: 1e-12 absolute, the project's
bound for such values.

Shapes.  The per-frame kernel gives a block 64 rows, one per lane: F runs over both sides of 64 and of
256 and past 1024.  The ordered sums work in tiles (KEY_TILE_ELEMS / dim = 320 rows of 12 bins for the
average, KEY_TILE_FRAMES = 1024 frames for the votes, csrc/kernels.h): the lengths run over both sides of
one tile and two tiles plus one, and over every threshold of EstimateKeySequence (3, 10, 20, 22)."""
import functools
import math

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library loads HIP (one HIP runtime in the process)

import key_ref as R
import sonar
from sonar import SonarError

pytestmark = pytest.mark.gpu

SEED = 1
SUM_TILE, VOTE_TILE = 320, 1024
LONG = 2 * VOTE_TILE + 1
SCALARS = ("key", "mode", "known", "confidence", "strength", "clarity", "ambiguity", "tonality")
EXACT = ("confidence", "strength", "clarity", "tonality")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ---- inputs and their reference, computed once -----------------------------------------------------

@functools.lru_cache(maxsize=None)
def _tonal(F, seed=SEED, profile=0):
    """A key profile that changes every 40 frames, divided by its maximum, plus 0.35 |N(0, 1)|."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((F, 12))
    for b in range(0, F, 40):
        code = int(rng.integers(0, 24))
        prof = np.array(R.PROFILES[profile][code & 1])
        rows[b:b + 40] = np.array([prof[(i + (code >> 1)) % 12] for i in range(12)]) / prof.max()
    rows += 0.35 * np.abs(rng.standard_normal((F, 12)))
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def _wide(F, dim):
    """The tonal rows spread over dim bins (bin j takes pitch class j * 12 // dim) plus a little noise."""
    rng = np.random.default_rng(100 + dim)
    if dim == 0:
        return np.zeros((F, 0))
    if dim == 12:
        return _tonal(F)
    rows = _tonal(F)[:, (np.arange(dim) * 12) // dim] + 0.05 * rng.random((F, dim))
    rows.setflags(write=False)
    return rows


def _pkey(p):
    return tuple(sorted(p.items()))


@functools.lru_cache(maxsize=None)
def _frames_ref(kind, F, pk):
    rows = _wide(F, kind)
    return R.process_batch([list(r) for r in rows], dict(pk))


def _lib_params(p):
    return sonar.key_params(**p)


def _check_frames(got, ref, p, skip=()):
    F = len(ref)
    nc = min(p["max_candidates"], 24)
    for n in ("key", "mode", "known"):
        if n not in skip:
            assert got[n].tolist() == [f[n] for f in ref], n
    for n in EXACT:
        if n not in skip:
            assert _same(got[n], [f[n] for f in ref]), n
    if "ambiguity" not in skip:
        assert got["ambiguity"].shape == (F,)
        assert np.all(np.abs(got["ambiguity"] - np.array([f["ambiguity"] for f in ref])) <= 1e-12)
    if "scores" not in skip:
        assert _same(got["scores"], np.array([f["scores"] for f in ref]).reshape(F, 24))
    if "candidates" not in skip:
        assert got["candidates"].shape == (F, nc)
        assert got["candidates"].tolist() == [f["candidates"] for f in ref]
    if "processed" not in skip:
        assert _same(got["processed"], np.array([f["processed"] for f in ref]).reshape(F, p["hpcp_size"]))
    for n in skip:
        assert got[n] is None


# ---- the inputs are what the tests need them to be (the checker alone) ------------------------------

def test_tonal_input_meets_its_conditions():
    frames = _frames_ref(12, LONG, _pkey(R.params(min_confidence=0.0)))
    gap = min(np.min(np.diff(np.sort(f["scores"]))) for f in frames)
    assert gap > 0.0                                         # every row's 24 scores are pairwise distinct
    conf = np.array([f["confidence"] for f in frames])
    assert 0 < np.sum(conf > 0.7) < np.sum(conf > 0.5) < len(conf) and np.sum(conf <= 0.5) > 0
    codes = [f["code"] for f in frames]
    assert len(set(c >> 1 for c in codes)) >= 3
    for F in (300, LONG):
        counts = sorted(np.bincount(codes[:F], minlength=24))
        assert counts[-1] > counts[-2]                       # the most frequent code is unique
        votes = sorted(R.global_key(_frames_ref(12, LONG, _pkey(R.DEFAULT))[:F])["votes"])
        assert votes[-1] > votes[-2] > 0.0                   # and so is the top vote
    seq = R.estimate_key_sequence(_tonal(300), R.DEFAULT, frames=_frames_ref(12, LONG, _pkey(R.DEFAULT))[:300])
    assert len(seq["modulations"]) >= 1


# ---- sonar_key_frames --------------------------------------------------------------------------------

@pytest.mark.parametrize("F", [1, 2, 3, 63, 64, 65, 255, 256, 257, 1025, LONG])
def test_frames_every_length(ctx, F):
    ref = _frames_ref(12, LONG, _pkey(R.DEFAULT))[:F]
    _check_frames(ctx.key_frames(_tonal(LONG)[:F]), ref, R.DEFAULT)


@pytest.mark.parametrize("dim,hs", [(1, 12), (11, 12), (13, 12), (36, 12), (120, 12), (24, 24), (36, 36), (0, 12),
                                    (12, 120), (12, 11)])
def test_frames_every_row_length(ctx, dim, hs):
    p = R.params(hpcp_size=hs)
    ref = _frames_ref(dim, 65, _pkey(p))
    got = ctx.key_frames(_wide(65, dim), _lib_params(p))
    _check_frames(got, ref, p)
    if hs != 12:                                             # F44: nothing is scored, the tonality still reads the row
        assert not got["scores"].any() and not got["key"].any() and got["tonality"].any()
    if dim == 0:
        assert not got["processed"].any() and not got["tonality"].any()


@pytest.mark.parametrize("profile", range(7))
def test_frames_every_profile(ctx, profile):
    p = R.params(profile=profile)
    _check_frames(ctx.key_frames(_tonal(257), _lib_params(p)), _frames_ref(12, 257, _pkey(p)), p)


def test_frames_profile_outside_the_table_is_krumhansl(ctx):
    want = ctx.key_frames(_tonal(65))
    for prof in (-1, 7):
        got = ctx.key_frames(_tonal(65), sonar.key_params(profile=prof))
        assert all(np.array_equal(got[n], want[n]) for n in got)


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("remove_mean", [0, 1])
@pytest.mark.parametrize("binary", [0, 1])
def test_frames_every_preprocessing_switch(ctx, normalize, remove_mean, binary):
    p = R.params(normalize_chroma=normalize, remove_mean=remove_mean, binary_mode=binary)
    _check_frames(ctx.key_frames(_tonal(257), _lib_params(p)), _frames_ref(12, 257, _pkey(p)), p)


@pytest.mark.parametrize("max_candidates", [1, 5, 24, 25])
@pytest.mark.parametrize("min_confidence", [0.0, 0.5, 0.9])
def test_frames_candidates_and_threshold(ctx, max_candidates, min_confidence):
    p = R.params(max_candidates=max_candidates, min_confidence=min_confidence)
    ref = _frames_ref(12, 257, _pkey(p))
    got = ctx.key_frames(_tonal(257), _lib_params(p))
    _check_frames(got, ref, p)
    known = got["known"].astype(bool)
    assert np.array_equal(known, got["strength"] >= min_confidence)      # F46: only the confidence is zeroed
    assert not got["confidence"][~known].any() and _same(got["confidence"][known], got["strength"][known])
    if min_confidence == 0.9:
        assert known.any() and (~known).any()


def test_frames_degenerate_rows_among_tonal_ones(ctx):
    """Rows of zeros and constant rows tie all (or many) of their scores: the candidates come in creation
    order (F45), here and in the checker."""
    rows = np.array(_tonal(130))
    rows[[0, 5, 63, 64, 129]] = 0.0
    rows[[1, 6, 65, 128]] = 0.75
    rows[[2, 66]] = 1.0
    for p in (R.params(max_candidates=24), R.params(max_candidates=24, normalize_chroma=0)):
        ref = R.process_batch([list(r) for r in rows], p)
        got = ctx.key_frames(rows, _lib_params(p))
        _check_frames(got, ref, p)
        assert got["candidates"][0].tolist() == list(range(24)) and got["known"][0] == 0
    assert got["candidates"][1].tolist() == list(range(24)) and not got["scores"][1].any()   # not normalised: exact zeros


def test_frames_every_output_null_in_turn(ctx):
    ref = _frames_ref(12, LONG, _pkey(R.DEFAULT))[:65]
    for name in sonar.KEY_FRAME_FIELDS:
        _check_frames(ctx.key_frames(_tonal(LONG)[:65], skip=(name,)), ref, R.DEFAULT, skip=(name,))
    got = ctx.key_frames(_tonal(LONG)[:65], skip=sonar.KEY_FRAME_FIELDS[:-1])
    _check_frames(got, ref, R.DEFAULT, skip=sonar.KEY_FRAME_FIELDS[:-1])


def test_frames_empty_input_touches_nothing(ctx):
    got = ctx.key_frames(np.zeros((0, 12)), sonar.key_params(max_candidates=0, hpcp_size=-3))   # no row, no panic
    assert got["key"].shape == (0,)


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _dev_outputs(shapes):
    out = {}
    for n, (shape, dt) in shapes.items():
        out[n] = torch.full(shape, -1, dtype=dt, device="cuda")
    torch.cuda.synchronize()
    return out


def _frame_shapes(F, nc=5, hs=12):
    i, d = torch.int32, torch.float64
    return {"key": ((F,), i), "mode": ((F,), i), "known": ((F,), i), "confidence": ((F,), d), "strength": ((F,), d),
            "clarity": ((F,), d), "ambiguity": ((F,), d), "tonality": ((F,), d), "scores": ((F, 24), d),
            "candidates": ((F, nc), i), "processed": ((F, hs), d)}


def _equal_bits(host, devt):
    dev = devt.cpu().numpy()
    host = np.asarray(host)
    if host.dtype == np.float64:
        return _same(host.reshape(dev.shape), dev)
    return np.array_equal(host.reshape(dev.shape), dev)


def test_frames_device_pointers_equal_host_pointers(ctx):
    F = 257
    host = ctx.key_frames(_tonal(F))
    d = _dev(_tonal(F))
    out = _dev_outputs(_frame_shapes(F))
    ctx.key_frames_device(d.data_ptr(), F, 12, **{n: t.data_ptr() for n, t in out.items()})
    for n, t in out.items():
        assert _equal_bits(host[n], t), n


# ---- sonar_key_sequence ------------------------------------------------------------------------------

SHORT_LENGTHS = [1, 2, 3, 10, 11, 19, 20, 21, 22, 23, 65]
SEQ_LENGTHS = SHORT_LENGTHS + [SUM_TILE - 1, SUM_TILE, SUM_TILE + 1, 2 * SUM_TILE + 1]


def _check_sequence(got, ref, p, skip=()):
    for n in ("key", "mode", "known"):
        if n not in skip:
            assert int(got[n]) == ref[n], n
    for n in EXACT + ("stability",):
        if n not in skip:
            assert _same(got[n], ref[n]), (n, got[n], ref[n])
    if "ambiguity" not in skip:
        assert abs(got["ambiguity"] - ref["ambiguity"]) <= 1e-12
    if "scores" not in skip:
        assert _same(got["scores"], ref["scores"])
    if "processed" not in skip:
        assert _same(got["processed"], ref["processed"])         # normalised: every bit of the average is in it
    if "modulations" not in skip and "n_modulations" not in skip:
        assert int(got["n_modulations"]) == len(ref["modulations"])
        assert got["modulations"].tolist() == ref["modulations"]


@functools.lru_cache(maxsize=None)
def _sequence_ref(F, pk):
    p = dict(pk)
    return R.estimate_key_sequence(_tonal(LONG)[:F], p, frames=_frames_ref(12, LONG, pk)[:F])


@pytest.mark.parametrize("F", SEQ_LENGTHS)
def test_sequence_every_length(ctx, F):
    ref = _sequence_ref(F, _pkey(R.DEFAULT))
    got = ctx.key_sequence(_tonal(LONG)[:F])
    _check_sequence(got, ref, R.DEFAULT)
    if F < 3:
        assert got["stability"] == 0.0
    if F < 22:
        assert int(got["n_modulations"]) == 0                # F47
    if F >= SUM_TILE - 1:
        assert int(got["n_modulations"]) >= 3


def test_sequence_average_is_bit_exact_unnormalised(ctx):
    """With every preprocessing step off the processed row is the average itself."""
    p = R.params(normalize_chroma=0)
    for F in (SUM_TILE - 1, 2 * SUM_TILE + 1):
        got = ctx.key_sequence(_tonal(LONG)[:F], _lib_params(p))
        assert _same(got["processed"], R.average_chroma([list(r) for r in _tonal(LONG)[:F]]))
        _check_sequence(got, _sequence_ref(F, _pkey(p)), p)


def test_sequence_22_frames_report_exactly_position_11(ctx):
    maj = R.PROFILES[0][0]
    c_major = [1.5 * x for x in maj]
    g_major = [maj[(i + 7) % 12] for i in range(12)]            # key 7's template (F42)
    rows = np.array([c_major] * 10 + [g_major] * 12)
    ref = R.estimate_key_sequence(rows)
    assert ref["modulations"] == [11]
    _check_sequence(ctx.key_sequence(rows), ref, R.DEFAULT)
    _check_sequence(ctx.key_sequence(rows[:21]), R.estimate_key_sequence(rows[:21]), R.DEFAULT)
    # F46: all frames Unknown: they still vote in the stability, and nothing can pass the 0.7 test
    p = R.params(min_confidence=1.5)
    got = ctx.key_sequence(rows, _lib_params(p))
    _check_sequence(got, R.estimate_key_sequence(rows, p), p)
    assert got["stability"] == 12.0 / 22.0 and int(got["n_modulations"]) == 0 and int(got["known"]) == 0


@pytest.mark.parametrize("dim,hs", [(36, 12), (11, 12), (24, 24), (120, 12), (0, 12)])
def test_sequence_every_row_length(ctx, dim, hs):
    p = R.params(hpcp_size=hs)
    for F in (45, 3840 // dim + 1 if dim else 50):            # past one tile of the column sums at this dim
        rows = _wide(360, dim)[:F]
        ref = R.estimate_key_sequence([list(r) for r in rows], p)
        _check_sequence(ctx.key_sequence(rows, _lib_params(p)), ref, p)


def test_sequence_empty_is_the_zero_result(ctx):
    got = ctx.key_sequence(np.zeros((0, 12)))
    assert all(not np.any(got[n]) for n in got) and got["modulations"].shape == (0,)


def test_sequence_every_output_null_in_turn(ctx):
    F = 65
    ref = _sequence_ref(F, _pkey(R.DEFAULT))
    for name in ctx._KEY_SEQ_FIELDS:
        got = ctx.key_sequence(_tonal(LONG)[:F], skip=(name,))
        assert got[name] is None
        _check_sequence(got, ref, R.DEFAULT, skip=(name,))
    got = ctx.key_sequence(_tonal(LONG)[:F], skip=("modulations",))
    assert int(got["n_modulations"]) == len(ref["modulations"])


def _seq_shapes(F, hs=12):
    i, d = torch.int32, torch.float64
    s = {n: ((1,), i if n in ("key", "mode", "known") else d) for n in SCALARS}
    s.update({"scores": ((24,), d), "processed": ((hs,), d), "stability": ((1,), d),
              "modulations": ((max(F - 20, 0),), i), "n_modulations": ((1,), torch.int64)})
    return s


def test_sequence_device_pointers_equal_host_pointers(ctx):
    F = 2 * SUM_TILE + 1
    host = ctx.key_sequence(_tonal(LONG)[:F])
    d = _dev(_tonal(LONG)[:F])
    out = _dev_outputs(_seq_shapes(F))
    ctx.key_sequence_device(d.data_ptr(), F, 12, **{n: t.data_ptr() for n, t in out.items()})
    nm = int(out["n_modulations"].cpu()[0])
    assert nm == int(host["n_modulations"]) and out["modulations"].cpu().numpy()[:nm].tolist() == host["modulations"].tolist()
    for n, t in out.items():
        if n != "modulations":
            assert _equal_bits(host[n], t), n


def test_device_hpcp_feeds_key_sequence(ctx):
    """sonar_hpcp's device profile goes into sonar_key_sequence as it is: the same result as the two calls
    through host memory."""
    sr, W, H = 44100, 2048, 512
    n = W + 39 * H                                            # 40 frames
    t = np.arange(n) / sr
    pcm = sum(np.sin(2 * np.pi * f * t) for f in (261.63, 329.63, 392.0))
    pcm[n // 2:] = sum(np.sin(2 * np.pi * f * t[n // 2:]) for f in (293.66, 369.99, 440.0))
    pcm += 0.01 * np.random.default_rng(7).standard_normal(n)
    F = sonar.hpcp_plan(n, W, H)["frames"]
    assert F == 40
    host = ctx.key_sequence(ctx.hpcp(pcm, sr, W, H)["hpcp"])
    d = _dev(pcm)
    prof = torch.zeros(F, 12, dtype=torch.float64, device="cuda")
    out = _dev_outputs(_seq_shapes(F))
    ctx.hpcp_device(d.data_ptr(), n, sr, prof.data_ptr(), W, H)
    ctx.key_sequence_device(prof.data_ptr(), F, 12, **{k: v.data_ptr() for k, v in out.items()})
    nm = int(out["n_modulations"].cpu()[0])
    assert nm == int(host["n_modulations"]) and out["modulations"].cpu().numpy()[:nm].tolist() == host["modulations"].tolist()
    for k, v in out.items():
        if k != "modulations":
            assert _equal_bits(host[k], v), k
    assert host["stability"] > 0.0 and np.any(host["scores"])


# ---- sonar_key_batch ---------------------------------------------------------------------------------

def _check_batch(got, frames, p, skip=()):
    _check_frames(got, frames, p, skip=tuple(n for n in skip if n in sonar.KEY_FRAME_FIELDS))
    g = R.global_key(frames)
    prog = R.key_progression(frames)
    if "global_code" not in skip:
        assert int(got["global_code"]) == g["code"]
    if "global_confidence" not in skip:
        assert _same(got["global_confidence"], g["confidence"]) or (math.isnan(g["confidence"]) and
                                                                    math.isnan(got["global_confidence"]))
    if "global_strength" not in skip:
        assert _same(got["global_strength"], g["strength"])
    if "votes" not in skip:
        assert _same(got["votes"], g["votes"])
    if "n_transitions" not in skip:
        assert int(got["n_transitions"]) == len(prog)
        for n, col in (("t_frame", 0), ("t_from", 1), ("t_to", 2), ("t_type", 4)):
            if n not in skip:
                assert got[n].tolist() == [r[col] for r in prog], n
        if "t_confidence" not in skip:
            assert _same(got["t_confidence"], [r[3] for r in prog])


@pytest.mark.parametrize("F", SHORT_LENGTHS + [VOTE_TILE - 1, VOTE_TILE, VOTE_TILE + 1, LONG])
def test_batch_every_length(ctx, F):
    frames = _frames_ref(12, LONG, _pkey(R.DEFAULT))[:F]
    got = ctx.key_batch(_tonal(LONG)[:F])
    _check_batch(got, frames, R.DEFAULT)
    if F >= 65:
        assert 0 < int(got["n_transitions"]) < F - 1 and len(set(got["t_type"].tolist())) >= 3


def test_batch_empty(ctx):
    got = ctx.key_batch(np.zeros((0, 12)))
    assert got["global_code"] == -1 and got["global_confidence"] == 0.0 and got["global_strength"] == 0.0
    assert int(got["n_transitions"]) == 0 and not got["votes"].any()


def test_batch_without_a_confident_frame(ctx):
    rows = np.zeros((70, 12))
    rows[1::2] = 0.75
    frames = R.process_batch([list(r) for r in rows])
    got = ctx.key_batch(rows)
    _check_batch(got, frames, R.DEFAULT)
    assert got["global_code"] == -1 and math.isnan(got["global_confidence"]) and got["global_strength"] == 0.0
    assert int(got["n_transitions"]) == 0


@pytest.mark.parametrize("min_confidence", [0.0, 0.9])
def test_batch_thresholds_meet_min_confidence(ctx, min_confidence):
    """The votes and the progression read the thresholded confidence against their own 0.5."""
    p = R.params(min_confidence=min_confidence, profile=2)
    frames = _frames_ref(12, 257, _pkey(p))
    _check_batch(ctx.key_batch(_tonal(257), _lib_params(p)), frames, p)


def test_batch_every_output_null_in_turn(ctx):
    F = 65
    frames = _frames_ref(12, LONG, _pkey(R.DEFAULT))[:F]
    for name in ctx._KEY_BATCH_FIELDS:
        got = ctx.key_batch(_tonal(LONG)[:F], skip=(name,))
        assert got[name] is None
        _check_batch(got, frames, R.DEFAULT, skip=(name,))
    only_global = tuple(n for n in ctx._KEY_BATCH_FIELDS if n != "global_code")
    assert int(ctx.key_batch(_tonal(LONG)[:F], skip=only_global)["global_code"]) == R.global_key(frames)["code"]


def test_batch_device_pointers_equal_host_pointers(ctx):
    F = LONG
    host = ctx.key_batch(_tonal(LONG)[:F])
    i, dd = torch.int32, torch.float64
    shapes = _frame_shapes(F)
    shapes.update({"global_code": ((1,), i), "global_confidence": ((1,), dd), "global_strength": ((1,), dd),
                   "votes": ((24,), dd), "t_frame": ((F - 1,), i), "t_from": ((F - 1,), i), "t_to": ((F - 1,), i),
                   "t_confidence": ((F - 1,), dd), "t_type": ((F - 1,), i), "n_transitions": ((1,), torch.int64)})
    d = _dev(_tonal(LONG)[:F])
    out = _dev_outputs(shapes)
    ctx.key_batch_device(d.data_ptr(), F, 12, **{n: t.data_ptr() for n, t in out.items()})
    nt = int(out["n_transitions"].cpu()[0])
    assert nt == int(host["n_transitions"]) > 0
    for n, t in out.items():
        if n.startswith("t_"):
            assert _equal_bits(host[n], t[:nt]), n
        else:
            assert _equal_bits(host[n], t), n


# ---- Go's panics and what the library does not reproduce ---------------------------------------------

@pytest.mark.parametrize("entry", ["key_frames", "key_sequence", "key_batch"])
def test_panics_and_unsupported(ctx, entry):
    call = getattr(ctx, entry)
    rows = _tonal(LONG)[:65]

    def fails(code, text, chroma=rows, **kw):
        with pytest.raises(SonarError) as e:
            call(chroma, sonar.key_params(**kw))
        assert e.value.code == code and text in e.value.msg, e.value.msg

    fails(sonar.ERR_PANIC, "runtime error: index out of range [0] with length 0", max_candidates=0)
    fails(sonar.ERR_PANIC, "runtime error: slice bounds out of range [:-1]", max_candidates=-1)
    fails(sonar.ERR_PANIC, "runtime error: slice bounds out of range [:-7]", max_candidates=-7)
    fails(sonar.ERR_PANIC, "runtime error: makeslice: len out of range", hpcp_size=-1)
    fails(sonar.ERR_PANIC, "runtime error: index out of range [0] with length 0", hpcp_size=0)
    fails(sonar.ERR_UNSUPPORTED, "above 120", hpcp_size=121)
    fails(sonar.ERR_UNSUPPORTED, "above 120", chroma=np.ones((3, 121)))
    for bad in (np.nan, np.inf, -np.inf):
        x = np.array(rows)
        x[64, 11] = bad
        fails(sonar.ERR_UNSUPPORTED, "non-finite", chroma=x)
    call(np.zeros((5, 0)))                                    # dim == 0 with a positive hpcp_size is legal
    _check_frames(ctx.key_frames(rows), _frames_ref(12, LONG, _pkey(R.DEFAULT))[:65], R.DEFAULT)   # and the context lives on
