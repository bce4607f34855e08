"""The inputs of the chord detection tests, shared by test_chord_cpu.py (which shows the checker's literal
and reduced forms equal on every one of them) and test_gpu_chord.py (which holds the library to the
literal form on them).  A case is (rows, params, bass_note, bass_confidence); its reference is computed
once per form and shared.

Shapes.  chord_rows_kernel reports CHORD_ROWS = 63 rows per block (lane 0 of the 64 holds the row before
them) and chord_chain_kernel stages CHORD_TILE_FRAMES = 1024 records (csrc/kernels.h): the lengths run
over both sides of 63, of 64 and of 126, and one past the chain's tile.  A shorter length is a prefix of
the longest one, and so is its reference: a frame's result depends on no later frame."""
import functools

import numpy as np

import chord_ref as R

BLOCK, TILE = 63, 1024
LONG = TILE + 1
LENGTHS = (1, 2, BLOCK - 1, BLOCK, BLOCK + 1, 65, 2 * BLOCK, 2 * BLOCK + 1, 129, LONG)
PF = 70          # rows of a parameter case: past one block
# F52: a steady unnormalised row; 67 candidates at the default threshold
STEADY = [.30, .02, .02, .05, .27, .02, .02, .25, .02, .12, .02, .02]


@functools.lru_cache(maxsize=None)
def rows_a(F=LONG, dim=12, seed=1):
    """(a) the tie regime under the default parameters: unit-energy rows score up to sqrt(3), so most
    first confidences clip to 1.0."""
    rows = np.random.default_rng(seed + dim).random((F, dim)) ** 3
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def rows_b(F=LONG, seed=2):
    """(b) for normalize_templates = 0: first confidences mostly below 1, few ties, more than 5 candidates."""
    rows = 0.35 * np.random.default_rng(seed).random((F, 12)) ** 2
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def bass(F=LONG, seed=3):
    """Bass notes over every pitch class (so they hit roots, chord tones and no chord tone among the 120
    slots) with confidences on both sides of 0.3."""
    rng = np.random.default_rng(seed)
    note = rng.integers(0, 12, F).astype(np.int32)
    conf = rng.choice([0.0, 0.1, 0.3, 0.30000000000000004, 0.31, 0.6, 0.95], F)
    note.setflags(write=False)
    conf.setflags(write=False)
    return note, conf


@functools.lru_cache(maxsize=None)
def rows_gaps(F=PF + 30):
    """Input (b) with runs of zero rows at the start, around the block seam, in the middle and at the end (F55)."""
    rows = rows_b()[:F].copy()
    for lo, hi in ((0, 3), (20, 21), (40, 45), (BLOCK - 1, BLOCK + 1), (F - 3, F)):
        rows[lo:hi] = 0.0
    rows.setflags(write=False)
    return rows


PB = dict(normalize_templates=0)      # the base of input (b)

OVERRIDES = [
    dict(), dict(use_inversions=0), dict(use_bass_detection=0), dict(detect_extensions=0), dict(max_extension=7),
    dict(max_extension=9), dict(max_extension=11), dict(use_temporal_smoothing=0), dict(use_functional_analysis=1),
    dict(method=1), dict(method=2), dict(method=3), dict(method=4), dict(method=5), dict(method=99), dict(method=-1),
    dict(max_candidates=0), dict(max_candidates=1), dict(max_candidates=120), dict(max_candidates=121),
    dict(min_chord_strength=-1.0), dict(min_chord_strength=0.0), dict(min_chord_strength=5.0),
    dict(temporal_window=-1), dict(temporal_window=0), dict(temporal_window=1), dict(temporal_window=64),
    dict(bass_weight=-0.5), dict(bass_weight=2.0), dict(use_temporal_smoothing=0, temporal_window=3),
    dict(use_temporal_smoothing=0, max_candidates=0),
]


def _oid(o):
    return "-".join("%s=%s" % kv for kv in sorted(o.items())) or "default"


def _build():
    cases = {}
    # every length, the two inputs, with and without the bass arrays
    for F in LENGTHS:
        cases["a-F%d" % F] = ("a", F, {}, False)
        cases["b-F%d" % F] = ("b", F, PB, False)
        cases["b-bass-F%d" % F] = ("b", F, PB, True)
    # every parameter switch, on both inputs, with the bass arrays
    for o in OVERRIDES:
        cases["a-" + _oid(o)] = ("a", PF, o, True)
        cases["b-" + _oid(o)] = ("b", PF, dict(PB, **o), True)
    # the longer rows (F54)
    for dim in (24, 36):
        for o in (dict(), dict(min_chord_strength=0.0), dict(min_chord_strength=-1.0), dict(bass_weight=-0.5,
                                                                                              min_chord_strength=-1.0)):
            cases["dim%d-%s" % (dim, _oid(o))] = ("a%d" % dim, PF, o, True)
    # zero rows among tonal ones (F55, F59)
    for o in (dict(), dict(max_candidates=0), dict(temporal_window=0), dict(temporal_window=1),
              dict(temporal_window=-1), dict(use_temporal_smoothing=0), dict(min_chord_strength=0.0)):
        cases["gaps-" + _oid(o)] = ("gaps", len(rows_gaps()), dict(PB, **o), False)
    # the steady row (F52): 67 candidates
    for w in (-1, 0, 1, 5, 50, 64):
        cases["steady-w%d" % w] = ("steady", 6, dict(PB, temporal_window=w), False)
    return cases


_CASES = _build()
CASE_IDS = sorted(_CASES)
SOURCES = {"a": lambda: rows_a(), "b": lambda: rows_b(), "a24": lambda: rows_a(PF, 24), "a36": lambda: rows_a(PF, 36),
           "gaps": rows_gaps, "steady": lambda: np.array([STEADY] * 6)}


def case(cid):
    """-> rows (F x dim), params, bass_note, bass_confidence (None without bass arrays)."""
    src, F, o, with_bass = _CASES[cid]
    rows = SOURCES[src]()[:F]
    bn, bc = bass()
    return rows, R.params(**o), (bn[:F] if with_bass else None), (bc[:F] if with_bass else None)


def _pkey(p):
    return tuple(sorted(p.items()))


@functools.lru_cache(maxsize=None)
def _span_ref(form, src, span, with_bass, pk):
    """The reference of the first span rows of a source; a case's is a prefix of it.  -> (results, panic):
    the literal form returns the frames before a Go panic and (frame, exception)."""
    rows = SOURCES[src]()[:span]
    bn, bc = bass() if with_bass else (None, None)
    p = dict(pk)
    if form == "frames":
        return R.frames(rows, p, bn, bc), None
    if form == "reduced":
        try:
            return R.sequence_reduced(rows, p, bn, bc), None
        except IndexError as e:
            return None, (None, e)
    det, out = R.Detector(p), []
    for f in range(len(rows)):
        try:
            out.append(det.detect(rows[f], *R._bass(bn, bc, f)))
        except IndexError as e:
            return out, (f, e)
    return out, None


def reference(cid, form):
    """form: "frames" (a fresh detector per row), "sequence" (the literal detector) or "reduced" (the
    chain the kernels run) -> (results, error): error is None, or the Go panic the call ends in and
    results is None."""
    src, F, o, with_bass = _CASES[cid]
    span = LONG if src in ("a", "b") and F in LENGTHS and cid.endswith("-F%d" % F) else F
    res, panic = _span_ref(form, src, span, with_bass, _pkey(R.params(**o)))
    if panic is not None and span != F and (panic[0] is None or panic[0] >= F):
        res, panic = _span_ref(form, src, F, with_bass, _pkey(R.params(**o)))
    if panic is not None:
        return None, panic[1]
    return res[:F], None
