"""The host layer the newer entries share (csrc/staging.h, cached_table in csrc/ctx.h): what a call returns
must not depend on where the caller's arrays live, on which optional outputs it asks for, or on whether a
cached table was built in this call or an earlier one.

Every comparison here is bit for bit: both modes launch the same kernels on the same values, so there is
no tolerance to choose.  The shapes are the smallest that reach every output of an entry (23 frames is the
first sequence with more than one modulation window, 1001 samples the first FFT length of the default
constructor).  The error texts are those of the entries' argument checks, in each entry's check order."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library loads HIP (one HIP runtime in the process)

import key_ref as KR
import sonar
from sonar import SonarError
from sonar._abi import CHROMA_DIST_METRICS, CHROMA_SIM_METHODS, CORR_METHODS, CORR_TYPES, KEY_FRAME_FIELDS, _ptr

pytestmark = pytest.mark.gpu

I32, I64, F64 = np.int32, np.int64, np.float64
DEV = object()          # stands for the device_ptrs argument
FILL = -3               # what every output holds before the call, in both modes


class In:
    def __init__(self, a):
        self.a = None if a is None else np.ascontiguousarray(a)


class Out:
    """An array output (host or device memory); upto names the count output that bounds its valid prefix."""
    def __init__(self, name, shape, dtype=F64, upto=None):
        self.name, self.shape, self.dtype, self.upto = name, shape, dtype, upto


class Ref:
    """A single value the entry writes through a host pointer in both modes."""
    def __init__(self, name, ctype):
        self.name, self.ctype = name, ctype


class Params:
    """A sonar_key_params ("key") or sonar_hpcp_params ("hpcp") with fields overridden, built at the call."""
    def __init__(self, kind, **kw):
        self.kind, self.kw = kind, kw

    def make(self):
        return (sonar.key_params if self.kind == "key" else sonar.hpcp_params)(**self.kw)


def _call(ctx, entry, spec, dev, skip=()):
    """Calls the C entry with the inputs and outputs of spec in host (dev = False) or device memory; the
    outputs named in skip are passed as null.  Returns name -> array (None for a skipped one)."""
    keep, args, outs = [], [ctx._h], {}
    for a in spec:
        if a is DEV:
            args.append(int(dev))
        elif isinstance(a, In):
            if a.a is None:
                args.append(None)
            elif dev:
                keep.append(torch.from_numpy(a.a.copy()).cuda())
                args.append(keep[-1].data_ptr())
            else:
                args.append(_ptr(a.a))
        elif isinstance(a, Out):
            if a.name in skip:
                outs[a.name] = None
                args.append(None)
            elif dev:
                t = torch.from_numpy(np.full(a.shape, FILL, a.dtype)).cuda()
                outs[a.name] = t
                args.append(t.data_ptr())
            else:
                outs[a.name] = np.full(a.shape, FILL, a.dtype)
                args.append(_ptr(outs[a.name]))
        elif isinstance(a, Params):
            keep.append(a.make())
            args.append(C.byref(keep[-1]))
        elif isinstance(a, Ref):
            if a.name in skip:
                outs[a.name] = None
                args.append(None)
            else:
                outs[a.name] = a.ctype(FILL)
                args.append(C.byref(outs[a.name]))
        else:
            args.append(a)
    if dev:
        torch.cuda.synchronize()
    ctx._check(getattr(ctx._L, entry)(*args))
    res = {}
    for n, v in outs.items():
        res[n] = None if v is None else v.cpu().numpy() if isinstance(v, torch.Tensor) else \
            v if isinstance(v, np.ndarray) else np.array([v.value])
    return res


def _bits(a):
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _agree(spec, host, dev, counts):
    """Every output of the two calls holds the same bits; an array bounded by a count only up to it."""
    assert host.keys() == dev.keys()
    for a in spec:
        if not isinstance(a, (Out, Ref)):
            continue
        h, d = host[a.name], dev[a.name]
        assert (h is None) == (d is None), a.name
        if h is None:
            continue
        n = int(counts[a.upto][0]) if getattr(a, "upto", None) else None
        assert h.shape == d.shape and np.array_equal(_bits(h.reshape(-1)[:n]), _bits(d.reshape(-1)[:n])), a.name


def _both_modes_every_null(ctx, entry, spec, optional, written=()):
    """The entry with every output, then with each optional output null in turn: host and device pointers
    agree each time, and a call without an output leaves the others as they were.  Returns the full result."""
    full = _call(ctx, entry, spec, False)
    for n in written:
        assert np.any(full[n] != FILL), n                          # the call reached this output
    _agree(spec, full, _call(ctx, entry, spec, True), full)
    for name in optional:
        host = _call(ctx, entry, spec, False, skip=(name,))
        assert host[name] is None
        _agree(spec, host, _call(ctx, entry, spec, True, skip=(name,)), full)
        _agree(spec, host, {k: (None if k == name else v) for k, v in full.items()}, full)
    return full


# ---- key estimation ---------------------------------------------------------------------------------

def _key_spec(entry, rows, params):
    F, dim = rows.shape
    hs = max(params.hpcp_size, 0)
    nc = min(max(params.max_candidates, 0), 24)
    per = 1 if entry == "sonar_key_sequence" else F
    i, d = I32, F64
    frame = {"key": ((per,), i), "mode": ((per,), i), "known": ((per,), i), "confidence": ((per,), d),
             "strength": ((per,), d), "clarity": ((per,), d), "ambiguity": ((per,), d), "tonality": ((per,), d),
             "scores": ((per, 24), d), "candidates": ((per, nc), i), "processed": ((per, hs), d)}
    spec = [In(rows if rows.size else None), F, dim, C.byref(params)]
    names = KEY_FRAME_FIELDS if entry != "sonar_key_sequence" else KEY_FRAME_FIELDS[:9] + ("processed",)
    spec += [Out(n, *frame[n]) for n in names]
    if entry == "sonar_key_sequence":
        spec += [Out("stability", (1,)), Out("modulations", (max(F - 20, 0),), i, upto="n_modulations"),
                 Out("n_modulations", (1,), I64)]
    if entry == "sonar_key_batch":
        cap = max(F - 1, 0)
        spec += [Out("global_code", (1,), i), Out("global_confidence", (1,)), Out("global_strength", (1,)),
                 Out("votes", (24,))]
        spec += [Out(n, (cap,), F64 if n == "t_confidence" else i, upto="n_transitions")
                 for n in ("t_frame", "t_from", "t_to", "t_confidence", "t_type")]
        spec += [Out("n_transitions", (1,), I64)]
    return spec + [DEV]


def _key_rows(codes):
    """One clean profile row per code (key * 2 + mode): every row is confidently its own key."""
    rows = []
    for c in codes:
        prof = KR.PROFILES[0][c & 1]
        rows.append([prof[(i + (c >> 1)) % 12] for i in range(12)])   # key k's template (F42)
    return np.array(rows)


def test_key_tables_survive_a_trim(ctx):
    """The profile table and, with dim != hpcp_size, the resize index table are rebuilt after sonar_trim."""
    rows12, rows24 = _key_rows([0, 14, 5]), np.repeat(_key_rows([0, 14, 5]), 2, axis=1)
    calls = [(rows12, sonar.key_params()), (rows24, sonar.key_params(hpcp_size=12))]
    before = [_call(ctx, "sonar_key_frames", _key_spec("sonar_key_frames", r, p), False) for r, p in calls]
    assert before[0]["key"].tolist() == [0, 7, 2] and before[1]["key"].tolist() == [0, 7, 2]
    ctx.trim()
    for (r, p), want in zip(calls, before):
        spec = _key_spec("sonar_key_frames", r, p)
        _agree(spec, _call(ctx, "sonar_key_frames", spec, False), want, want)
        _agree(spec, _call(ctx, "sonar_key_frames", spec, False), want, want)     # and served from the cache


def test_key_sequence_23_frames_both_modes_every_null(ctx):
    rows = _key_rows([0] * 10 + [14] * 13)
    rows[:10] *= 1.5                                            # the louder half keeps the first window in its key
    assert KR.estimate_key_sequence(rows)["modulations"] == [11]
    spec = _key_spec("sonar_key_sequence", rows, sonar.key_params())
    full = _both_modes_every_null(ctx, "sonar_key_sequence", spec, [a.name for a in spec if isinstance(a, Out)],
                                  written=("key", "scores", "processed", "stability", "modulations", "n_modulations"))
    assert int(full["n_modulations"][0]) == len(KR.estimate_key_sequence(rows)["modulations"])


def test_key_batch_3_frames_both_modes_every_null(ctx):
    rows = _key_rows([0, 14, 5])
    assert len(KR.key_progression(KR.process_batch([list(r) for r in rows]))) == 2
    spec = _key_spec("sonar_key_batch", rows, sonar.key_params())
    full = _both_modes_every_null(ctx, "sonar_key_batch", spec, [a.name for a in spec if isinstance(a, Out)],
                                  written=("key", "candidates", "votes", "global_code", "t_frame", "t_type"))
    assert int(full["n_transitions"][0]) == 2


@pytest.mark.parametrize("entry", ["sonar_key_sequence", "sonar_key_batch"])
def test_key_empty_input_zero_fill_both_modes(ctx, entry):
    spec = _key_spec(entry, np.zeros((0, 12)), sonar.key_params())
    host, dev = _call(ctx, entry, spec, False), _call(ctx, entry, spec, True)
    _agree(spec, host, dev, host)
    if entry == "sonar_key_sequence":                          # the zero result: every output it has is zeroed
        assert all(not v.any() for v in host.values())
    else:                                                      # no vote: code -1, the rest of the global result zero
        assert host["global_code"][0] == -1 and not host["votes"].any() and host["n_transitions"][0] == 0
        assert host["global_confidence"][0] == 0.0 and host["global_strength"][0] == 0.0
    opt = [a.name for a in spec if isinstance(a, Out)]
    _agree(spec, _call(ctx, entry, spec, False, skip=opt), _call(ctx, entry, spec, True, skip=opt), host)


# ---- spectral peaks and HPCP -------------------------------------------------------------------------

WS, SR, K = 32, 8000, 17


def _mag(F=2, k=K):
    rng = np.random.default_rng(17)
    return rng.random((F, k)) + 0.01


def _peaks_spec(mag, F, k):
    P = max(sonar.spectral_peaks_width(k, 60), 0)
    return [In(mag), F, k, WS, SR, 1e-5, 20.0, 60, Out("count", (F,), I32), Out("bin", (F, P), I32),
            Out("magnitude", (F, P)), Out("frequency", (F, P)), DEV]


def _hpcp_spec(mag, F, k, params):
    return [In(mag), F, k, WS, SR, C.byref(params), Out("hpcp", (F, max(params.size, 0))), Out("energy", (F,)),
            Out("entropy", (F,)), DEV]


def test_spectral_peaks_both_modes_every_null(ctx):
    full = _both_modes_every_null(ctx, "sonar_spectral_peaks", _peaks_spec(_mag(), 2, K), ["frequency"],
                                  written=("count", "bin", "magnitude", "frequency"))
    assert full["count"].min() >= 1


def test_hpcp_from_spectrum_both_modes_every_null(ctx):
    spec = _hpcp_spec(_mag(), 2, K, sonar.hpcp_params(min_freq=100.0, max_freq=3900.0))
    full = _both_modes_every_null(ctx, "sonar_hpcp_from_spectrum", spec, ["energy", "entropy"],
                                  written=("hpcp", "energy", "entropy"))
    assert full["hpcp"].any() and full["energy"].all()


def test_zero_fill_branches_both_modes(ctx):
    spec = _peaks_spec(None, 2, 0)                              # K == 0: no peaks, the counts are zeroed
    host, dev = _call(ctx, "sonar_spectral_peaks", spec, False), _call(ctx, "sonar_spectral_peaks", spec, True)
    _agree(spec, host, dev, host)
    assert not host["count"].any()
    for k, params in ((0, sonar.hpcp_params()), (K, sonar.hpcp_params(size=0))):   # K == 0 | size == 0
        spec = _hpcp_spec(_mag(2, k) if k else None, 2, k, params)
        for skip in ((), ("energy",), ("entropy",)):
            host = _call(ctx, "sonar_hpcp_from_spectrum", spec, False, skip)
            _agree(spec, host, _call(ctx, "sonar_hpcp_from_spectrum", spec, True, skip), host)
            assert all(v is None or not v.any() for v in host.values())
    # sonar_hpcp with size == 0: nothing is launched, energy and entropy are zeroed on the device and copied back
    n, params = 1024 + 256, sonar.hpcp_params(size=0)
    spec = [In(np.random.default_rng(3).standard_normal(n)), n, 44100, 1024, 256, sonar.WINDOWS["hann"], C.byref(params),
            Out("hpcp", (2, 0)), Out("energy", (2,)), Out("entropy", (2,)), DEV]
    for skip in ((), ("energy",), ("entropy",), ("hpcp",)):
        host = _call(ctx, "sonar_hpcp", spec, False, skip)
        _agree(spec, host, _call(ctx, "sonar_hpcp", spec, True, skip), host)
        assert all(v is None or not v.any() for v in host.values())


# ---- constant-Q chroma and cross-correlation -----------------------------------------------------------

CQT = (8000, 200.0, 1600.0, 12, 5.0, 440.0)                    # 36 bins


def test_chroma_cqt_one_frame_both_modes_every_null(ctx):
    n, hop = 300, 5000                                          # the hop exceeds the signal: one frame
    x = 0.5 + 0.1 * np.random.default_rng(n).standard_normal(n)
    spec = [In(x), n, hop, *CQT, Out("chroma", (1, 12)), Out("cqt", (1, 36)), DEV]
    full = _both_modes_every_null(ctx, "sonar_chroma_cqt", spec, ["cqt"], written=("chroma", "cqt"))
    assert abs(full["chroma"].sum() - 1.0) <= 1e-12


@pytest.mark.parametrize("n,corr_type,use_fft", [(8, "pearson", 0), (8, "zncc", 0), (1001, "pearson", 1)])
def test_xcorr_both_modes_every_null(ctx, n, corr_type, use_fft):
    rng = np.random.default_rng(n)
    a, b = rng.standard_normal(n), rng.standard_normal(n)
    spec = [In(a), n, In(b), n, 5, CORR_TYPES[corr_type], CORR_METHODS["time"], use_fft, Out("corr", (11,)),
            Ref("metrics", C.c_double * 12), DEV]
    host = _call_xcorr(ctx, spec, False)
    assert host["metrics"][10] == (CORR_METHODS["frequency"] if use_fft else CORR_METHODS["time"])
    for skip in ((), ("corr",), ("metrics",)):
        h, d = _call_xcorr(ctx, spec, False, skip), _call_xcorr(ctx, spec, True, skip)
        for name in ("corr", "metrics"):
            assert (h[name] is None) == (d[name] is None) == (name in skip)
            if name not in skip:
                assert np.array_equal(_bits(h[name]), _bits(d[name])) and np.array_equal(_bits(h[name]), _bits(host[name]))
    # the signal against itself takes the one-input path
    same = [In(a), n, In(a), n, 5, CORR_TYPES[corr_type], CORR_METHODS["time"], use_fft, Out("corr", (11,)),
            Ref("metrics", C.c_double * 12), DEV]
    auto = [In(a), n, 5, CORR_TYPES[corr_type], CORR_METHODS["frequency" if use_fft else "time"], Out("corr", (11,)),
            Ref("metrics", C.c_double * 12), DEV]
    want = _call_xcorr(ctx, auto, False, entry="sonar_autocorr")
    got = _call_xcorr(ctx, auto, True, entry="sonar_autocorr")
    assert np.array_equal(_bits(want["corr"]), _bits(got["corr"]))
    assert np.array_equal(_bits(want["corr"]), _bits(_call_xcorr(ctx, same, False)["corr"]))


def _call_xcorr(ctx, spec, dev, skip=(), entry="sonar_xcorr_params"):
    """The metrics are a host array in both modes."""
    m = np.full(12, float(FILL))
    args = [_ptr(m) if (isinstance(a, Ref) and a.name not in skip) else None if isinstance(a, Ref) else a for a in spec]
    res = _call(ctx, entry, args, dev, skip)
    res["metrics"] = None if "metrics" in skip else m
    return res


# ---- chroma sequence similarity -----------------------------------------------------------------------

def _chroma_seqs():
    rng = np.random.default_rng(34)
    return rng.random((3, 12)) + 0.05, rng.random((4, 12)) + 0.05


def _similarity(ctx, method, dev, skip=()):
    q, r = _chroma_seqs()
    cap = 3 + 4
    spec = [In(q), 3, In(r), 4, 12, CHROMA_SIM_METHODS[method], CHROMA_DIST_METRICS["cosine"], 0.4, 10, 50, 0,
            Out("matrix", (3, 4)), Ref("matrix_is_nil", C.c_int32), Ref("overall", C.c_double),
            Ref("best_transposition", C.c_int32), Out("path_q", (cap,), I32, upto="path_len"),
            Out("path_r", (cap,), I32, upto="path_len"), Out("path_score", (cap,), F64, upto="path_len"),
            Ref("path_len", C.c_int64)]
    return spec, _call(ctx, "sonar_chroma_similarity", spec, dev, skip)


def test_chroma_frame_matrix_3x4_both_modes(ctx):
    q, r = _chroma_seqs()
    for metric, shift, sim in (("cosine", 0, 0), ("euclidean", 5, 1)):
        spec = [In(q), 3, In(r), 4, 12, CHROMA_DIST_METRICS[metric], shift, sim, Out("out", (3, 4))]
        host, dev = _call(ctx, "sonar_chroma_frame_matrix", spec, False), _call(ctx, "sonar_chroma_frame_matrix", spec, True)
        _agree(spec, host, dev, host)
        assert np.all(host["out"] != FILL)


@pytest.mark.parametrize("method", ["smith_waterman", "dtw"])
def test_chroma_similarity_3x4_both_modes_every_null(ctx, method):
    spec, full = _similarity(ctx, method, False)
    P = int(full["path_len"][0])
    assert 1 <= P <= 7 and np.all(full["matrix"] != FILL) and full["matrix_is_nil"][0] == 0
    assert np.all(full["path_q"][:P] != FILL) and np.all(full["path_score"][:P] != FILL)
    _agree(spec, full, _similarity(ctx, method, True)[1], full)
    for name in [a.name for a in spec if isinstance(a, (Out, Ref))]:
        host, dev = _similarity(ctx, method, False, (name,))[1], _similarity(ctx, method, True, (name,))[1]
        assert host[name] is None
        _agree(spec, host, dev, full)
        _agree(spec, host, {k: (None if k == name else v) for k, v in full.items()}, full)


# ---- error texts ----------------------------------------------------------------------------------------

def _err_cases():
    """(id, entry, arguments after the context, code, text): one invalid argument per check, in the entry's
    check order; everything before the invalid argument is valid."""
    x8 = np.linspace(0.1, 0.8, 8)
    rows = _key_rows([0, 14, 5])
    mag = _mag()
    q, r = _chroma_seqs()
    P, U, I, E = sonar.ERR_PANIC, sonar.ERR_UNSUPPORTED, sonar.ERR_INVALID, sonar.ERR_EMPTY
    cases = []
    for entry, n_out in (("sonar_key_frames", 11), ("sonar_key_sequence", 13), ("sonar_key_batch", 21)):
        def key(idn, code, text, chroma=rows, F=3, dim=12, params=True, out=False, entry=entry, n_out=n_out, **kw):
            outs = [Out("key", (3,), I32) if out else None] + [None] * (n_out - 1)
            cases.append((f"{entry}-{idn}", entry, [In(chroma), F, dim, Params("key", **kw) if params else None] + outs + [0],
                          code, text))
        key("negF", I, "key estimation: negative frame count or row length, or null params", F=-1)
        key("negdim", I, "key estimation: negative frame count or row length, or null params", dim=-1)
        key("nullparams", I, "key estimation: negative frame count or row length, or null params", params=False)
        key("hs<0", P, "runtime error: makeslice: len out of range", hpcp_size=-1)
        key("cand<0", P, "runtime error: slice bounds out of range [:-2]", max_candidates=-2)
        key("cand0", P, "runtime error: index out of range [0] with length 0", max_candidates=0)
        key("hs0", P, "runtime error: index out of range [0] with length 0", hpcp_size=0)
        key("dim>max", U, "key estimation: dim or hpcp_size above 120 is not supported", chroma=np.ones((3, 121)), dim=121)
        key("hs>max", U, "key estimation: dim or hpcp_size above 120 is not supported", hpcp_size=121)
        key("F>int32", U, "key estimation: more than 2^31 - 1 frames are not supported", F=1 << 31)
        key("nullchroma", I, "key estimation: null chroma pointer", chroma=None)
        bad = rows.copy()
        bad[2, 11] = np.inf
        key("nonfinite", U, "key estimation: a non-finite chroma value is not reproduced (a NaN score leaves the order "
            "of sort.Slice undefined)", chroma=bad, out=True)

    def peaks(idn, code, text, m=mag, F=2, k=K, ws=WS, sr=SR, max_peaks=60, count=True, outs=True):
        o = [Out("count", (2,), I32) if count else None] + ([Out("bin", (2, 8), I32), Out("magnitude", (2, 8))] if outs
                                                            else [None, None])
        cases.append((f"peaks-{idn}", "sonar_spectral_peaks", [In(m), F, k, ws, sr, 1e-5, 20.0, max_peaks] + o + [None, 0],
                      code, text))
    peaks("negF", I, "spectral peaks: negative row count or row length", F=-1)
    peaks("negK", I, "spectral peaks: negative row count or row length", k=-1)
    peaks("nullcount", I, "spectral peaks: null count pointer", count=False)
    peaks("max_peaks<0", P, "runtime error: slice bounds out of range [:-4]", max_peaks=-4)
    peaks("sr0", U, "spectral peaks: sample_rate or window_size <= 0 is not reproduced", sr=0)
    peaks("ws0", U, "spectral peaks: sample_rate or window_size <= 0 is not reproduced", ws=0)
    peaks("K>max", U, "spectral peaks: rows of more than 8192 bins are not supported", k=8193)
    peaks("nullmag", I, "spectral peaks: null magnitude pointer", m=None)
    peaks("nullbin", I, "spectral peaks: null bin or magnitude pointer", outs=False)

    def hpcp(idn, code, text, m=mag, F=2, k=K, ws=WS, sr=SR, params=True, out=True, **kw):
        p = Params("hpcp", **kw) if params else None
        cases.append((f"hpcp-{idn}", "sonar_hpcp_from_spectrum",
                      [In(m), F, k, ws, sr, p, Out("hpcp", (2, 12)) if out else None, None, None, 0], code, text))
    hpcp("negF", I, "HPCP: negative row count or row length, or null params", F=-1)
    hpcp("negK", I, "HPCP: negative row count or row length, or null params", k=-1)
    hpcp("nullparams", I, "HPCP: negative row count or row length, or null params", params=False)
    hpcp("size<0", P, "runtime error: makeslice: len out of range", size=-1)
    hpcp("ref0", U, "HPCP: a non-finite or non-positive reference_freq is not reproduced", reference_freq=0.0)
    hpcp("win<0", U, "HPCP: a non-finite or negative window_size (semitones) is not reproduced", window_size=-1.0)
    hpcp("size>max", U, "HPCP: size above 120 is not supported", size=121)
    hpcp("harm>16", U, "HPCP: max_harmonics above 16 is not supported", max_harmonics=17)
    hpcp("win>12", U, "HPCP: a window_size above 12 semitones is not supported", window_size=12.5)
    hpcp("sr0", U, "spectral peaks: sample_rate or window_size <= 0 is not reproduced", sr=0)
    hpcp("K>max", U, "spectral peaks: rows of more than 8192 bins are not supported", k=8193)
    hpcp("K0-nullout", I, "HPCP: null hpcp pointer", m=None, k=0, out=False)
    hpcp("nullmag", I, "HPCP: null magnitude or hpcp pointer", m=None)
    hpcp("nullout", I, "HPCP: null magnitude or hpcp pointer", out=False)

    def full_hpcp(idn, code, text, pcm=np.linspace(-1, 1, 1280), n=1280, sr=44100, ws=1024, hop=256, params=True,
                  out=True, **kw):
        p = Params("hpcp", **kw) if params else None
        cases.append((f"hpcp_pcm-{idn}", "sonar_hpcp", [In(pcm), n, sr, ws, hop, sonar.WINDOWS["hann"], p,
                                                       Out("hpcp", (2, 12)) if out else None, None, None, 0], code, text))
    full_hpcp("nullparams", I, "HPCP: null params", params=False)
    full_hpcp("short", sonar.ERR_TOO_SHORT, "signal too short for given window size and hop size", n=512)
    full_hpcp("size<0", P, "runtime error: makeslice: len out of range", size=-1)
    full_hpcp("sr0", U, "spectral peaks: sample_rate or window_size <= 0 is not reproduced", sr=0)
    full_hpcp("nullout", I, "HPCP: null hpcp pointer", out=False)

    def cqt(idn, code, text, pcm=x8, n=8, hop=4, cfg=CQT, chroma=True, **kw):
        names = ("sample_rate", "min_freq", "max_freq", "bins_per_octave", "q_factor", "tuning_freq")
        c = dict(zip(names, cfg), **kw)
        cases.append((f"cqt-{idn}", "sonar_chroma_cqt", [In(pcm), n, hop] + [c[k] for k in names] +
                      [Out("chroma", (1, 12)) if chroma else None, None, 0], code, text))
    cqt("nullpcm", I, "chroma CQT: null pcm or chroma pointer", pcm=None)
    cqt("nullchroma", I, "chroma CQT: null pcm or chroma pointer", chroma=False)
    cqt("q0", U, "chroma CQT: a non-finite or non-positive min_freq, max_freq, q_factor or tuning_freq is not "
        "reproduced", q_factor=0.0)
    cqt("bpo0", U, "chroma CQT: bins_per_octave < 1 is not reproduced", bins_per_octave=0)
    cqt("sr5", U, "chroma CQT: sample_rate < 6 is not reproduced", sample_rate=5)
    cqt("bins>max", U, "chroma CQT: more than 65536 bins are not supported", bins_per_octave=1 << 20)
    cqt("K<0", P, "runtime error: makeslice: len out of range", max_freq=100.0)
    cqt("K0", P, "runtime error: index out of range [0] with length 0", max_freq=200.0)
    cqt("hop0", P, "runtime error: integer divide by zero", hop=0)
    bad = x8.copy()
    bad[3] = np.nan
    cqt("nonfinite", U, "chroma CQT: non-finite PCM is not reproduced (the reference spreads it through its FFT)", pcm=bad)

    def xc(idn, code, text, a=x8, na=8, b=x8[::-1], nb=8, method=CORR_METHODS["time"], use_fft=0):
        cases.append((f"xcorr-{idn}", "sonar_xcorr_params", [In(a), na, In(b), nb, 5, 0, method, use_fft, None, None, 0],
                      code, text))
    xc("na0", E, "empty signals provided", na=0)
    xc("nullb", E, "empty signals provided", b=None)
    xc("method", I, "unsupported correlation method", method=7)
    xc("fftlimit", U, "frequency-domain correlation: len(signal1) + len(signal2) - 1 = 8388607 exceeds the FFT limit of "
       "4194304 points", na=1 << 22, nb=1 << 22, use_fft=1)

    def fm(idn, code, text, qq=q, nq=3, rr=r, nr=4, dim=12, shift=0, out=True):
        cases.append((f"frame_matrix-{idn}", "sonar_chroma_frame_matrix",
                      [In(qq), nq, In(rr), nr, dim, 2, shift, 0, Out("out", (3, 4)) if out else None], code, text))

    def cs(idn, code, text, qq=q, nq=3, rr=r, nr=4, dim=12, method="direct"):
        cases.append((f"similarity-{idn}", "sonar_chroma_similarity",
                      [In(qq), nq, In(rr), nr, dim, CHROMA_SIM_METHODS[method], 2, 0.4, 10, 50, 0] + [None] * 8, code, text))
    for f in (fm, cs):
        f("negnq", I, "chroma similarity: negative frame count", nq=-1)
        f("dim0", I, "chroma similarity: dim must be >= 1", dim=0)
        f("nullq", I, "chroma similarity: null sequence pointer", qq=None)
        f("long", U, "chroma similarity: sequences too long", nq=1 << 31)
    fm("shift<0", P, "runtime error: index out of range [-5]", shift=-5)
    fm("nullout", I, "chroma frame matrix: null output pointer", out=False)
    cs("dtw-empty", P, "runtime error: index out of range [0] with length 0", nq=0, method="dtw")
    cs("cells", U, "chroma similarity: Smith-Waterman and DTW take at most 2^30 cells (nq * nr)", nq=1 << 20,
       nr=(1 << 10) + 1, method="smith_waterman")
    return cases


_ERR = _err_cases()


@pytest.mark.parametrize("entry,args,code,text", [c[1:] for c in _ERR], ids=[c[0] for c in _ERR])
def test_error_code_and_text(ctx, entry, args, code, text):
    with pytest.raises(SonarError) as e:
        _call(ctx, entry, args, False)
    assert e.value.code == code and e.value.msg == text, (e.value.code, e.value.msg)
