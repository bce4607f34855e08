"""The host layer of the fingerprint entries (csrc/fp_api.cpp): what a call returns must not depend on which
configurations the context has served before, on sonar_trim, or on whether the headline kernel's table
builder refused the bank; and a flagged output that is null is reported by its own text, in a fixed order.

Every comparison is bit for bit: the same kernels run on the same tables, so there is no tolerance to
choose.  The signals are four frames long (W + 3 H samples): enough for a frame pair with an odd frame
left over in the pair kernel, more than one frame per wave batch in the fused kernel, and flux rows."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library loads HIP (one HIP runtime in the process)

import sonar
from sonar._abi import (F32, F64, FP_COMPLEX, FP_ENERGY, FP_GENERIC, FP_MAGNITUDE, FP_MFCC, FP_PHASE, FP_SPECTRAL,
                        FP_ZCR, OK, PLAN_DFT, PLAN_PAIR, PLAN_WAVE, SPECTRAL_NAMES, _ptr, energy_frames, fp_kernel_plan)

pytestmark = pytest.mark.gpu

ALL6 = FP_MFCC | FP_MAGNITUDE | FP_COMPLEX | FP_PHASE | FP_ZCR | FP_ENERGY
# flag, field of sonar_fp_out, the text when it is null; in the order the entry reports them
OUTPUTS = [(FP_MFCC, "mfcc", "out->mfcc is null or allocation failed"),
           (FP_MAGNITUDE, "magnitude", "out->magnitude is null"),
           (FP_COMPLEX, "complex", "out->complex is null"),
           (FP_PHASE, "phase", "out->phase is null"),
           (FP_ZCR, "zcr", "out->zcr is null"),
           (FP_ENERGY, "energy", "out->energy is null")]


def _signal(W, H, dtype=np.float64, seed=5):
    return np.random.default_rng(seed).standard_normal(W + 3 * H).astype(dtype)


def _cfg(plan, flags, **kw):
    """A configuration that runs on the given plan: the pair kernel (float32 all through, W = 1024), the
    fused kernel (W = 512) or the DFT path (W = 1000)."""
    if plan == PLAN_PAIR:
        base = dict(window_size=1024, hop_size=256, precision=F32, pcm_dtype=F32, out_dtype=F32)
    elif plan == PLAN_WAVE:
        base = dict(window_size=512, hop_size=128)
    else:
        base = dict(window_size=1000, hop_size=250)
    base.update(n_filters=40, energy_window=256, energy_hop=128, flags=flags)
    base.update(kw)
    return sonar.Context.config(**base)


def _pcm(cfg, seed=5):
    return _signal(cfg.window_size, cfg.hop_size, np.float64 if cfg.pcm_dtype == F64 else np.float32, seed)


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def _call_with_nulls(ctx, cfg, nulls):
    x = _pcm(cfg)
    cfg.device_ptrs = 0
    assert fp_kernel_plan(cfg, len(x)) in (PLAN_PAIR, PLAN_WAVE, PLAN_DFT)
    assert not (cfg.flags & FP_ENERGY) or energy_frames(len(x), cfg.energy_window, cfg.energy_hop) > 0
    res, out = ctx._fp_outputs(len(x), cfg)
    for name in nulls:
        assert getattr(out, name)                                   # the flag is set and the buffer was there
        setattr(out, name, None)
    rc = ctx._L.sonar_fingerprint(ctx._h, _ptr(x), len(x), C.byref(cfg), C.byref(out))
    return rc, ctx._L.sonar_last_error(ctx._h).decode(), res


def _null_cases():
    cases = []
    for plan, pname, flags in ((PLAN_PAIR, "pair", FP_MFCC | FP_ZCR | FP_ENERGY), (PLAN_WAVE, "fused", ALL6),
                               (PLAN_DFT, "dft", ALL6)):
        for flag, name, text in OUTPUTS:
            if flags & flag:
                cases.append(pytest.param(plan, flags, name, text, id=f"{pname}-{name}"))
    return cases


@pytest.mark.parametrize("plan,flags,name,text", _null_cases())
def test_null_output_code_and_text(ctx, plan, flags, name, text):
    cfg = _cfg(plan, flags)
    assert fp_kernel_plan(cfg, len(_pcm(cfg))) == plan
    rc, msg, _ = _call_with_nulls(ctx, cfg, [name])
    assert (rc, msg) == (sonar.ERR_INVALID, text)


@pytest.mark.parametrize("plan", [PLAN_WAVE, PLAN_DFT], ids=["fused", "dft"])
def test_two_null_outputs_report_the_earlier(ctx, plan):
    names = [o[1] for o in OUTPUTS]
    for i in range(len(names)):
        for j in range(i + 1, len(names)):
            rc, msg, _ = _call_with_nulls(ctx, _cfg(plan, ALL6), [names[j], names[i]])
            assert (rc, msg) == (sonar.ERR_INVALID, OUTPUTS[i][2]), (names[i], names[j])


@pytest.mark.parametrize("plan", [PLAN_WAVE, PLAN_DFT], ids=["fused", "dft"])
def test_spectral_with_every_descriptor_null_succeeds(ctx, plan):
    rc, msg, _ = _call_with_nulls(ctx, _cfg(plan, FP_SPECTRAL), SPECTRAL_NAMES)
    assert rc == OK, msg


def _hps(c):
    return c.hps(_signal(512, 128), 44100, window_size=512, hop_size=128, skip=())


def test_one_context_many_configurations():
    """Tables of earlier configurations (the DFT path's without and with MFCC, both precisions of one fused
    window size, the raw-window table of sonar_hps) do not leak into later calls."""
    def fp(plan, flags, **kw):
        cfg = _cfg(plan, flags, **kw)
        return lambda c: c.fingerprint(_pcm(cfg), cfg)
    steps = [fp(PLAN_DFT, FP_MAGNITUDE), fp(PLAN_DFT, FP_MFCC), fp(PLAN_DFT, FP_MFCC | FP_SPECTRAL),
             fp(PLAN_WAVE, FP_MFCC | FP_MAGNITUDE, precision=F32), fp(PLAN_WAVE, FP_MFCC | FP_MAGNITUDE, precision=F64),
             _hps, fp(PLAN_WAVE, FP_MFCC | FP_MAGNITUDE, precision=F32)]
    one = sonar.Context(0)
    try:
        for i, step in enumerate(steps):
            got = step(one)
            fresh = sonar.Context(0)
            try:
                want = step(fresh)
            finally:
                fresh.close()
            assert all(v is not None and v.size for v in want.values()), i
            _same(got, want)
    finally:
        one.close()


PLAN_CALLS = [(PLAN_PAIR, FP_MFCC, "mfcc_pair_kernel"), (PLAN_WAVE, FP_MFCC | FP_MAGNITUDE, "fp_wave_kernel"),
              (PLAN_DFT, FP_MFCC | FP_MAGNITUDE, "stft_dft_kernel")]


def test_tables_survive_a_trim():
    c = sonar.Context(0)
    try:
        def run():
            out = []
            for plan, flags, kernel in PLAN_CALLS:
                cfg = _cfg(plan, flags)
                out.append((c.fingerprint(_pcm(cfg), cfg), c.last_fp_kernel()))
                assert out[-1][1] == kernel
            return out
        before = run()
        c.trim()
        after = run()
        for (a, ka), (b, kb) in zip(before, after):
            assert ka == kb
            _same(a, b)
    finally:
        c.close()


def test_refused_pair_bank_falls_to_the_fused_kernel():
    """n_mfcc = 20 is above the pair kernel's 16 coefficients: the plan still says PAIR (it does not build
    tables), the builder refuses, the refusal is remembered and both calls run the fused kernel."""
    kw = dict(n_mfcc=20, n_filters=40)
    cfg = _cfg(PLAN_PAIR, FP_MFCC, **kw)
    x = _pcm(cfg)
    assert fp_kernel_plan(cfg, len(x)) == PLAN_PAIR
    c = sonar.Context(0)
    try:
        a = c.fingerprint(x, cfg)
        assert c.last_fp_kernel() == "fp_wave_kernel"
        b = c.fingerprint(x, cfg)
        assert c.last_fp_kernel() == "fp_wave_kernel"
        g = c.fingerprint(x, _cfg(PLAN_PAIR, FP_MFCC | FP_GENERIC, **kw))
        assert c.last_fp_kernel() == "fp_wave_kernel"
    finally:
        c.close()
    assert a["mfcc"].shape == (4, 20) and np.all(np.isfinite(a["mfcc"])) and a["mfcc"].any()
    _same(a, b)
    _same(a, g)
