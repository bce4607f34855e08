"""Read forms of the float32 mfcc_pair_kernel (DESIGN.md Kernel 1a "Read forms"): the T2 loads as
sixteen single-address reads (hop-256 headline instances) and the filterbank weights two bins per
16-byte read at the row stride mfcc_pair_w_stride(J), with an odd J's last bin read singly.

Every bank below is compared with the general kernel (SONAR_FP_GENERIC, fp_wave_kernel) on the same
samples at the float32 MFCC rule of tests/parity.py (1e-4).  The chunk lengths J are the ones
tools/pair_lds_model.py's chunking gives (tests/test_pair_read_forms_cpu.py holds them):

  44.1 kHz x 40 -> J 12 (the compile-time instance)     44.1 kHz x 26 -> J 10 (even, runtime loop)
  44.1 kHz x 32 -> J 11 (odd tail)                      44.1 kHz x 48 -> J 15 (odd tail, stride 18)
  22.05 kHz x 48 -> J 14 (even, stride 14)

Each runs at hop 256 (J = 12: the compile-time hop) and hop 100 (the runtime-hop instance), with 1, 2,
3 and 67 frames."""
import numpy as np
import pytest

import sonar
from parity import assert_mfcc
from sonar import synth

pytestmark = pytest.mark.gpu

BANKS = [(44100, 40), (44100, 26), (44100, 32), (44100, 48), (22050, 48)]
FRAMES = (1, 2, 3, 67)


@pytest.fixture(scope="module")
def pcm():
    """2 s: seeded noise plus a sweep (float32)"""
    n = 2 * 44100
    rng = np.random.default_rng(20250)
    return (0.1 * rng.standard_normal(n) + synth.sweep(2.0)[:n]).astype(np.float32)


def _cfg(ctx, **kw):
    base = dict(window_size=1024, hop_size=256, sample_rate=44100, n_filters=40, n_mfcc=13,
                precision=sonar.F32, pcm_dtype=sonar.F32, out_dtype=sonar.F32)
    base.update(kw)
    return ctx.config(**base)


def _both(ctx, x, **kw):
    got = ctx.fingerprint(x, _cfg(ctx, **kw))["mfcc"]
    assert ctx.last_fp_kernel() == "mfcc_pair_kernel"
    ref = ctx.fingerprint(x, _cfg(ctx, flags=sonar.FP_MFCC | sonar.FP_GENERIC, **kw))["mfcc"]
    assert ctx.last_fp_kernel() == "fp_wave_kernel"
    return got.astype(np.float64), ref.astype(np.float64)


@pytest.mark.parametrize("H", [256, 100])
@pytest.mark.parametrize("sr,nf", BANKS)
def test_pair_kernel_matches_generic(ctx, pcm, sr, nf, H):
    for F in FRAMES:
        x = pcm[1000: 1000 + 1024 + (F - 1) * H]
        got, ref = _both(ctx, x, sample_rate=sr, n_filters=nf, hop_size=H)
        assert got.shape == ref.shape == (F, 13), (F, got.shape)
        assert_mfcc(got, ref, 1e-4)
    got, ref = _both(ctx, pcm, sample_rate=sr, n_filters=nf, hop_size=H)       # many pairs per wave
    assert_mfcc(got, ref, 1e-4)


def test_power_input(ctx, pcm):
    got, ref = _both(ctx, pcm, mfcc_input_power=1)
    assert_mfcc(got, ref, 1e-4)


def test_batch_equals_single_calls(ctx, pcm):
    """three short signals (3, 8 and 67 frames) at the headline bank: the batched instance's rows
    are the per-signal rows bit for bit"""
    cfg = _cfg(ctx)
    sigs = [pcm[5000: 5000 + 1024 + 2 * 256], pcm[20000: 20000 + 1024 + 7 * 256 + 100],
            pcm[40000: 40000 + 1024 + 66 * 256]]
    got = ctx.fingerprint_batch(sigs, cfg)
    assert ctx.last_fp_kernel() == "mfcc_pair_kernel"
    for i, (g, x) in enumerate(zip(got, sigs)):
        one = ctx.fingerprint(x, cfg)["mfcc"]
        assert ctx.last_fp_kernel() == "mfcc_pair_kernel"
        assert g["mfcc"].shape == one.shape == (sonar.stft_frames(len(x), 1024, 256), 13)
        assert np.array_equal(g["mfcc"], one), f"signal {i}"
