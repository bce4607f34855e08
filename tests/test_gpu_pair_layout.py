"""mfcc_pair_kernel's T2 layout on the device (DESIGN.md Kernel 1a "One T2 store sequence"): every
lane role of the transpose, float32 and float64, against the oracle at the kernel's existing
tolerances (parity.assert_mfcc: 1e-4 of the row norm for float32, 1e-9 for float64).

Shapes: one pair (n = 1280), an odd frame count (n = 1536: the last pair carries one frame) and
26 frames = 13 pairs, more than the 12 (float32) / 8 (float64) waves of a block, so one wave runs
the layout twice.

Inputs: a unit impulse (flat spectrum: every residue of the transpose carries the same magnitude,
a misplaced one changes the phase sum of a bin), tones exactly on bins 0, 8, 16, 64, 120, 448 and
512 -- the residues the lanes with k1 & 7 == 0 carry, whose store bases differ from the other
lanes' -- and seeded noise.  The tones ride on white noise 40 dB down: MFCCs take the logarithm
of every mel band, and behind a pure on-bin tone under a Hann window the other bands hold
nothing but rounding error (about 1e-14 of the peak power in float32, 1e-32 in the float64
oracle), whose logarithm no tolerance could compare.  With the floor, a float32 FFT's error
(~2e-6 absolute per bin for a unit tone: eps sqrt(log2 N) times the rms spectrum level of 11)
is 1e-5 of a floor bin's amplitude of 0.2, so every band is determined to a few 1e-5 of itself,
inside all of assert_mfcc's tiers, and a tone routed to a wrong bin still moves 40 dB of
energy between bands.  The impulse rides on the same floor: the kernel transforms two frames as
one complex FFT, so an exactly silent frame next to the impulse's (frame 3 of the 26) comes out
of the split as float32 cancellation noise, not as the zeros whose logarithm the oracle floors --
a property of the pair method at any layout, and not what this file is about."""
import numpy as np
import pytest

import oracle as O
import sonar
from parity import assert_mfcc

pytestmark = pytest.mark.gpu

SIZES = [1280, 1536, 1024 + 256 * 25]
TONES = [0, 8, 16, 64, 120, 448, 512]
KINDS = ["impulse", "noise"] + [f"tone{k}" for k in TONES]


def _signal(kind, n):
    t = np.arange(n)
    rng = np.random.default_rng(1234 + n)
    if kind == "impulse":
        x = 1e-2 * rng.standard_normal(n)
        x[700] += 1.0           # inside frames 0, 1 and 2, off the Hann window's zero at sample 0
        return x
    if kind == "noise":
        return rng.standard_normal(n) * 0.25
    k = int(kind[4:])
    return np.cos(2 * np.pi * k * t / 1024 + 0.3) + 1e-2 * rng.standard_normal(n)


_REF = {}


def _ref(kind, n, f64):
    """oracle MFCCs of the signal as the kernel sees it (float32 PCM widened exactly), computed once"""
    key = (kind, n, f64)
    if key not in _REF:
        x = _signal(kind, n)
        x = x if f64 else x.astype(np.float32)
        mag = O.stft_mag(x.astype(np.float64), 1024, 256, window_type="hann")
        ref = O.mfcc_frames(mag, 44100, n_coef=13, n_mels=40)
        ref.setflags(write=False)
        _REF[key] = (x, ref)
    return _REF[key]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_every_lane_role_matches_oracle(ctx, f64, n, kind):
    x, ref = _ref(kind, n, f64)
    dt = sonar.F64 if f64 else sonar.F32
    cfg = ctx.config(window_size=1024, hop_size=256, sample_rate=44100, n_filters=40, n_mfcc=13,
                     precision=dt, pcm_dtype=dt, out_dtype=dt)
    got = ctx.fingerprint(x, cfg)["mfcc"]
    assert ctx.last_fp_kernel() == "mfcc_pair_kernel"
    assert got.dtype == (np.float64 if f64 else np.float32)
    assert got.shape == ref.shape == ((n - 1024) // 256 + 1, 13)
    e = assert_mfcc(got.astype(np.float64), ref, 1e-9 if f64 else 1e-4)
    print(f"{kind} n={n} {'f64' if f64 else 'f32'}: row-norm error {e:.3e}")
