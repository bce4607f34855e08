"""Signal builders and case tables shared by test_feature_variants_cpu.py (the coverage conditions,
on the oracle alone) and test_gpu_feature_variants.py (the kernels of misc_kernels.hip against the
oracle).  Test infrastructure.

* YIN: ``yin_lag_signal`` holds one 1024-sample frame per period P = 2..511.  yin_kernel (and
  or_yin_raw) pre-emphasise every frame afresh (x_i - 0.97 x_{i-1}) and multiply by the Hann window
  w; the builder undoes both, so the difference function sees a P-periodic sequence apart from a
  64-sample ramp at the start (and the zeroed end points), and the chosen lag is P.  pitch_yin
  frames the signal at hop 512: frame 2k is the frame built for P = k + 2, the odd frames straddle
  two periods and are extra cases.  ``yin_sine_signal`` is the same with sinusoids: frames whose
  lag is decided by the local-minimum test, which the noise frames never exercise.
* chroma: ``CHROMA_CASES`` is one (frame size, sample rate, frames) per launch path of
  launch_chroma; ``chroma_signal`` gives n = fs F + r samples (r < F), so that n / F == fs.
"""
import functools

import numpy as np

import oracle as O

YIN_W = 1024
YIN_HOP = 512
YIN_PERIODS = tuple(range(2, 512))
YIN_RATES = (8000, 16000, 44100)


def yin_window():
    return 0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(YIN_W) / (YIN_W - 1)))


@functools.lru_cache(maxsize=None)
def yin_lag_signal():
    """The 510 designed frames, concatenated (522,240 samples, read-only)."""
    u = np.stack([np.tile(np.random.default_rng(P).standard_normal(P), YIN_W // P + 1)[:YIN_W] for P in YIN_PERIODS])
    x = _yin_undo(u).reshape(-1)
    x.setflags(write=False)
    return x


def _yin_undo(u):
    """Rows of what YIN should see -> rows of PCM: divide the window out (with the 64-sample ramp)
    and invert the per-frame pre-emphasis."""
    w = yin_window()
    g = np.minimum(1.0, w / w[64])
    y = np.zeros_like(u)
    y[:, 1:YIN_W - 1] = u[:, 1:YIN_W - 1] * g[1:YIN_W - 1] / w[1:YIN_W - 1]
    x = np.zeros_like(y)
    x[:, 0] = y[:, 0]
    for i in range(1, YIN_W):
        x[:, i] = y[:, i] + 0.97 * x[:, i - 1]
    return x


YIN_SINE_PERIODS = tuple(range(9, 511))


@functools.lru_cache(maxsize=None)
def yin_sine_signal():
    """One frame per P = 9..510 holding a sinusoid of period P - 0.3, built like yin_lag_signal.
    The noise frames' CMNDF dips below the threshold at the period alone, so there the local-minimum
    test never rejects a lag; a sinusoid's CMNDF descends smoothly through the threshold, so the
    lags before the minimum are rejected one by one (cm[tau] < cm[tau + 1] is false), among them
    lags with tau % 8 == 7, whose successor is read from the next lane."""
    i = np.arange(YIN_W)
    u = np.stack([np.sin(2 * np.pi * i / (P - 0.3) + 0.7 * P) for P in YIN_SINE_PERIODS])
    x = _yin_undo(u).reshape(-1)
    x.setflags(write=False)
    return x


def yin_cmndf_model(frame):
    """numpy restatement of the CMNDF of one frame (coverage conditions only: not bit-exact)."""
    w = yin_window()
    x = np.array(frame, float)
    x[1:] = frame[1:] - 0.97 * frame[:-1]
    x *= w
    s = np.lib.stride_tricks.sliding_window_view(x, YIN_W // 2)[:YIN_W // 2]      # s[tau, j] = x[tau + j]
    d = ((x[None, :YIN_W // 2] - s) ** 2).sum(axis=1)
    cm = np.ones(YIN_W // 2)
    with np.errstate(invalid="ignore", divide="ignore"):
        cm[1:] = d[1:] / (np.cumsum(d[1:]) / np.arange(1, YIN_W // 2))
    return cm


def yin_pick_model(cm, successor=lambda cm, tau: cm[tau + 1]):
    """The first tau in 1..510 below 0.15 that is smaller than its successor; `successor` lets a
    condition ask what a wrong neighbour read would choose."""
    for tau in np.flatnonzero(cm[1:511] < 0.15) + 1:
        if cm[tau] < successor(cm, tau):
            return int(tau)
    return -1


@functools.lru_cache(maxsize=None)
def yin_flat_signal():
    """Zero, constant and white-noise frames: 5 x 1024 samples, 9 frames at hop 512 (9 % 4 == 1);
    frames 0 / 2 / 4 / 6 / 8 are zero / one / noise / zero / noise."""
    rng = np.random.default_rng(7)
    x = np.concatenate([np.zeros(YIN_W), np.ones(YIN_W), rng.standard_normal(YIN_W), np.zeros(YIN_W),
                        0.01 * rng.standard_normal(YIN_W)])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def yin_oracle(which, sr):
    """(pitch, conf, tau) of O.yin_raw over every hop-512 frame of a builder's signal, computed once."""
    x = {"lag": yin_lag_signal, "sine": yin_sine_signal, "flat": yin_flat_signal}[which]()
    F = int(O.lib().or_pitch_frames(len(x)))
    p, c, t = np.zeros(F), np.zeros(F), np.zeros(F, np.int32)
    for i in range(F):
        p[i], c[i], t[i] = O.yin_raw(x[i * YIN_HOP: i * YIN_HOP + YIN_W], sr)
    for a in (p, c, t):
        a.setflags(write=False)
    return p, c, t


# (fs, sample rate, frames): the path launch_chroma selects is in the comment
CHROMA_CASES = (
    (3, 8000, 7),          # direct DFT, odd, tiny
    (4, 8000, 7),          # chroma_kernel FFT path, 2 stages
    (8, 8000, 7),          # ... 3 stages
    (64, 8000, 7),         # ... 6 stages
    (128, 8000, 7),        # ... 7 stages
    (1024, 44100, 7),      # ... the largest size that takes it
    (255, 44100, 7),       # direct DFT next to the wave size
    (257, 44100, 7),
    (256, 44100, 7),       # chroma_wave_kernel<4>, short signal, partial block
    (512, 44100, 7),       # chroma_wave_kernel<8>: odd stage count, the lone last stage
    (302, 44100, 7),       # K + 12 even: no pad double before the trig table
    (1166, 44100, 7),      # the last size with the trig table in LDS
    (1167, 44100, 7),      # the first with the trig table in global memory
    (2048, 44100, 7),      # powers of two whose FFT work arrays do not fit: direct DFT
    (4096, 44100, 7),
    (5453, 44100, 7),      # 64 KB of dynamic LDS exactly: no attribute
    (5454, 44100, 7),      # above 64 KB: the raised dynamic-LDS attribute
    (13645, 44100, 2),     # 160 KB: the largest frame launch_chroma accepts
)
CHROMA_REFUSED_FS = 13646
CHROMA_QUIET_FS = (256, 512, 300)


def chroma_len(fs, F):
    """n with n // F == fs and a remainder (F - 1 where that keeps a frame at or beyond n)."""
    return fs * F + min(F - 1, 2)


def chroma_hops(fs, F):
    """hop = fs (the frames tile the signal), fs + fs // 3 (the late frames straddle n; with F = 7
    the last starts at or beyond it), and for F = 2 also hop = n: frame 1 starts at n."""
    hops = [fs, fs + fs // 3]
    if (F - 1) * hops[1] < chroma_len(fs, F):
        hops.append(chroma_len(fs, F))
    return tuple(hops)


@functools.lru_cache(maxsize=None)
def chroma_signal(fs, sr, F):
    n = chroma_len(fs, F)
    rng = np.random.default_rng(fs)
    x = 0.1 * rng.standard_normal(n) + 0.5 * np.sin(2 * np.pi * 440.0 * np.arange(n) / sr)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def chroma_oracle(fs, sr, F, hop):
    ref = O.chroma_frames(chroma_signal(fs, sr, F), F, hop, fs, sr)
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def chroma_quiet_signal(fs):
    """The fs case's signal scaled so that every frame's class total is positive and at most 1e-10
    (normalizeChromaFrame then leaves the row as it is): the loudest frame's total becomes 2.5e-11."""
    x = chroma_signal(fs, 44100, 7)
    raw = _chroma_raw_totals(x, 7, fs, fs, 44100)
    y = x * np.sqrt(2.5e-11 / raw.max())
    y.setflags(write=False)
    return y


def _chroma_raw_totals(x, F, hop, fs, sr):
    """Per-frame class totals before normalisation, by scaling the signal until no frame normalises."""
    s = 1e-12
    rows = O.chroma_frames(x * s, F, hop, fs, sr)
    tot = rows.sum(axis=1)
    assert np.all(tot <= 1e-10), "scale too large to read the raw totals"
    return tot / (s * s)


MUSIC_SR = 44100
# (query, reference) seconds of the batched pairs: at hop 512 every length gives n // F == 512
PAIR512_SECONDS = ((12.0, 13.3), (13.9, 12.2), (12.7, 12.7), (14.0, 12.05), (12.4, 13.6), (13.1, 12.9))


@functools.lru_cache(maxsize=None)
def music512_signal():
    """12 s of the C3 pair signal: 529,200 samples, 1,032 STFT frames at hop 512, n // F == 512."""
    from sonar import synth
    x = np.ascontiguousarray(synth.c3_pair(12.0, 0.3)[0])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def pairs512():
    from sonar import synth
    rng = np.random.default_rng(13)
    qs, rs = [], []
    for k, (sq, sr_) in enumerate(PAIR512_SECONDS):
        q, r = synth.c3_pair(max(sq, sr_), 0.4 + 0.3 * k)[:2]
        nq, nr = int(round(sq * MUSIC_SR)), int(round(sr_ * MUSIC_SR))
        qs.append(np.ascontiguousarray(q[:nq]))
        rs.append(np.ascontiguousarray(r[:nr] + 1e-3 * rng.standard_normal(nr)))
    return qs, rs


def zcr_cases():
    """(name, float64 signal, alpha, W, H, sample rate).  With only the ZCR flag sonar_fingerprint
    runs no transform, so it takes every window > 0: all of 2, 3, 63, 64, 65 and 1000 are here.  The
    hops give frame counts with F % 4 in {1, 2, 3} (a partial 4-frame block), and n < W gives the
    single truncated frame (len < 2 for n = 1)."""
    rng = np.random.default_rng(5)
    zeros_mix = np.array([0.0, -0.0, 1.0, 0.0, -1.0, -0.0, 0.0, -1.0, -1.0, 0.0, 0.0, 1.0, -1.0, 1.0, -0.0, -0.0] * 70
                         )[:1103]
    alt = np.where(np.arange(1500) % 2 == 0, 1.0, -1.0)
    alt3 = np.where((np.arange(1500) // 3) % 2 == 0, 0.5, -0.5)
    sparse = np.zeros(1400)
    sparse[::7] = -0.25
    sparse[3::11] = 0.25
    square = np.where((np.arange(4000) // 37) % 2 == 0, 1.0, -1.0)
    noise = rng.standard_normal(3000)
    cases = []
    for W, H in [(2, 1), (2, 3), (3, 2), (63, 20), (64, 64), (65, 33), (1000, 10), (1000, 7)]:
        for name, x in [("zeros_mix", zeros_mix), ("alt", alt), ("alt3", alt3), ("sparse", sparse)]:
            cases.append((f"{name}-a0-W{W}-H{H}", x, 0.0, W, H, 16000))
        cases.append((f"square-a97-W{W}-H{H}", square, 0.97, W, H, 16000))
        cases.append((f"noise-a97-W{W}-H{H}", noise, 0.97, W, H, 44100))
    # truncated single frames: n < W (go_frames gives 1), len 1 and len 2
    cases.append(("one-sample-W3", np.array([-1.0]), 0.0, 3, 3, 16000))
    cases.append(("two-samples-W3", np.array([1.0, -1.0]), 0.0, 3, 3, 16000))
    cases.append(("short-W65", alt[:40], 0.0, 65, 33, 16000))
    return cases
