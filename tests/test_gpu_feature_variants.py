"""The per-frame feature kernels of misc_kernels.hip at every launch path and lane, against the
oracle (signals and case tables: feature_variants.py; that they reach these paths is asserted on the
oracle alone in test_feature_variants_cpu.py).

* yin_kernel: one frame per lag 2..511, so the chosen lag visits every lane (lags 8l..8l+7) and
  every residue: the neighbour-lane reads of the local-minimum test and of the parabola, the
  first-hit ballot, the last admitted lag 510, the frequency gate.  Those frames dip below the
  threshold at the period alone, so a second set of sinusoid frames makes the local-minimum test
  (and its read of the next lane at tau % 8 == 7) decide the lag.  Bit-exact (==), the kernel's
  own claim.
* chroma: one case per path of launch_chroma (chroma_wave_kernel<4> / <8>, alone and batched;
  chroma_kernel's radix-2 path, its direct DFT with the trig table in LDS or global memory, with and
  without the pad double, below and above the 64 KB dynamic-LDS attribute, the largest frame that
  fits and the refusal above it), frames that straddle or start beyond the end of the signal, the
  un-normalised branch, an all-zero signal.  Bound: 1e-9 absolute, the project's chroma bound.
  Observed worst over CHROMA_CASES on an MI355X: 1.0e-15 (fs 1167, direct DFT with the trig table
  in global memory; the radix-2 and wave-kernel cases are at or below 2.3e-16, fs 13645 at
  2.3e-16); the music entry at fs 512: 1.4e-16; quiet frames, relative to the row's largest
  element: 2.3e-15 (fs 300), 4.4e-16 (fs 512), 4.0e-16 (fs 256).
* zcr_kernel: exact zeros and -0.0, windows that are no multiple of 64, truncated frames, frame
  counts that leave a partial 4-frame block; equal to the oracle (array_equal).  With only the ZCR
  flag sonar_fingerprint runs no transform and takes every window, so none of 2, 3, 63, 64, 65 and
  1000 is dropped.
"""
import numpy as np
import pytest
import torch  # noqa: F401 -- before the library loads HIP (one HIP runtime in the process)

import oracle as O
import sonar
import feature_variants as V

pytestmark = pytest.mark.gpu


# ---- YIN -------------------------------------------------------------------------------------

@pytest.mark.parametrize("sr", V.YIN_RATES)
def test_yin_every_lag_bit_exact(ctx, sr):
    x = V.yin_lag_signal()
    p, c, tau = ctx.pitch_yin(x, sr)
    rp, rc, rt = V.yin_oracle("lag", sr)
    assert len(tau) == len(rt) == 1019
    bad = np.flatnonzero(tau != rt)
    assert bad.size == 0, (bad[:10], tau[bad[:10]], rt[bad[:10]])
    bad = np.flatnonzero((p != rp) | (c != rc))
    assert bad.size == 0, (bad[:10], rt[bad[:10]], p[bad[:10]], rp[bad[:10]], c[bad[:10]], rc[bad[:10]])


@pytest.mark.parametrize("sr", V.YIN_RATES)
def test_yin_sine_frames_bit_exact(ctx, sr):
    """Frames whose lag the local-minimum test decides (the successor of a lag with tau % 8 == 7
    comes from the next lane through __shfl_down); the noise frames above are blind to it."""
    x = V.yin_sine_signal()
    p, c, tau = ctx.pitch_yin(x, sr)
    rp, rc, rt = V.yin_oracle("sine", sr)
    assert len(tau) == len(rt) == 1003
    bad = np.flatnonzero(tau != rt)
    assert bad.size == 0, (bad[:10], tau[bad[:10]], rt[bad[:10]])
    bad = np.flatnonzero((p != rp) | (c != rc))
    assert bad.size == 0, (bad[:10], rt[bad[:10]], p[bad[:10]], rp[bad[:10]], c[bad[:10]], rc[bad[:10]])


@pytest.mark.parametrize("sr", V.YIN_RATES)
def test_yin_flat_frames(ctx, sr):
    x = V.yin_flat_signal()
    p, c, tau = ctx.pitch_yin(x, sr)
    rp, rc, rt = V.yin_oracle("flat", sr)
    assert len(tau) == 9
    assert np.all(tau[0::2] == -1) and np.all(p[0::2] == 0) and np.all(c[0::2] == 0)
    assert np.array_equal(tau, rt) and np.array_equal(p, rp) and np.array_equal(c, rc)


# ---- chroma ----------------------------------------------------------------------------------

@pytest.mark.parametrize("fs,sr,F", V.CHROMA_CASES, ids=[f"fs{c[0]}" for c in V.CHROMA_CASES])
def test_chroma_launch_paths(ctx, fs, sr, F):
    x = V.chroma_signal(fs, sr, F)
    assert len(x) // F == fs
    for hop in V.chroma_hops(fs, F):
        got = ctx.chroma_stft(x, F, hop, sr, preprocess=False)
        ref = V.chroma_oracle(fs, sr, F, hop)
        err = float(np.max(np.abs(got - ref)))
        print(f"chroma fs={fs} hop={hop}: max abs err {err:.3e}")
        assert err < 1e-9, (fs, hop, err)
        beyond = np.arange(F) * hop >= len(x)
        assert np.all(got[beyond] == 0)


def test_chroma_refuses_frame_above_lds(ctx):
    x = V.chroma_signal(V.CHROMA_REFUSED_FS, 44100, 1)
    assert len(x) == V.CHROMA_REFUSED_FS
    with pytest.raises(sonar.SonarError, match="chroma launch failed"):
        ctx.chroma_stft(x, 1, V.CHROMA_REFUSED_FS, 44100, preprocess=False)
    # the context still serves the next call
    y = V.chroma_signal(256, 44100, 7)
    assert np.max(np.abs(ctx.chroma_stft(y, 7, 256, 44100, preprocess=False) - V.chroma_oracle(256, 44100, 7, 256))) < 1e-9


@pytest.mark.parametrize("fs", V.CHROMA_QUIET_FS)
def test_chroma_quiet_frames_unnormalised(ctx, fs):
    y = V.chroma_quiet_signal(fs)
    got = ctx.chroma_stft(y, 7, fs, 44100, preprocess=False)
    ref = O.chroma_frames(y, 7, fs, fs, 44100)
    top = np.max(np.abs(ref), axis=1, keepdims=True)
    assert np.all(top > 0) and np.all(ref.sum(axis=1) <= 1e-10)
    err = float(np.max(np.abs(got - ref) / top))
    print(f"chroma quiet fs={fs}: max err relative to the row's largest element {err:.3e}")
    assert err < 1e-9, (fs, err)


@pytest.mark.parametrize("fs,F", [(256, 7), (512, 7), (300, 7), (64, 7), (1167, 3)])
def test_chroma_zero_signal(ctx, fs, F):
    got = ctx.chroma_stft(np.zeros(fs * F + 2), F, fs, 44100, preprocess=False)
    assert got.shape == (F, 12) and np.all(got == 0)


def test_music_features_512_sample_chroma_frames(ctx):
    """The music extractor's own entry at hop 512 on 12 s: n // F == 512, chroma_wave_kernel<8> after
    the DC-removal scan; energies as in test_gpu_pairs."""
    x = V.music512_signal()
    F = O.stft_frames(len(x), 1024, 512)
    assert len(x) // F == 512
    e, ch = ctx.music_alignment_features(x, 44100, 1024, 512, 1024, 512)
    ref = O.chroma_music(x, F, 512, 44100)
    assert ch.shape == ref.shape
    err = float(np.max(np.abs(ch - ref)))
    print(f"music chroma fs=512: max abs err {err:.3e}")
    assert err < 1e-9, err
    z = O.preemphasis(O.dc_removal(x, 0.995), 0.95)
    re = O.short_time_energy(z, 1024, 512)
    assert e.shape == re.shape
    assert np.max(np.abs(e - re) / np.maximum(np.abs(re), 1e-300)) < 1e-12


def _same(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(
        np.nan_to_num(a), np.nan_to_num(b))


def test_batched_equals_unbatched_at_hop_512(ctx, monkeypatch):
    """chroma_wave_kernel<8, true> (the batched feature launches at 512-sample chroma frames) against
    the unbatched path: identical records, the rule of test_batched_equals_unbatched_mixed_lengths."""
    qs, rs = V.pairs512()
    for x in qs + rs:
        assert len(x) // O.stft_frames(len(x), 1024, 512) == 512
    qd = [torch.from_numpy(x).cuda() for x in qs]
    rd = [torch.from_numpy(x).cuda() for x in rs]
    torch.cuda.synchronize()

    def run(**env):
        env.setdefault("SONAR_PAIR_RETRY", 0)     # a timed-out pipeline is an error here, never a silent redo
        for k, v in env.items():
            monkeypatch.setenv(k, str(v))
        try:
            ctx.dtw_counters(reset=True)
            out = ctx.align_pairs([q.data_ptr() for q in qd], [r.data_ptr() for r in rd],
                                  nq=[q.numel() for q in qd], nr=[r.numel() for r in rd], hop=512,
                                  max_lag_seconds=4.0, workers=8, device_ptrs=True)
            assert ctx.dtw_counters(reset=True)["dtw_timeouts"] == 0
            return out
        finally:
            for k in env:
                monkeypatch.delenv(k)

    ref = run(SONAR_PAIR_BATCH=0)
    got = run()
    assert np.all(ref["status"] == 0) and np.all(got["status"] == 0)
    assert np.all(got["flags"] == 0)
    for f in sonar.PAIR_FIELDS:
        assert _same(got[f], ref[f]), f


# ---- ZCR -------------------------------------------------------------------------------------

@pytest.mark.parametrize("pcm_dtype", [sonar.F64, sonar.F32], ids=["f64", "f32"])
def test_zcr_variants(ctx, pcm_dtype):
    for name, x, alpha, W, H, sr in V.zcr_cases():
        if pcm_dtype == sonar.F32:
            x = x.astype(np.float32)
        x64 = x.astype(np.float64)
        F = O.stft_frames(len(x), W, H)
        cfg = ctx.config(flags=sonar.FP_ZCR, window_size=W, hop_size=H, sample_rate=sr, preemph_alpha=alpha,
                         pcm_dtype=pcm_dtype, out_dtype=sonar.F64)
        got = ctx.fingerprint(x, cfg)["zcr"]
        ref = O.zcr_frames(O.preemphasis(x64, alpha), F, W, H, sr)
        assert got.shape == ref.shape == (F,), name
        assert np.array_equal(got, ref), (name, np.flatnonzero(got != ref)[:10])
