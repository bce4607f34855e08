"""Coverage conditions of test_gpu_feature_variants.py, checked on the oracle alone: the builders of
feature_variants.py must keep reaching the code paths the GPU tests are there for (every YIN lag,
lane and residue; the frequency gate; every launch path of launch_chroma; frames at or beyond the end
of the signal; the un-normalised chroma branch; the ZCR sign rule on exact zeros), so a change to a
builder cannot quietly stop covering them."""
import numpy as np

import oracle as O
import feature_variants as V


# ---- YIN -------------------------------------------------------------------------------------

def test_yin_builder_controls_the_lag():
    """The even frame built for period P chooses tau == P for P = 2..510 at any sample rate (the lag
    does not depend on it); P = 511 is past the last lag the rule admits (tau + 1 < 512)."""
    want = np.array(V.YIN_PERIODS, np.int32)
    want[-1] = -1
    assert len(V.yin_lag_signal()) == 522_240
    for sr in V.YIN_RATES:
        _, _, tau = V.yin_oracle("lag", sr)
        assert len(tau) == 1019
        assert np.array_equal(tau[0::2], want), sr


def test_yin_pitched_lags_cover_every_lane_and_residue():
    """Over 8 kHz and 44.1 kHz every tau in 9..510 is reported with a nonzero pitch (the parabola
    and the neighbour-lane reads run and their result is visible): all 8 residues, lanes 1..63, both
    ends of every lane.  At each rate some chosen lags are gated to pitch 0 (outside 80-1000 Hz)."""
    pitched = set()
    for sr in (8000, 44100):
        p, c, tau = V.yin_oracle("lag", sr)
        pe, te = p[0::2], tau[0::2]
        pitched |= set(te[(pe != 0) & (te > 0)].tolist())
        gated = (te > 0) & (pe == 0)
        assert gated.any(), sr
        assert np.all(c[0::2][gated] == 0)
        f = sr / te[te > 0]
        assert (f < 79).any() or (f > 1001).any()       # the gate, not a failed detection
    assert pitched >= set(range(9, 511)), sorted(set(range(9, 511)) - pitched)
    assert {t % 8 for t in pitched} == set(range(8))
    assert {t // 8 for t in pitched} >= set(range(1, 64))
    # the lags that straddle two lanes: the local-minimum test at tau % 8 == 7 and the parabola's
    # tau - 1 at tau % 8 == 0 read the neighbour lane
    assert {t for t in pitched if t % 8 == 7} >= set(range(15, 511, 8))
    assert {t for t in pitched if t % 8 == 0} >= set(range(16, 511, 8))
    assert 510 in pitched


def test_yin_odd_frames_are_extra_cases():
    """The straddling frames are not designed; they must still be a mix of detections and none."""
    _, _, tau = V.yin_oracle("lag", 16000)
    odd = tau[1::2]
    assert (odd > 0).any() and (odd == -1).any()


def test_yin_sine_frames_make_the_neighbour_lane_read_decide():
    """In the noise frames the CMNDF is below the threshold at the period alone, so the
    local-minimum test (cm[tau] < cm[tau + 1]) rejects nothing and a wrong successor would go
    unnoticed: stated here, so that nobody takes those frames for a test of it.  The sinusoid frames
    descend through the threshold: lags with tau % 8 == 7 (successor in the next lane) are rejected
    before the chosen one in most frames and in every lane 1..61, and the choice changes if that
    successor came from the own lane, from two lanes on, or from the next lane's second lag."""
    own = lambda cm, t: cm[t - 7] if t % 8 == 7 else cm[t + 1]
    two_on = lambda cm, t: cm[min(t + 9, 511)] if t % 8 == 7 else cm[t + 1]
    second = lambda cm, t: cm[min(t + 2, 511)] if t % 8 == 7 else cm[t + 1]
    mutants = (own, two_on, second)

    x = V.yin_lag_signal()
    _, _, tau = V.yin_oracle("lag", 16000)
    for k in range(0, 1019, 2):
        cm = V.yin_cmndf_model(x[k * 512: k * 512 + 1024])
        assert V.yin_pick_model(cm) == tau[k]
        assert all(V.yin_pick_model(cm, m) == tau[k] for m in mutants)      # blind to the successor

    x = V.yin_sine_signal()
    _, _, tau = V.yin_oracle("sine", 16000)
    assert len(tau) == 2 * len(V.YIN_SINE_PERIODS) - 1
    changed = [0, 0, 0]
    lanes, chosen = set(), set()
    for k in range(0, len(tau), 2):
        cm = V.yin_cmndf_model(x[k * 512: k * 512 + 1024])
        assert V.yin_pick_model(cm) == tau[k] and tau[k] > 0, k     # the model is the oracle's rule
        chosen.add(int(tau[k]))
        below = np.flatnonzero(cm[1:tau[k]] < 0.15) + 1
        lanes |= {int(t) // 8 for t in below if t % 8 == 7}
        for q, m in enumerate(mutants):
            changed[q] += V.yin_pick_model(cm, m) != tau[k]
    # (lane 62's lag 503 would need a period of 504..510 whose dip is 7 lags wide on the near side)
    assert lanes >= set(range(1, 62)), sorted(set(range(1, 62)) - lanes)
    assert changed[0] >= 400 and changed[1] >= 200 and changed[2] >= 20, changed
    assert {t % 8 for t in chosen} == set(range(8)) and {t // 8 for t in chosen} >= set(range(2, 63))
    for sr in (8000, 44100):                                        # pitched and gated frames here too
        p = V.yin_oracle("sine", sr)[0]
        assert (p != 0).any() and (p == 0).any()


def test_yin_flat_frames_have_no_pitch():
    x = V.yin_flat_signal()
    assert int(O.lib().or_pitch_frames(len(x))) % 4 != 0
    for sr in V.YIN_RATES:
        p, c, tau = V.yin_oracle("flat", sr)
        assert np.all(tau[0::2] == -1) and np.all(p[0::2] == 0) and np.all(c[0::2] == 0)


# ---- chroma ----------------------------------------------------------------------------------

def launch_path(fs):
    """launch_chroma's choice for frame size fs (misc_kernels.hip), restated: the kernel, and for
    chroma_kernel whether the trig table is in LDS, the radix-2 path, the pad double and the raised
    dynamic-LDS attribute.  None: refused (more than 160 KB)."""
    if fs in (256, 512):
        return ("wave", fs // 64)
    K = fs // 2 + 1
    lds = 8 * (fs + K + 12)
    if lds > 160 * 1024:
        return None
    pad = (K + 12) & 1
    lds_t = 8 * (fs + K + 12 + pad + 2 * fs)
    trig_lds = lds_t <= 32 * 1024
    if trig_lds:
        lds = lds_t
    fft = fs & (fs - 1) == 0 and fs >= 2 and lds + 16 * fs <= 48 * 1024
    if fft:
        lds += 16 * fs + 8
    return ("block", "fft" if fft else "dft", "lds" if trig_lds else "global", pad, lds > 64 * 1024, lds)


def test_chroma_cases_select_every_launch_path():
    paths = {fs: launch_path(fs) for fs, _, _ in V.CHROMA_CASES}
    assert paths[256] == ("wave", 4) and paths[512] == ("wave", 8)
    fft = sorted(fs for fs, p in paths.items() if p[0] == "block" and p[1] == "fft")
    assert fft == [4, 8, 64, 128, 1024]
    assert {int(np.log2(fs)) % 2 for fs in fft} == {0, 1}           # even and odd stage counts
    assert launch_path(2048)[1] == "dft" and launch_path(4096)[1] == "dft"
    for fs in (3, 255, 257, 302, 1166):
        assert paths[fs][1:3] == ("dft", "lds"), fs
    assert paths[302][3] == 0 and paths[257][3] == 1                # with and without the pad double
    assert paths[1166][2] == "lds" and paths[1167][2] == "global"   # the two sides of trig_lds
    assert paths[5453][5] == 64 * 1024 and not paths[5453][4]       # the two sides of the attribute
    assert paths[5454][4]
    assert paths[13645][5] == 160 * 1024                            # the largest frame that fits
    assert launch_path(V.CHROMA_REFUSED_FS) is None
    assert launch_path(300) == ("block", "dft", "lds", launch_path(300)[3], False, launch_path(300)[5])


def test_chroma_cases_fix_the_frame_size_and_have_content():
    for fs, sr, F in V.CHROMA_CASES:
        x = V.chroma_signal(fs, sr, F)
        n = len(x)
        assert n // F == fs and 0 <= n - fs * F < F
        beyond = 0
        for hop in V.chroma_hops(fs, F):
            ref = V.chroma_oracle(fs, sr, F, hop)
            assert np.all(np.isfinite(ref))
            rows = np.abs(ref).sum(axis=1)
            assert (rows > 0).any(), (fs, hop)
            starts = np.arange(F) * hop
            out = starts >= n
            beyond += int(out.sum())
            assert np.all(ref[out] == 0), (fs, hop)                 # a frame of zero padding only
            if hop == fs + fs // 3 and fs >= 64:                    # (a few samples cannot be relied on to)
                assert ((starts < n) & (starts + fs > n)).any(), (fs, hop)   # a frame straddles n
            # a normalised row sums to 1
            live = rows > 1e-6
            assert np.allclose(ref[live].sum(axis=1), 1.0, rtol=0, atol=1e-12)
        assert beyond >= 1, fs


def test_chroma_oracle_agrees_with_numpy_rfft():
    """The oracle against an independent restatement (numpy.fft.rfft, the same window and class map)."""
    worst = 0.0
    for fs, sr, F in V.CHROMA_CASES:
        x = V.chroma_signal(fs, sr, F)
        hop = V.chroma_hops(fs, F)[1]
        win = O.window("hann", fs)
        fr = np.arange(fs // 2 + 1) * (sr / fs)
        ok = (fr >= 80.0) & (fr <= 8000.0)
        with np.errstate(divide="ignore"):
            cls = np.where(ok, np.round(69.0 + 12.0 * np.log2(np.where(fr > 0, fr, 1.0) / 440.0)).astype(int) % 12, -1)
        ref = V.chroma_oracle(fs, sr, F, hop)
        for t in range(F):
            seg = np.zeros(fs)
            s = t * hop
            if s < len(x):
                seg[: min(fs, len(x) - s)] = x[s: s + fs]
            pw = np.abs(np.fft.rfft(seg * win)) ** 2
            row = np.array([pw[cls == b].sum() for b in range(12)])
            if row.sum() > 1e-10:
                row = row / row.sum()
            worst = max(worst, float(np.max(np.abs(row - ref[t]))))
    assert worst < 1e-12, worst


def test_chroma_quiet_frames_take_the_unnormalised_branch():
    for fs in V.CHROMA_QUIET_FS:
        y = V.chroma_quiet_signal(fs)
        ref = O.chroma_frames(y, 7, fs, fs, 44100)
        tot = ref.sum(axis=1)
        assert np.all(tot > 0) and np.all(tot <= 1e-10), (fs, tot)
        assert np.all(np.abs(ref).max(axis=1) > 0)
        assert np.all(np.abs(tot - 1.0) > 0.5)                      # rows are left as they are


def test_music_and_pair_signals_have_512_sample_chroma_frames():
    x = V.music512_signal()
    F = O.stft_frames(len(x), 1024, 512)
    assert len(x) // F == 512
    lens = set()
    for sq, sr_ in V.PAIR512_SECONDS:
        for sec in (sq, sr_):
            assert 12.0 <= sec <= 14.0
            n = int(round(sec * V.MUSIC_SR))
            assert n // O.stft_frames(n, 1024, 512) == 512, sec
            lens.add(n)
    assert len(V.PAIR512_SECONDS) == 6 and len(lens) >= 10          # unequal lengths


# ---- ZCR -------------------------------------------------------------------------------------

def _count(x, rule):
    a, b = x[:-1], x[1:]
    return int(np.count_nonzero(rule(a, b)))


def test_zcr_cases_cover_windows_blocks_and_the_sign_rule():
    cases = V.zcr_cases()
    assert {W for _, _, _, W, _, _ in cases} == {2, 3, 63, 64, 65, 1000}
    res, short = set(), set()
    for name, x, alpha, W, H, sr in cases:
        F = O.stft_frames(len(x), W, H)
        assert F >= 1, name
        res.add(F % 4)
        if len(x) < W:
            assert F == 1
            short.add(len(x))
    assert res >= {1, 2, 3}
    assert 1 in short and 2 in short                                # len < 2 and the shortest counted frame
    # the zero / -0.0 signal: Go's (a >= 0 && b < 0) || (a < 0 && b >= 0) differs there from a
    # product rule and from a sign-bit rule, so only that rule gives the oracle's counts
    zm = next(x for name, x, *_ in cases if name.startswith("zeros_mix"))
    assert np.any((zm == 0) & np.signbit(zm)) and np.any((zm == 0) & ~np.signbit(zm))
    go = _count(zm, lambda a, b: ((a >= 0) & (b < 0)) | ((a < 0) & (b >= 0)))
    assert go != _count(zm, lambda a, b: a * b < 0)
    assert go != _count(zm, lambda a, b: np.signbit(a) != np.signbit(b))
    got = O.zcr_frames(O.preemphasis(zm, 0.0), 1, len(zm), 1, 16000)[0]
    assert got == go / (len(zm) / 16000)
    assert O.zcr_frames(np.array([-1.0]), 1, 3, 3, 16000)[0] == 0.0
    sq = next(x for name, x, *_ in cases if name.startswith("square"))
    assert set(np.unique(sq)) == {-1.0, 1.0}
