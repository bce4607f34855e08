"""The inputs of the LPC formant tests, shared by test_formant_cpu.py (checker against oracle, census,
undecided cap) and test_gpu_formants.py (the library against the checker and the oracle on them).
A case is at most 16 frames of PCM with its sample rate, frame size and hop; its checker reference is
computed once and shared.  The generators and their seeds are committed, not arrays; the seeds were
found by search against the checker (formant_ref.py) and the oracle, and test_formant_cpu.py asserts
what they reach (census(), REQUIRED) so a change of inputs cannot lose it silently.

Why designed inputs.  R = Correlations[:p+1] are the lags L .. L-p, L = min(1024, W-1) (F11), so on
natural signals R[0] is a far lag, |k| > 1 within a few steps and the recursion ends at order 1-4 with
E <= 0.  The recursion is also the reference's in-place one (lpc.go:118-120 reads coefficients the same
step already rewrote), so even an exact autocorrelation sequence leaves |k| < 1 once the spectrum is
peaky: only mild spectra, or lags made for this recursion, run to order p.  Four kinds of input do:

  periodic  (W 2048) white noise of a period dividing 1024, tiled: lag 1024 is a multiple of the period
            and R is close to the signal's short-lag autocorrelation.  The hop is no multiple of the
            period, so the frames differ.
  burst     (W 2048) both halves of the windowed, pre-emphasised frame carry the same zero-sum burst y
            on [64, 960): R[m] = sum z[i] z[i+1024-m] is then y's linear autocorrelation at lag m.
            y is white noise plus a drawn share of a resonant impulse response.
  edge      (W 1024) L = 1023 and R[m] = sum_{i<=m} z[i] z[i+1023-m], products of the frame's two ends.
            The windowed frame is (1, 0 x p, filler, rho[p] .. rho[0]) with zero sum, so
            R[m] = z[0] z[1023-m] = rho[m], the autocorrelation of a burst as above.
  spike     (any W) the windowed frame is a unit spike at c and a block R[m] at c + L - m, so the lags
            are any sequence wanted: the one on which the in-place recursion takes a drawn set of
            reflection coefficients |k| < 1 (those of a polynomial with drawn resonances).

burst, edge and spike frames do not overlap (hop = frame size) and are built backwards from the
windowed frame: divide by the Hamming window, then undo the pre-emphasis (x[0] = sig[0], format.go:130).
Every such frame has its own seed and draws its own resonances.  A seed is kept only if the oracle's
FFT lags and the checker's exact lags agree on its frame (d, DESIGN.md Kernel 3c); ill-conditioned
frames, where they do not, cannot hold a third implementation to anything."""
import functools
import math

import numpy as np

import formant_ref as R

def _resonances(rng, sr, prof):
    """(centre Hz, bandwidth Hz) pairs of one frame."""
    k = int(rng.integers(prof["k"][0], prof["k"][1] + 1))
    fc = np.sort(rng.uniform(prof["f"][0], prof["f"][1], k))
    bw = np.exp(rng.uniform(math.log(prof["b"][0]), math.log(prof["b"][1]), k))
    out = list(zip(fc.tolist(), bw.tolist()))
    if rng.random() < prof.get("pair", 0.0):             # two narrow neighbours under 200 Hz apart
        f0 = float(rng.uniform(prof["f"][0], min(prof["f"][1], 3000.0)))
        b = float(rng.uniform(15.0, 50.0))
        out += [(f0, b), (f0 + float(rng.uniform(100.0, 190.0)), b)]
    return out


def _burst(rng, sr, n, prof):
    """n samples: white noise plus `mix` times a unit-rms impulse response of the frame's resonators,
    Hann-tapered, zero sum.  The in-place recursion only runs deep on mild spectra (DESIGN.md Kernel 3c)."""
    mix = float(np.exp(rng.uniform(math.log(prof["mix"][0]), math.log(prof["mix"][1]))))
    white = rng.standard_normal(n)
    y = (0.1 * rng.standard_normal(n)).tolist()
    y[n // 16] += 1.0
    for fc, bw in _resonances(rng, sr, prof):
        r = math.exp(-math.pi * bw / sr)
        c1, c2 = 2.0 * r * math.cos(2.0 * math.pi * fc / sr), r * r
        y1 = y2 = 0.0
        for i in range(n):
            y[i] = y[i] + c1 * y1 - c2 * y2
            y2, y1 = y1, y[i]
    y = np.array(y)
    y = white + mix * y / math.sqrt(float(np.mean(y * y)))
    t = 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(n) + 0.5) / n)
    y = y * t
    y -= t * (np.sum(y) / np.sum(t))
    return y / np.max(np.abs(y))


def _deemphasise(xw, W):
    """The PCM whose pre-emphasised, Hamming-windowed frame is xw."""
    x = xw / R.hamming(W)
    s = x.tolist()
    for i in range(1, W):
        s[i] = x[i] + 0.97 * s[i - 1]
    return np.array(s)


def burst_signal(sr, seeds, prof):
    W, p = R.geometry(sr)
    assert W == 2048
    out = []
    for seed in seeds:
        rng = np.random.Generator(np.random.PCG64(seed))
        y = _burst(rng, sr, 896, prof)
        xw = np.zeros(W)
        xw[64:960] = y
        xw[1024 + 64:1024 + 960] = y
        s = _deemphasise(xw, W)
        out.append(s / np.max(np.abs(s)))
    return np.concatenate(out + [np.zeros(1)])            # frames while i < n - frameSize


def edge_signal(sr, seeds, prof):
    W, p = R.geometry(sr)
    assert W == 1024
    out = []
    for seed in seeds:
        rng = np.random.Generator(np.random.PCG64(seed))
        y = _burst(rng, sr, prof["n"], prof)
        rho = np.array([float(np.dot(y[:len(y) - m], y[m:])) for m in range(p + 1)])
        rho /= rho[0]
        xw = np.zeros(W)
        xw[0] = 1.0
        xw[W - 1 - np.arange(p + 1)] = rho
        t = np.zeros(W)
        t[128:896] = 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(768) + 0.5) / 768)
        g = 0.05 * rng.standard_normal(W) * t
        xw += g - t * ((np.sum(xw) + np.sum(g)) / np.sum(t))
        s = _deemphasise(xw, W)
        out.append(s / np.max(np.abs(s)))
    return np.concatenate(out + [np.zeros(1)])


def _reflection(a, p):
    """The reflection coefficients of a stable polynomial (the textbook step-down), or None."""
    a = np.array(a, dtype=np.float64)
    ks = np.zeros(p)
    for i in range(p, 0, -1):
        k = a[i]
        ks[i - 1] = k
        if abs(k) >= 1:
            return None
        b = a.copy()
        for j in range(1, i):
            b[j] = (a[j] - k * a[i - j]) / (1 - k * k)
        b[i] = 0.0
        a = b
    return ks


def _lags_of(ks, p):
    """R[0..p] with R[0] = 1 on which the reference's in-place recursion (lpc.go:85-135) takes the
    reflection coefficients ks: each step solved for its R[i]."""
    Rr, a, E = [1.0] + [0.0] * p, [1.0] + [0.0] * p, 1.0
    for i in range(1, p + 1):
        k = float(ks[i - 1])
        Rr[i] = k * E + sum(a[j] * Rr[i - j] for j in range(1, i))
        a[i] = k
        for j in range(1, i):
            a[j] = a[j] - k * a[i - j]
        E *= (1 - k * k)
    return Rr


def _design(rng, sr, p, prof):
    """Reflection coefficients for one frame: those of a polynomial with the frame's resonances (and a
    small random remainder up to order p), sign and scale drawn; |k| < 1, so E stays positive."""
    A = np.array([1.0])
    for fc, bw in _resonances(rng, sr, prof):
        r = math.exp(-math.pi * bw / sr)
        A = np.convolve(A, [1.0, -2.0 * r * math.cos(2.0 * math.pi * fc / sr), r * r])
    a = np.convolve(A, np.concatenate([[1.0], 0.03 * rng.standard_normal(p - len(A) + 1)]))
    sign = 1.0 if rng.random() < 0.5 else -1.0
    scale = float(rng.uniform(0.5, 1.0))
    ks = _reflection(a, p)
    assert ks is not None, "a seed whose polynomial is not minimum phase"
    return sign * scale * ks


def spike_signal(sr, seeds, prof):
    """Frames whose z-scored form is a unit spike at c and R[m] at c + L - m (c = 0 at W 1024, 512 at
    W 2048) with a small zero-sum filler that no lag L - m pairs with either: R is the designed sequence."""
    W, p = R.geometry(sr)
    L = min(1024, W - 1)
    c = 0 if W == 1024 else 512
    lo, n = (128, 768) if W == 1024 else (100, 200)
    out = []
    for seed in seeds:
        rng = np.random.Generator(np.random.PCG64(seed))
        xw = np.zeros(W)
        xw[c] = 1.0
        xw[c + L - np.arange(p + 1)] = _lags_of(_design(rng, sr, p, prof), p)
        t = np.zeros(W)
        t[lo:lo + n] = 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(n) + 0.5) / n)
        g = 0.05 * rng.standard_normal(W) * t
        xw += g - t * ((np.sum(xw) + np.sum(g)) / np.sum(t))
        s = _deemphasise(xw, W)
        out.append(s / np.max(np.abs(s)))
    return np.concatenate(out + [np.zeros(1)])


def periodic_signal(sr, seed, period, hop, frames=14):
    """White noise of one period, tiled and peak-normalised; the hop is no multiple of the period."""
    W, _ = R.geometry(sr)
    n = W + (frames - 1) * hop + 1
    e = np.random.Generator(np.random.PCG64(seed)).standard_normal(period)
    sig = np.tile(e, -(-n // period))[:n]
    return sig / np.max(np.abs(sig))


# resonances per frame, centre and bandwidth ranges (Hz), mix of the resonant part, close-pair odds
MILD_1K = dict(k=(1, 3), f=(60.0, 950.0), b=(40.0, 250.0), mix=(0.2, 3.0), n=256)
MILD_8K = dict(k=(2, 5), f=(100.0, 3800.0), b=(30.0, 300.0), mix=(0.2, 3.0), n=384, pair=0.3)
MILD_16K = dict(k=(2, 6), f=(150.0, 5000.0), b=(30.0, 400.0), mix=(0.2, 3.0), n=512, pair=0.4)
SPIKE_2K = dict(k=(1, 3), f=(60.0, 950.0), b=(40.0, 250.0))
SPIKE_8K = dict(k=(1, 5), f=(100.0, 3800.0), b=(30.0, 300.0), pair=0.3)
SPIKE_16K = dict(k=(1, 5), f=(200.0, 5000.0), b=(30.0, 400.0), pair=0.6)

# sample rate -> W, p (NewFormantAnalyzer, format.go:48-69)
RATES = {2000: (1024, 14), 8000: (1024, 20), 15999: (1024, 27), 16000: (2048, 28), 44100: (2048, 56),
         52000: (2048, 64)}

# id -> (kind, sample rate, arguments); the seeds come from a search against formant_ref (see above)
CASES = {
    "spike-2000": ("spike", 2000, ((0, 1, 3, 4, 8, 9, 14, 23, 39, 40, 49, 195, 240, 255), SPIKE_2K)),
    "spike-8000": ("spike", 8000, ((3, 4, 19, 24, 26, 31, 34, 42, 57, 63, 86, 159, 202, 417), SPIKE_8K)),
    "spike-15999": ("spike", 15999, ((10, 11, 14, 16, 27, 34, 42, 48, 50, 74, 107, 1652, 1798, 1891), SPIKE_16K)),
    "spike-16000": ("spike", 16000, ((5, 14, 21, 34, 35, 41, 42, 74, 82, 105, 107, 697, 1388, 1453), SPIKE_16K)),
    "spike-44100": ("spike", 44100, ((14, 34, 49, 148, 160, 214, 482, 567, 591, 676, 1457, 1877, 2324, 2778),
                                     SPIKE_16K)),
    "spike-52000": ("spike", 52000, ((34, 48, 69, 114, 160, 186, 273, 389, 459, 1050, 1210, 2574, 2717, 2936),
                                     SPIKE_16K)),
    "edge-2000": ("edge", 2000, ((0, 1, 4, 5, 19, 21, 37, 67, 98, 104, 114, 183, 318, 2212, 2488, 2870), MILD_1K)),
    "edge-8000": ("edge", 8000, ((0, 1, 4, 5, 12, 27, 37, 46, 100, 112, 140, 191, 217, 881, 2003, 2819), MILD_8K)),
    "edge-15999": ("edge", 15999, ((0, 4, 7, 15, 17, 39, 59, 70, 75, 95, 358, 486, 1001, 1494, 2251, 2711), MILD_16K)),
    "burst-16000": ("burst", 16000, ((0, 4, 5, 6, 13, 17, 43, 47, 216, 217, 259, 530, 1380, 1535, 2344, 2768), MILD_16K)),
    "burst-44100": ("burst", 44100, ((0, 4, 9, 22, 38, 115, 295, 345, 575, 750, 787, 863, 927, 963, 2502, 2792),
                                     MILD_16K)),
    "burst-52000": ("burst", 52000, ((0, 4, 13, 14, 52, 140, 278, 281, 400, 488, 890, 927, 1201, 1480, 1973, 2038),
                                     MILD_16K)),
    "periodic-16000": ("periodic", 16000, (0, 128, 1000)),
    "periodic-16000-merge": ("periodic", 16000, (109, 64, 1023)),
    "periodic-44100": ("periodic", 44100, (554, 256, 1030)),
    "periodic-52000": ("periodic", 52000, (554, 256, 1030)),
}
CASE_IDS = sorted(CASES)


def class_cases(sr):
    return [c for c in CASE_IDS if CASES[c][1] == sr]


@functools.lru_cache(maxsize=None)
def case(cid):
    """-> pcm (read-only), sample rate, frame_size, hop_size as sonar_formants takes them."""
    kind, sr, args = CASES[cid]
    W, _ = R.geometry(sr)
    if kind == "periodic":
        seed, period, hop = args
        pcm, fs, hp = periodic_signal(sr, seed, period, hop), 0, hop
    else:
        pcm = dict(burst=burst_signal, edge=edge_signal, spike=spike_signal)[kind](sr, *args)
        fs, hp = W, W
    pcm = np.ascontiguousarray(pcm, dtype=np.float64)
    pcm.setflags(write=False)
    return pcm, sr, fs, hp


@functools.lru_cache(maxsize=None)
def reference(cid):
    """The checker's frames of a case (formant_ref.frames), computed once; treat as read-only."""
    pcm, sr, fs, hp = case(cid)
    return R.frames(pcm, sr, fs, hp)


def full_order(f, p):
    return f["status"] == 0 and f["order"] == p and f["residual_energy"] > 0


def _unclamped(b, side, seams):
    return b["clamp"] is None and not b[side + "_none"] and b[side + "_seams"] == seams


def census(sr):
    """What the class's cases reach, from the checker alone: counts of decided frames per branch
    (those under "full_" of decided frames that ran to order p with E > 0)."""
    _, p = RATES[sr]
    fr = [f for c in class_cases(sr) for f in reference(c) if f["status"] == 0]
    dec = [f for f in fr if f["decided"]]
    full = [f for f in dec if full_order(f, p)]
    bws = [b for f in dec for b in f["census"]["bw"]]
    n = lambda pool, pred: sum(1 for f in pool if pred(f))
    out = dict(frames=len(fr), decided=len(dec), full=len(full), max_order=max(f["order"] for f in fr),
               full_distinct=len(set(tuple(f["lpc_coeffs"]) for f in full)))
    for k in range(5):
        out["full_nf%d" % k] = n(full, lambda f: f["n_formants"] == k)
    out.update(full_peaks_over_4=n(full, lambda f: f["census"]["peaks_before_cut"] > 4),
               full_merge=n(full, lambda f: f["census"]["merges"] > 0),
               full_merge_replaced=n(full, lambda f: f["census"]["merge_replaced"] > 0),
               full_vtl=n(full, lambda f: f["vocal_tract_length"] != 17.5),
               full_stable0=n(full, lambda f: f["stable"] == 0), full_stable1=n(full, lambda f: f["stable"] == 1),
               full_drop_conf=n(full, lambda f: f["census"]["drop_conf"] > 0),
               full_vtl_rejected_conf=n(full, lambda f: f["census"]["vtl_rejected_conf"] > 0),
               full_vtl_rejected_window=n(full, lambda f: f["census"]["vtl_rejected_window"] > 0),
               quality_E_pos=n(dec, lambda f: f["census"]["quality_arm"] == "E>0"),
               quality_E_nonpos=n(dec, lambda f: f["census"]["quality_arm"] == "E<=0"),
               chunks3=n(dec, lambda f: len(set(f["census"]["peak_chunks"])) >= 3),
               scan_none=sum(1 for b in bws if b["left_none"] or b["right_none"]),
               clamp50=sum(1 for b in bws if b["clamp"] == 50), clamp500=sum(1 for b in bws if b["clamp"] == 500),
               unclamped=sum(1 for b in bws if b["clamp"] is None),
               left1=sum(1 for b in bws if _unclamped(b, "left", 1)), left2=sum(1 for b in bws if _unclamped(b, "left", 2)),
               right1=sum(1 for b in bws if _unclamped(b, "right", 1)),
               right2=sum(1 for b in bws if _unclamped(b, "right", 2)))
    for arm in ("300-3500", "100-5000", "outside"):
        out["freq_" + arm] = sum(1 for f in dec for a in f["census"]["freq_arm"] if a == arm)
    for arm in ("50-300", "30-500", "outside"):
        out["bw_" + arm] = sum(1 for f in dec for a in f["census"]["bw_arm"] if a == arm)
    return out


# What the cases must reach, per rate class, as minimum counts of census() (DESIGN.md Kernel 3c has the
# table and the branches no search reached: a spacing merge in a full-order frame at 44,100 and
# 52,000 Hz, where 200 Hz is under five envelope bins, and an unclamped half-height scan across a chunk
# seam at 8,000 Hz and above, where 65 bins are already more than 500 Hz).
_FULL = dict(full=8, full_distinct=8, full_nf2=1, full_nf3=1, full_nf4=1, full_peaks_over_4=1, full_vtl=1,
             full_stable0=1, full_stable1=1, quality_E_pos=8, scan_none=1, clamp50=1, clamp500=1, unclamped=1)
REQUIRED = {
    2000: dict(_FULL, max_order=14, left1=1, left2=1, right1=1, right2=1, chunks3=1, full_merge=1, full_merge_replaced=1),
    8000: dict(_FULL, max_order=20, chunks3=1, full_merge=1, full_merge_replaced=1),
    15999: dict(_FULL, max_order=27, chunks3=1),
    16000: dict(_FULL, max_order=28, full_merge=1, full_merge_replaced=1),
    44100: dict(_FULL, max_order=56),
    52000: dict(_FULL, max_order=64),
}


@functools.lru_cache(maxsize=None)
def oracle_frames(cid):
    """The oracle's records, coefficients and reflection coefficients of a case, computed once."""
    import oracle as O
    pcm, sr, fs, hp = case(cid)
    return O.formant_frames(pcm, sr, fs, hp, want_lpc=True)


def rel_to_largest(got, ref):
    """max |got - ref| per frame, relative to the frame's largest |ref|."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.max(np.abs(got - ref), axis=1) / np.max(np.abs(ref), axis=1)


@functools.lru_cache(maxsize=None)
def measured_d(cid):
    """d: the largest disagreement over the case's ok frames between two references of the same
    operation, the oracle's FFT autocorrelation path and the checker's exact direct sums: on the LPC
    and reflection coefficients relative to the frame's largest, on the residual energy and the gain
    (where it is a number) relative to themselves.  A third summation order (the device's) is allowed
    max(1e-12, 16 d); a case with 16 d > 1e-6 is replaced, not admitted."""
    ref, o = reference(cid), oracle_frames(cid)
    ok = [i for i, f in enumerate(ref) if f["status"] == 0]
    d = max(np.max(rel_to_largest(o["lpc_coeffs"][ok], [ref[i]["lpc_coeffs"] for i in ok])),
            np.max(rel_to_largest(o["reflection"][ok], [ref[i]["reflection"] for i in ok])))
    for i in ok:
        E = ref[i]["residual_energy"]
        d = max(d, abs(o["residual_energy"][i] - E) / abs(E))
        if E > 0:
            d = max(d, abs(o["gain"][i] - ref[i]["gain"]) / ref[i]["gain"])
    return float(d)


def front_end_bound(cid):
    return max(1e-12, 16.0 * measured_d(cid))
