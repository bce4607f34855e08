"""Python checker of ChromaCQT.ComputeChroma (algorithms/chroma/chroma_cqt.go), float64 numpy.

A restatement of the reference, literal where it matters: the kernels are built in the time domain in
the reference's order of operations (:120-135), pass through complexToReal's cmplx.Abs (:139,
:306-312), are zero-padded to the FFT size and transformed; every frame is zero-padded to the FFT size
and transformed (:183-191); the CQT bin is the magnitude of the sum over ALL FFT bins of
frameFFT * conj(kernelFFT) (:198-203); the fold adds the squared magnitudes by pitch class and divides
a frame by its sum when that is > 1e-10 (:213-268).  np.fft.fft stands in for go-dsp's FFTReal (the
full-length complex spectrum of a real input).

It also returns scale[f][k] = N |frame[:L_k]| |g_k|, the size of the terms the bin sums: the
tolerance of every magnitude comparison is a fraction of it."""
import math

import numpy as np

DEFAULT = dict(min_freq=65.4, max_freq=2093.0, bins_per_octave=12, q_factor=25.0, tuning_freq=440.0)  # :57-66


def go_div(a, b):
    """Go's integer division: truncates toward zero; a zero divisor panics."""
    if b == 0:
        raise ZeroDivisionError("runtime error: integer divide by zero")
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def go_round(x):
    """math.Round: half away from zero."""
    return math.copysign(math.floor(abs(x) + 0.5), x)


def kernel_length(sample_rate, q_factor, frequency):
    """calculateKernelLength (:147-165)."""
    n = int(q_factor * float(sample_rate) / frequency)
    if n % 2 == 0:
        n += 1
    if n < 3:
        n = 3
    if n > sample_rate // 2:
        n = sample_rate // 2
    return n


def next_power_of_two(n):
    """nextPowerOfTwo (:315-325)."""
    if n <= 0:
        return 1
    p = 1
    while p < n:
        p <<= 1
    return p


def n_frames(n, hop):
    """computeCQTSpectrogram's frame count (:169-172); ComputeChroma returns nil for n == 0 (:70-72)."""
    if n == 0:
        return 0
    f = go_div(n - hop, hop)
    return f if f > 0 else 1


def plan(sample_rate, min_freq=65.4, max_freq=2093.0, bins_per_octave=12, q_factor=25.0, tuning_freq=440.0):
    """computeCQTKernel's integer side (:95-115) and the fold's bin map (:224-230, :245-252)."""
    total = int(math.log2(max_freq / min_freq) * float(bins_per_octave))
    if total < 0:
        raise ValueError("runtime error: makeslice: len out of range")
    if total == 0:
        raise IndexError("runtime error: index out of range [0] with length 0")
    freqs = [min_freq * math.pow(2.0, float(k) / float(bins_per_octave)) for k in range(total)]
    lens = [kernel_length(sample_rate, q_factor, f) for f in freqs]
    cls = []
    for f in freqs:
        midi = 0.0 if f <= 0 else 69.0 + 12.0 * math.log2(f / tuning_freq)
        c = int(math.fmod(go_round(midi), 12))              # Go's %: the sign of the dividend
        cls.append(c + 12 if c < 0 else c)
    return {"total_bins": total, "freqs": np.array(freqs), "kernel_len": np.array(lens, np.int64),
            "fft_size": next_power_of_two(lens[0] * 2), "chroma_bin": np.array(cls, np.int64),
            "sum_taps": int(sum(lens))}


def taps(sample_rate, freq, length, q_factor):
    """One kernel's time-domain taps after complexToReal (:120-139, :306-312)."""
    bandwidth = freq / q_factor
    sigma = float(sample_rate) / (2.0 * math.pi * bandwidth)
    center = length // 2
    g = np.empty(length)
    for n in range(length):
        t = float(n - center)
        window = math.exp(-(t * t) / (2.0 * sigma * sigma))
        phase = 2.0 * math.pi * freq * t / float(sample_rate)
        g[n] = math.hypot(window * math.cos(phase), window * math.sin(phase))   # |complex(window, 0) * exp(i phase)|
    return g


def fold(cqt, chroma_bin):
    """convertCQTToChroma + normalizeChromaFrame (:213-268) -> (chroma, each frame's total energy)."""
    F = cqt.shape[0]
    chroma, totals = np.zeros((F, 12)), np.zeros(F)
    for f in range(F):
        row = [0.0] * 12
        for k, c in enumerate(chroma_bin):
            row[int(c)] += float(cqt[f, k]) * float(cqt[f, k])
        total = 0.0
        for e in row:
            total += e
        totals[f] = total
        if total > 1e-10:
            row = [e / total for e in row]
        chroma[f] = row
    return chroma, totals


def chroma_cqt(signal, hop, sample_rate, min_freq=65.4, max_freq=2093.0, bins_per_octave=12, q_factor=25.0,
               tuning_freq=440.0):
    """ComputeChroma(signal, hop) -> dict: chroma (F x 12), cqt (F x K), scale (F x K), energy (F: the
    un-normalised frame totals), plan (see plan) and g (the K tap arrays).  None for an empty signal."""
    x = np.ascontiguousarray(signal, dtype=np.float64)
    if len(x) == 0:
        return None
    p = plan(sample_rate, min_freq, max_freq, bins_per_octave, q_factor, tuning_freq)
    N, K = p["fft_size"], p["total_bins"]
    g = [taps(sample_rate, p["freqs"][k], int(p["kernel_len"][k]), q_factor) for k in range(K)]
    kern = np.zeros((K, N))
    for k in range(K):
        kern[k, :len(g[k])] = g[k]
    kernel_fft = np.fft.fft(kern, axis=1)                     # :139
    F = n_frames(len(x), hop)
    frames = np.zeros((F, N))
    for f in range(F):                                       # :179-188
        start = f * hop
        seg = x[start:start + N]
        frames[f, :len(seg)] = seg
    frame_fft = np.fft.fft(frames, axis=1)                   # :191
    cqt = np.abs(frame_fft @ np.conj(kernel_fft).T)          # :195-203: the sum runs over all N bins
    gnorm = np.array([math.sqrt(math.fsum(v * v for v in gk)) for gk in g])
    csq = np.cumsum(frames * frames, axis=1)
    scale = float(N) * np.sqrt(csq[:, p["kernel_len"] - 1]) * gnorm[None, :]
    chroma, energy = fold(cqt, p["chroma_bin"])
    return {"chroma": chroma, "cqt": cqt, "scale": scale, "energy": energy, "plan": p, "g": g, "frames": frames}
