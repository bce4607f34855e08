"""Python checker of FormantAnalyzer.AnalyzeFormants (algorithms/speech/format.go:85-411) over
LPCAnalyzer.Analyze (lpc.go:44-265), in stages that can each be fed from outside: this project's own
restatement of the reference's statements in float64, in Go's operation order, with the reference's
line numbers.  Python floats are IEEE doubles and Python never fuses a multiply and an add.

  preprocess(sig, sr)   the z-scored frame: pre-emphasis 0.97, symmetric Hamming (format.go:127-146),
                        mean / population sd with the sd < 1e-10 rule (stats/correlation.go:464-501)
  lags(z, p)            R[0..p] = r(L - m), L = min(1024, W - 1) (F11: Correlations[:p+1] starts at
                        lag -L), each a direct sum accumulated with math.fsum
  levinson(R, p)        status, a, k, E, order reached: in place as written (lpc.go:85-135)
  envelope(a, p)        513 points with libm cos(-i w) / sin(-i w) (lpc.go:233-265) and the per-bin
                        relative bound below
  tail(a, E, sr)        the record fields, a census of every branch taken and the decided flag
  frame(sig, sr)        all of them on one frame

The envelope's admissible error.  formant_kernel steps (cos, sin)(-i w) by a rotation recurrence
from (cos w, -sin w).  One step is two products and a sum per component, each rounded once, on
operands of magnitude <= 1: it adds at most 3 u to the absolute error of the pair, u = 2^-53, and the
rotation itself does not grow what is already there.  After i steps (cos, sin) is off by at most
about 3 i u.  rp = 1 + sum a_i cos(-i w) and ip = sum a_i sin(-i w) then carry at most
3 p u S each, S = sum |a_i|, and so does |A| = sqrt(rp^2 + ip^2) to first order.  env = 1 / |A|, so
its relative error is d|A| / |A| = 3 p u S env.  The p roundings of each sum and its products are of
the same form (at most u S per term) and are covered by a factor 4:

    rel_k = 4 * 3 * p * u * S * env_k              (BOUND_FACTOR * p * U * S * env_k)

This is derived, not fitted to any implementation.  test_formant_cpu.py checks with 50-digit
arithmetic that this module's own libm envelope lies inside it.

decided.  Two envelopes within rel_k of the true one differ by at most 2 rel_k env_k at bin k.  A
frame is decided when no comparison of the tail can come out differently between two such envelopes:
the strict neighbour tests up to the last peak kept, e / maxv > 0.1, every env[t] <= hh the two
half-height scans evaluate, cf < 0.2, vc > 0.3 and the merge's vc[i] > vc[ns-1].  The frequency and
bandwidth ladders, the 200 Hz spacing and the VTL window take bin indices times sr / 1024 only, so
they are decided once the peaks and crossings are; min(e, 1) and the final clamp are continuous."""
import functools
import math

import numpy as np

U = 2.0 ** -53
BOUND_FACTOR = 12.0
NFFT = 1024
MAX_FORMANTS = 4


def geometry(sr):
    """NewFormantAnalyzer (format.go:48-69) -> W, p."""
    return (2048 if sr >= 16000 else 1024), 12 + sr // 1000


@functools.lru_cache(maxsize=None)
def hamming(W):
    h = np.array([0.54 - 0.46 * math.cos(2.0 * math.pi * float(i) / float(W - 1)) for i in range(W)])
    h.setflags(write=False)
    return h


def _seq_sum(v):
    return float(np.cumsum(v)[-1])          # cumsum accumulates left to right, as Go's loop does


def preprocess(sig, sr):
    W, _ = geometry(sr)
    sig = np.asarray(sig, dtype=np.float64)[:W]
    assert len(sig) == W
    x = sig.copy()
    x[1:] = sig[1:] - 0.97 * sig[:-1]
    x = x * hamming(W)
    mean = _seq_sum(x) / float(W)
    d = x - mean
    sd = math.sqrt(_seq_sum(d * d) / float(W))
    return d if sd < 1e-10 else d / sd


def lags(z, p):
    W = len(z)
    L = min(1024, W - 1)
    return [math.fsum(z[:W - (L - m)] * z[L - m:]) for m in range(p + 1)]


def levinson(R, p):
    """-> status (0 ok, 3 zero energy, 4 prediction error became zero), a[0..p], k[0..p-1], E, order."""
    a, k = [0.0] * (p + 1), [0.0] * p
    E = R[0]
    if R[0] == 0:
        return 3, a, k, E, 0
    a[0] = 1.0
    order = 0
    for i in range(1, p + 1):
        num = R[i]
        for j in range(1, i):
            num -= a[j] * R[i - j]
        if E == 0:
            return 4, a, k, E, order
        k[i - 1] = num / E
        a[i] = k[i - 1]
        for j in range(1, i):
            a[j] = a[j] - k[i - 1] * a[i - j]          # in place, as written
        E *= (1 - k[i - 1] * k[i - 1])
        order = i
        if E <= 0:
            break
    return 0, a, k, E, order


def envelope(a, p):
    """-> env[513], rel[513]: GetSpectralEnvelope at nfft 1024 and the relative bound of the docstring."""
    env = np.zeros(NFFT // 2 + 1)
    for kk in range(NFFT // 2 + 1):
        w = 2.0 * math.pi * float(kk) / float(NFFT)
        rp, ip = 1.0, 0.0
        for i in range(1, p + 1):
            ang = -float(i) * w
            rp += a[i] * math.cos(ang)
            ip += a[i] * math.sin(ang)
        m = math.sqrt(rp * rp + ip * ip)
        env[kk] = 1.0 / m if m > 0 else 0.0
    S = math.fsum(abs(v) for v in a[1:p + 1])
    return env, BOUND_FACTOR * p * U * S * env


def _gmin(a, b):
    return a if a < b else b


def _gmax(a, b):
    return a if a > b else b


def tail(a, E, sr, env=None, rel=None):
    """findFormantsFromLPC .. calculateAnalysisQuality (format.go:148-411) on given coefficients.
    -> dict of the record fields, `census`, `decided` and `bound` (what two admissible envelopes may
    differ by: per formant for amplitude and confidence, one figure for quality and VTL)."""
    p = len(a) - 1
    if env is None:
        env, rel = envelope(a, p)
    err = 2.0 * rel * env                                # two admissible envelopes, absolute
    decided = True
    stable = 1
    for i in range(1, p + 1):
        if abs(a[i]) >= 1.0:
            stable = 0
    res = float(sr) / float(NFFT)
    maxv, imax = 0.0, 0
    for i in range(NFFT // 2 + 1):
        if env[i] > maxv:
            maxv, imax = env[i], i
    peaks = []
    if maxv != 0:
        for i in range(1, NFFT // 2):                     # findSpectralPeaks :193-222
            up, dn = env[i] - env[i - 1], env[i] - env[i + 1]
            mu, md = err[i] + err[i - 1], err[i] + err[i + 1]
            fr = float(i) * res
            in_range = not (fr < 50.0 or fr > float(sr) / 2.0)
            if len(peaks) < MAX_FORMANTS and in_range and env[i] / maxv > 0.1 - 0.1 * (rel[i] + rel[imax]) * 4:
                # a bin whose peak status two admissible envelopes could disagree on
                if (abs(up) <= mu and dn > -md) or (abs(dn) <= md and up > -mu):
                    decided = False
            if not (up > 0 and dn > 0):
                continue
            ratio = env[i] / maxv
            if len(peaks) < MAX_FORMANTS and in_range and abs(ratio - 0.1) <= 0.1 * (2 * (rel[i] + rel[imax]) + 4 * U):
                decided = False
            if not ratio > 0.1:
                continue
            if not in_range:
                continue
            peaks.append(i)
    census = dict(peaks_before_cut=len(peaks), peaks_kept=min(len(peaks), MAX_FORMANTS), peak_chunks=[], bw=[],
                  freq_arm=[], bw_arm=[], drop_conf=0, merges=0, merge_replaced=0, vtl_accepted=0,
                  vtl_rejected_conf=0, vtl_rejected_window=0, quality_arm=None, stable=stable)
    fq, bw, am, cf, ce = [], [], [], [], []
    for pk in peaks[:MAX_FORMANTS]:                       # the peaks ascend: the first 4 survive the cut
        ei = env[pk]
        fr = float(pk) * res
        hh = ei / 2.0                                     # estimateFormantBandwidth :225-262
        li = ri = pk
        for t in range(pk - 1, -1, -1):
            if abs(env[t] - hh) <= err[t] + err[pk] / 2.0:
                decided = False
            if env[t] <= hh:
                li = t
                break
        for t in range(pk + 1, NFFT // 2 + 1):
            if abs(env[t] - hh) <= err[t] + err[pk] / 2.0:
                decided = False
            if env[t] <= hh:
                ri = t
                break
        b = float(ri - li) * res
        clamp = None
        if b < 50.0:
            b, clamp = 50.0, 50
        elif b > 500.0:
            b, clamp = 500.0, 500
        # a search runs in 64-bin chunks from pk -+ 1: the seams it crossed before its hit
        census["bw"].append(dict(left_seams=(pk - 1 - li) // 64 if li != pk else (pk - 1) // 64,
                                 right_seams=(ri - pk - 1) // 64 if ri != pk else (NFFT // 2 - pk - 1) // 64,
                                 left_none=li == pk, right_none=ri == pk, clamp=clamp))
        census["peak_chunks"].append((pk - 1) // 64)
        c = 1.0                                           # calculateFormantConfidence :265-289
        if fr >= 300 and fr <= 3500:
            c *= 1.0
            census["freq_arm"].append("300-3500")
        elif fr >= 100 and fr <= 5000:
            c *= 0.7
            census["freq_arm"].append("100-5000")
        else:
            c *= 0.3
            census["freq_arm"].append("outside")
        c *= _gmin(ei, 1.0)
        if b >= 50 and b <= 300:
            c *= 1.0
            census["bw_arm"].append("50-300")
        elif b >= 30 and b <= 500:
            c *= 0.8
            census["bw_arm"].append("30-500")
        else:
            c *= 0.5
            census["bw_arm"].append("outside")
        c = _gmax(0.0, _gmin(1.0, c))
        fq.append(fr); bw.append(b); am.append(ei); cf.append(c)
        ce.append(err[pk] + 4 * U * c)                    # the ladder factors are <= 1
    vf, vb, va, vc, ve = [], [], [], [], []
    for i in range(len(fq)):                              # validateFormants :292-315
        if fq[i] < 50.0 or fq[i] > float(sr) / 2.0:
            continue
        if abs(cf[i] - 0.2) <= ce[i]:
            decided = False
        if cf[i] < 0.2:
            census["drop_conf"] += 1
            continue
        if bw[i] <= 0 or bw[i] > 1000:
            continue
        vf.append(fq[i]); vb.append(bw[i]); va.append(am[i]); vc.append(cf[i]); ve.append(ce[i])
    if len(vf) > 1:                                       # ensureProperSpacing :318-343
        keep = [0]
        for i in range(1, len(vf)):
            j = keep[-1]
            if vf[i] - vf[j] >= 200.0:
                keep.append(i)
            else:
                census["merges"] += 1
                if abs(vc[i] - vc[j]) <= ve[i] + ve[j]:
                    decided = False
                if vc[i] > vc[j]:
                    keep[-1] = i
                    census["merge_replaced"] += 1
        vf, vb, va, vc, ve = ([v[i] for i in keep] for v in (vf, vb, va, vc, ve))
    nv = len(vf)
    vtl = 17.5                                            # estimateVocalTractLength :346-377
    if nv > 0:
        tot, cnt = 0.0, 0
        for i in range(nv):
            if abs(vc[i] - 0.3) <= ve[i]:
                decided = False
            if vf[i] > 0 and vc[i] > 0.3:
                v = (2.0 * (i + 1) - 1.0) * 35000.0 / (4.0 * vf[i])
                if v >= 10.0 and v <= 25.0:
                    tot += v
                    cnt += 1
                    census["vtl_accepted"] += 1
                else:
                    census["vtl_rejected_window"] += 1
            else:
                census["vtl_rejected_conf"] += 1
        if cnt > 0:
            vtl = tot / float(cnt)
    quality = 0.0                                         # calculateAnalysisQuality :380-411
    if nv > 0:
        q1 = _gmin(float(nv) / 3.0, 1.0)
        ac = 0.0
        for i in range(nv):
            ac += vc[i]
        ac /= float(nv)
        lq = 1.0
        if E > 0:
            lq = _gmax(0.0, 1.0 - _gmin(1.0, E))
            census["quality_arm"] = "E>0"
        else:
            census["quality_arm"] = "E<=0"
        quality = (q1 + ac + lq + (1.0 if stable else 0.0)) / 4.0
    pad = [0.0] * (MAX_FORMANTS - nv)
    bound = dict(amplitude=[err[int(round(f / res))] + 4 * U * x for f, x in zip(vf, va)] + pad, confidence=ve + pad,
                 quality=(max(ve) if ve else 0.0) + 8 * U, vocal_tract_length=8 * U * vtl)
    return dict(n_formants=nv, frequency=vf + pad, bandwidth=vb + pad, amplitude=va + pad, confidence=vc + pad,
                vocal_tract_length=vtl, quality=quality, stable=stable, census=census, decided=decided, bound=bound)


def frame(sig, sr):
    """AnalyzeFormants (format.go:85-124) on one frame of at least W samples -> dict: the record fields,
    lpc_coeffs, reflection, residual_energy, gain, order, and for an ok frame tail()'s census / decided / bound."""
    W, p = geometry(sr)
    if len(sig) < W:
        return dict(status=1, order=0)
    R = lags(preprocess(sig, sr), p)
    status, a, k, E, order = levinson(R, p)
    out = dict(status=status, lpc_coeffs=a, reflection=k, residual_energy=E, order=order, R=R,
               gain=math.sqrt(E) if E >= 0 else float("nan"))
    if status == 0:
        out.update(tail(a, E, sr))
    return out


def frames(pcm, sr, frame_size=0, hop_size=0):
    """AnalyzeMultipleFrames (format.go:427-449): for i := 0; i < n - frameSize; i += hop."""
    W, _ = geometry(sr)
    fs = frame_size if frame_size > 0 else W
    hop = hop_size if hop_size > 0 else fs // 2
    return [frame(pcm[i:i + fs], sr) for i in range(0, len(pcm) - fs, hop)]
