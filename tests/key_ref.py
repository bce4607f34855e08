"""Python checker of KeyEstimator and KeyEstimationBatch (algorithms/tonal/key_estimation.go): this
project's own restatement of the reference's formulas, statement by statement, with the reference's
line numbers.  Python floats are IEEE doubles, Python never fuses a multiply and an add, and every
sum below is a Python loop in the reference's order, so what differs from Go is libm (log) alone.

Parameters are dicts with the fields of sonar_key_params (DEFAULT is NewKeyEstimator's, :141-166).
Results are dicts; a key and mode pair travels as the code key * 2 + mode.

Three orders the reference leaves open are fixed here as the library fixes them:
sort.Slice on equal confidences keeps the candidates' creation order; findMode's map iteration gives
the lowest code among the most frequent; GetGlobalKey's map iteration gives the lowest code among
equal votes, and -1 (Go's empty name) when nothing voted.  common.Mean is gonum's stat.Mean; its sum
is taken in index order here and in the library."""
import math

DEFAULT = dict(profile=0, hpcp_size=12, normalize_chroma=1, remove_mean=0, binary_mode=0, max_candidates=5,
               min_confidence=0.5)
INV_LN2 = 1.4426950408889634      # Go's constant 1 / Ln2
KEY_NAMES = ["C", "C#", "D", "D#", "E", "F", "F#", "G", "G#", "A", "A#", "B"]
TRANSITIONS = ["same_key", "parallel", "relative", "dominant", "subdominant", "distant"]

# initializeKeyProfiles (:404-460): (major, minor) per KeyProfile value
PROFILES = [
    ([6.35, 2.23, 3.48, 2.33, 4.38, 4.09, 2.52, 5.19, 2.39, 3.66, 2.29, 2.88],
     [6.33, 2.68, 3.52, 5.38, 2.60, 3.53, 2.54, 4.75, 3.98, 2.69, 3.34, 3.17]),
    ([5.0, 2.0, 3.5, 2.0, 4.5, 4.0, 2.0, 4.5, 2.0, 3.5, 1.5, 4.0],
     [5.0, 2.0, 3.5, 4.5, 2.0, 4.0, 2.0, 4.5, 3.5, 2.0, 1.5, 4.0]),
    ([6.6, 2.0, 3.5, 2.3, 4.6, 4.0, 2.5, 5.2, 2.4, 3.7, 2.3, 3.4],
     [6.5, 2.7, 3.5, 5.4, 2.6, 3.5, 2.5, 4.7, 4.0, 2.7, 3.4, 3.2]),
    ([17.7661, 0.145624, 14.9265, 0.160186, 19.8049, 11.3587, 0.291248, 22.062, 0.145624, 8.15494, 0.232998, 4.95122],
     [18.2648, 0.737619, 14.0499, 16.8599, 0.702494, 14.4362, 0.702494, 18.6161, 4.56621, 1.93186, 7.37619, 1.75623]),
    ([16.8, 0.86, 12.95, 1.41, 13.49, 11.93, 1.25, 20.28, 1.80, 8.04, 0.62, 10.57],
     [18.16, 0.69, 12.99, 13.34, 1.07, 11.15, 1.38, 21.07, 7.49, 1.53, 6.24, 1.61]),
    ([5.0, 0.0, 3.0, 0.0, 4.0, 3.5, 0.0, 4.5, 0.0, 3.0, 0.0, 2.0],
     [5.0, 0.0, 3.0, 3.5, 0.0, 3.5, 0.0, 4.5, 3.0, 0.0, 2.0, 0.0]),
    ([5.0, 0.0, 0.0, 0.0, 3.0, 0.0, 0.0, 4.0, 0.0, 0.0, 0.0, 0.0],
     [5.0, 0.0, 0.0, 3.0, 0.0, 0.0, 0.0, 4.0, 0.0, 0.0, 0.0, 0.0]),
]


def params(**kw):
    p = dict(DEFAULT)
    p.update(kw)
    return p


def go_log2(x):
    """math.Log2 (log10.go): Frexp, exact for powers of two, else exp + Log(frac) * (1 / Ln2)."""
    frac, exp = math.frexp(x)
    if frac == 0.5:
        return float(exp - 1)
    return float(exp) + math.log(frac) * INV_LN2


def key_name(code):
    return "" if code < 0 else KEY_NAMES[(code >> 1) % 12] + (" minor" if code & 1 else " major")   # :707-716


def mean(values):
    """common.Mean (common/math.go:14-19): 0 for an empty slice, else the sum / n."""
    if len(values) == 0:
        return 0.0
    s = 0.0
    for v in values:
        s += v
    return s / float(len(values))


def resize_indices(n, target):
    """resizeChromaVector's source index per entry (:464-485); -1 where the entry stays 0."""
    if target < 0:
        raise IndexError("runtime error: makeslice: len out of range")
    ratio = float(n) / float(target) if target else 0.0      # :471 (never used when target is 0)
    out = []
    for i in range(target):
        src = float(i) * ratio                               # :474
        out.append(int(src) if int(src) < n else -1)         # :475-477
    return out


def preprocess(values, p):
    """preprocessChroma (:273-297)."""
    v = [float(x) for x in values]
    if len(v) != p["hpcp_size"]:                             # :277-279
        v = [v[k] if k >= 0 else 0.0 for k in resize_indices(len(v), p["hpcp_size"])]
    if p["normalize_chroma"] and len(v) > 0:                 # energyNormalize (common/normalization.go:113-134)
        energy = 0.0
        for x in v:
            energy += x * x
        if not energy < 1e-10:
            norm = math.sqrt(energy)
            v = [x / norm for x in v]
    if p["remove_mean"]:                                     # :487-498
        m = mean(v)
        v = [x - m for x in v]
    if p["binary_mode"]:                                     # :500-515
        thr = mean(v)
        v = [1.0 if x > thr else 0.0 for x in v]
    return v


def pearson(a, b):
    """stats.PearsonCorrelationFunc (stats/distance.go:111-145)."""
    n = len(a)
    if n == 0:
        return 0.0
    mean_a = mean_b = 0.0
    for i in range(n):
        mean_a += a[i]
        mean_b += b[i]
    mean_a /= float(n)
    mean_b /= float(n)
    num = ss_a = ss_b = 0.0
    for i in range(n):
        da = a[i] - mean_a
        db = b[i] - mean_b
        num += da * db
        ss_a += da * da
        ss_b += db * db
    if ss_a == 0 or ss_b == 0:
        return 0.0
    return num / math.sqrt(ss_a * ss_b)


def correlate_with_profile(chroma, profile, shift):
    """correlateWithProfile (:387-401)."""
    if len(chroma) != len(profile):
        return 0.0
    shifted = [profile[(i + shift) % len(profile)] for i in range(len(profile))]
    return pearson(chroma, shifted)


def uniformity(values):
    """computeUniformity (chroma/chroma_vector.go:385-408)."""
    s = 0.0
    for v in values:
        s += v
    if s == 0:
        return 1.0
    expected = s / float(len(values))
    var = 0.0
    for v in values:
        d = v - expected
        var += d * d
    var /= float(len(values))
    return 1.0 / (1.0 + var)


def estimate_key(values, p=DEFAULT):
    """EstimateKey (:196-233) -> dict of code, key, mode, known, confidence, strength, clarity, ambiguity,
    tonality, scores (24), candidates (codes), related (codes), processed."""
    v = preprocess(values, p)
    major, minor = PROFILES[p["profile"]] if 0 <= p["profile"] <= 6 else PROFILES[0]   # :301-305
    scores = [0.0] * 24
    cands = []
    for key in range(12):                                    # :311-339
        scores[key] = correlate_with_profile(v, major, key)
        cands.append((key * 2, scores[key]))
        scores[key + 12] = correlate_with_profile(v, minor, key)
        cands.append((key * 2 + 1, scores[key + 12]))
    cands.sort(key=lambda c: -c[1])                          # :342-344; Python's sort is stable: creation order
    mc = p["max_candidates"]
    if len(cands) > mc:                                      # :347-349
        if mc < 0:
            raise IndexError(f"runtime error: slice bounds out of range [:{mc}]")
        cands = cands[:mc]
    if not cands:                                            # :352
        raise IndexError("runtime error: index out of range [0] with length 0")
    code, best = cands[0]
    srt = sorted(scores, reverse=True)                       # calculateClarity (:517-533)
    clarity = (srt[0] - srt[1]) / srt[0] if srt[0] > 0 else 0.0
    total = 0.0                                              # calculateAmbiguity (:535-559)
    for s in scores:
        if s > 0:
            total += s
    ambiguity = 0.0
    if total != 0:
        entropy = 0.0
        for s in scores:
            if s > 0:
                prob = s / total
                entropy -= prob * go_log2(prob)
        ambiguity = entropy / go_log2(24.0)
    if len(v) == 0:                                          # ComputeStats' values[0] (chroma_vector.go:107)
        raise IndexError("runtime error: index out of range [0] with length 0")
    tonality = 1.0 - uniformity(v)                           # :688-692
    confidence, known = best, 1
    if confidence < p["min_confidence"]:                     # :680-683
        confidence, known = 0.0, 0
    return dict(code=code, key=code >> 1, mode=code & 1, known=known, confidence=confidence, strength=best,
                clarity=clarity, ambiguity=ambiguity, tonality=tonality, scores=scores,
                candidates=[c for c, _ in cands], related=[c for c, _ in cands[1:4]], processed=v)


def average_chroma(rows):
    """computeAverageChroma (:575-596); every row has the first row's length here."""
    size = len(rows[0])
    avg = [0.0] * size
    for r in rows:
        for i in range(size):
            avg[i] += r[i]
    count = float(len(rows))
    return [a / count for a in avg]


def find_mode(values):
    """findMode (:657-673) with the lowest value among the most frequent."""
    counts = {}
    for v in values:
        counts[v] = counts.get(v, 0) + 1
    best, mode = 0, 0
    for v in sorted(counts):
        if counts[v] > best:
            best, mode = counts[v], v
    return mode


def estimate_key_sequence(rows, p=DEFAULT, frames=None):
    """EstimateKeySequence (:250-270) -> estimate_key's dict of the average row plus stability and
    modulations; None for an empty sequence (Go's zero result).  frames: process_batch(rows, p), when
    the caller has it already."""
    rows = [[float(x) for x in r] for r in rows]
    if len(rows) == 0:
        return None
    res = estimate_key(average_chroma(rows), p)
    stability = 0.0                                          # analyzeTemporalStability (:598-622)
    if len(rows) >= 3:
        frames = frames if frames is not None else process_batch(rows, p)
        codes = [f["code"] for f in frames]
        m = find_mode(codes)
        stability = float(sum(1 for c in codes if c == m)) / float(len(codes))
    res["stability"] = stability
    mods = []                                                # detectModulations (:624-655)
    if len(rows) > 10 and len(rows) >= 20:
        prev = -1
        for i in range(10, len(rows) - 10):
            start, end = i - 5, i + 5
            if start >= 0 and end < len(rows):
                r = estimate_key(average_chroma(rows[start:end]), p)
                if prev != -1 and r["code"] != prev and r["confidence"] > 0.7:
                    mods.append(i)
                prev = r["code"]
    res["modulations"] = mods
    return res


def process_batch(rows, p=DEFAULT):
    """ProcessBatch (:911-920)."""
    return [estimate_key(r, p) for r in rows]


def global_key(frames):
    """GetGlobalKey (:923-959) -> dict of code (-1: no vote), confidence, strength, votes (24)."""
    if len(frames) == 0:
        return dict(code=-1, confidence=0.0, strength=0.0, votes=[0.0] * 24)
    votes = [0.0] * 24
    total = 0.0
    for f in frames:
        if f["confidence"] > 0.5:
            votes[f["code"]] += f["confidence"]
            total += f["confidence"]
    code, best = -1, 0.0
    for c in range(24):
        if votes[c] > best:
            best, code = votes[c], c
    return dict(code=code, confidence=best / total if total != 0 else float("nan"),
                strength=best / float(len(frames)), votes=votes)


def relative_key(key, mode):
    return ((key - 3 + 12) % 12, 1) if mode == 0 else ((key + 3) % 12, 0)     # :776-786


def _go_mod(a, b):
    return int(math.fmod(a, b))                              # Go's % keeps the dividend's sign


def analyze_key_transition(fk, fm, tk, tm):
    """AnalyzeKeyTransition (:843-894) -> dict of type (index of TRANSITIONS), transition_type,
    semitone_distance, fifths_distance, transition_strength."""
    distance = _go_mod(tk - fk + 12, 12)
    if fk == tk and fm == tm:
        t = 0
    elif fk == tk:
        t = 1
    elif (tk, tm) == ((_go_mod(fk - 3 + 12, 12), 1) if fm == 0 else (_go_mod(fk + 3, 12), 0)):
        t = 2
    elif (tk, tm) == (_go_mod(fk + 7, 12), fm):
        t = 3
    elif (tk, tm) == (_go_mod(fk - 7 + 12, 12), fm):
        t = 4
    else:
        t = 5
    fifths = 0 if t in (0, 1) else 1 if t in (2, 3, 4) else min(distance, 12 - distance)
    return dict(type=t, transition_type=TRANSITIONS[t], semitone_distance=distance, fifths_distance=fifths,
                transition_strength=1.0 / (1.0 + float(fifths)))


def key_progression(frames):
    """GetKeyProgression (:962-989) -> list of (frame, from code, to code, confidence, type)."""
    out = []
    for i in range(1, len(frames)):
        a, b = frames[i - 1], frames[i]
        if a["confidence"] > 0.5 and b["confidence"] > 0.5:
            t = analyze_key_transition(a["key"], a["mode"], b["key"], b["mode"])["type"]
            out.append((i, a["code"], b["code"], (a["confidence"] + b["confidence"]) / 2.0, t))
    return out
