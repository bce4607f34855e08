"""Python checker of ChordDetector and ChordProgressionAnalyzer (algorithms/tonal/chord_detection.go
:217-1048, :1108-1173): this project's own restatement of the reference's statements, with the
reference's line numbers.  Python floats are IEEE doubles, Python never fuses a multiply and an add,
every sum below is a Python loop in the reference's order, and nothing on the path calls libm besides
sqrt, so the library is held to these values bit for bit.

Parameters are dicts with the fields of sonar_chord_params (DEFAULT is NewChordDetector's, :217-244).
A detector is fed chroma rows (what extractChromaFeatures returns) and the bass pair detectBassNote
returns; with use_bass_detection off the bass is (0, 0.0) whatever is passed, as in DetectChord (:421-426).

Four orders the reference leaves open are fixed here as the library fixes them:
  - the iteration of the templates map (:595) is the order of TEMPLATES: ascending quality code, then
    root 0..11; a candidate's slot is t * 12 + root and TemplateScores is indexed by slot;
  - sort.Slice (:453) on equal confidences keeps that creation order (a stable sort);
  - the iteration of extensionIntervals (:866) builds a bit mask (1 << interval) and so has no order;
  - the iteration of qualityCounts (:1164) gives the lowest quality code among equal counts.

Go's slices are modelled where the reference aliases them: chordHistory shares the backing array of
the candidate slice that DetectChord sorts in place after applyTemporalSmoothing returned (Slice below).
Detector is that literal form; sequence_reduced is the form the kernels run (DESIGN.md Kernel 4f): a
per-frame record, an integer chain over the records, and a parallel pass that applies the resolved
boosts.  test_chord_cpu.py shows the two equal on every GPU test input."""
import math

DEFAULT = dict(method=0, normalize_templates=1, use_inversions=1, max_candidates=5, use_bass_detection=1,
               detect_extensions=1, max_extension=13, use_temporal_smoothing=1, temporal_window=5,
               use_functional_analysis=0, min_chord_strength=0.2, bass_weight=0.3)
METHODS = ["template_matching", "harmonic_analysis", "cqt_based", "statistical", "ml_based", "hybrid"]
NOTE_NAMES = ["C", "C#", "D", "D#", "E", "F", "F#", "G", "G#", "A", "A#", "B"]
ROLES = ["", "tonic", "subdominant", "dominant", "leading_tone", "other"]
INVERSION_NAMES = ["", "/1st", "/2nd", "/3rd", "/4th"]
EXTENSION_ORDER = [10, 11, 2, 5, 9]     # the map literal's order (:857-863); the mask carries none

# initializeTemplates (:268-367) in ascending quality code: (quality, name, pattern, intervals, weight, consonance)
TEMPLATES = [
    (0, "major", [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0], [0, 4, 7], 1.0, 0.9),
    (1, "minor", [1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0], [0, 3, 7], 1.0, 0.85),
    (2, "diminished", [1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0], [0, 3, 6], 0.8, 0.3),
    (3, "augmented", [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0], [0, 4, 8], 0.7, 0.4),
    (4, "sus2", [1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0], [0, 2, 7], 0.7, 0.6),
    (5, "sus4", [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0], [0, 5, 7], 0.7, 0.6),
    (6, "major7", [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], [0, 4, 7, 11], 0.85, 0.8),
    (7, "minor7", [1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0], [0, 3, 7, 10], 0.85, 0.75),
    (8, "dominant7", [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0], [0, 4, 7, 10], 0.9, 0.7),
    (23, "power", [1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0], [0, 7], 0.6, 0.8),
]
NUM_SLOTS = len(TEMPLATES) * 12
QUALITY_CODES = [t[0] for t in TEMPLATES]
TEMPLATE_OF_QUALITY = {t[0]: i for i, t in enumerate(TEMPLATES)}

# GetChordQualityName (:1053-1086)
QUALITY_NAMES = ["major", "minor", "diminished", "augmented", "sus2", "sus4", "major7", "minor7", "dominant7",
                 "minor-major7", "augmented7", "diminished7", "half-diminished7", "add9", "major9", "minor9",
                 "dominant9", "major11", "minor11", "dominant11", "major13", "minor13", "dominant13", "power",
                 "unknown"]


def params(**kw):
    p = dict(DEFAULT)
    p.update(kw)
    return p


def quality_name(q):
    return QUALITY_NAMES[q] if 0 <= q < len(QUALITY_NAMES) else "unknown"


def slot_root(slot):
    return slot % 12


def slot_quality(slot):
    return QUALITY_CODES[slot // 12]


def chord_name(root, quality, inversion):
    """getChordName (:949-973)."""
    t = TEMPLATE_OF_QUALITY.get(quality)
    qn = TEMPLATES[t][1] if t is not None else "unknown"
    name = NOTE_NAMES[root % 12]
    if qn != "major":
        name += qn
    if inversion != 0 and inversion < len(INVERSION_NAMES):
        name += INVERSION_NAMES[inversion]
    return name


def method_name(method):
    return METHODS[method] if 0 <= method < len(METHODS) else "unknown"       # :975-989


def extension_list(mask):
    """The intervals of a mask in the order of the reference's map literal."""
    return [i for i in EXTENSION_ORDER if mask >> i & 1]


def inversion_patterns(t):
    """generateInversions (:376-405): the pattern itself, then per further interval twelve zeros with the
    chord tones copied from the pattern and 1.5 at that interval."""
    _, _, pattern, intervals, _, _ = TEMPLATES[t]
    out = [list(pattern)]
    for inv in range(1, len(intervals)):
        ip = [0.0] * 12
        for i, interval in enumerate(intervals):
            pos = (interval + 12) % 12
            ip[pos] = 1.5 if i == inv else pattern[pos]
        out.append(ip)
    return out


INVERSIONS = [inversion_patterns(t) for t in range(len(TEMPLATES))]


def normalize_chroma(chroma, p):
    """normalizeChroma (:703-710) over energyNormalize (common/normalization.go:113-134)."""
    if not p["normalize_templates"] or len(chroma) == 0:
        return chroma
    energy = 0.0
    for v in chroma:
        energy += v * v
    if energy < 1e-10:
        return chroma
    norm = math.sqrt(energy)
    return [v / norm for v in chroma]


def rotate_pattern(pattern, semitones):
    out = [0.0] * len(pattern)                                  # :712-719
    for i, v in enumerate(pattern):
        out[(i + semitones) % len(pattern)] = v
    return out


def template_score(chroma, template, weight):
    if len(chroma) != len(template):                            # :721-733
        return 0.0
    score = 0.0
    for i in range(len(chroma)):
        score += chroma[i] * template[i]
    return score * weight


def bass_bonus(root, bass_note, bass_conf, t, p):
    for interval in TEMPLATES[t][3]:                            # :735-750
        if (root + interval) % 12 == bass_note:
            return p["bass_weight"] * bass_conf
    return 0.0


def detect_inversion(chroma, t, root, bass_note):
    best_inv, best_score = 0, 0.0                               # :752-781
    intervals, weight = TEMPLATES[t][3], TEMPLATES[t][4]
    for inv in range(len(INVERSIONS[t])):
        if inv >= len(intervals):
            break
        if (root + intervals[inv]) % 12 == bass_note:
            score = template_score(chroma, rotate_pattern(INVERSIONS[t][inv], root), weight)
            if score > best_score:
                best_score, best_inv = score, inv
    return best_inv, best_score


def matching_bass(p, bass_note, bass_conf):
    """The bass pair templateMatching receives: DetectChord's (:421-445)."""
    if not p["use_bass_detection"]:
        return 0, 0.0
    if p["method"] in (1, 2, 3):                                # harmonicAnalysis, cqtBasedDetection, statistical
        return 0, 0.0
    return bass_note, bass_conf


def template_matching(chroma, bass_note, bass_conf, p):
    """templateMatching (:586-641) -> candidates in creation order (dicts of slot, inversion, confidence,
    strength) and the 120 template scores."""
    cands, scores = [], []
    nc = normalize_chroma(chroma, p)
    for t, (_, _, pattern, _, weight, _) in enumerate(TEMPLATES):
        for root in range(12):
            score = template_score(nc, rotate_pattern(pattern, root), weight)
            scores.append(score)
            if p["use_bass_detection"] and bass_conf > 0.3:
                score += bass_bonus(root, bass_note, bass_conf, t, p)
            if score >= p["min_chord_strength"]:
                c = dict(slot=t * 12 + root, inversion=0, confidence=min(score, 1.0), strength=score)
                if p["use_inversions"] and bass_conf > 0.3:
                    inv, inv_score = detect_inversion(nc, t, root, bass_note)
                    if inv_score > score:
                        c.update(inversion=inv, confidence=min(inv_score, 1.0), strength=inv_score)
                cands.append(c)
    return cands, scores


def variance(values):
    if len(values) == 0:                                        # :991-1010
        return 0.0
    mean = 0.0
    for v in values:
        mean += v
    mean /= float(len(values))
    var = 0.0
    for v in values:
        d = v - mean
        var += d * d
    return var / float(len(values))


def harmonic_tension(chroma):
    tension = 0.0                                               # :1012-1035
    for i in range(12):
        if chroma[i] > 0.2:
            for j in range(i + 1, 12):
                if chroma[j] > 0.2:
                    for dissonant in (1, 6, 11):
                        if j - i == dissonant:
                            tension += chroma[i] * chroma[j]
    return min(tension, 1.0)


def extension_number(interval):
    return {2: 9, 5: 11, 9: 13}.get(interval, 7)                # :1037-1048


def extensions_mask(chroma, slot, p):
    """analyzeExtensions (:840-894) as a mask of 1 << interval."""
    root, intervals = slot_root(slot), TEMPLATES[slot // 12][3]
    mask = 0
    for interval in EXTENSION_ORDER:
        if chroma[(root + interval) % 12] > 0.3 and interval not in intervals:
            if interval in (10, 11) or p["max_extension"] >= extension_number(interval):
                mask |= 1 << interval
    return mask


def role_code(quality):
    return {0: 1, 1: 2, 8: 3, 2: 4}.get(quality, 5)             # :896-917, an index into ROLES


def check_row(chroma):
    if len(chroma) not in (12, 24, 36):                         # :416-419 over :559-560
        raise ValueError("failed to extract chroma features: unsupported chroma size: %d" % len(chroma))


def finish_result(chroma, kept, n_found, scores, conf_history, p):
    """DetectChord from :462 to :497 on the cut candidate list."""
    r = dict(root=0, quality=0, inversion=0, n_found=n_found, confidence=0.0, strength=0.0, clarity=0.0,
             ambiguity=0.0, consonance=0.0, tension=0.0, stability=0.0, extensions=0, role=0,
             template_scores=scores, candidates=[c["slot"] for c in kept],
             cand_inversion=[c["inversion"] for c in kept], cand_confidence=[c["confidence"] for c in kept],
             cand_strength=[c["strength"] for c in kept], name="")
    if len(kept) == 0:
        return r
    best = kept[0]
    root, quality = slot_root(best["slot"]), slot_quality(best["slot"])
    r.update(root=root, quality=quality, inversion=best["inversion"], confidence=best["confidence"],
             strength=best["strength"], name=chord_name(root, quality, best["inversion"]))
    r["clarity"] = kept[0]["confidence"] - kept[1]["confidence"] if len(kept) > 1 else kept[0]["confidence"]
    r["ambiguity"] = 1.0 - r["clarity"]
    r["consonance"] = TEMPLATES[best["slot"] // 12][5]
    if len(conf_history) > 0:                                   # :829-834
        r["stability"] = max(0.0, 1.0 - variance(conf_history))
    else:
        r["stability"] = r["confidence"]
    r["tension"] = harmonic_tension(chroma)
    if p["detect_extensions"]:
        r["extensions"] = extensions_mask(chroma, best["slot"], p)
    if p["use_functional_analysis"]:
        r["role"] = role_code(quality)
    return r


class Slice:
    """A Go slice header over a shared backing list."""

    def __init__(self, arr, off, n):
        self.arr, self.off, self.n = arr, off, n

    def __len__(self):
        return self.n

    def __iter__(self):
        return iter(self.arr[self.off:self.off + self.n])

    def tail(self):                                             # s[1:]
        if self.n < 1:
            raise IndexError("runtime error: slice bounds out of range [1:0]")
        return Slice(self.arr, self.off + 1, self.n - 1)


class Detector:
    """The literal form: one ChordDetector, fed frame after frame."""

    def __init__(self, p=None):
        self.p = dict(DEFAULT) if p is None else p
        self.chord_history = Slice([], 0, 0)
        self.confidence_history = []

    def apply_temporal_smoothing(self, cands):
        """:783-806; cands is the Slice DetectChord sorts afterwards."""
        if len(self.chord_history) == 0:
            self.chord_history = cands
            return
        for c in cands:
            for h in self.chord_history:
                if c["slot"] == h["slot"]:                      # Root and Quality
                    c["confidence"] = min(c["confidence"] * 1.1, 1.0)
        self.chord_history = cands
        if len(self.chord_history) > self.p["temporal_window"]:
            self.chord_history = self.chord_history.tail()

    def detect(self, chroma, bass_note=0, bass_conf=0.0):
        p = self.p
        chroma = [float(v) for v in chroma]
        check_row(chroma)
        bn, bc = matching_bass(p, bass_note, bass_conf)
        arr, scores = template_matching(chroma, bn, bc, p)
        cands = Slice(arr, 0, len(arr))
        if p["use_temporal_smoothing"]:
            self.apply_temporal_smoothing(cands)
        arr.sort(key=lambda c: -c["confidence"])                # :453, in place and stable
        n_found = len(arr)
        if n_found > p["max_candidates"]:                       # :458-460
            if p["max_candidates"] < 0:
                raise IndexError("runtime error: slice bounds out of range [:%d]" % p["max_candidates"])
            kept = arr[:p["max_candidates"]]
        else:
            kept = arr
        kept = [dict(c) for c in kept]
        r = finish_result(chroma, kept, n_found, scores, self.confidence_history, p)
        if len(kept) > 0:                                       # updateTemporalTracking (:919-926)
            self.confidence_history = self.confidence_history + [kept[0]["confidence"]]
            if len(self.confidence_history) > p["temporal_window"]:
                self.confidence_history = self.confidence_history[1:]
        return r


def _bass(bass_notes, bass_confs, f):
    return (0 if bass_notes is None else int(bass_notes[f]), 0.0 if bass_confs is None else float(bass_confs[f]))


def frames(rows, p=None, bass_notes=None, bass_confs=None):
    """Every row through a fresh detector."""
    p = dict(DEFAULT) if p is None else p
    return [Detector(p).detect(rows[f], *_bass(bass_notes, bass_confs, f)) for f in range(len(rows))]


def sequence(rows, p=None, bass_notes=None, bass_confs=None):
    """One detector fed the rows in order (the literal form)."""
    d = Detector(dict(DEFAULT) if p is None else p)
    return [d.detect(rows[f], *_bass(bass_notes, bass_confs, f)) for f in range(len(rows))]


# ---- the reduced chain (what the kernels run) --------------------------------------------------------

HIST_EMPTY, HIST_FULL = -2, -1      # the history before a frame; >= 0: the full set minus that slot


def _boosted(c, boost):
    return min(c["confidence"] * 1.1, 1.0) if c["slot"] in boost else c["confidence"]


def _first(cands, boost):
    """The slot a stable descending sort puts first when the slots of boost are boosted; -1 without candidates."""
    best, best_conf = -1, 0.0
    for c in cands:
        conf = _boosted(c, boost)
        if best < 0 or conf > best_conf:
            best, best_conf = c["slot"], conf
    return best


def frame_records(per_row):
    """Per frame (n, topN, top0, top1) from rows t - 1 and t alone: the first candidate without a boost,
    with every member of C[t-1] boosted, and with every member but top0."""
    recs = []
    for t, cands in enumerate(per_row):
        prev = {c["slot"] for c in per_row[t - 1]} if t > 0 else set()
        top_n = _first(cands, set())
        top0 = _first(cands, prev)
        top1 = _first(cands, prev - {top0})
        recs.append((len(cands), top_n, top0, top1))
    return recs


def resolve_chain(recs, p):
    """The integer recurrence: the history state before every frame, every frame's first slot and the
    number of frames before it that kept a candidate."""
    w, smoothing, keeps = p["temporal_window"], p["use_temporal_smoothing"], p["max_candidates"] > 0
    state, states, firsts, kidx, kept = HIST_EMPTY, [], [], [], 0
    for n, top_n, top0, top1 in recs:
        states.append(state)
        kidx.append(kept)
        if not smoothing or state == HIST_EMPTY:
            first = top_n
            if smoothing:
                state = HIST_FULL if n > 0 else HIST_EMPTY
        else:
            first = top0 if state == HIST_FULL or state != top0 else top1
            if n == 0 and w < 0:
                raise IndexError("runtime error: slice bounds out of range [1:0]")
            if n > w:
                state = first if n > 1 else HIST_EMPTY
            else:
                state = HIST_FULL if n > 0 else HIST_EMPTY
        firsts.append(first)
        if n > 0 and keeps:
            kept += 1
    return states, firsts, kidx


def sequence_reduced(rows, p=None, bass_notes=None, bass_confs=None):
    p = dict(DEFAULT) if p is None else p
    rows = [[float(v) for v in r] for r in rows]
    per_row, per_scores = [], []
    for f, row in enumerate(rows):
        check_row(row)
        bn, bc = matching_bass(p, *_bass(bass_notes, bass_confs, f))
        cands, scores = template_matching(row, bn, bc, p)
        if p["max_candidates"] < 0:                             # len(candidates) >= 0 > MaxCandidates (:458)
            raise IndexError("runtime error: slice bounds out of range [:%d]" % p["max_candidates"])
        per_row.append(cands)
        per_scores.append(scores)
    states, firsts, kidx = resolve_chain(frame_records(per_row), p)
    out, kconf = [], []
    for t, cands in enumerate(per_row):
        boost = set()
        if states[t] != HIST_EMPTY:
            boost = {c["slot"] for c in per_row[t - 1]} - {states[t]}
        ranked = sorted((dict(c, confidence=_boosted(c, boost)) for c in cands), key=lambda c: -c["confidence"])
        kept = ranked[:p["max_candidates"]]
        assert not ranked or ranked[0]["slot"] == firsts[t]
        w = p["temporal_window"]
        hist = kconf[max(kidx[t] - w, 0):kidx[t]] if w > 0 else []
        out.append(finish_result(rows[t], kept, len(cands), per_scores[t], hist, p))
        if kept:
            kconf.append(kept[0]["confidence"])
    return out


def progression(quality, confidence):
    """AnalyzeProgression (:1128-1173) -> dict; below two chords num_chords and insufficient_data alone."""
    n = len(quality)
    if n < 2:
        return dict(num_chords=n, insufficient_data=1)
    total = 0.0
    for c in confidence:
        total += c
    counts = {}
    for q in quality:
        counts[q] = counts.get(q, 0) + 1
    most, max_count = 0, 0
    for q in sorted(counts):
        if counts[q] > max_count:
            most, max_count = q, counts[q]
    return dict(num_chords=n, insufficient_data=0, average_confidence=total / float(n), most_common_quality=most)
