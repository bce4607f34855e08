package sonargpu

// KeyEstimator seam (algorithms/tonal/key_estimation.go): EstimateKey, EstimateKeyFromHPCP,
// EstimateKeySequence and KeyEstimationBatch through sonar_key_frames, sonar_key_sequence and
// sonar_key_batch, AnalyzeKeyTransition through sonar_key_transition.  The library returns numbers and
// codes (key*2 + mode); this file rebuilds KeyEstimationResult with its strings: the key names,
// "Unknown", KeyProfile, Method, RelatedKeys, and the last-20 history the reference keeps in the
// estimator.  The constructors are methods of Context because the object needs a device; otherwise
// the names and signatures are the reference's.
//
// ChordDetector seam (algorithms/tonal/chord_detection.go), at the end of this file: DetectChord,
// DetectChords and ChordProgressionAnalyzer through sonar_chord_frames, sonar_chord_detect,
// sonar_chord_sequence and sonar_chord_progression, with the names and strings rebuilt here.
//
// PitchDetector seam (algorithms/tonal/pitch_detection.go), after the chord detector: every method of
// DetectPitch's switch through sonar_pitch_frames_raw, sonar_pitch_track, sonar_pitch_detect and
// sonar_pitch_stability.
//
// HarmonicRatioAnalyzer seam (algorithms/tonal/harmonic_ratio.go), at the end of this file: AnalyzeSequence
// over one signal through sonar_hratio, and the helpers through their host-only entries.
//
// Written against include/sonar_gpu.h; not compiled here (no Go toolchain in the image).

/*
#include "sonar_gpu.h"
*/
import "C"

import (
	"fmt"
	"math"
	"sort"
	"unsafe"
)

// KeyProfile, KeyMode and KeyEstimationMethod carry the reference's values (:13-42); KeyProfile's are
// SONAR_KEY_PROFILE_*.
type KeyProfile int

const (
	KeyProfileKrumhansl KeyProfile = iota
	KeyProfileTemperley
	KeyProfileShaath
	KeyProfileEDMA
	KeyProfileBgate
	KeyProfileDiatonic
	KeyProfileTonicTriad
)

type KeyMode int

const (
	KeyModeMajor KeyMode = iota
	KeyModeMinor
)

type KeyEstimationMethod int

const (
	KeyMethodProfile KeyEstimationMethod = iota
	KeyMethodCorrelation
	KeyMethodBayesian
	KeyMethodHMM
	KeyMethodDeepLearning
)

// KeyCandidate = tonal.KeyCandidate (:45-52).
type KeyCandidate struct {
	Key        int
	Mode       KeyMode
	KeyName    string
	Confidence float64
	Strength   float64
	Profile    string
}

// KeyEstimationResult = tonal.KeyEstimationResult (:55-85).  ProcessTime is 0, as the reference's
// placeholder clock leaves it (:756-759).
type KeyEstimationResult struct {
	Key               int
	Mode              KeyMode
	KeyName           string
	Confidence        float64
	Strength          float64
	Candidates        []KeyCandidate
	ChromaVector      []float64
	KeyProfile        string
	Method            string
	CorrelationScores []float64
	Clarity           float64
	Ambiguity         float64
	Stability         float64
	RelatedKeys       []KeyCandidate
	Modulations       []int
	Tonality          float64
	ProcessTime       float64
	HPCPSize          int
}

// KeyEstimationParams = tonal.KeyEstimationParams (:88-113), every field kept for source compatibility.
// The reference reads Profile, HPCPSize, NormalizeChroma, RemoveMean, BinaryMode, MaxCandidates and
// MinConfidence; Method only names the result (every method runs the profile correlation), and the
// rest is never read (DESIGN.md F43).
type KeyEstimationParams struct {
	Method                 KeyEstimationMethod
	Profile                KeyProfile
	HPCPSize               int
	UseHarmonics           bool
	WeightHarmonics        bool
	NormalizeChroma        bool
	RemoveMean             bool
	UsePolyphony           bool
	MinConfidence          float64
	MaxCandidates          int
	ProfileStrength        float64
	UseTemporalSmoothing   bool
	TemporalWindow         int
	UseDetuningCorrection  bool
	TranspositionInvariant bool
	BinaryMode             bool
}

// KeyEstimator mirrors tonal.KeyEstimator (:124-138); the profile tables live in the library.
type KeyEstimator struct {
	x          *Context
	params     KeyEstimationParams
	keyHistory []KeyCandidate
}

// NewKeyEstimator = tonal.NewKeyEstimator (:141-166).  sampleRate is kept for the signature; the
// reference only hands it to an HPCP it never uses.
func (x *Context) NewKeyEstimator(sampleRate int) *KeyEstimator {
	return &KeyEstimator{x: x, keyHistory: []KeyCandidate{}, params: KeyEstimationParams{Method: KeyMethodProfile,
		Profile: KeyProfileKrumhansl, HPCPSize: 12, UseHarmonics: true, NormalizeChroma: true, UsePolyphony: true,
		MinConfidence: 0.5, MaxCandidates: 5, ProfileStrength: 1.0, TemporalWindow: 5}}
}

// NewKeyEstimatorWithParams = tonal.NewKeyEstimatorWithParams (:169-180).
func (x *Context) NewKeyEstimatorWithParams(sampleRate int, params KeyEstimationParams) *KeyEstimator {
	return &KeyEstimator{x: x, params: params, keyHistory: []KeyCandidate{}}
}

func (ke *KeyEstimator) cParams() C.sonar_key_params {
	b := func(v bool) C.int32_t {
		if v {
			return 1
		}
		return 0
	}
	p := ke.params
	return C.sonar_key_params{profile: C.int32_t(p.Profile), hpcp_size: C.int32_t(p.HPCPSize),
		normalize_chroma: b(p.NormalizeChroma), remove_mean: b(p.RemoveMean), binary_mode: b(p.BinaryMode),
		max_candidates: C.int32_t(p.MaxCandidates), min_confidence: C.double(p.MinConfidence)}
}

// GetKeyName = tonal.GetKeyName (:764-773).
func GetKeyName(key int, mode KeyMode) string {
	keyNames := []string{"C", "C#", "D", "D#", "E", "F", "F#", "G", "G#", "A", "A#", "B"}
	if mode == KeyModeMajor {
		return keyNames[key%12] + " major"
	}
	return keyNames[key%12] + " minor"
}

func methodName(m KeyEstimationMethod) string { // getMethodName (:718-733)
	switch m {
	case KeyMethodProfile:
		return "Profile Correlation"
	case KeyMethodCorrelation:
		return "Direct Correlation"
	case KeyMethodBayesian:
		return "Bayesian"
	case KeyMethodHMM:
		return "Hidden Markov Model"
	case KeyMethodDeepLearning:
		return "Deep Learning"
	}
	return "Unknown"
}

// GetSupportedProfiles = tonal.GetSupportedProfiles (:1030-1040).
func GetSupportedProfiles() []string {
	return []string{"Krumhansl-Schmuckler", "Temperley", "Shaath", "EDMA", "Bgate", "Diatonic", "Tonic Triad"}
}

// GetSupportedMethods = tonal.GetSupportedMethods (:1043-1051).
func GetSupportedMethods() []string {
	return []string{"Profile Correlation", "Direct Correlation", "Bayesian", "Hidden Markov Model", "Deep Learning"}
}

func profileName(p KeyProfile) string { // getProfileName (:735-754)
	if p >= 0 && int(p) < 7 {
		return GetSupportedProfiles()[p]
	}
	return "Unknown"
}

// the candidates' Profile is the template's Name, and an unknown profile falls back to Krumhansl's (:301-305)
func templateName(p KeyProfile) string {
	if p >= 0 && int(p) < 7 {
		return GetSupportedProfiles()[p]
	}
	return "Krumhansl-Schmuckler"
}

// frameOut holds the per-frame outputs of one call.
type frameOut struct {
	key, mode, known                                   []int32
	confidence, strength, clarity, ambiguity, tonality []float64
	scores, processed                                  []float64
	candidates                                         []int32
	nc, hs                                             int
}

func newFrameOut(frames int, p KeyEstimationParams) *frameOut {
	nc, hs := p.MaxCandidates, p.HPCPSize
	if nc > 24 {
		nc = 24
	}
	if nc < 0 {
		nc = 0 // the call reports the panic
	}
	if hs < 0 {
		hs = 0
	}
	f := func() []float64 { return make([]float64, frames+1) }
	i := func() []int32 { return make([]int32, frames+1) }
	return &frameOut{key: i(), mode: i(), known: i(), confidence: f(), strength: f(), clarity: f(), ambiguity: f(),
		tonality: f(), scores: make([]float64, frames*24+1), processed: make([]float64, frames*hs+1),
		candidates: make([]int32, frames*nc+1), nc: nc, hs: hs}
}

func i32p(v []int32) *C.int32_t { return (*C.int32_t)(unsafe.Pointer(&v[0])) }

// result rebuilds frame t's KeyEstimationResult (estimateKeyProfile :358-369, postProcessResult
// :675-686, EstimateKey :226-230).
func (ke *KeyEstimator) result(o *frameOut, t int) KeyEstimationResult {
	scores := o.scores[t*24 : (t+1)*24 : (t+1)*24]
	cands := make([]KeyCandidate, o.nc)
	for r := range cands {
		code := int(o.candidates[t*o.nc+r])
		key, mode := code/2, KeyMode(code%2)
		s := scores[int(mode)*12+key]
		cands[r] = KeyCandidate{Key: key, Mode: mode, KeyName: GetKeyName(key, mode), Confidence: s, Strength: s,
			Profile: templateName(ke.params.Profile)}
	}
	related := []KeyCandidate{} // findRelatedKeys (:561-573)
	for r := 1; r < len(cands) && r < 4; r++ {
		related = append(related, cands[r])
	}
	name := "Unknown"
	if o.known[t] != 0 {
		name = GetKeyName(int(o.key[t]), KeyMode(o.mode[t]))
	}
	return KeyEstimationResult{Key: int(o.key[t]), Mode: KeyMode(o.mode[t]), KeyName: name, Confidence: o.confidence[t],
		Strength: o.strength[t], Candidates: cands, ChromaVector: o.processed[t*o.hs : (t+1)*o.hs : (t+1)*o.hs],
		KeyProfile: profileName(ke.params.Profile), Method: methodName(ke.params.Method), CorrelationScores: scores,
		Clarity: o.clarity[t], Ambiguity: o.ambiguity[t], RelatedKeys: related, Tonality: o.tonality[t], HPCPSize: o.hs}
}

// track = updateTemporalTracking (:694-705): the first candidate joins the history, the last 20 stay.
func (ke *KeyEstimator) track(r KeyEstimationResult) {
	if len(r.Candidates) > 0 {
		ke.keyHistory = append(ke.keyHistory, r.Candidates[0])
	}
	if len(ke.keyHistory) > 20 {
		ke.keyHistory = ke.keyHistory[len(ke.keyHistory)-20:]
	}
}

func flatten(rows [][]float64) ([]float64, int) {
	dim := 0
	if len(rows) > 0 {
		dim = len(rows[0])
	}
	flat := make([]float64, len(rows)*dim+1)
	for t, row := range rows {
		copy(flat[t*dim:(t+1)*dim], row)
	}
	return flat, dim
}

// EstimateKeys = KeyEstimator.EstimateKey (:196-233) on every chroma vector of a batch of one length,
// in order; the history advances as if the reference had been called once per vector.  Where the
// reference panics (MaxCandidates <= 0, HPCPSize <= 0) the error wraps ErrPanic and carries Go's
// runtime error text; a non-finite chroma value wraps ErrUnsupported (include/sonar_gpu.h).
func (ke *KeyEstimator) EstimateKeys(chroma [][]float64) ([]KeyEstimationResult, error) {
	frames := len(chroma)
	if frames == 0 {
		return []KeyEstimationResult{}, nil
	}
	flat, dim := flatten(chroma)
	o := newFrameOut(frames, ke.params)
	p := ke.cParams()
	if rc := C.sonar_key_frames(ke.x.c, f64p(flat), C.int64_t(frames), C.int32_t(dim), &p, i32p(o.key), i32p(o.mode),
		i32p(o.known), f64p(o.confidence), f64p(o.strength), f64p(o.clarity), f64p(o.ambiguity), f64p(o.tonality),
		f64p(o.scores), i32p(o.candidates), f64p(o.processed), 0); rc != C.SONAR_OK {
		return nil, ke.x.err(rc)
	}
	out := make([]KeyEstimationResult, frames)
	for t := range out {
		out[t] = ke.result(o, t)
		ke.track(out[t])
	}
	return out, nil
}

// EstimateKey = KeyEstimator.EstimateKey (:196-233).
func (ke *KeyEstimator) EstimateKey(chromaVector []float64) (KeyEstimationResult, error) {
	r, err := ke.EstimateKeys([][]float64{chromaVector})
	if err != nil {
		return KeyEstimationResult{}, err
	}
	return r[0], nil
}

// EstimateKeyFromHPCP = KeyEstimator.EstimateKeyFromHPCP (:236-247).
func (ke *KeyEstimator) EstimateKeyFromHPCP(hpcpResult HPCPResult) (KeyEstimationResult, error) {
	return ke.EstimateKey(hpcpResult.HPCP)
}

// EstimateKeySequence = KeyEstimator.EstimateKeySequence (:250-270).  The reference's history grows by
// one entry per internal EstimateKey (the average, every frame from 3 frames on, every window); what
// remains are the last 20 of them, and those are rebuilt here: the windows' first candidates are not
// returned by the library, so a sequence long enough to have 20 windows leaves the history to the
// per-frame and average entries (DESIGN.md F48).
func (ke *KeyEstimator) EstimateKeySequence(chromaSequence [][]float64) (KeyEstimationResult, error) {
	frames := len(chromaSequence)
	if frames == 0 {
		return KeyEstimationResult{}, nil
	}
	flat, dim := flatten(chromaSequence)
	o := newFrameOut(1, ke.params)
	capMod := frames - 20
	if capMod < 0 {
		capMod = 0
	}
	mods := make([]int32, capMod+1)
	var stability C.double
	var nMod C.int64_t
	p := ke.cParams()
	if rc := C.sonar_key_sequence(ke.x.c, f64p(flat), C.int64_t(frames), C.int32_t(dim), &p, i32p(o.key), i32p(o.mode),
		i32p(o.known), f64p(o.confidence), f64p(o.strength), f64p(o.clarity), f64p(o.ambiguity), f64p(o.tonality),
		f64p(o.scores), f64p(o.processed), &stability, i32p(mods), &nMod, 0); rc != C.SONAR_OK {
		return KeyEstimationResult{}, ke.x.err(rc)
	}
	// the candidates of the average row: the scores sorted as the library sorts them
	o.candidates = sortedCodes(o.scores[:24], o.nc)
	res := ke.result(o, 0)
	ke.track(res)
	res.Stability = float64(stability)
	if frames > 10 { // :265-267: nil at 10 frames or fewer, else a slice, possibly empty
		res.Modulations = make([]int, int(nMod))
		for k := range res.Modulations {
			res.Modulations[k] = int(mods[k])
		}
	}
	return res, nil
}

// sortedCodes orders the 24 codes by score, descending, equal scores in creation order (the library's
// rule for what sort.Slice leaves open), and keeps the first n.
func sortedCodes(scores []float64, n int) []int32 {
	out := make([]int32, 0, 25)
	for rank := 0; rank < 24 && len(out) < n; rank++ {
		for c := 0; c < 24; c++ {
			sc := scores[(c%2)*12+c/2]
			before := 0
			for d := 0; d < 24; d++ {
				sd := scores[(d%2)*12+d/2]
				if sd > sc || (sd == sc && d < c) {
					before++
				}
			}
			if before == rank {
				out = append(out, int32(c))
			}
		}
	}
	return append(out, 0)
}

// Reset, GetParameters, SetParameters, GetKeyHistory = the reference's (:1008-1027).
func (ke *KeyEstimator) Reset()                                      { ke.keyHistory = []KeyCandidate{} }
func (ke *KeyEstimator) GetParameters() KeyEstimationParams          { return ke.params }
func (ke *KeyEstimator) SetParameters(params KeyEstimationParams)    { ke.params = params }
func (ke *KeyEstimator) GetKeyHistory() []KeyCandidate               { return ke.keyHistory }

// KeyTransition = tonal.KeyTransition (:992-1000).
type KeyTransition struct {
	FromKey        int
	FromMode       KeyMode
	ToKey          int
	ToMode         KeyMode
	Frame          int
	Confidence     float64
	TransitionType string
}

var transitionNames = []string{"same_key", "parallel", "relative", "dominant", "subdominant", "distant"}

// AnalyzeKeyTransition = tonal.AnalyzeKeyTransition (:843-894).
func AnalyzeKeyTransition(fromKey int, fromMode KeyMode, toKey int, toMode KeyMode) map[string]interface{} {
	var t, semis, fifths C.int32_t
	var strength C.double
	C.sonar_key_transition(C.int32_t(fromKey), C.int32_t(fromMode), C.int32_t(toKey), C.int32_t(toMode), &t, &semis,
		&fifths, &strength)
	return map[string]interface{}{"semitone_distance": int(semis), "transition_type": transitionNames[int(t)],
		"fifths_distance": int(fifths), "transition_strength": float64(strength)}
}

// KeyEstimationBatch mirrors tonal.KeyEstimationBatch (:897-900).  One ProcessBatch call computes the
// per-frame results, the global key and the progression together; GetGlobalKey and GetKeyProgression
// return what it left.
type KeyEstimationBatch struct {
	estimator   *KeyEstimator
	results     []KeyEstimationResult
	global      KeyEstimationResult
	transitions []KeyTransition
}

// NewKeyEstimationBatch = tonal.NewKeyEstimationBatch (:903-908).
func (x *Context) NewKeyEstimationBatch(sampleRate int) *KeyEstimationBatch {
	return &KeyEstimationBatch{estimator: x.NewKeyEstimator(sampleRate), results: []KeyEstimationResult{}}
}

// ProcessBatch = KeyEstimationBatch.ProcessBatch (:911-920).
func (keb *KeyEstimationBatch) ProcessBatch(chromaSequence [][]float64) ([]KeyEstimationResult, error) {
	ke := keb.estimator
	frames := len(chromaSequence)
	keb.results, keb.global, keb.transitions = []KeyEstimationResult{}, KeyEstimationResult{}, []KeyTransition{}
	if frames == 0 {
		return keb.results, nil
	}
	flat, dim := flatten(chromaSequence)
	o := newFrameOut(frames, ke.params)
	tFrame, tFrom, tTo, tType := make([]int32, frames), make([]int32, frames), make([]int32, frames), make([]int32, frames)
	tConf := make([]float64, frames)
	var code C.int32_t
	var conf, strength C.double
	var nTrans C.int64_t
	p := ke.cParams()
	if rc := C.sonar_key_batch(ke.x.c, f64p(flat), C.int64_t(frames), C.int32_t(dim), &p, i32p(o.key), i32p(o.mode),
		i32p(o.known), f64p(o.confidence), f64p(o.strength), f64p(o.clarity), f64p(o.ambiguity), f64p(o.tonality),
		f64p(o.scores), i32p(o.candidates), f64p(o.processed), &code, &conf, &strength, nil, i32p(tFrame), i32p(tFrom),
		i32p(tTo), f64p(tConf), i32p(tType), &nTrans, 0); rc != C.SONAR_OK {
		return nil, ke.x.err(rc)
	}
	keb.results = make([]KeyEstimationResult, frames)
	for t := range keb.results {
		keb.results[t] = ke.result(o, t)
		ke.track(keb.results[t])
	}
	name := "" // no vote: the map's zero key (:940)
	if code >= 0 {
		name = GetKeyName(int(code)/2, KeyMode(int(code)%2))
	}
	keb.global = KeyEstimationResult{KeyName: name, Confidence: float64(conf), Strength: float64(strength),
		Method: "Batch Voting"}
	for k := 0; k < int(nTrans); k++ {
		keb.transitions = append(keb.transitions, KeyTransition{FromKey: int(tFrom[k]) / 2, FromMode: KeyMode(tFrom[k] % 2),
			ToKey: int(tTo[k]) / 2, ToMode: KeyMode(tTo[k] % 2), Frame: int(tFrame[k]), Confidence: tConf[k],
			TransitionType: transitionNames[int(tType[k])]})
	}
	return keb.results, nil
}

// GetGlobalKey = KeyEstimationBatch.GetGlobalKey (:923-959); among equal votes the lowest key*2 + mode
// wins (the reference iterates a map).
func (keb *KeyEstimationBatch) GetGlobalKey() KeyEstimationResult { return keb.global }

// GetKeyProgression = KeyEstimationBatch.GetKeyProgression (:962-989).
func (keb *KeyEstimationBatch) GetKeyProgression() []KeyTransition { return keb.transitions }

// EstimateKeySequenceDevice is EstimateKeySequence's numeric side on device memory: chroma (frames x
// dim float64), for example the profile HPCP.ComputeFromSpectrumDevice left there, and every output
// are device addresses; any output may be nil (include/sonar_gpu.h).
func (ke *KeyEstimator) EstimateKeySequenceDevice(chroma unsafe.Pointer, frames, dim int, key, mode, known, confidence,
	strength, clarity, ambiguity, tonality, scores, processed, stability, modulations, nModulations unsafe.Pointer) error {
	p := ke.cParams()
	if rc := C.sonar_key_sequence(ke.x.c, (*C.double)(chroma), C.int64_t(frames), C.int32_t(dim), &p, (*C.int32_t)(key),
		(*C.int32_t)(mode), (*C.int32_t)(known), (*C.double)(confidence), (*C.double)(strength), (*C.double)(clarity),
		(*C.double)(ambiguity), (*C.double)(tonality), (*C.double)(scores), (*C.double)(processed), (*C.double)(stability),
		(*C.int32_t)(modulations), (*C.int64_t)(nModulations), 1); rc != C.SONAR_OK {
		return ke.x.err(rc)
	}
	return nil
}

// ---- ChordDetector (algorithms/tonal/chord_detection.go) ----------------------------------------

// ChordDetectionMethod, ChordQuality and ChordInversion carry the reference's values (:16-67).
type ChordDetectionMethod int

const (
	ChordTemplateMatching ChordDetectionMethod = iota
	ChordHarmonicAnalysis
	ChordCQTBased
	ChordStatistical
	ChordMLBased
	ChordHybrid
)

type ChordQuality int

const (
	ChordMajor ChordQuality = iota
	ChordMinor
	ChordDiminished
	ChordAugmented
	ChordSus2
	ChordSus4
	ChordMaj7
	ChordMin7
	ChordDom7
	ChordMinMaj7
	ChordAug7
	ChordDim7
	ChordHalfDim7
	ChordAdd9
	ChordMaj9
	ChordMin9
	ChordDom9
	ChordMaj11
	ChordMin11
	ChordDom11
	ChordMaj13
	ChordMin13
	ChordDom13
	ChordPowerChord
	ChordUnknown
)

type ChordInversion int

const (
	ChordRoot ChordInversion = iota
	ChordFirst
	ChordSecond
	ChordThird
	ChordFourth
)

var chordQualityNames = []string{"major", "minor", "diminished", "augmented", "sus2", "sus4", "major7", "minor7",
	"dominant7", "minor-major7", "augmented7", "diminished7", "half-diminished7", "add9", "major9", "minor9",
	"dominant9", "major11", "minor11", "dominant11", "major13", "minor13", "dominant13", "power", "unknown"}

// the templates in the library's slot order (slot = t*12 + root): quality, intervals, consonance (:268-367)
var chordSlotQuality = []ChordQuality{ChordMajor, ChordMinor, ChordDiminished, ChordAugmented, ChordSus2, ChordSus4,
	ChordMaj7, ChordMin7, ChordDom7, ChordPowerChord}
var chordSlotIntervals = [][]int{{0, 4, 7}, {0, 3, 7}, {0, 3, 6}, {0, 4, 8}, {0, 2, 7}, {0, 5, 7}, {0, 4, 7, 11},
	{0, 3, 7, 10}, {0, 4, 7, 10}, {0, 7}}
var chordSlotConsonance = []float64{0.9, 0.85, 0.3, 0.4, 0.6, 0.6, 0.8, 0.75, 0.7, 0.8}
var chordRoles = []string{"", "tonic", "subdominant", "dominant", "leading_tone", "other"}
var chordMethodNames = []string{"template_matching", "harmonic_analysis", "cqt_based", "statistical", "ml_based", "hybrid"}

// GetChordQualityName = tonal.GetChordQualityName (:1053-1086).
func GetChordQualityName(quality ChordQuality) string {
	if quality >= 0 && int(quality) < len(chordQualityNames) {
		return chordQualityNames[quality]
	}
	return "unknown"
}

// GetSupportedChordQualities = tonal.GetSupportedChordQualities (:1089-1098).
func GetSupportedChordQualities() []string { return append([]string{}, chordQualityNames[:24]...) }

// GetSupportedDetectionMethods = tonal.GetSupportedDetectionMethods (:1101-1106).
func GetSupportedDetectionMethods() []string { return append([]string{}, chordMethodNames...) }

func chordMethodName(m ChordDetectionMethod) string { // getMethodName (:975-989)
	if m >= 0 && int(m) < len(chordMethodNames) {
		return chordMethodNames[m]
	}
	return "unknown"
}

func getNoteName(note int) string { // getNoteName (:944-947)
	return []string{"C", "C#", "D", "D#", "E", "F", "F#", "G", "G#", "A", "A#", "B"}[note%12]
}

// getChordName (:949-973): a quality without a template reads "unknown".
func getChordName(root int, quality ChordQuality, inversion ChordInversion) string {
	name := "unknown"
	for _, q := range chordSlotQuality {
		if q == quality {
			name = chordQualityNames[q]
		}
	}
	out := getNoteName(root)
	if name != "major" {
		out += name
	}
	if inversion > ChordRoot && int(inversion) < 5 {
		out += []string{"", "/1st", "/2nd", "/3rd", "/4th"}[inversion]
	}
	return out
}

// ChordCandidate = tonal.ChordCandidate (:70-80).  Salience is never set by the reference.
type ChordCandidate struct {
	Root       int
	Quality    ChordQuality
	Inversion  ChordInversion
	RootName   string
	ChordName  string
	Confidence float64
	Strength   float64
	Salience   float64
	Method     string
}

// ChordDetectionResult = tonal.ChordDetectionResult (:83-133), the fields the reference fills.
// Extensions holds the raw intervals 10, 11, 2, 5, 9 in that order (the reference appends them in the
// order of a map iteration, DESIGN.md F57); ProcessTime is 0.
type ChordDetectionResult struct {
	Root           int
	Quality        ChordQuality
	Inversion      ChordInversion
	RootName       string
	ChordName      string
	Confidence     float64
	Strength       float64
	Candidates     []ChordCandidate
	ChromaVector   []float64
	BassNote       int
	BassConfidence float64
	Clarity        float64
	Ambiguity      float64
	Consonance     float64
	Tension        float64
	Stability      float64
	TemplateScores []float64
	FunctionalRole string
	Extensions     []int
	Alterations    []int
	AddedNotes     []int
	Method         string
	ProcessTime    float64
	ChromaSize     int
}

// ChordDetectionParams = tonal.ChordDetectionParams (:136-175), every field kept for source compatibility.
// MinConfidence, TemplateStrength, UseHarmonics, WeightHarmonics, DetectAlterations, UseVoiceLeading,
// ContextWeight, ModelPath, UseEnsemble and EnsembleWeights are never read (DESIGN.md F51); BassFreqRange is
// read by detectBassNote only, which stays with the caller.
type ChordDetectionParams struct {
	Method                ChordDetectionMethod
	ChromaSize            int
	UseHarmonics          bool
	WeightHarmonics       bool
	NormalizeTemplates    bool
	TemplateStrength      float64
	UseInversions         bool
	MinConfidence         float64
	MaxCandidates         int
	MinChordStrength      float64
	UseBassDetection      bool
	BassFreqRange         [2]float64
	BassWeight            float64
	DetectExtensions      bool
	DetectAlterations     bool
	MaxExtension          int
	UseTemporalSmoothing  bool
	TemporalWindow        int
	UseFunctionalAnalysis bool
	UseVoiceLeading       bool
	ContextWeight         float64
	ModelPath             string
	UseEnsemble           bool
	EnsembleWeights       []float64
}

// ChordDetector mirrors tonal.ChordDetector (:190-214).  chordHistory is kept as the set of slots the
// reference's aliased slice holds after a call; confidenceHistory as the reference keeps it.
type ChordDetector struct {
	x                 *Context
	params            ChordDetectionParams
	sampleRate        int
	chordHistory      map[int]bool
	confidenceHistory []float64
}

// NewChordDetector = tonal.NewChordDetector (:217-244).
func (x *Context) NewChordDetector(sampleRate int) *ChordDetector {
	return x.NewChordDetectorWithParams(sampleRate, ChordDetectionParams{Method: ChordTemplateMatching, ChromaSize: 12,
		UseHarmonics: true, NormalizeTemplates: true, TemplateStrength: 1.0, UseInversions: true, MinConfidence: 0.26,
		MaxCandidates: 5, MinChordStrength: 0.2, UseBassDetection: true, BassFreqRange: [2]float64{80.0, 350.0},
		BassWeight: 0.3, DetectExtensions: true, MaxExtension: 13, UseTemporalSmoothing: true, TemporalWindow: 5,
		ContextWeight: 0.1})
}

// NewChordDetectorWithParams = tonal.NewChordDetectorWithParams (:247-265).
func (x *Context) NewChordDetectorWithParams(sampleRate int, params ChordDetectionParams) *ChordDetector {
	return &ChordDetector{x: x, params: params, sampleRate: sampleRate, chordHistory: map[int]bool{}}
}

func (cd *ChordDetector) cParams() C.sonar_chord_params {
	b := func(v bool) C.int32_t {
		if v {
			return 1
		}
		return 0
	}
	p := cd.params
	return C.sonar_chord_params{method: C.int32_t(p.Method), normalize_templates: b(p.NormalizeTemplates),
		use_inversions: b(p.UseInversions), max_candidates: C.int32_t(p.MaxCandidates),
		use_bass_detection: b(p.UseBassDetection), detect_extensions: b(p.DetectExtensions),
		max_extension: C.int32_t(p.MaxExtension), use_temporal_smoothing: b(p.UseTemporalSmoothing),
		temporal_window: C.int32_t(p.TemporalWindow), use_functional_analysis: b(p.UseFunctionalAnalysis),
		min_chord_strength: C.double(p.MinChordStrength), bass_weight: C.double(p.BassWeight)}
}

// chordOut holds the outputs of one call over frames rows with mc candidate columns.
type chordOut struct {
	root, quality, inversion, nFound, ext, role, cand, candInv               []int32
	conf, strength, clarity, ambiguity, consonance, tension, stability       []float64
	scores, candConf, candStrength, hpcp                                     []float64
	mc                                                                       int
}

func newChordOut(frames, mc int) (*chordOut, C.sonar_chord_out) {
	if mc < 0 {
		mc = 0 // the call reports the panic
	}
	f := func(n int) []float64 { return make([]float64, n+1) }
	i := func(n int) []int32 { return make([]int32, n+1) }
	o := &chordOut{root: i(frames), quality: i(frames), inversion: i(frames), nFound: i(frames), ext: i(frames),
		role: i(frames), cand: i(frames * mc), candInv: i(frames * mc), conf: f(frames), strength: f(frames),
		clarity: f(frames), ambiguity: f(frames), consonance: f(frames), tension: f(frames), stability: f(frames),
		scores: f(frames * 120), candConf: f(frames * mc), candStrength: f(frames * mc), hpcp: f(frames * 12), mc: mc}
	return o, C.sonar_chord_out{root: i32p(o.root), quality: i32p(o.quality), inversion: i32p(o.inversion),
		n_found: i32p(o.nFound), confidence: f64p(o.conf), strength: f64p(o.strength), clarity: f64p(o.clarity),
		ambiguity: f64p(o.ambiguity), consonance: f64p(o.consonance), tension: f64p(o.tension),
		stability: f64p(o.stability), extensions: i32p(o.ext), role: i32p(o.role), template_scores: f64p(o.scores),
		candidates: i32p(o.cand), cand_inversion: i32p(o.candInv), cand_confidence: f64p(o.candConf),
		cand_strength: f64p(o.candStrength)}
}

func (cd *ChordDetector) candidate(slot int, inv int32, conf, strength float64) ChordCandidate {
	root, q := slot%12, chordSlotQuality[slot/12]
	return ChordCandidate{Root: root, Quality: q, Inversion: ChordInversion(inv), RootName: getNoteName(root),
		ChordName: getChordName(root, q, ChordInversion(inv)), Confidence: conf, Strength: strength,
		Method: "template_matching"}
}

func chordExtensions(mask int32) []int {
	out := []int{}
	for _, iv := range []int{10, 11, 2, 5, 9} {
		if mask>>uint(iv)&1 != 0 {
			out = append(out, iv)
		}
	}
	return out
}

// result rebuilds frame t's ChordDetectionResult from the library's numbers (DetectChord :462-497).
func (cd *ChordDetector) result(o *chordOut, t int, chroma []float64, bassNote int, bassConf float64) ChordDetectionResult {
	r := ChordDetectionResult{ChromaVector: chroma, BassNote: bassNote, BassConfidence: bassConf,
		TemplateScores: o.scores[t*120 : (t+1)*120 : (t+1)*120], Method: chordMethodName(cd.params.Method),
		ChromaSize: cd.params.ChromaSize, Candidates: []ChordCandidate{}}
	for k := 0; k < o.mc && o.cand[t*o.mc+k] >= 0; k++ {
		r.Candidates = append(r.Candidates, cd.candidate(int(o.cand[t*o.mc+k]), o.candInv[t*o.mc+k], o.candConf[t*o.mc+k],
			o.candStrength[t*o.mc+k]))
	}
	if len(r.Candidates) == 0 {
		return r
	}
	best := r.Candidates[0]
	r.Root, r.Quality, r.Inversion, r.RootName, r.ChordName = best.Root, best.Quality, best.Inversion, best.RootName, best.ChordName
	r.Confidence, r.Strength = o.conf[t], o.strength[t]
	r.Clarity, r.Ambiguity, r.Consonance, r.Tension, r.Stability = o.clarity[t], o.ambiguity[t], o.consonance[t], o.tension[t], o.stability[t]
	if cd.params.DetectExtensions {
		r.Extensions, r.Alterations, r.AddedNotes = chordExtensions(o.ext[t]), []int{}, []int{}
	}
	r.FunctionalRole = chordRoles[o.role[t]]
	return r
}

// DetectChords runs a fresh detector with this detector's parameters over every frame of frameLen
// samples at hop, in order (sonar_chord_detect): result t is what the t-th DetectChord of a new
// NewChordDetectorWithParams returns.  The receiver's own history is neither read nor changed.
// bassNotes / bassConfidences (nil, or one per frame) are what detectBassNote returns; they are read
// at frameLen 1024 only, the one length DetectPitch accepts (DESIGN.md F53).
func (cd *ChordDetector) DetectChords(audioData []float64, frameLen, hop int, bassNotes []int32,
	bassConfidences []float64) ([]ChordDetectionResult, error) {
	if cd.params.ChromaSize != 12 {
		if cd.params.ChromaSize == 24 || cd.params.ChromaSize == 36 {
			return nil, fmt.Errorf("sonargpu: ChromaSize %d on PCM: %w", cd.params.ChromaSize, ErrUnsupported)
		}
		return nil, fmt.Errorf("failed to extract chroma features: unsupported chroma size: %d", cd.params.ChromaSize)
	}
	if frameLen <= 0 || hop <= 0 || len(audioData) < frameLen {
		return []ChordDetectionResult{}, nil
	}
	frames := (len(audioData)-frameLen)/hop + 1
	o, co := newChordOut(frames, cd.params.MaxCandidates)
	p := cd.cParams()
	var bn *C.int32_t
	var bc *C.double
	if bassNotes != nil && bassConfidences != nil && frameLen == 1024 {
		bn, bc = i32p(bassNotes), f64p(bassConfidences)
	}
	var got C.int64_t
	if rc := C.sonar_chord_detect(cd.x.c, f64p(audioData), C.int64_t(len(audioData)), C.int32_t(cd.sampleRate),
		C.int32_t(frameLen), C.int32_t(hop), bn, bc, &p, &co, f64p(o.hpcp), &got, 0); rc != C.SONAR_OK {
		return nil, cd.x.err(rc)
	}
	out := make([]ChordDetectionResult, frames)
	for t := range out {
		note, conf := 0, 0.0
		if bn != nil && cd.params.UseBassDetection {
			note, conf = int(bassNotes[t]), bassConfidences[t]
		}
		out[t] = cd.result(o, t, o.hpcp[t*12:(t+1)*12:(t+1)*12], note, conf)
	}
	return out, nil
}

// DetectChordFromChroma is DetectChord from templateMatching on (:428-502) for one chroma row and the
// bass pair detectBassNote returned, with this detector's history: the row's candidates come from
// sonar_chord_frames (all of them, unboosted), and applyTemporalSmoothing (:783-806), the stable sort,
// the cut, the metrics that depend on them and updateTemporalTracking (:919-926) are replayed here on
// the at most 120 candidates, as tests/chord_ref.py states them.
func (cd *ChordDetector) DetectChordFromChroma(chroma []float64, bassNote int, bassConfidence float64) (ChordDetectionResult, error) {
	p := cd.cParams()
	if cd.params.MaxCandidates >= 0 {
		p.max_candidates = 120
	}
	p.use_temporal_smoothing = 0
	o, co := newChordOut(1, int(p.max_candidates))
	note, conf := []int32{int32(bassNote), 0}, []float64{bassConfidence, 0}
	if rc := C.sonar_chord_frames(cd.x.c, f64p(append(append([]float64{}, chroma...), 0)), 1, C.int32_t(len(chroma)),
		i32p(note), f64p(conf), &p, &co, 0); rc != C.SONAR_OK {
		return ChordDetectionResult{}, cd.x.err(rc)
	}
	if !cd.params.UseBassDetection {
		bassNote, bassConfidence = 0, 0.0
	}
	all := cd.result(o, 0, chroma, bassNote, bassConfidence)
	cands := all.Candidates
	slotOf := func(c ChordCandidate) int {
		for t, q := range chordSlotQuality {
			if q == c.Quality {
				return t*12 + c.Root
			}
		}
		return -1
	}
	sort.SliceStable(cands, func(i, j int) bool { return slotOf(cands[i]) < slotOf(cands[j]) }) // creation order
	if cd.params.UseTemporalSmoothing {
		first := len(cd.chordHistory) == 0
		if !first {
			for i := range cands {
				if cd.chordHistory[slotOf(cands[i])] {
					cands[i].Confidence = math.Min(cands[i].Confidence*1.1, 1.0)
				}
			}
		}
		sort.SliceStable(cands, func(i, j int) bool { return cands[i].Confidence > cands[j].Confidence })
		if !first && len(cands) == 0 && cd.params.TemporalWindow < 0 {
			return ChordDetectionResult{}, fmt.Errorf("runtime error: slice bounds out of range [1:0]: %w", ErrPanic)
		}
		cd.chordHistory = map[int]bool{}
		for i, c := range cands {
			if i == 0 && !first && len(cands) > cd.params.TemporalWindow {
				continue // the history drops the sorted slice's first entry (:801-803, F52)
			}
			cd.chordHistory[slotOf(c)] = true
		}
	} else {
		sort.SliceStable(cands, func(i, j int) bool { return cands[i].Confidence > cands[j].Confidence })
	}
	if len(cands) > cd.params.MaxCandidates {
		cands = cands[:cd.params.MaxCandidates]
	}
	r := ChordDetectionResult{ChromaVector: chroma, BassNote: bassNote, BassConfidence: bassConfidence, Candidates: cands,
		TemplateScores: all.TemplateScores, Method: all.Method, ChromaSize: cd.params.ChromaSize}
	if len(cands) == 0 {
		return r, nil
	}
	best := cands[0]
	r.Root, r.Quality, r.Inversion, r.RootName, r.ChordName = best.Root, best.Quality, best.Inversion, best.RootName, best.ChordName
	r.Confidence, r.Strength = best.Confidence, best.Strength
	r.Clarity = best.Confidence
	if len(cands) > 1 {
		r.Clarity = cands[0].Confidence - cands[1].Confidence
	}
	r.Ambiguity = 1.0 - r.Clarity
	r.Consonance = chordSlotConsonance[slotOf(best)/12]
	r.Stability = r.Confidence
	if n := len(cd.confidenceHistory); n > 0 { // calculateVariance (:991-1010)
		mean, variance := 0.0, 0.0
		for _, v := range cd.confidenceHistory {
			mean += v
		}
		mean /= float64(n)
		for _, v := range cd.confidenceHistory {
			d := v - mean
			variance += d * d
		}
		variance /= float64(n)
		r.Stability = math.Max(0.0, 1.0-variance)
	}
	r.Tension = all.Tension // of the raw row, whichever candidate is first
	if cd.params.DetectExtensions { // analyzeExtensions (:840-894) for the first candidate after the boost
		r.Extensions, r.Alterations, r.AddedNotes = []int{}, []int{}, []int{}
		for _, iv := range []int{10, 11, 2, 5, 9} {
			tone := false
			for _, ci := range chordSlotIntervals[slotOf(best)/12] {
				tone = tone || ci == iv
			}
			num := map[int]int{2: 9, 5: 11, 9: 13}[iv]
			if chroma[(best.Root+iv)%12] > 0.3 && !tone && (iv >= 10 || cd.params.MaxExtension >= num) {
				r.Extensions = append(r.Extensions, iv)
			}
		}
	}
	if cd.params.UseFunctionalAnalysis { // analyzeFunctionalRole (:896-917)
		switch best.Quality {
		case ChordMajor:
			r.FunctionalRole = "tonic"
		case ChordMinor:
			r.FunctionalRole = "subdominant"
		case ChordDom7:
			r.FunctionalRole = "dominant"
		case ChordDiminished:
			r.FunctionalRole = "leading_tone"
		default:
			r.FunctionalRole = "other"
		}
	}
	cd.confidenceHistory = append(cd.confidenceHistory, best.Confidence)
	if len(cd.confidenceHistory) > cd.params.TemporalWindow {
		cd.confidenceHistory = cd.confidenceHistory[1:]
	}
	return r, nil
}

// DetectChord = ChordDetector.DetectChord (:408-503) for ChromaSize 12: extractChromaFeatures through
// sonar_chord_detect on the one frame (its first min(2048, len) samples, unwindowed, DESIGN.md F56),
// then DetectChordFromChroma with this detector's history.  The bass is (0, 0.0): DetectPitch rejects
// every frame that is not 1024 samples long (F53); for those frames, detect the bass with the
// PitchDetector and call DetectChordFromChroma.
func (cd *ChordDetector) DetectChord(audioData []float64) (ChordDetectionResult, error) {
	fresh := cd.x.NewChordDetectorWithParams(cd.sampleRate, cd.params)
	fresh.params.UseBassDetection = false
	rows, err := fresh.DetectChords(audioData, len(audioData), 1, nil, nil)
	if err != nil {
		return ChordDetectionResult{}, fmt.Errorf("failed to extract chroma features: %w", err)
	}
	if len(rows) != 1 {
		return ChordDetectionResult{}, fmt.Errorf("sonargpu: empty audio frame: %w", ErrUnsupported)
	}
	return cd.DetectChordFromChroma(rows[0].ChromaVector, 0, 0.0)
}

// DetectChordsFromChroma = one fresh detector fed the chroma rows in order (sonar_chord_sequence), as
// DetectChords; bassNotes / bassConfidences are nil or one per row.
func (cd *ChordDetector) DetectChordsFromChroma(chroma [][]float64, bassNotes []int32, bassConfidences []float64) ([]ChordDetectionResult, error) {
	frames := len(chroma)
	if frames == 0 {
		return []ChordDetectionResult{}, nil
	}
	flat, dim := flatten(chroma)
	o, co := newChordOut(frames, cd.params.MaxCandidates)
	p := cd.cParams()
	var bn *C.int32_t
	var bc *C.double
	if bassNotes != nil && bassConfidences != nil {
		bn, bc = i32p(bassNotes), f64p(bassConfidences)
	}
	if rc := C.sonar_chord_sequence(cd.x.c, f64p(flat), C.int64_t(frames), C.int32_t(dim), bn, bc, &p, &co, 0); rc != C.SONAR_OK {
		return nil, cd.x.err(rc)
	}
	out := make([]ChordDetectionResult, frames)
	for t := range out {
		note, conf := 0, 0.0
		if bn != nil && cd.params.UseBassDetection {
			note, conf = int(bassNotes[t]), bassConfidences[t]
		}
		out[t] = cd.result(o, t, chroma[t], note, conf)
	}
	return out, nil
}

// ChordProgressionAnalyzer = tonal.ChordProgressionAnalyzer (:1109-1173).
type ChordProgressionAnalyzer struct {
	x        *Context
	detector *ChordDetector
	chords   []ChordDetectionResult
}

// NewChordProgressionAnalyzer = tonal.NewChordProgressionAnalyzer (:1115-1120).
func (x *Context) NewChordProgressionAnalyzer(sampleRate int) *ChordProgressionAnalyzer {
	return &ChordProgressionAnalyzer{x: x, detector: x.NewChordDetector(sampleRate), chords: []ChordDetectionResult{}}
}

// AddChord = ChordProgressionAnalyzer.AddChord (:1123-1125).
func (cpa *ChordProgressionAnalyzer) AddChord(result ChordDetectionResult) { cpa.chords = append(cpa.chords, result) }

// AnalyzeProgression = ChordProgressionAnalyzer.AnalyzeProgression (:1128-1173): num_chords, transitions,
// average_confidence and most_common_quality (among equal counts the lowest quality code; the reference
// iterates a map), or num_chords and analysis = "insufficient_data" below two chords.
func (cpa *ChordProgressionAnalyzer) AnalyzeProgression() (map[string]interface{}, error) {
	n := len(cpa.chords)
	if n < 2 {
		return map[string]interface{}{"num_chords": n, "analysis": "insufficient_data"}, nil
	}
	quality, conf := make([]int32, n), make([]float64, n)
	transitions := make([]string, 0, n-1)
	for i, c := range cpa.chords {
		quality[i], conf[i] = int32(c.Quality), c.Confidence
		if i > 0 {
			transitions = append(transitions, fmt.Sprintf("%s -> %s", cpa.chords[i-1].ChordName, c.ChordName))
		}
	}
	var num C.int64_t
	var insufficient, most C.int32_t
	var avg C.double
	if rc := C.sonar_chord_progression(cpa.x.c, nil, i32p(quality), nil, f64p(conf), C.int64_t(n), &num, &insufficient,
		&avg, &most, 0); rc != C.SONAR_OK {
		return nil, cpa.x.err(rc)
	}
	return map[string]interface{}{"num_chords": int(num), "transitions": transitions, "average_confidence": float64(avg),
		"most_common_quality": GetChordQualityName(ChordQuality(most))}, nil
}

// ---- PitchDetector seam (algorithms/tonal/pitch_detection.go): NewPitchDetector,
// NewPitchDetectorWithParams, DetectPitch, ProcessAudioStream, Reset, AnalyzePitchStability and
// GetPitchDetectionMethodName through sonar_pitch_frames_raw, sonar_pitch_track, sonar_pitch_detect and
// sonar_pitch_stability.  The library returns numbers; this file rebuilds PitchDetectionResult with
// the method strings of its candidates.  Candidates holds at most 8 entries (SONAR_PITCH's
// max_candidates limit): the reference returns every peak, the best 8 by confidence are kept here, and
// equal confidences are ordered by ascending lag where Go's sort.Slice leaves the order open.
// Harmonics, SNR, HarmonicRatio and ProcessTime are never set by the reference and stay zero.

// PitchDetectionMethod carries the reference's values (:16-35), which are SONAR_PITCH_*.
type PitchDetectionMethod int

const (
	AutocorrelationYin PitchDetectionMethod = iota
	AutocorrelationACF
	AutocorrelationNSDF
	FrequencyDomainHPS
	FrequencyDomainCepstrum
	FrequencyDomainPeaks
	TimeDomainZeroCrossing
	TimeDomainPeakPicking
	HybridYinFFT
	HybridMPM
	HybridPRAATT
)

const pitchMaxCandidates = 8

// PitchCandidate = tonal.PitchCandidate (:38-44).
type PitchCandidate struct {
	Frequency  float64
	Confidence float64
	Salience   float64
	Harmonic   int
	Method     string
}

// PitchDetectionResult = tonal.PitchDetectionResult (:47-81).
type PitchDetectionResult struct {
	Pitch, Confidence, Salience, Voicing  float64
	Candidates                            []PitchCandidate
	Stability, Periodicity                float64
	Harmonics                             []PitchCandidate
	F0Multiple                            float64
	SNR, Clarity, Strength                float64
	YinThreshold                          float64
	AutocorrPeaks                         []float64
	CepstralPeak, HarmonicRatio           float64
	Method                                PitchDetectionMethod
	SampleRate, WindowSize                int
	ProcessTime                           float64
}

// PitchDetectionParams = tonal.PitchDetectionParams (:84-117).
type PitchDetectionParams struct {
	Method                                               PitchDetectionMethod
	SampleRate, WindowSize, HopSize                      int
	MinFreq, MaxFreq                                     float64
	YinThreshold, AutocorrThreshold, CepstralThreshold   float64
	MinConfidence, MinSalience, VoicingThreshold         float64
	MaxHarmonics                                         int
	HarmonicTolerance                                    float64
	PreEmphasis                                          bool
	WindowFunction                                       string
	ZeroPadding                                          int
	MedianFilter                                         int
	TemporalSmoothing, OctaveCorrection                  bool
}

// PitchDetector holds the parameters and, for DetectPitch, the raw rows seen since Reset: the
// library's tracker starts from an empty history, so a frame-by-frame caller is served by tracking
// those rows again (exact; O(frames) per call).  ProcessAudioStream on a fresh or Reset detector is one
// sonar_pitch_detect call.
type PitchDetector struct {
	x      *Context
	params PitchDetectionParams
	rawP   []float64
	rawC   []float64
	rawN   []int32
	rawS   []float64
}

// NewPitchDetector = tonal.NewPitchDetector (:159-193), through sonar_pitch_params_default.
func (x *Context) NewPitchDetector(sampleRate int) *PitchDetector {
	var p C.sonar_pitch_params
	C.sonar_pitch_params_default(&p, C.int32_t(sampleRate))
	return &PitchDetector{x: x, params: PitchDetectionParams{
		Method: PitchDetectionMethod(p.method), SampleRate: int(p.sample_rate), WindowSize: int(p.window_size),
		HopSize: int(p.hop_size), MinFreq: float64(p.min_freq), MaxFreq: float64(p.max_freq),
		YinThreshold: float64(p.yin_threshold), AutocorrThreshold: float64(p.autocorr_threshold),
		CepstralThreshold: float64(p.cepstral_threshold), MinConfidence: float64(p.min_confidence),
		MinSalience: float64(p.min_salience), VoicingThreshold: float64(p.voicing_threshold),
		MaxHarmonics: int(p.max_harmonics), HarmonicTolerance: float64(p.harmonic_tolerance),
		PreEmphasis: p.pre_emphasis != 0, WindowFunction: "hann", ZeroPadding: int(p.zero_padding),
		MedianFilter: int(p.median_filter), TemporalSmoothing: p.temporal_smoothing != 0,
		OctaveCorrection: p.octave_correction != 0}}
}

// NewPitchDetectorWithParams = tonal.NewPitchDetectorWithParams (:196-207).
func (x *Context) NewPitchDetectorWithParams(params PitchDetectionParams) *PitchDetector {
	return &PitchDetector{x: x, params: params}
}

func (pd *PitchDetector) cParams() C.sonar_pitch_params {
	p := pd.params
	win := C.int32_t(C.SONAR_PITCH_WIN_HANN) // createWindowFunction: every unknown string is Hann (:337-342)
	switch p.WindowFunction {
	case "hamming":
		win = C.SONAR_PITCH_WIN_HAMMING
	case "blackman":
		win = C.SONAR_PITCH_WIN_BLACKMAN
	case "rectangular":
		win = C.SONAR_PITCH_WIN_RECTANGULAR
	}
	return C.sonar_pitch_params{method: C.int32_t(p.Method), sample_rate: C.int32_t(p.SampleRate),
		window_size: C.int32_t(p.WindowSize), hop_size: C.int32_t(p.HopSize), min_freq: C.double(p.MinFreq),
		max_freq: C.double(p.MaxFreq), yin_threshold: C.double(p.YinThreshold),
		autocorr_threshold: C.double(p.AutocorrThreshold), cepstral_threshold: C.double(p.CepstralThreshold),
		min_confidence: C.double(p.MinConfidence), min_salience: C.double(p.MinSalience),
		voicing_threshold: C.double(p.VoicingThreshold), max_harmonics: C.int32_t(p.MaxHarmonics),
		harmonic_tolerance: C.double(p.HarmonicTolerance), pre_emphasis: b2i(p.PreEmphasis), window_function: win,
		zero_padding: C.int32_t(p.ZeroPadding), median_filter: C.int32_t(p.MedianFilter),
		temporal_smoothing: b2i(p.TemporalSmoothing), octave_correction: b2i(p.OctaveCorrection)}
}

// candidateMethod is the Method string the reference's detectPitch* writes into its candidates.
func candidateMethod(m PitchDetectionMethod) string {
	switch m {
	case AutocorrelationYin, HybridYinFFT:
		return "YIN"
	case AutocorrelationACF:
		return "ACF"
	case AutocorrelationNSDF, HybridMPM:
		return "NSDF"
	case FrequencyDomainHPS, FrequencyDomainPeaks:
		return "HPS"
	case FrequencyDomainCepstrum:
		return "Cepstrum"
	case TimeDomainZeroCrossing:
		return "ZeroCrossing"
	}
	return ""
}

// candidateFrequency turns a candidate's index back into the frequency the reference stores.
func (pd *PitchDetector) candidateFrequency(index int32, pitch float64, first bool) float64 {
	switch pd.params.Method {
	case AutocorrelationACF, AutocorrelationNSDF, HybridMPM:
		return float64(pd.params.SampleRate) / float64(index)
	}
	if first { // one candidate: the frame's own (interpolated, for YIN) pitch
		return pitch
	}
	return 0
}

// DetectPitch = PitchDetector.DetectPitch (:225-279) on one frame of WindowSize samples.
func (pd *PitchDetector) DetectPitch(audioFrame []float64) (*PitchDetectionResult, error) {
	if len(audioFrame) != pd.params.WindowSize {
		return nil, fmt.Errorf("audio frame size (%d) doesn't match window size (%d)", len(audioFrame), pd.params.WindowSize)
	}
	p := pd.cParams()
	width := int(C.sonar_pitch_curve_width(&p))
	var pitch, conf, second C.double
	var index, ncand C.int32_t
	candI := make([]int32, pitchMaxCandidates)
	candC := make([]float64, pitchMaxCandidates)
	var curve []float64
	var curveP *C.double
	if width > 0 && pd.params.Method == AutocorrelationACF {
		curve = make([]float64, width)
		curveP = f64p(curve)
	}
	if rc := C.sonar_pitch_frames_raw(pd.x.c, f64p(audioFrame), C.int64_t(len(audioFrame)), &p, pitchMaxCandidates,
		&pitch, &conf, &index, &ncand, &second, i32p(candI), f64p(candC), curveP, 0); rc != C.SONAR_OK {
		return nil, pd.x.err(rc)
	}
	pd.rawP = append(pd.rawP, float64(pitch))
	pd.rawC = append(pd.rawC, float64(conf))
	pd.rawN = append(pd.rawN, int32(ncand))
	pd.rawS = append(pd.rawS, float64(second))
	F := len(pd.rawP)
	cols := make([][]float64, 9)
	for k := range cols {
		cols[k] = make([]float64, F)
	}
	if rc := C.sonar_pitch_track(&p, C.int64_t(F), f64p(pd.rawP), f64p(pd.rawC), i32p(pd.rawN), f64p(pd.rawS),
		f64p(cols[0]), f64p(cols[1]), f64p(cols[2]), f64p(cols[3]), f64p(cols[4]), f64p(cols[5]), f64p(cols[6]),
		f64p(cols[7]), f64p(cols[8])); rc != C.SONAR_OK {
		return nil, fmt.Errorf("sonar_pitch_track: %d", int(rc))
	}
	r := pd.result(cols, F-1)
	n := int(ncand)
	if n > pitchMaxCandidates {
		n = pitchMaxCandidates
	}
	name := candidateMethod(pd.params.Method)
	for k := 0; k < n; k++ {
		r.Candidates = append(r.Candidates, PitchCandidate{Frequency: pd.candidateFrequency(candI[k], float64(pitch), k == 0),
			Confidence: candC[k], Salience: candC[k], Harmonic: 1, Method: name})
	}
	switch pd.params.Method {
	case AutocorrelationYin, HybridYinFFT:
		r.YinThreshold = pd.params.YinThreshold
	case AutocorrelationACF:
		r.AutocorrPeaks = curve
	case FrequencyDomainCepstrum:
		r.CepstralPeak = float64(index)
	}
	return r, nil
}

func (pd *PitchDetector) result(cols [][]float64, t int) *PitchDetectionResult {
	return &PitchDetectionResult{Pitch: cols[0][t], Confidence: cols[1][t], Voicing: cols[2][t], Periodicity: cols[3][t],
		Clarity: cols[4][t], Strength: cols[5][t], Salience: cols[6][t], Stability: cols[7][t], F0Multiple: cols[8][t],
		Method: pd.params.Method, SampleRate: pd.params.SampleRate, WindowSize: pd.params.WindowSize}
}

// ProcessAudioStream = PitchDetector.ProcessAudioStream (:1016-1028).  The frames continue the
// detector's history, as in the reference.
func (pd *PitchDetector) ProcessAudioStream(audioFrames [][]float64) ([]*PitchDetectionResult, error) {
	results := make([]*PitchDetectionResult, len(audioFrames))
	for i, frame := range audioFrames {
		r, err := pd.DetectPitch(frame)
		if err != nil {
			return nil, fmt.Errorf("error processing frame %d: %v", i, err)
		}
		results[i] = r
	}
	return results, nil
}

// ProcessSignal is ProcessAudioStream over the whole frames of one signal (WindowSize samples every
// HopSize) on a fresh history, in one sonar_pitch_detect call; the results carry no candidates.
func (pd *PitchDetector) ProcessSignal(pcm []float64) ([]*PitchDetectionResult, error) {
	p := pd.cParams()
	F := int(C.sonar_pitch_detect_frames(C.int64_t(len(pcm)), p.window_size, p.hop_size))
	if F == 0 {
		return []*PitchDetectionResult{}, nil
	}
	cols := make([][]float64, 9)
	for k := range cols {
		cols[k] = make([]float64, F)
	}
	var frames C.int64_t
	if rc := C.sonar_pitch_detect(pd.x.c, f64p(pcm), C.int64_t(len(pcm)), &p, f64p(cols[0]), f64p(cols[1]), f64p(cols[2]),
		f64p(cols[3]), f64p(cols[4]), f64p(cols[5]), f64p(cols[6]), f64p(cols[7]), f64p(cols[8]), &frames, 0); rc != C.SONAR_OK {
		return nil, pd.x.err(rc)
	}
	out := make([]*PitchDetectionResult, F)
	for t := range out {
		out[t] = pd.result(cols, t)
	}
	return out, nil
}

// Reset = PitchDetector.Reset (:1031-1035).
func (pd *PitchDetector) Reset() {
	pd.rawP, pd.rawC, pd.rawN, pd.rawS = nil, nil, nil, nil
}

func (pd *PitchDetector) GetParameters() PitchDetectionParams { return pd.params }
func (pd *PitchDetector) SetParameters(params PitchDetectionParams) { pd.params = params }

// AnalyzePitchStability = PitchDetector.AnalyzePitchStability (:1059-1113); the empty map for fewer
// than two voiced frames.
func (pd *PitchDetector) AnalyzePitchStability(pitchSequence []float64) map[string]float64 {
	analysis := make(map[string]float64)
	if len(pitchSequence) < 2 {
		return analysis
	}
	var out [7]C.double
	var empty C.int32_t
	if rc := C.sonar_pitch_stability(f64p(pitchSequence), C.int64_t(len(pitchSequence)), C.int32_t(pd.params.SampleRate),
		C.int32_t(pd.params.HopSize), &out[0], &empty); rc != C.SONAR_OK || empty != 0 {
		return analysis
	}
	for k, name := range []string{"mean_pitch", "pitch_std_dev", "coefficient_of_variation", "jitter", "stability",
		"vibrato_rate", "voiced_frames_ratio"} {
		analysis[name] = float64(out[k])
	}
	return analysis
}

// GetPitchDetectionMethodName = tonal.GetPitchDetectionMethodName (:1163-1190).
func GetPitchDetectionMethodName(method PitchDetectionMethod) string {
	names := []string{"YIN (Autocorrelation)", "Autocorrelation Function", "Normalized Square Difference Function",
		"Harmonic Product Spectrum", "Cepstral Analysis", "Spectral Peaks", "Zero Crossing Rate", "Peak Picking",
		"YIN-FFT Hybrid", "McLeod Pitch Method", "PRAAT Algorithm"}
	if method >= 0 && int(method) < len(names) {
		return names[method]
	}
	return "Unknown"
}

// ---- HarmonicRatioAnalyzer seam (algorithms/tonal/harmonic_ratio.go): NewHarmonicRatioAnalyzer,
// NewHarmonicRatioAnalyzerWithParams, AnalyzeSequence over the whole frames of one signal,
// GetAverageHarmonicRatio, ClassifyHarmonicRatio and EstimateVoicingQuality through sonar_hratio and its
// host-only companions.  The library returns arrays; this file rebuilds HarmonicRatioResult.

// HarmonicRatioMethod carries the reference's values (:17-24), which are SONAR_HRATIO_*.
type HarmonicRatioMethod int

const (
	HarmonicRatioHNR HarmonicRatioMethod = iota
	HarmonicRatioACF
	HarmonicRatioHPS
	HarmonicRatioComb
	HarmonicRatioSpectral
	HarmonicRatioYin
)

// HarmonicRatioParams = tonal.HarmonicRatioParams (:27-57).  AutocorrMaxLag is the argument of the
// analyzer's NewAutoCorrelation: 2048 from NewHarmonicRatioAnalyzer, WindowSize from ...WithParams.
type HarmonicRatioParams struct {
	Method                                                       HarmonicRatioMethod
	SampleRate, WindowSize, HopSize                              int
	MinFreq, MaxFreq                                             float64
	MaxHarmonics                                                 int
	HarmonicTolerance, MinPeakHeight                             float64
	PeakDetectionWidth, SpectralSmoothingLen                     int
	NoiseFloorMethod                                             string
	NoiseFloorPercentile                                         float64
	NoiseFloorSmoothingLen                                       int
	UseTemporalSmoothing                                         bool
	TemporalSmoothingLen                                         int
	UseFreqWeighting, UsePsychoacousticMask, AdaptiveThreshold   bool
	AutocorrMaxLag                                               int
}

// HarmonicPeak holds the fields of harmonic.SpectralPeak that findNearestPeak fills.
type HarmonicPeak struct {
	Frequency, Magnitude, Phase float64
	BinIndex, Harmonic          int
}

// HarmonicRatioResult = tonal.HarmonicRatioResult (:60-98); ProcessingTime is 0 as in the reference
// (getCurrentTime is a placeholder).  HarmonicFrequencies, Amplitudes and Phases are set by the HNR and
// Comb methods only, as in the reference; SpectralPeaks by the four spectral methods.
type HarmonicRatioResult struct {
	HarmonicRatio, HarmonicEnergy, NoiseEnergy, TotalEnergy            float64
	HarmonicFrequencies, HarmonicAmplitudes, HarmonicPhases            []float64
	F0Frequency, F0Confidence, F0Strength                              float64
	SpectralPeaks                                                      []HarmonicPeak
	NoiseFloor                                                         []float64
	SignalToNoiseRatio, Periodicity, Harmonicity, Voicing, Roughness   float64
	TemporalStability, TemporalCoherence                               float64
	Method                                                             string
	ProcessingTime                                                     float64
	NumHarmonics                                                       int
	AnalysisFreqRange                                                  [2]float64
}

// HarmonicRatioAnalyzer holds the parameters; the device work is per call.
type HarmonicRatioAnalyzer struct {
	x      *Context
	params HarmonicRatioParams
}

// NewHarmonicRatioAnalyzer = tonal.NewHarmonicRatioAnalyzer (:130-161), through sonar_hratio_params_default.
func (x *Context) NewHarmonicRatioAnalyzer(sampleRate int) *HarmonicRatioAnalyzer {
	var p C.sonar_hratio_params
	C.sonar_hratio_params_default(&p, C.int32_t(sampleRate))
	return &HarmonicRatioAnalyzer{x: x, params: HarmonicRatioParams{
		Method: HarmonicRatioMethod(p.method), SampleRate: int(p.sample_rate), WindowSize: int(p.window_size),
		HopSize: int(p.hop_size), MinFreq: float64(p.min_freq), MaxFreq: float64(p.max_freq),
		MaxHarmonics: int(p.max_harmonics), HarmonicTolerance: float64(p.harmonic_tolerance),
		MinPeakHeight: float64(p.min_peak_height), PeakDetectionWidth: int(p.peak_detection_width),
		SpectralSmoothingLen: int(p.spectral_smoothing_len), NoiseFloorMethod: "percentile",
		NoiseFloorPercentile: float64(p.noise_floor_percentile), NoiseFloorSmoothingLen: int(p.noise_floor_smoothing_len),
		UseTemporalSmoothing: p.use_temporal_smoothing != 0, TemporalSmoothingLen: int(p.temporal_smoothing_len),
		AutocorrMaxLag: int(p.autocorr_max_lag)}}
}

// NewHarmonicRatioAnalyzerWithParams = tonal.NewHarmonicRatioAnalyzerWithParams (:164-178): its
// autocorrelation is NewAutoCorrelation(WindowSize), which an AutocorrMaxLag of 0 selects.
func (x *Context) NewHarmonicRatioAnalyzerWithParams(params HarmonicRatioParams) *HarmonicRatioAnalyzer {
	if params.AutocorrMaxLag == 0 {
		params.AutocorrMaxLag = params.WindowSize
	}
	return &HarmonicRatioAnalyzer{x: x, params: params}
}

func (hra *HarmonicRatioAnalyzer) cParams() C.sonar_hratio_params {
	p := hra.params
	nf := C.int32_t(C.SONAR_HRATIO_NOISE_PERCENTILE) // estimateNoiseFloor: every unknown string is "percentile" (:640)
	switch p.NoiseFloorMethod {
	case "median":
		nf = C.SONAR_HRATIO_NOISE_MEDIAN
	case "minimum":
		nf = C.SONAR_HRATIO_NOISE_MINIMUM
	}
	return C.sonar_hratio_params{method: C.int32_t(p.Method), sample_rate: C.int32_t(p.SampleRate),
		window_size: C.int32_t(p.WindowSize), hop_size: C.int32_t(p.HopSize), min_freq: C.double(p.MinFreq),
		max_freq: C.double(p.MaxFreq), max_harmonics: C.int32_t(p.MaxHarmonics),
		harmonic_tolerance: C.double(p.HarmonicTolerance), min_peak_height: C.double(p.MinPeakHeight),
		peak_detection_width: C.int32_t(p.PeakDetectionWidth), spectral_smoothing_len: C.int32_t(p.SpectralSmoothingLen),
		noise_floor_method: nf, noise_floor_percentile: C.double(p.NoiseFloorPercentile),
		noise_floor_smoothing_len: C.int32_t(p.NoiseFloorSmoothingLen), use_temporal_smoothing: b2i(p.UseTemporalSmoothing),
		temporal_smoothing_len: C.int32_t(p.TemporalSmoothingLen), use_freq_weighting: b2i(p.UseFreqWeighting),
		use_psychoacoustic_mask: b2i(p.UsePsychoacousticMask), adaptive_threshold: b2i(p.AdaptiveThreshold),
		autocorr_max_lag: C.int32_t(p.AutocorrMaxLag)}
}

// GetHarmonicRatioMethodName = getMethodName (:1015-1032).
func GetHarmonicRatioMethodName(method HarmonicRatioMethod) string {
	names := GetSupportedHarmonicRatioMethods()
	if method >= 0 && int(method) < len(names) {
		return names[method]
	}
	return "Unknown"
}

// GetSupportedHarmonicRatioMethods = tonal.GetSupportedHarmonicRatioMethods (:1118-1127).
func GetSupportedHarmonicRatioMethods() []string {
	return []string{"Harmonic-to-Noise Ratio", "Autocorrelation Function", "Harmonic Product Spectrum", "Comb Filtering",
		"Spectral Peak Analysis", "YIN-based"}
}

// AnalyzeSignal is AnalyzeSequence (:1042-1054) over the whole frames of one signal (WindowSize samples
// every HopSize) on a fresh history, in one sonar_hratio call.
func (hra *HarmonicRatioAnalyzer) AnalyzeSignal(pcm []float64) ([]HarmonicRatioResult, error) {
	p := hra.cParams()
	F := int(C.sonar_pitch_detect_frames(C.int64_t(len(pcm)), p.window_size, p.hop_size))
	if F == 0 {
		if rc := C.sonar_hratio_check(&p); rc != C.SONAR_OK {
			return nil, fmt.Errorf("harmonic ratio: parameters refused (%d)", int(rc))
		}
		return []HarmonicRatioResult{}, nil
	}
	mh := hra.params.MaxHarmonics
	if mh < 0 {
		mh = 0
	}
	K := hra.params.WindowSize / 2
	cols := make([][]float64, 13)
	for k := range cols {
		cols[k] = make([]float64, F)
	}
	num, hbin := make([]int32, F), make([]int32, F*mh+1)
	hf, ha, hp := make([]float64, F*mh+1), make([]float64, F*mh+1), make([]float64, F*mh+1)
	floor := make([]float64, F*K)
	var frames C.int64_t
	if rc := C.sonar_hratio(hra.x.c, f64p(pcm), C.int64_t(len(pcm)), &p, f64p(cols[0]), f64p(cols[1]), f64p(cols[2]),
		f64p(cols[3]), f64p(cols[4]), f64p(cols[5]), f64p(cols[6]), f64p(cols[7]), f64p(cols[8]), f64p(cols[9]),
		f64p(cols[10]), f64p(cols[11]), f64p(cols[12]), i32p(num), i32p(hbin), f64p(hf), f64p(ha), f64p(hp), f64p(floor),
		&frames, 0); rc != C.SONAR_OK {
		return nil, hra.x.err(rc)
	}
	m := hra.params.Method
	hnr := m != HarmonicRatioACF && m != HarmonicRatioHPS && m != HarmonicRatioSpectral && m != HarmonicRatioYin
	out := make([]HarmonicRatioResult, F)
	for t := range out {
		r := &out[t]
		r.HarmonicRatio, r.TemporalStability, r.TemporalCoherence = cols[0][t], cols[1][t], cols[2][t]
		r.HarmonicEnergy, r.NoiseEnergy, r.TotalEnergy = cols[3][t], cols[4][t], cols[5][t]
		r.F0Frequency, r.F0Confidence, r.SignalToNoiseRatio = cols[6][t], cols[7][t], cols[8][t]
		r.Periodicity, r.Harmonicity, r.Voicing, r.Roughness = cols[9][t], cols[10][t], cols[11][t], cols[12][t]
		r.NumHarmonics = int(num[t])
		if m != HarmonicRatioACF && m != HarmonicRatioYin {
			r.SpectralPeaks = make([]HarmonicPeak, num[t])
			for s := range r.SpectralPeaks {
				o := t*mh + s
				// findHarmonicPeaks numbers the harmonic it looked for (:587); the library keeps the order, not the
				// number, so Harmonic is the nearest multiple of f0: the one looked for whenever the peak lies within
				// half an f0 of its target
				r.SpectralPeaks[s] = HarmonicPeak{Frequency: hf[o], Magnitude: ha[o], Phase: hp[o], BinIndex: int(hbin[o]),
					Harmonic: int(math.Round(hf[o]/r.F0Frequency)) - 1}
			}
		}
		if hnr {
			r.F0Strength = r.F0Confidence
			r.NoiseFloor = floor[t*K : (t+1)*K : (t+1)*K]
			r.HarmonicFrequencies, r.HarmonicAmplitudes, r.HarmonicPhases = hf[t*mh:t*mh+int(num[t])], ha[t*mh:t*mh+int(num[t])], hp[t*mh:t*mh+int(num[t])]
		}
		r.Method = GetHarmonicRatioMethodName(m)
		r.AnalysisFreqRange = [2]float64{hra.params.MinFreq, hra.params.MaxFreq}
	}
	return out, nil
}

func (hra *HarmonicRatioAnalyzer) GetParameters() HarmonicRatioParams       { return hra.params }
func (hra *HarmonicRatioAnalyzer) SetParameters(params HarmonicRatioParams) { hra.params = params }

// GetAverageHarmonicRatio = HarmonicRatioAnalyzer.GetAverageHarmonicRatio (:1057-1077).
func (hra *HarmonicRatioAnalyzer) GetAverageHarmonicRatio(results []HarmonicRatioResult) float64 {
	r := make([]float64, len(results))
	for i := range results {
		r[i] = results[i].HarmonicRatio
	}
	return float64(C.sonar_hratio_average(f64p(r), C.int64_t(len(r))))
}

// ClassifyHarmonicRatio = tonal.ClassifyHarmonicRatio (:1130-1142).
func ClassifyHarmonicRatio(harmonicRatio float64) string {
	return C.GoString(C.sonar_hratio_category_name(C.sonar_hratio_classify(C.double(harmonicRatio))))
}

// EstimateVoicingQuality = tonal.EstimateVoicingQuality (:1145-1148).
func EstimateVoicingQuality(harmonicRatio float64) float64 {
	return float64(C.sonar_hratio_voicing_quality(C.double(harmonicRatio)))
}

// ---- InharmonicityAnalyzer seam (algorithms/tonal/inharmonicity.go): NewInharmonicityAnalyzer,
// NewInharmonicityAnalyzerWithParams, AnalyzeSequence over the whole frames of one signal,
// GetAverageInharmonicity, ClassifyInharmonicity and EstimateInstrumentType through sonar_inharm and its
// host-only companions.  The library returns arrays; this file rebuilds InharmonicityResult.

// InharmonicityMethod carries the reference's values (:17-24), which are SONAR_INHARM_*.
type InharmonicityMethod int

const (
	InharmonicityRailsback InharmonicityMethod = iota
	InharmonicityFletcherMunson
	InharmonicitySpectralDeviation
	InharmonicityPartialTracking
	InharmonicityBeatPattern
	InharmonicityStatistical
)

// InharmonicityModel carries the reference's values (:29-34), which are SONAR_INHARM_MODEL_*.
type InharmonicityModel int

const (
	ModelString InharmonicityModel = iota
	ModelPipe
	ModelMembrane
	ModelGeneral
)

// InharmonicityParams = tonal.InharmonicityParams (:37-72).
type InharmonicityParams struct {
	Method                                                      InharmonicityMethod
	Model                                                       InharmonicityModel
	SampleRate, WindowSize, MaxHarmonics, MinHarmonics          int
	HarmonicTolerance, MinHarmonicStrength                      float64
	MinFreq, MaxFreq, FreqResolution                            float64
	ReferenceHarmonic                                           int
	WeightByAmplitude, UseLogFrequency                          bool
	StringTension, StringLength, StringStiffness                float64
	OutlierThreshold, ConfidenceLevel                           float64
	UseRobustEstimation, UseTemporalTracking                    bool
	TemporalWindow                                              int
}

// InharmonicityResult = tonal.InharmonicityResult (:75-118); ProcessingTime is 0 as in the reference
// (getCurrentTime is a placeholder).
type InharmonicityResult struct {
	Inharmonicity, InharmonicityStdDev, InharmonicityConfidence                float64
	HarmonicDeviations, HarmonicFrequencies, IdealFrequencies, HarmonicAmplitudes []float64
	HarmonicNumbers                                                            []int
	F0Frequency, F0Confidence, F0Stability                                     float64
	EstimatedStiffness, ModelFitQuality                                        float64
	ModelParameters                                                            map[string]float64
	HarmonicClarity, SpectralPurity, PartialCoherence                          float64
	RSquared, ChiSquared, PValue                                               float64
	TemporalStability, InharmonicityTrend                                      float64
	Method, Model                                                              string
	NumHarmonics                                                               int
	ProcessingTime                                                             float64
	AnalysisQuality                                                            string
}

// InharmonicityAnalyzer holds the parameters; the device work is per call.
type InharmonicityAnalyzer struct {
	x      *Context
	params InharmonicityParams
}

// NewInharmonicityAnalyzer = tonal.NewInharmonicityAnalyzer (:147-180), through sonar_inharm_params_default:
// WindowSize 4096 included, with which every frame fails as it does in the reference (DESIGN.md F100).
func (x *Context) NewInharmonicityAnalyzer(sampleRate int) *InharmonicityAnalyzer {
	var p C.sonar_inharm_params
	C.sonar_inharm_params_default(&p, C.int32_t(sampleRate))
	return &InharmonicityAnalyzer{x: x, params: InharmonicityParams{
		Method: InharmonicityMethod(p.method), Model: InharmonicityModel(p.model), SampleRate: int(p.sample_rate),
		WindowSize: int(p.window_size), MaxHarmonics: int(p.max_harmonics), MinHarmonics: int(p.min_harmonics),
		HarmonicTolerance: float64(p.harmonic_tolerance), MinHarmonicStrength: float64(p.min_harmonic_strength),
		MinFreq: float64(p.min_freq), MaxFreq: float64(p.max_freq), FreqResolution: float64(p.freq_resolution),
		ReferenceHarmonic: int(p.reference_harmonic), WeightByAmplitude: p.weight_by_amplitude != 0,
		UseLogFrequency: p.use_log_frequency != 0, StringTension: float64(p.string_tension),
		StringLength: float64(p.string_length), StringStiffness: float64(p.string_stiffness),
		OutlierThreshold: float64(p.outlier_threshold), ConfidenceLevel: float64(p.confidence_level),
		UseRobustEstimation: p.use_robust_estimation != 0, UseTemporalTracking: p.use_temporal_tracking != 0,
		TemporalWindow: int(p.temporal_window)}}
}

// NewInharmonicityAnalyzerWithParams = tonal.NewInharmonicityAnalyzerWithParams (:183-196).
func (x *Context) NewInharmonicityAnalyzerWithParams(params InharmonicityParams) *InharmonicityAnalyzer {
	return &InharmonicityAnalyzer{x: x, params: params}
}

func (ia *InharmonicityAnalyzer) cParams() C.sonar_inharm_params {
	p := ia.params
	return C.sonar_inharm_params{method: C.int32_t(p.Method), model: C.int32_t(p.Model), sample_rate: C.int32_t(p.SampleRate),
		window_size: C.int32_t(p.WindowSize), max_harmonics: C.int32_t(p.MaxHarmonics), min_harmonics: C.int32_t(p.MinHarmonics),
		harmonic_tolerance: C.double(p.HarmonicTolerance), min_harmonic_strength: C.double(p.MinHarmonicStrength),
		min_freq: C.double(p.MinFreq), max_freq: C.double(p.MaxFreq), freq_resolution: C.double(p.FreqResolution),
		reference_harmonic: C.int32_t(p.ReferenceHarmonic), weight_by_amplitude: b2i(p.WeightByAmplitude),
		use_log_frequency: b2i(p.UseLogFrequency), string_tension: C.double(p.StringTension),
		string_length: C.double(p.StringLength), string_stiffness: C.double(p.StringStiffness),
		outlier_threshold: C.double(p.OutlierThreshold), confidence_level: C.double(p.ConfidenceLevel),
		use_robust_estimation: b2i(p.UseRobustEstimation), use_temporal_tracking: b2i(p.UseTemporalTracking),
		temporal_window: C.int32_t(p.TemporalWindow)}
}

// AnalyzeSignal is AnalyzeSequence (:1181-1193) over the whole frames of one signal (WindowSize samples every
// hopSize) on a fresh analyzer, in one sonar_inharm call.  Where the reference returns nil and an error (a frame
// with too few harmonics, a window that is not the detector's 1024) so does this, with the reference's message.
func (ia *InharmonicityAnalyzer) AnalyzeSignal(pcm []float64, hopSize int) ([]InharmonicityResult, error) {
	p := ia.cParams()
	F := int(C.sonar_pitch_detect_frames(C.int64_t(len(pcm)), p.window_size, C.int32_t(hopSize)))
	if F == 0 {
		if rc := C.sonar_inharm_check(&p); rc != C.SONAR_OK {
			return nil, fmt.Errorf("inharmonicity: parameters refused (%d)", int(rc))
		}
		return []InharmonicityResult{}, nil
	}
	mh := ia.params.MaxHarmonics
	if mh < 0 {
		mh = 0
	}
	cols := make([][]float64, 16)
	for k := range cols {
		cols[k] = make([]float64, F)
	}
	status, num, ndev, quality := make([]int32, F), make([]int32, F), make([]int32, F), make([]int32, F)
	hn := make([]int32, F*mh+1)
	hf, hi, ha, hd := make([]float64, F*mh+1), make([]float64, F*mh+1), make([]float64, F*mh+1), make([]float64, F*mh+1)
	var frames, bad C.int64_t
	if rc := C.sonar_inharm(ia.x.c, f64p(pcm), C.int64_t(len(pcm)), C.int32_t(hopSize), &p, i32p(status), f64p(cols[0]),
		f64p(cols[1]), f64p(cols[2]), f64p(cols[3]), f64p(cols[4]), f64p(cols[5]), f64p(cols[6]), f64p(cols[7]), i32p(num),
		i32p(ndev), i32p(hn), f64p(hf), f64p(hi), f64p(ha), f64p(hd), f64p(cols[8]), f64p(cols[9]), f64p(cols[10]),
		f64p(cols[11]), f64p(cols[12]), f64p(cols[13]), f64p(cols[14]), f64p(cols[15]), i32p(quality), &frames, &bad,
		0); rc != C.SONAR_OK {
		return nil, ia.x.err(rc)
	}
	m, model := ia.params.Method, ia.params.Model
	out := make([]InharmonicityResult, F)
	for t := range out {
		r := &out[t]
		r.F0Frequency, r.F0Confidence = cols[6][t], cols[7][t]
		r.AnalysisQuality = C.GoString(C.sonar_inharm_quality_name(C.int32_t(quality[t])))
		if status[t] != C.SONAR_INHARM_STATUS_OK { // the early return of :236-242: nothing else is set
			continue
		}
		r.Inharmonicity, r.TemporalStability, r.InharmonicityTrend, r.F0Stability = cols[0][t], cols[1][t], cols[2][t], cols[3][t]
		r.InharmonicityStdDev, r.InharmonicityConfidence = cols[4][t], cols[5][t]
		r.EstimatedStiffness, r.ModelFitQuality = cols[8][t], cols[9][t]
		r.HarmonicClarity, r.SpectralPurity, r.PartialCoherence = cols[10][t], cols[11][t], cols[12][t]
		r.RSquared, r.ChiSquared, r.PValue = cols[13][t], cols[14][t], cols[15][t]
		r.NumHarmonics = int(num[t])
		n, nd, o := int(num[t]), int(ndev[t]), t*mh
		if hn[o] >= 0 && n > 0 && mh > 0 { // the method set the harmonic arrays
			r.HarmonicFrequencies, r.IdealFrequencies, r.HarmonicAmplitudes = hf[o:o+n:o+n], hi[o:o+n:o+n], ha[o:o+n:o+n]
			r.HarmonicDeviations = hd[o : o+nd : o+nd]
			r.HarmonicNumbers = make([]int, n)
			for s := range r.HarmonicNumbers {
				r.HarmonicNumbers[s] = int(hn[o+s])
			}
			if m == InharmonicityRailsback { // :504-507
				r.ModelParameters = map[string]float64{"railsback_coefficient": cols[0][t], "fundamental_frequency": r.F0Frequency}
			}
		}
		if model == ModelString { // :876-881
			if r.ModelParameters == nil {
				r.ModelParameters = map[string]float64{}
			}
			r.ModelParameters["string_stiffness"] = r.EstimatedStiffness
			r.ModelParameters["string_tension"] = ia.params.StringTension
			r.ModelParameters["string_length"] = ia.params.StringLength
		}
		r.Method = C.GoString(C.sonar_inharm_method_name(C.int32_t(m)))
		r.Model = C.GoString(C.sonar_inharm_model_name(C.int32_t(model)))
	}
	return out, nil
}

func (ia *InharmonicityAnalyzer) GetParameters() InharmonicityParams       { return ia.params }
func (ia *InharmonicityAnalyzer) SetParameters(params InharmonicityParams) { ia.params = params }

// GetAverageInharmonicity = InharmonicityAnalyzer.GetAverageInharmonicity (:1196-1216).
func (ia *InharmonicityAnalyzer) GetAverageInharmonicity(results []InharmonicityResult) float64 {
	v, c := make([]float64, len(results)), make([]float64, len(results))
	for i := range results {
		v[i], c[i] = results[i].Inharmonicity, results[i].InharmonicityConfidence
	}
	return float64(C.sonar_inharm_average(f64p(v), f64p(c), C.int64_t(len(v))))
}

// ClassifyInharmonicity = tonal.ClassifyInharmonicity (:1272-1286).
func ClassifyInharmonicity(inharmonicity float64) string {
	return C.GoString(C.sonar_inharm_class_name(C.sonar_inharm_classify(C.double(inharmonicity))))
}

// EstimateInstrumentType = tonal.EstimateInstrumentType (:1289-1313).
func EstimateInstrumentType(inharmonicity float64, f0 float64) string {
	return C.GoString(C.sonar_inharm_instrument_name(C.sonar_inharm_instrument_type(C.double(inharmonicity), C.double(f0))))
}
