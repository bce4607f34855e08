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
