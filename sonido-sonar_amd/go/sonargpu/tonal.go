package sonargpu

// KeyEstimator seam (algorithms/tonal/key_estimation.go): EstimateKey, EstimateKeyFromHPCP,
// EstimateKeySequence and KeyEstimationBatch through sonar_key_frames, sonar_key_sequence and
// sonar_key_batch, AnalyzeKeyTransition through sonar_key_transition.  The library returns numbers and
// codes (key*2 + mode); this file rebuilds KeyEstimationResult with its strings: the key names,
// "Unknown", KeyProfile, Method, RelatedKeys, and the last-20 history the reference keeps in the
// estimator.  The constructors are methods of Context because the object needs a device; otherwise
// the names and signatures are the reference's.
//
// Written against include/sonar_gpu.h; not compiled here (no Go toolchain in the image).

/*
#include "sonar_gpu.h"
*/
import "C"

import (
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
