package sonargpu

// ChromaCQT seam (algorithms/chroma/chroma_cqt.go): the constant-Q chromagram through
// sonar_chroma_cqt.  MusicFeatureExtractor builds one beside its ChromaSTFT (music.go:91-93) and
// the chord detector calls it on whole recordings (tonal/chord_detection.go:534, 657).  The
// constructors are methods of Context because the object needs a device; otherwise the names and
// signatures are the reference's.
//
// ChromaSequenceSimilarity (algorithms/chroma/chroma_similarity.go) follows at the end of the file,
// through sonar_chroma_similarity.
//
// Written against include/sonar_gpu.h; not compiled here (no Go toolchain in the image).

/*
#include "sonar_gpu.h"
*/
import "C"

import (
	"math"
	"unsafe"
)

// ChromaCQT mirrors chroma.ChromaCQT (:26-40).  The kernel itself lives in the library, cached in
// the context per parameter set; kernelComputed only keeps GetCQTFrequencies' behaviour (:276-284).
type ChromaCQT struct {
	x              *Context
	sampleRate     int
	minFreq        float64
	maxFreq        float64
	binsPerOctave  int
	qFactor        float64
	tuningFreq     float64
	freqBins       []float64
	kernelComputed bool
}

// NewChromaCQT = chroma.NewChromaCQT (:43-54).
func (x *Context) NewChromaCQT(sampleRate int, minFreq, maxFreq float64, binsPerOctave int, qFactor, tuningFreq float64) *ChromaCQT {
	return &ChromaCQT{x: x, sampleRate: sampleRate, minFreq: minFreq, maxFreq: maxFreq, binsPerOctave: binsPerOctave,
		qFactor: qFactor, tuningFreq: tuningFreq}
}

// NewChromaCQTDefault = chroma.NewChromaCQTDefault (:57-66): C2 to C7, semitone bins, Q 25, A4 = 440 Hz.
func (x *Context) NewChromaCQTDefault(sampleRate int) *ChromaCQT {
	return x.NewChromaCQT(sampleRate, 65.4, 2093.0, 12, 25.0, 440.0)
}

// ComputeChroma = ChromaCQT.ComputeChroma (:69-92).  An empty signal returns nil, nil as in Go.  Where
// the reference panics (no bins, a negative bin count, hop 0) the error wraps ErrPanic and carries
// Go's runtime error text; parameters and samples the library does not reproduce wrap
// ErrUnsupported (include/sonar_gpu.h).
func (cqt *ChromaCQT) ComputeChroma(signal []float64, hopSize int) ([][]float64, error) {
	if len(signal) == 0 {
		return nil, nil
	}
	var totalBins, fftSize, nFrames, sumTaps C.int64_t
	if rc := C.sonar_chroma_cqt_plan(C.int32_t(cqt.sampleRate), C.double(cqt.minFreq), C.double(cqt.maxFreq),
		C.int32_t(cqt.binsPerOctave), C.double(cqt.qFactor), C.double(cqt.tuningFreq), C.int64_t(len(signal)),
		C.int64_t(hopSize), &totalBins, &fftSize, &nFrames, &sumTaps, nil, nil); rc != C.SONAR_OK {
		nFrames = 0 // the call below reports the error in Go's words; it writes nothing
	}
	flat := make([]float64, int(nFrames)*12+1)
	if rc := C.sonar_chroma_cqt(cqt.x.c, f64p(signal), C.int64_t(len(signal)), C.int64_t(hopSize),
		C.int32_t(cqt.sampleRate), C.double(cqt.minFreq), C.double(cqt.maxFreq), C.int32_t(cqt.binsPerOctave),
		C.double(cqt.qFactor), C.double(cqt.tuningFreq), f64p(flat), nil, 0); rc != C.SONAR_OK {
		return nil, cqt.x.err(rc)
	}
	if !cqt.kernelComputed { // computeCQTKernel's frequency bins (:100-104)
		cqt.freqBins = make([]float64, int(totalBins))
		for k := range cqt.freqBins {
			cqt.freqBins[k] = cqt.minFreq * math.Pow(2.0, float64(k)/float64(cqt.binsPerOctave))
		}
		cqt.kernelComputed = true
	}
	chromagram := make([][]float64, int(nFrames))
	for t := range chromagram {
		chromagram[t] = flat[t*12 : (t+1)*12 : (t+1)*12]
	}
	return chromagram, nil
}

// GetChromaLabels = ChromaCQT.GetChromaLabels (:271-273).
func (cqt *ChromaCQT) GetChromaLabels() []string {
	return []string{"C", "C#", "D", "D#", "E", "F", "F#", "G", "G#", "A", "A#", "B"}
}

// GetCQTFrequencies = ChromaCQT.GetCQTFrequencies (:276-284): empty until a ComputeChroma has built the
// kernel, and again after SetTuning / SetQFactor.
func (cqt *ChromaCQT) GetCQTFrequencies() []float64 {
	if !cqt.kernelComputed {
		return []float64{}
	}
	freqs := make([]float64, len(cqt.freqBins))
	copy(freqs, cqt.freqBins)
	return freqs
}

// SetTuning = ChromaCQT.SetTuning (:287-290).  The next ComputeChroma uses the new parameter set's
// table (built on first use, cached beside the old one until Context.Trim).
func (cqt *ChromaCQT) SetTuning(tuningFreq float64) {
	cqt.tuningFreq = tuningFreq
	cqt.kernelComputed = false
}

// GetQFactor = ChromaCQT.GetQFactor (:293-295).
func (cqt *ChromaCQT) GetQFactor() float64 {
	return cqt.qFactor
}

// SetQFactor = ChromaCQT.SetQFactor (:298-301).
func (cqt *ChromaCQT) SetQFactor(qFactor float64) {
	cqt.qFactor = qFactor
	cqt.kernelComputed = false
}

// ChromaSimilarityMethod and ChromaDistanceMetric carry the reference's values
// (chroma_similarity.go:10-17, chroma_vector.go:41-50), which are SONAR_CHROMA_SIM_* / SONAR_CHROMA_DIST_*.
type ChromaSimilarityMethod int

const (
	ChromaSimilarityDirect ChromaSimilarityMethod = iota
	ChromaSimilarityBinary
	ChromaSimilaritySmithWaterman
	ChromaSimilarityDTW
	ChromaSimilarityQMax
	ChromaSimilarityOTI
)

type ChromaDistanceMetric int

const (
	ChromaDistanceEuclidean ChromaDistanceMetric = iota
	ChromaDistanceManhattan
	ChromaDistanceCosine
	ChromaDistancePearson
	ChromaDistanceKLDivergence
	ChromaDistanceJSDistance
	ChromaDistanceHellinger
)

// ChromaSimilarityParams mirrors chroma.ChromaSimilarityParams (:20-30).  FrameStackSize,
// FrameStackStride and NormalizeSimilarity are kept for source compatibility; the reference never reads
// them, and neither does the library.
type ChromaSimilarityParams struct {
	Method                 ChromaSimilarityMethod
	DistanceMetric         ChromaDistanceMetric
	BinaryThreshold        float64
	FrameStackSize         int
	FrameStackStride       int
	OTIRadius              int
	DTWBandRadius          int
	NormalizeSimilarity    bool
	TranspositionInvariant bool
}

// DefaultChromaSimilarityParams = the parameters of chroma.NewChromaSequenceSimilarity (:59-74).
func DefaultChromaSimilarityParams() ChromaSimilarityParams {
	return ChromaSimilarityParams{Method: ChromaSimilarityDirect, DistanceMetric: ChromaDistanceCosine,
		BinaryThreshold: 0.4, FrameStackSize: 1, FrameStackStride: 1, OTIRadius: 10, DTWBandRadius: 50,
		NormalizeSimilarity: true}
}

// AlignmentPoint mirrors chroma.AlignmentPoint (:45-49).
type AlignmentPoint struct {
	QueryFrame     int
	ReferenceFrame int
	Score          float64
}

// ChromaSimilarityResult mirrors chroma.ChromaSimilarityResult (:33-42) without ComputationTime, which
// the reference never sets.  SimilarityMatrix is nil where the reference's is (OTI with no winning shift).
type ChromaSimilarityResult struct {
	SimilarityMatrix  [][]float64
	OverallSimilarity float64
	OptimalPath       []AlignmentPoint
	BestTransposition int
	Method            ChromaSimilarityMethod
	QueryFrames       int
	ReferenceFrames   int
}

// ChromaSequenceSimilarity = NewChromaSequenceSimilarityWithParams(params).ComputeSimilarity(query, ref)
// (:77-103) on frames of equal width.  Method in the result is params.Method as given, except that
// Binary, Smith-Waterman, DTW, QMax and OTI set their own (an unknown value runs Direct and is reported
// unchanged, :100-101, :155).  Where the reference panics (DTW on an empty sequence) the error wraps
// ErrPanic and carries Go's runtime error text.
func (x *Context) ChromaSequenceSimilarity(params ChromaSimilarityParams, query, ref [][]float64) (*ChromaSimilarityResult, error) {
	q, dq := rows2(query)
	r, dr := rows2(ref)
	dim := dq
	if len(query) == 0 {
		dim = dr
	}
	if dim == 0 {
		dim = 1
	}
	nq, nr := len(query), len(ref)
	flat := make([]float64, nq*nr+1)
	pq := make([]int32, nq+nr+1)
	pr := make([]int32, nq+nr+1)
	ps := make([]float64, nq+nr+1)
	var isNil, best C.int32_t
	var overall C.double
	var plen C.int64_t
	ti := 0
	if params.TranspositionInvariant {
		ti = 1
	}
	if rc := C.sonar_chroma_similarity(x.c, f64p(q), C.int64_t(nq), f64p(r), C.int64_t(nr), C.int32_t(dim),
		C.int32_t(params.Method), C.int32_t(params.DistanceMetric), C.double(params.BinaryThreshold),
		C.int32_t(params.OTIRadius), C.int32_t(params.DTWBandRadius), C.int32_t(ti), f64p(flat), &isNil, &overall,
		&best, (*C.int32_t)(unsafe.Pointer(&pq[0])), (*C.int32_t)(unsafe.Pointer(&pr[0])), f64p(ps), &plen); rc != C.SONAR_OK {
		return nil, x.err(rc)
	}
	res := &ChromaSimilarityResult{OverallSimilarity: float64(overall), BestTransposition: int(best),
		Method: params.Method, QueryFrames: nq, ReferenceFrames: nr}
	if isNil == 0 {
		res.SimilarityMatrix = split(flat, nq, nr)
	}
	if params.Method == ChromaSimilaritySmithWaterman || params.Method == ChromaSimilarityDTW {
		for k := 0; k < int(plen); k++ {
			res.OptimalPath = append(res.OptimalPath, AlignmentPoint{int(pq[k]), int(pr[k]), ps[k]})
		}
	}
	return res, nil
}
