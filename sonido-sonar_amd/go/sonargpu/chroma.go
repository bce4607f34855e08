package sonargpu

// ChromaCQT seam (algorithms/chroma/chroma_cqt.go): the constant-Q chromagram through
// sonar_chroma_cqt.  MusicFeatureExtractor builds one beside its ChromaSTFT (music.go:91-93) and
// the chord detector calls it on whole recordings (tonal/chord_detection.go:534, 657).  The
// constructors are methods of Context because the object needs a device; otherwise the names and
// signatures are the reference's.
//
// Written against include/sonar_gpu.h; not compiled here (no Go toolchain in the image).

/*
#include "sonar_gpu.h"
*/
import "C"

import (
	"math"
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
