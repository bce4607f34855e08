package sonargpu

// ChromaCQT seam (algorithms/chroma/chroma_cqt.go): the constant-Q chromagram through
// sonar_chroma_cqt.  MusicFeatureExtractor builds one beside its ChromaSTFT (music.go:91-93) and
// the chord detector calls it on whole recordings (tonal/chord_detection.go:534, 657).  The
// constructors are methods of Context because the object needs a device; otherwise the names and
// signatures are the reference's.
//
// ChromaSequenceSimilarity (algorithms/chroma/chroma_similarity.go) follows at the end of the file,
// through sonar_chroma_similarity, then HPCP and SpectralPeaks (algorithms/chroma/hpcp.go,
// algorithms/harmonic/spectral_peaks.go) through sonar_hpcp_from_spectrum, sonar_hpcp and
// sonar_spectral_peaks.
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

// ---- HPCP and spectral peaks (algorithms/chroma/hpcp.go, algorithms/harmonic/spectral_peaks.go) ----
//
// The harmonic pitch class profile through sonar_hpcp_from_spectrum / sonar_hpcp and the peak picker
// through sonar_spectral_peaks.  MusicFeatureExtractor builds an HPCP beside its two chromagrams
// (music.go:93); the chord detector and the key estimator call ComputeFromSpectrum frame by frame
// (tonal/chord_detection.go:529, key_estimation.go:236).  Here a call takes a batch of spectra.

// HPCPParams = chroma.HPCPParams (hpcp.go:11-26).
type HPCPParams struct {
	Size              int
	ReferenceFreq     float64
	HarmonicsRemoval  bool
	Normalized        bool
	WeightType        string // "none", "cosine", "squared_cosine"; anything else is "none", as in Go
	WindowSize        float64
	MaxShifted        bool
	NonLinear         bool
	BandPreset        bool
	MinFreq           float64
	MaxFreq           float64
	SplitFreq         float64
	HarmonicsStrength float64
	MaxHarmonics      int
}

// HPCPResult = chroma.HPCPResult (hpcp.go:29-36).
type HPCPResult struct {
	HPCP       []float64
	Size       int
	Resolution float64
	RefFreq    float64
	Energy     float64
	Entropy    float64
}

// HPCP mirrors chroma.HPCP (:39-51); the contribution table lives in the library, cached in the
// context per parameter set.
type HPCP struct {
	x          *Context
	params     HPCPParams
	sampleRate int
}

// NewHPCP = chroma.NewHPCP (:54-75).
func (x *Context) NewHPCP(sampleRate int) *HPCP {
	return x.NewHPCPWithParams(sampleRate, HPCPParams{Size: 12, ReferenceFreq: 440.0, Normalized: true,
		WeightType: "cosine", WindowSize: 1.0, BandPreset: true, MinFreq: 40.0, MaxFreq: 5000.0, SplitFreq: 500.0,
		HarmonicsStrength: 1.0})
}

// NewHPCPWithParams = chroma.NewHPCPWithParams (:78-84).
func (x *Context) NewHPCPWithParams(sampleRate int, params HPCPParams) *HPCP {
	return &HPCP{x: x, params: params, sampleRate: sampleRate}
}

// GetParams / SetParams = HPCP.GetParams / SetParams (:408-416).
func (h *HPCP) GetParams() HPCPParams        { return h.params }
func (h *HPCP) SetParams(params HPCPParams) { h.params = params }

func (h *HPCP) cParams() C.sonar_hpcp_params {
	b := func(v bool) C.int32_t {
		if v {
			return 1
		}
		return 0
	}
	p := h.params
	wt := C.int32_t(C.SONAR_HPCP_WEIGHT_NONE)
	switch p.WeightType {
	case "cosine":
		wt = C.SONAR_HPCP_WEIGHT_COSINE
	case "squared_cosine":
		wt = C.SONAR_HPCP_WEIGHT_SQUARED_COSINE
	}
	return C.sonar_hpcp_params{size: C.int32_t(p.Size), harmonics_removal: b(p.HarmonicsRemoval),
		normalized: b(p.Normalized), weight_type: wt, max_shifted: b(p.MaxShifted), non_linear: b(p.NonLinear),
		band_preset: b(p.BandPreset), max_harmonics: C.int32_t(p.MaxHarmonics), reference_freq: C.double(p.ReferenceFreq),
		window_size: C.double(p.WindowSize), min_freq: C.double(p.MinFreq), max_freq: C.double(p.MaxFreq),
		split_freq: C.double(p.SplitFreq), harmonics_strength: C.double(p.HarmonicsStrength)}
}

func (h *HPCP) results(flat, energy, entropy []float64, frames int) []HPCPResult {
	size := h.params.Size
	out := make([]HPCPResult, frames)
	for t := range out {
		out[t] = HPCPResult{HPCP: flat[t*size : (t+1)*size : (t+1)*size], Size: size, Resolution: 12.0 / float64(size),
			RefFreq: h.params.ReferenceFreq, Energy: energy[t], Entropy: entropy[t]}
	}
	return out
}

// ComputeFromSpectrum = HPCP.ComputeFromSpectrum (:205-221) on every row of a batch of magnitude
// spectra of one length (the chord detector's rows hold all windowSize bins, the STFT's
// windowSize/2 + 1).  Size < 0 wraps ErrPanic with Go's makeslice text; parameters the library
// does not reproduce wrap ErrUnsupported (include/sonar_gpu.h).
func (h *HPCP) ComputeFromSpectrum(magnitudes [][]float64, windowSize int) ([]HPCPResult, error) {
	frames := len(magnitudes)
	if frames == 0 {
		return nil, nil
	}
	bins := len(magnitudes[0])
	flatMag := make([]float64, frames*bins+1)
	for t, row := range magnitudes {
		copy(flatMag[t*bins:(t+1)*bins], row)
	}
	size := h.params.Size
	if size < 0 {
		size = 0 // the call reports the panic
	}
	flat := make([]float64, frames*size+1)
	energy, entropy := make([]float64, frames), make([]float64, frames)
	p := h.cParams()
	if rc := C.sonar_hpcp_from_spectrum(h.x.c, f64p(flatMag), C.int64_t(frames), C.int32_t(bins), C.int32_t(windowSize),
		C.int32_t(h.sampleRate), &p, f64p(flat), f64p(energy), f64p(entropy), 0); rc != C.SONAR_OK {
		return nil, h.x.err(rc)
	}
	return h.results(flat, energy, entropy, frames), nil
}

// ComputeFromSignal is SpectralAnalyzer.ComputeSTFTWithWindow(signal, windowSize, hopSize,
// windowType).Magnitude -> ComputeFromSpectrum per frame in one call (sonar_hpcp): the spectrogram
// stays on the device, in a bounded scratch.  windowType is a SONAR_WIN_* value.
func (h *HPCP) ComputeFromSignal(signal []float64, windowSize, hopSize, windowType int) ([]HPCPResult, error) {
	var frames, chunkFrames, nChunks C.int64_t
	if rc := C.sonar_hpcp_plan(C.int64_t(len(signal)), C.int32_t(windowSize), C.int32_t(hopSize), &frames, &chunkFrames,
		&nChunks); rc != C.SONAR_OK {
		frames = 0 // the call below reports the error in Go's words; it writes nothing
	}
	size := h.params.Size
	if size < 0 {
		size = 0
	}
	flat := make([]float64, int(frames)*size+1)
	energy, entropy := make([]float64, int(frames)+1), make([]float64, int(frames)+1)
	p := h.cParams()
	var pcm *C.double
	if len(signal) > 0 {
		pcm = f64p(signal)
	}
	if rc := C.sonar_hpcp(h.x.c, pcm, C.int64_t(len(signal)), C.int32_t(h.sampleRate), C.int32_t(windowSize),
		C.int32_t(hopSize), C.int32_t(windowType), &p, f64p(flat), f64p(energy), f64p(entropy), 0); rc != C.SONAR_OK {
		return nil, h.x.err(rc)
	}
	return h.results(flat, energy, entropy, int(frames)), nil
}

// ComputeFromSpectrumDevice is ComputeFromSpectrum on device memory: mag (frames x bins float64) and
// hpcp (frames x Size) are device addresses, energy and entropy (frames each) may be nil.  The profile
// can go to ChromaSequenceSimilarity's device form as it is, without leaving the device.
func (h *HPCP) ComputeFromSpectrumDevice(mag unsafe.Pointer, frames, bins, windowSize int, hpcp, energy, entropy unsafe.Pointer) error {
	p := h.cParams()
	if rc := C.sonar_hpcp_from_spectrum(h.x.c, (*C.double)(mag), C.int64_t(frames), C.int32_t(bins), C.int32_t(windowSize),
		C.int32_t(h.sampleRate), &p, (*C.double)(hpcp), (*C.double)(energy), (*C.double)(entropy), 1); rc != C.SONAR_OK {
		return h.x.err(rc)
	}
	return nil
}

// SpectralPeak = harmonic.SpectralPeak (spectral_peaks.go:9-15).
type SpectralPeak struct {
	Frequency float64
	Magnitude float64
	Phase     float64
	BinIndex  int
	Harmonic  int
}

// SpectralPeaks mirrors harmonic.SpectralPeaks (:18-23).
type SpectralPeaks struct {
	x               *Context
	sampleRate      int
	minPeakHeight   float64
	minPeakDistance float64
	maxPeaks        int
}

// NewSpectralPeaks = harmonic.NewSpectralPeaks (:26-33).
func (x *Context) NewSpectralPeaks(sampleRate int, minPeakHeight, minPeakDistance float64, maxPeaks int) *SpectralPeaks {
	return &SpectralPeaks{x: x, sampleRate: sampleRate, minPeakHeight: minPeakHeight, minPeakDistance: minPeakDistance,
		maxPeaks: maxPeaks}
}

// DetectPeaks = SpectralPeaks.DetectPeaks (:36-100) on every row of a batch of magnitude spectra of
// one length: per row the peaks by magnitude, descending; equal magnitudes come in ascending bin
// order (sort.Slice leaves that open).  A negative maxPeaks wraps ErrPanic with Go's slice-bounds text.
func (sp *SpectralPeaks) DetectPeaks(magnitudeSpectra [][]float64, windowSize int) ([][]SpectralPeak, error) {
	frames := len(magnitudeSpectra)
	if frames == 0 {
		return nil, nil
	}
	bins := len(magnitudeSpectra[0])
	flatMag := make([]float64, frames*bins+1)
	for t, row := range magnitudeSpectra {
		copy(flatMag[t*bins:(t+1)*bins], row)
	}
	width := int(C.sonar_spectral_peaks_width(C.int64_t(bins), C.int64_t(sp.maxPeaks)))
	count := make([]int32, frames)
	bin := make([]int32, frames*width+1)
	mag, freq := make([]float64, frames*width+1), make([]float64, frames*width+1)
	if rc := C.sonar_spectral_peaks(sp.x.c, f64p(flatMag), C.int64_t(frames), C.int32_t(bins), C.int32_t(windowSize),
		C.int32_t(sp.sampleRate), C.double(sp.minPeakHeight), C.double(sp.minPeakDistance), C.int32_t(sp.maxPeaks),
		(*C.int32_t)(unsafe.Pointer(&count[0])), (*C.int32_t)(unsafe.Pointer(&bin[0])), f64p(mag), f64p(freq), 0); rc != C.SONAR_OK {
		return nil, sp.x.err(rc)
	}
	out := make([][]SpectralPeak, frames)
	for t := range out {
		out[t] = make([]SpectralPeak, int(count[t]))
		for r := range out[t] {
			o := t*width + r
			out[t][r] = SpectralPeak{Frequency: freq[o], Magnitude: mag[o], Phase: 0.0, BinIndex: int(bin[o]), Harmonic: -1}
		}
	}
	return out, nil
}
