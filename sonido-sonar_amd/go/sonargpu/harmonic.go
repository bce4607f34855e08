package sonargpu

// HarmonicProduct seam (algorithms/harmonic/harmonic_product.go): ComputeHPS,
// ComputeHPSWithInterpolation, EstimateF0, EstimateF0WithConfidence, ComputeHarmonicStrength,
// ComputeHarmonicity and GetOptimalNumHarmonics through sonar_hps_from_spectrum, sonar_hps and
// sonar_hps_optimal_harmonics.  The constructor is a method of Context because the object needs a
// device; otherwise the names and signatures are the reference's.  The per-frame and per-row batch
// forms (EstimateFrames, EstimateRows) are what the GPU is for: one call per spectrogram, not per frame.
//
// Written against include/sonar_gpu.h; not compiled here (no Go toolchain in the image).

/*
#include "sonar_gpu.h"
*/
import "C"

import "unsafe"

// HarmonicProduct mirrors harmonic.HarmonicProduct (:10-17); the FFT lives in the library.
type HarmonicProduct struct {
	x            *Context
	sampleRate   int
	numHarmonics int
	minF0        float64
	maxF0        float64
}

// NewHarmonicProduct = harmonic.NewHarmonicProduct (:20-29).
func (x *Context) NewHarmonicProduct(sampleRate int, numHarmonics int, minF0, maxF0 float64) *HarmonicProduct {
	return &HarmonicProduct{x: x, sampleRate: sampleRate, numHarmonics: numHarmonics, minF0: minF0, maxF0: maxF0}
}

// HarmonicEstimate is one row's or one frame's result: the peak bin of findF0Peak, EstimateF0's
// frequency, ComputeHarmonicity at it and ComputeHarmonicStrength's values (zeros when F0 is 0).
type HarmonicEstimate struct {
	Bin        int
	F0         float64
	Confidence float64
	Strengths  []float64
}

func (hp *HarmonicProduct) harmonics() int {
	if hp.numHarmonics < 0 {
		return 0
	}
	return hp.numHarmonics
}

func (hp *HarmonicProduct) estimates(frames int, bins []int32, f0, conf, strengths []float64) []HarmonicEstimate {
	nh := hp.harmonics()
	out := make([]HarmonicEstimate, frames)
	for t := range out {
		out[t] = HarmonicEstimate{Bin: int(bins[t]), F0: f0[t], Confidence: conf[t], Strengths: strengths[t*nh : (t+1)*nh]}
	}
	return out
}

// EstimateRows runs findF0Peak over ComputeHPS (ComputeHPSWithInterpolation when interpolated) of
// every magnitude row, with signalLength as the reference's len(signal), and the strengths and the
// harmonicity at the row's f0.  Rows must share one length.
func (hp *HarmonicProduct) EstimateRows(magnitudeSpectra [][]float64, signalLength int, interpolated bool) ([]HarmonicEstimate, error) {
	frames := len(magnitudeSpectra)
	if frames == 0 {
		return []HarmonicEstimate{}, nil
	}
	flat, K := flatten(magnitudeSpectra)
	nh := hp.harmonics()
	bins := make([]int32, frames)
	f0, conf, strengths := make([]float64, frames), make([]float64, frames), make([]float64, frames*nh+1)
	interp := C.int32_t(0)
	if interpolated {
		interp = 1
	}
	if rc := C.sonar_hps_from_spectrum(hp.x.c, f64p(flat), C.int64_t(frames), C.int32_t(K), C.int32_t(signalLength),
		C.int32_t(hp.sampleRate), C.int32_t(hp.numHarmonics), C.double(hp.minF0), C.double(hp.maxF0), interp,
		i32p(bins), f64p(f0), f64p(conf), f64p(strengths), nil, 0); rc != C.SONAR_OK {
		return nil, hp.x.err(rc)
	}
	return hp.estimates(frames, bins, f0, conf, strengths), nil
}

// hpsRow is ComputeHPS / ComputeHPSWithInterpolation of one row: the spectrum the peak search runs on.
func (hp *HarmonicProduct) hpsRow(magnitudeSpectrum []float64, interpolated C.int32_t) []float64 {
	if len(magnitudeSpectrum) == 0 {
		return []float64{}
	}
	out := make([]float64, len(magnitudeSpectrum))
	var bin int32
	var f0 float64
	// the range does not matter to the HPS; 1 / 1 keeps every check quiet
	if rc := C.sonar_hps_from_spectrum(hp.x.c, f64p(magnitudeSpectrum), 1, C.int32_t(len(magnitudeSpectrum)), 1, 1,
		C.int32_t(hp.numHarmonics), 0, 0, interpolated, (*C.int32_t)(unsafe.Pointer(&bin)),
		(*C.double)(unsafe.Pointer(&f0)), nil, nil, f64p(out), 0); rc != C.SONAR_OK {
		return []float64{}
	}
	return out
}

// ComputeHPS = HarmonicProduct.ComputeHPS (:32-58).
func (hp *HarmonicProduct) ComputeHPS(magnitudeSpectrum []float64) []float64 {
	return hp.hpsRow(magnitudeSpectrum, 0)
}

// ComputeHPSWithInterpolation = HarmonicProduct.ComputeHPSWithInterpolation (:163-191).
func (hp *HarmonicProduct) ComputeHPSWithInterpolation(magnitudeSpectrum []float64) []float64 {
	return hp.hpsRow(magnitudeSpectrum, 1)
}

// EstimateFrames = EstimateF0WithConfidence (:276-298) on every frame of windowSize samples at hopSize:
// applyWindow's window, the float64 transform, then EstimateRows' work, in one call.
func (hp *HarmonicProduct) EstimateFrames(signal []float64, windowSize, hopSize int) ([]HarmonicEstimate, error) {
	var frames, chunk, chunks C.int64_t
	if rc := C.sonar_hps_plan(C.int64_t(len(signal)), C.int32_t(windowSize), C.int32_t(hopSize), &frames, &chunk, &chunks); rc != C.SONAR_OK {
		return nil, hp.x.err(rc)
	}
	n, nh := int(frames), hp.harmonics()
	bins := make([]int32, n)
	f0, conf, strengths := make([]float64, n), make([]float64, n), make([]float64, n*nh+1)
	if rc := C.sonar_hps(hp.x.c, f64p(signal), C.int64_t(len(signal)), C.int32_t(hp.sampleRate), C.int32_t(windowSize),
		C.int32_t(hopSize), C.int32_t(hp.numHarmonics), C.double(hp.minF0), C.double(hp.maxF0), 0, i32p(bins), f64p(f0),
		f64p(conf), f64p(strengths), nil, &frames, 0); rc != C.SONAR_OK {
		return nil, hp.x.err(rc)
	}
	return hp.estimates(n, bins, f0, conf, strengths), nil
}

// EstimateF0WithConfidence = HarmonicProduct.EstimateF0WithConfidence (:276-298): the signal is one frame.
// The reference returns (0, 0) where it cannot estimate; so does this on a library error.
func (hp *HarmonicProduct) EstimateF0WithConfidence(signal []float64) (float64, float64) {
	if len(signal) == 0 {
		return 0.0, 0.0
	}
	r, err := hp.EstimateFrames(signal, len(signal), len(signal))
	if err != nil || len(r) == 0 {
		return 0.0, 0.0
	}
	return r[0].F0, r[0].Confidence
}

// EstimateF0 = HarmonicProduct.EstimateF0 (:61-91).
func (hp *HarmonicProduct) EstimateF0(signal []float64) float64 {
	f0, _ := hp.EstimateF0WithConfidence(signal)
	return f0
}

// GetOptimalNumHarmonics = HarmonicProduct.GetOptimalNumHarmonics (:301-314); 2, the reference's
// floor, where the library does not reproduce the conversion (minF0 <= 0 or not finite).
func (hp *HarmonicProduct) GetOptimalNumHarmonics() int {
	var n C.int32_t
	if rc := C.sonar_hps_optimal_harmonics(C.int32_t(hp.sampleRate), C.double(hp.minF0), &n); rc != C.SONAR_OK {
		return 2
	}
	return int(n)
}

// EstimateFramesDevice is EstimateFrames on device memory: pcm (n float64), f0Bin (frames int32), f0
// and the optional confidence, strengths (frames x numHarmonics) and magnitude (frames x
// windowSize/2+1) are device addresses; it returns the frame count.
func (hp *HarmonicProduct) EstimateFramesDevice(pcm unsafe.Pointer, n, windowSize, hopSize int, interpolated bool,
	f0Bin, f0, confidence, strengths, magnitude unsafe.Pointer) (int, error) {
	var frames C.int64_t
	interp := C.int32_t(0)
	if interpolated {
		interp = 1
	}
	if rc := C.sonar_hps(hp.x.c, (*C.double)(pcm), C.int64_t(n), C.int32_t(hp.sampleRate), C.int32_t(windowSize),
		C.int32_t(hopSize), C.int32_t(hp.numHarmonics), C.double(hp.minF0), C.double(hp.maxF0), interp,
		(*C.int32_t)(f0Bin), (*C.double)(f0), (*C.double)(confidence), (*C.double)(strengths), (*C.double)(magnitude),
		&frames, 1); rc != C.SONAR_OK {
		return 0, hp.x.err(rc)
	}
	return int(frames), nil
}
