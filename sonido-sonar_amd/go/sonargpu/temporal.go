package sonargpu

// OnsetDetection and TempoEstimation seam (algorithms/temporal/onset_detection.go, tempo_estimation.go):
// DetectOnsets, DetectOnsetsEnergy, DetectOnsetsComplex, ComputeOnsetDensity, AdaptiveThreshold,
// EstimateTempo, EstimateTempoAutocorrelation, EstimateTempoRange and ClassifyTempoCategory through
// sonar_onsets_flux, sonar_onsets_energy, sonar_onsets_complex, sonar_onset_adaptive_threshold,
// sonar_tempo_from_onsets, sonar_tempo_autocorrelation and sonar_tempo.  The constructors are methods of
// Context because the objects need a device; otherwise the names and signatures are the reference's.
// SpectralFlux and ComputeRMS have the reference's names too (Flux, ComputeRMS).
//
// Written against include/sonar_gpu.h; not compiled here (no Go toolchain in the image).

/*
#include "sonar_gpu.h"
*/
import "C"

import "unsafe"

func i64p(v []int64) *C.int64_t {
	if len(v) == 0 {
		return nil
	}
	return (*C.int64_t)(unsafe.Pointer(&v[0]))
}

func toInts(v []int64, n int) []int {
	out := make([]int, n)
	for i := range out {
		out[i] = int(v[i])
	}
	return out
}

// OnsetDetection mirrors temporal.OnsetDetection (:10-14); the STFT lives in the library.
type OnsetDetection struct {
	x *Context
}

// NewOnsetDetection = temporal.NewOnsetDetection (:17-23).
func (x *Context) NewOnsetDetection() *OnsetDetection {
	return &OnsetDetection{x: x}
}

// Flux = SpectralFlux.Compute (spectral_flux.go:17-36), or ComputeAllChanges (:39-56), over rows of one length.
func (od *OnsetDetection) Flux(spectrogram [][]float64, allChanges bool) ([]float64, error) {
	frames := len(spectrogram)
	if frames < 2 {
		return []float64{}, nil
	}
	flat, K := flatten(spectrogram)
	out := make([]float64, frames-1)
	all := C.int32_t(0)
	if allChanges {
		all = 1
	}
	if rc := C.sonar_spectral_flux(od.x.c, f64p(flat), C.int64_t(frames), C.int32_t(K), all, f64p(out), 0); rc != C.SONAR_OK {
		return nil, od.x.err(rc)
	}
	return out, nil
}

// ComputeRMS = Envelope.ComputeRMS (envelope.go:18-43).
func (od *OnsetDetection) ComputeRMS(signal []float64, frameSize, hopSize int) []float64 {
	n := int(C.sonar_rms_envelope_frames(C.int64_t(len(signal)), C.int32_t(frameSize), C.int32_t(hopSize)))
	if n == 0 {
		return []float64{}
	}
	out := make([]float64, n)
	if rc := C.sonar_rms_envelope(od.x.c, f64p(signal), C.int64_t(len(signal)), C.int32_t(frameSize), C.int32_t(hopSize),
		f64p(out), nil, 0); rc != C.SONAR_OK {
		return []float64{}
	}
	return out
}

// FindPeaks = findFluxPeaks (:97-120) on any curve.
func (od *OnsetDetection) FindPeaks(curve []float64, threshold, minInterval float64, hopSize, sampleRate int) ([]int, error) {
	width := int(C.sonar_onset_peaks_width(C.int64_t(len(curve))))
	index := make([]int64, width+1)
	var count C.int64_t
	if rc := C.sonar_onset_peaks(od.x.c, f64p(curve), C.int64_t(len(curve)), C.double(threshold), C.double(minInterval),
		C.int32_t(hopSize), C.int32_t(sampleRate), i64p(index), &count, 0); rc != C.SONAR_OK {
		return nil, od.x.err(rc)
	}
	return toInts(index, int(count)), nil
}

// AdaptiveThreshold = OnsetDetection.AdaptiveThreshold (:200-222).
func (od *OnsetDetection) AdaptiveThreshold(flux []float64) float64 {
	var v float64
	if rc := C.sonar_onset_adaptive_threshold(od.x.c, f64p(flux), C.int64_t(len(flux)), (*C.double)(unsafe.Pointer(&v)), 0); rc != C.SONAR_OK {
		return 0.0
	}
	return v
}

// DetectOnsets = OnsetDetection.DetectOnsets (:26-56).
func (od *OnsetDetection) DetectOnsets(signal []float64, sampleRate int, threshold float64, minInterval float64) ([]int, error) {
	if len(signal) == 0 {
		return []int{}, nil
	}
	frames := int(C.sonar_stft_frames(C.int64_t(len(signal)), C.SONAR_ONSET_WINDOW, C.SONAR_ONSET_HOP))
	if frames < 0 {
		frames = 0
	}
	onsets := make([]int64, int(C.sonar_onset_peaks_width(C.int64_t(frames-1)))+1)
	var count C.int64_t
	if rc := C.sonar_onsets_flux(od.x.c, f64p(signal), C.int64_t(len(signal)), C.int32_t(sampleRate), 0, 0, C.double(threshold),
		C.double(minInterval), i64p(onsets), &count, nil, nil, nil, 0); rc != C.SONAR_OK {
		return nil, od.x.err(rc)
	}
	return toInts(onsets, int(count)), nil
}

// DetectOnsetsEnergy = OnsetDetection.DetectOnsetsEnergy (:59-94); empty where the library declines the
// parameters, as the reference has no error to return.
func (od *OnsetDetection) DetectOnsetsEnergy(signal []float64, sampleRate int, threshold float64, minInterval float64) []int {
	env := int(C.sonar_rms_envelope_frames(C.int64_t(len(signal)), C.SONAR_ONSET_ENERGY_FRAME, C.SONAR_ONSET_ENERGY_HOP))
	onsets := make([]int64, int(C.sonar_onset_peaks_width(C.int64_t(env-1)))+1)
	var count C.int64_t
	if rc := C.sonar_onsets_energy(od.x.c, f64p(signal), C.int64_t(len(signal)), C.int32_t(sampleRate), 0, 0, C.double(threshold),
		C.double(minInterval), i64p(onsets), &count, nil, nil, 0); rc != C.SONAR_OK {
		return []int{}
	}
	return toInts(onsets, int(count))
}

func (od *OnsetDetection) complex(signal []float64, sampleRate int) ([]int, float64, error) {
	onsets := make([]int64, int(C.sonar_onsets_complex_width(C.int64_t(len(signal))))+1)
	var count C.int64_t
	var density C.double
	if rc := C.sonar_onsets_complex(od.x.c, f64p(signal), C.int64_t(len(signal)), C.int32_t(sampleRate), i64p(onsets), &count,
		&density, 0); rc != C.SONAR_OK {
		return nil, 0.0, od.x.err(rc)
	}
	return toInts(onsets, int(count)), float64(density), nil
}

// DetectOnsetsComplex = OnsetDetection.DetectOnsetsComplex (:123-146).
func (od *OnsetDetection) DetectOnsetsComplex(signal []float64, sampleRate int) ([]int, error) {
	onsets, _, err := od.complex(signal, sampleRate)
	return onsets, err
}

// ComputeOnsetDensity = OnsetDetection.ComputeOnsetDensity (:185-197).
func (od *OnsetDetection) ComputeOnsetDensity(signal []float64, sampleRate int) (float64, error) {
	_, density, err := od.complex(signal, sampleRate)
	return density, err
}

// TempoEstimation mirrors temporal.TempoEstimation (:8-11).
type TempoEstimation struct {
	x *Context
}

// NewTempoEstimation = temporal.NewTempoEstimation (:14-19).
func (x *Context) NewTempoEstimation() *TempoEstimation {
	return &TempoEstimation{x: x}
}

// TempoResult is sonar_tempo_result: both estimates, EstimateTempoRange's three values, the category of
// the average and the onset count.
type TempoResult struct {
	OnsetTempo, AutocorrTempo, Tempo, Confidence, Difference float64
	OnsetCount, BestLag                                      int
	Category                                                 string
}

// Estimate is EstimateTempo, EstimateTempoAutocorrelation, EstimateTempoRange and ClassifyTempoCategory
// in one call, the samples staged once.
func (te *TempoEstimation) Estimate(signal []float64, sampleRate int) (TempoResult, error) {
	var r C.sonar_tempo_result
	if rc := C.sonar_tempo(te.x.c, f64p(signal), C.int64_t(len(signal)), C.int32_t(sampleRate), &r, 0); rc != C.SONAR_OK {
		return TempoResult{}, te.x.err(rc)
	}
	return TempoResult{OnsetTempo: float64(r.onset_tempo), AutocorrTempo: float64(r.autocorr_tempo), Tempo: float64(r.tempo),
		Confidence: float64(r.confidence), Difference: float64(r.difference), OnsetCount: int(r.onset_count),
		BestLag: int(r.best_lag), Category: C.GoString(C.sonar_tempo_category_name(r.category))}, nil
}

// EstimateTempo = TempoEstimation.EstimateTempo (:22-48).
func (te *TempoEstimation) EstimateTempo(signal []float64, sampleRate int) (float64, error) {
	if len(signal) == 0 {
		return 0.0, nil
	}
	od := OnsetDetection{x: te.x}
	onsets, err := od.DetectOnsetsComplex(signal, sampleRate)
	if err != nil {
		return 0.0, err
	}
	list := make([]int64, len(onsets)+1)
	for i, v := range onsets {
		list[i] = int64(v)
	}
	var tempo C.double
	if rc := C.sonar_tempo_from_onsets(i64p(list), C.int64_t(len(onsets)), C.int32_t(sampleRate), &tempo, nil); rc != C.SONAR_OK {
		return 0.0, te.x.err(rc)
	}
	return float64(tempo), nil
}

// EstimateTempoAutocorrelation = TempoEstimation.EstimateTempoAutocorrelation (:51-74); only the lags the
// peak search reads are computed.
func (te *TempoEstimation) EstimateTempoAutocorrelation(signal []float64, sampleRate int) float64 {
	var tempo float64
	if rc := C.sonar_tempo_autocorrelation(te.x.c, f64p(signal), C.int64_t(len(signal)), C.int32_t(sampleRate),
		(*C.double)(unsafe.Pointer(&tempo)), nil, nil, nil, 0); rc != C.SONAR_OK {
		return 0.0
	}
	return tempo
}

// EstimateTempoRange = TempoEstimation.EstimateTempoRange (:204-217): average, confidence, difference.
func (te *TempoEstimation) EstimateTempoRange(signal []float64, sampleRate int) (float64, float64, float64) {
	r, err := te.Estimate(signal, sampleRate)
	if err != nil {
		return 0.0, 0.0, 0.0
	}
	return r.Tempo, r.Confidence, r.Difference
}

// ClassifyTempoCategory = TempoEstimation.ClassifyTempoCategory (:220-232).
func (te *TempoEstimation) ClassifyTempoCategory(tempo float64) string {
	return C.GoString(C.sonar_tempo_category_name(C.sonar_tempo_category(C.double(tempo))))
}
