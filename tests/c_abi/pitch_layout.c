/* pitch_layout.c -- size and field offsets of sonar_pitch_params as a C99 compiler lays it out; the
 * test compares them with the ctypes mirror (sonar.PitchParams). */
#include <stddef.h>
#include <stdio.h>

#include "sonar_gpu.h"

#define OFF(f) printf("offset %s %lu\n", #f, (unsigned long)offsetof(sonar_pitch_params, f))

int main(void) {
  printf("size sonar_pitch_params %lu\n", (unsigned long)sizeof(sonar_pitch_params));
  OFF(method); OFF(sample_rate); OFF(window_size); OFF(hop_size);
  OFF(min_freq); OFF(max_freq); OFF(yin_threshold); OFF(autocorr_threshold); OFF(cepstral_threshold);
  OFF(min_confidence); OFF(min_salience); OFF(voicing_threshold);
  OFF(max_harmonics); OFF(harmonic_tolerance);
  OFF(pre_emphasis); OFF(window_function); OFF(zero_padding); OFF(median_filter); OFF(temporal_smoothing);
  OFF(octave_correction);
  printf("enum yin %d praat %d rectangular %d\n", SONAR_PITCH_YIN, SONAR_PITCH_PRAAT, SONAR_PITCH_WIN_RECTANGULAR);
  return 0;
}
