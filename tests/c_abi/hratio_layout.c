/* hratio_layout.c -- size and field offsets of sonar_hratio_params as a C99 compiler lays it out; the
 * test compares them with the ctypes mirror (sonar.HratioParams). */
#include <stddef.h>
#include <stdio.h>

#include "sonar_gpu.h"

#define OFF(f) printf("offset %s %lu\n", #f, (unsigned long)offsetof(sonar_hratio_params, f))

int main(void) {
  printf("size sonar_hratio_params %lu\n", (unsigned long)sizeof(sonar_hratio_params));
  OFF(method); OFF(sample_rate); OFF(window_size); OFF(hop_size);
  OFF(min_freq); OFF(max_freq); OFF(max_harmonics); OFF(harmonic_tolerance);
  OFF(min_peak_height); OFF(peak_detection_width); OFF(spectral_smoothing_len);
  OFF(noise_floor_method); OFF(noise_floor_percentile); OFF(noise_floor_smoothing_len);
  OFF(use_temporal_smoothing); OFF(temporal_smoothing_len);
  OFF(use_freq_weighting); OFF(use_psychoacoustic_mask); OFF(adaptive_threshold); OFF(autocorr_max_lag);
  printf("enum hnr %d yin %d minimum %d very_high %d max_harmonics %d\n", SONAR_HRATIO_HNR, SONAR_HRATIO_YIN,
         SONAR_HRATIO_NOISE_MINIMUM, SONAR_HRATIO_VERY_HIGH, SONAR_HRATIO_MAX_HARMONICS);
  return 0;
}
