/* inharm_layout.c -- size and field offsets of sonar_inharm_params as a C99 compiler lays it out; the
 * test compares them with the ctypes mirror (sonar.InharmParams). */
#include <stddef.h>
#include <stdio.h>

#include "sonar_gpu.h"

#define OFF(f) printf("offset %s %lu\n", #f, (unsigned long)offsetof(sonar_inharm_params, f))

int main(void) {
  printf("size sonar_inharm_params %lu\n", (unsigned long)sizeof(sonar_inharm_params));
  OFF(method); OFF(model); OFF(sample_rate); OFF(window_size); OFF(max_harmonics); OFF(min_harmonics);
  OFF(harmonic_tolerance); OFF(min_harmonic_strength); OFF(min_freq); OFF(max_freq); OFF(freq_resolution);
  OFF(reference_harmonic); OFF(weight_by_amplitude); OFF(use_log_frequency);
  OFF(string_tension); OFF(string_length); OFF(string_stiffness); OFF(outlier_threshold); OFF(confidence_level);
  OFF(use_robust_estimation); OFF(use_temporal_tracking); OFF(temporal_window);
  printf("enum railsback %d statistical %d general %d invalid_f0 %d insufficient %d very_high %d unknown %d max %d\n",
         SONAR_INHARM_RAILSBACK, SONAR_INHARM_STATISTICAL, SONAR_INHARM_MODEL_GENERAL, SONAR_INHARM_QUALITY_INVALID_F0,
         SONAR_INHARM_STATUS_INSUFFICIENT, SONAR_INHARM_VERY_HIGH, SONAR_INHARM_INSTRUMENT_UNKNOWN,
         SONAR_INHARM_MAX_HARMONICS);
  return 0;
}
