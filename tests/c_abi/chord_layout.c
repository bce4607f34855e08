/* Sizes and member offsets of the chord detection structs of include/sonar_gpu.h as a C99 compiler lays
 * them out, in layout.c's line format ("struct <name> <size>", "member <struct>.<member> <offset>");
 * tests/test_chord_cpu.py holds the ctypes mirrors to them. */
#include <stddef.h>
#include <stdio.h>

#include "sonar_gpu.h"

#define S(T) printf("struct %s %zu\n", #T, sizeof(T))
#define M(T, m) printf("member %s.%s %zu\n", #T, #m, offsetof(T, m))

int main(void) {
  S(sonar_chord_params);
  M(sonar_chord_params, method);
  M(sonar_chord_params, normalize_templates);
  M(sonar_chord_params, use_inversions);
  M(sonar_chord_params, max_candidates);
  M(sonar_chord_params, use_bass_detection);
  M(sonar_chord_params, detect_extensions);
  M(sonar_chord_params, max_extension);
  M(sonar_chord_params, use_temporal_smoothing);
  M(sonar_chord_params, temporal_window);
  M(sonar_chord_params, use_functional_analysis);
  M(sonar_chord_params, min_chord_strength);
  M(sonar_chord_params, bass_weight);
  S(sonar_chord_out);
  M(sonar_chord_out, root);
  M(sonar_chord_out, quality);
  M(sonar_chord_out, inversion);
  M(sonar_chord_out, n_found);
  M(sonar_chord_out, confidence);
  M(sonar_chord_out, strength);
  M(sonar_chord_out, clarity);
  M(sonar_chord_out, ambiguity);
  M(sonar_chord_out, consonance);
  M(sonar_chord_out, tension);
  M(sonar_chord_out, stability);
  M(sonar_chord_out, extensions);
  M(sonar_chord_out, role);
  M(sonar_chord_out, template_scores);
  M(sonar_chord_out, candidates);
  M(sonar_chord_out, cand_inversion);
  M(sonar_chord_out, cand_confidence);
  M(sonar_chord_out, cand_strength);
  return 0;
}
