// key_api.cpp -- sonar_key_frames, sonar_key_sequence, sonar_key_batch and the host-only
// sonar_key_params_default and sonar_key_transition: KeyEstimator and KeyEstimationBatch
// (algorithms/tonal/key_estimation.go).  The host side: Go's panics and the argument checks, the
// profile table (per (mode, key) the shifted profile's diffB and sumSqB of PearsonCorrelationFunc,
// stats/distance.go:111-145, in Go's operation order) and resizeChromaVector's index table (:464-485),
// one cached table per (profile, dim, hpcp_size) (ctx.h, cached_table), and the launch sequences over
// the staged arrays (staging.h).  The kernels are key_kernels.hip's.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"
#include "go_math.h"
#include "kernels.h"
#include "staging.h"

using sonar::go_log2;
using sonar::detail::fail;
using sonar::detail::Staging;
using sonar::detail::timed_begin;
using sonar::detail::timed_end;

namespace {

// initializeKeyProfiles (:404-460): [profile][major | minor][12]
const double kProfiles[7][2][12] = {
    {{6.35, 2.23, 3.48, 2.33, 4.38, 4.09, 2.52, 5.19, 2.39, 3.66, 2.29, 2.88},
     {6.33, 2.68, 3.52, 5.38, 2.60, 3.53, 2.54, 4.75, 3.98, 2.69, 3.34, 3.17}},
    {{5.0, 2.0, 3.5, 2.0, 4.5, 4.0, 2.0, 4.5, 2.0, 3.5, 1.5, 4.0},
     {5.0, 2.0, 3.5, 4.5, 2.0, 4.0, 2.0, 4.5, 3.5, 2.0, 1.5, 4.0}},
    {{6.6, 2.0, 3.5, 2.3, 4.6, 4.0, 2.5, 5.2, 2.4, 3.7, 2.3, 3.4},
     {6.5, 2.7, 3.5, 5.4, 2.6, 3.5, 2.5, 4.7, 4.0, 2.7, 3.4, 3.2}},
    {{17.7661, 0.145624, 14.9265, 0.160186, 19.8049, 11.3587, 0.291248, 22.062, 0.145624, 8.15494, 0.232998, 4.95122},
     {18.2648, 0.737619, 14.0499, 16.8599, 0.702494, 14.4362, 0.702494, 18.6161, 4.56621, 1.93186, 7.37619, 1.75623}},
    {{16.8, 0.86, 12.95, 1.41, 13.49, 11.93, 1.25, 20.28, 1.80, 8.04, 0.62, 10.57},
     {18.16, 0.69, 12.99, 13.34, 1.07, 11.15, 1.38, 21.07, 7.49, 1.53, 6.24, 1.61}},
    {{5.0, 0.0, 3.0, 0.0, 4.0, 3.5, 0.0, 4.5, 0.0, 3.0, 0.0, 2.0},
     {5.0, 0.0, 3.0, 3.5, 0.0, 3.5, 0.0, 4.5, 3.0, 0.0, 2.0, 0.0}},
    {{5.0, 0.0, 0.0, 0.0, 3.0, 0.0, 0.0, 4.0, 0.0, 0.0, 0.0, 0.0},
     {5.0, 0.0, 0.0, 3.0, 0.0, 0.0, 0.0, 4.0, 0.0, 0.0, 0.0, 0.0}},
};

int check_params(const sonar_key_params& p, int64_t F, int32_t dim, std::string& msg) {
  if (p.hpcp_size < 0) { msg = "runtime error: makeslice: len out of range"; return SONAR_ERR_PANIC; }   // :470
  if (p.max_candidates < 0) {                                                                           // :347-349
    msg = "runtime error: slice bounds out of range [:" + std::to_string(p.max_candidates) + "]";
    return SONAR_ERR_PANIC;
  }
  if (p.max_candidates == 0 || p.hpcp_size == 0) {   // candidates[0] (:352); ComputeStats' values[0]
    msg = "runtime error: index out of range [0] with length 0";
    return SONAR_ERR_PANIC;
  }
  if (dim > sonar::KEY_MAX_SIZE || p.hpcp_size > sonar::KEY_MAX_SIZE) {
    msg = "key estimation: dim or hpcp_size above " + std::to_string(sonar::KEY_MAX_SIZE) + " is not supported";
    return SONAR_ERR_UNSUPPORTED;
  }
  if (F > INT32_MAX) { msg = "key estimation: more than 2^31 - 1 frames are not supported"; return SONAR_ERR_UNSUPPORTED; }
  return SONAR_OK;
}

// The device image of one (profile, dim, hpcp_size): 24 x KEY_TAB_ROW doubles, then hpcp_size int32
int device_tables(sonar_ctx* c, const sonar_key_params& p, int32_t dim, sonar::KeyArgs* a) {
  const int prof = (p.profile >= 0 && p.profile <= 6) ? p.profile : 0;   // :301-305
  const int hs = p.hpcp_size;
  char key[96];
  std::snprintf(key, sizeof key, "key.tab.%d.%d.%d", prof, dim, hs);
  const size_t tab_bytes = (size_t)24 * sonar::KEY_TAB_ROW * 8;
  const unsigned char* base = nullptr;
  const int rc = sonar::detail::cached_table(c, key, "key profile table", [&](std::vector<unsigned char>& img, int64_t&) {
    img.assign(tab_bytes + (size_t)hs * 4, 0);
    double* tab = (double*)img.data();
    for (int mode = 0; mode < 2; ++mode)
      for (int k = 0; k < 12; ++k) {
        double shifted[12], mean_b = 0.0, ssb = 0.0;
        for (int i = 0; i < 12; ++i) shifted[i] = kProfiles[prof][mode][(i + k) % 12];   // :393-397
        for (int i = 0; i < 12; ++i) mean_b += shifted[i];
        mean_b /= 12.0;
        double* row = tab + (mode * 12 + k) * sonar::KEY_TAB_ROW;
        for (int i = 0; i < 12; ++i) {
          row[i] = shifted[i] - mean_b;
          ssb += row[i] * row[i];
        }
        row[12] = ssb;
      }
    int32_t* ridx = (int32_t*)(img.data() + tab_bytes);
    const double ratio = (double)dim / (double)hs;           // :471
    for (int i = 0; i < hs; ++i) {
      const double src = (double)i * ratio;
      ridx[i] = (int64_t)src < dim ? (int32_t)src : -1;     // :474-477
    }
    return SONAR_OK;
  }, &base);
  if (rc != SONAR_OK) return rc;
  a->tab = (const double*)base;
  a->ridx = dim != hs ? (const int32_t*)(base + tab_bytes) : nullptr;
  return SONAR_OK;
}

struct FrameOuts {
  int32_t *key, *mode, *known;
  double *confidence, *strength, *clarity, *ambiguity, *tonality, *scores;
  int32_t* candidates;
  double* processed;
};

void base_args(const sonar_key_params& p, int32_t dim, sonar::KeyArgs& a) {
  a.dim = dim;
  a.hs = p.hpcp_size;
  a.normalize = p.normalize_chroma != 0;
  a.remove_mean = p.remove_mean != 0;
  a.binary = p.binary_mode != 0;
  a.ncand = p.max_candidates < 24 ? p.max_candidates : 24;
  a.min_conf = p.min_confidence;
  a.log2_24 = go_log2(24.0);
}

void frame_outs(Staging& o, const FrameOuts& u, size_t F, const sonar::KeyArgs& base, sonar::KeyArgs& a) {
  a.key = o.out("key", u.key, F);
  a.mode = o.out("mode", u.mode, F);
  a.known = o.out("known", u.known, F);
  a.conf = o.out("conf", u.confidence, F);
  a.strength = o.out("strength", u.strength, F);
  a.clarity = o.out("clarity", u.clarity, F);
  a.ambiguity = o.out("ambiguity", u.ambiguity, F);
  a.tonality = o.out("tonality", u.tonality, F);
  a.scores = o.out("scores", u.scores, F * 24);
  a.cand = o.out("cand", u.candidates, F * (size_t)base.ncand);
  a.processed = o.out("processed", u.processed, F * (size_t)base.hs);
}

int launch_rows(sonar_ctx* c, const sonar::KeyArgs& a) {
  const int rc = sonar::launch_key_rows(a, c->stream);
  if (rc == -1) return fail(c, SONAR_ERR_UNSUPPORTED, "key estimation: a shape the kernel does not take");
  if (rc != 0) return fail(c, SONAR_ERR_DEVICE, "key estimation launch failed");
  return SONAR_OK;
}

// the chromagram on the device and the non-finite flag (the call's status word)
void stage_input(Staging& o, const double* chroma, int64_t F, int32_t dim, sonar::KeyArgs& a) {
  a.chroma = o.in("in", chroma, (size_t)F * (size_t)dim);
  a.nonfinite = o.flag();
}

// the end of an entry: the outputs and the flag are back; a non-finite input is reported
int done(sonar_ctx* c, Staging& o) {
  const int rc = o.finish();
  if (rc != SONAR_OK) return rc;
  if (o.flags())
    return fail(c, SONAR_ERR_UNSUPPORTED,
                "key estimation: a non-finite chroma value is not reproduced (a NaN score leaves the order of "
                "sort.Slice undefined)");
  return SONAR_OK;
}

int common_checks(sonar_ctx* c, const double* chroma, int64_t F, int32_t dim, const sonar_key_params* params) {
  if (F < 0 || dim < 0 || !params)
    return fail(c, SONAR_ERR_INVALID, "key estimation: negative frame count or row length, or null params");
  if (F == 0) return SONAR_OK;
  std::string msg;
  const int rc = check_params(*params, F, dim, msg);
  if (rc != SONAR_OK) return fail(c, rc, msg);
  if (dim > 0 && !chroma) return fail(c, SONAR_ERR_INVALID, "key estimation: null chroma pointer");
  return SONAR_OK;
}

}  // namespace

extern "C" {

void sonar_key_params_default(sonar_key_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->profile = SONAR_KEY_PROFILE_KRUMHANSL;
  p->hpcp_size = 12;
  p->normalize_chroma = 1;
  p->max_candidates = 5;
  p->min_confidence = 0.5;
}

int sonar_key_transition(int32_t from_key, int32_t from_mode, int32_t to_key, int32_t to_mode, int32_t* type,
                         int32_t* semitone_distance, int32_t* fifths_distance, double* strength) {
  const int distance = (to_key - from_key + 12) % 12;                                   // :847
  const int t = sonar::key_transition_type(from_key, from_mode, to_key, to_mode);
  int fifths = 0;                                                                       // :875-888
  if (t == SONAR_KEY_TRANSITION_RELATIVE || t == SONAR_KEY_TRANSITION_DOMINANT || t == SONAR_KEY_TRANSITION_SUBDOMINANT)
    fifths = 1;
  else if (t == SONAR_KEY_TRANSITION_DISTANT)
    fifths = distance < 12 - distance ? distance : 12 - distance;
  if (type) *type = t;
  if (semitone_distance) *semitone_distance = distance;
  if (fifths_distance) *fifths_distance = fifths;
  if (strength) *strength = 1.0 / (1.0 + (double)fifths);                               // :891
  return SONAR_OK;
}

int sonar_key_frames(sonar_ctx* c, const double* chroma, int64_t F, int32_t dim, const sonar_key_params* params,
                     int32_t* key, int32_t* mode, int32_t* known, double* confidence, double* strength,
                     double* clarity, double* ambiguity, double* tonality, double* scores, int32_t* candidates,
                     double* processed, int32_t device_ptrs) {
  if (!c) return SONAR_ERR_INVALID;
  int rc = common_checks(c, chroma, F, dim, params);
  if (rc != SONAR_OK || F == 0) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  Staging o{c, "key.", device_ptrs != 0};
  sonar::KeyArgs a{};
  base_args(*params, dim, a);
  rc = device_tables(c, *params, dim, &a);
  if (rc != SONAR_OK) return rc;
  stage_input(o, chroma, F, dim, a);
  a.F = F;
  frame_outs(o, {key, mode, known, confidence, strength, clarity, ambiguity, tonality, scores, candidates, processed},
             (size_t)F, a, a);
  rc = o.ready("device allocation failed");
  if (rc != SONAR_OK) return rc;
  hipEvent_t tend = timed_begin(c, c->stream);
  rc = launch_rows(c, a);
  if (rc != SONAR_OK) return rc;
  timed_end(c, c->stream, tend);
  return done(c, o);
}

int sonar_key_sequence(sonar_ctx* c, const double* chroma, int64_t F, int32_t dim, const sonar_key_params* params,
                       int32_t* key, int32_t* mode, int32_t* known, double* confidence, double* strength,
                       double* clarity, double* ambiguity, double* tonality, double* scores, double* processed,
                       double* stability, int32_t* modulations, int64_t* n_modulations, int32_t device_ptrs) {
  if (!c) return SONAR_ERR_INVALID;
  if (F < 0 || dim < 0 || !params)
    return fail(c, SONAR_ERR_INVALID, "key estimation: negative frame count or row length, or null params");
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  Staging o{c, "key.", device_ptrs != 0};
  if (F == 0) {                                             // :251-253: the zero result
    const size_t hs = params->hpcp_size > 0 ? (size_t)params->hpcp_size : 0;
    return o.zero({{key, 4}, {mode, 4}, {known, 4}, {confidence, 8}, {strength, 8}, {clarity, 8}, {ambiguity, 8},
                   {tonality, 8}, {scores, 24 * 8}, {processed, hs * 8}, {stability, 8}, {n_modulations, 8}});
  }
  int rc = common_checks(c, chroma, F, dim, params);
  if (rc != SONAR_OK) return rc;
  sonar::KeyArgs base{};
  base_args(*params, dim, base);
  rc = device_tables(c, *params, dim, &base);
  if (rc != SONAR_OK) return rc;
  stage_input(o, chroma, F, dim, base);
  const double* din = base.chroma;
  // the average row and its estimate
  double* avg = o.tmp<double>("avg", (size_t)dim);
  sonar::KeyArgs one = base;
  one.chroma = avg;
  one.F = 1;
  frame_outs(o, {key, mode, known, confidence, strength, clarity, ambiguity, tonality, scores, nullptr, processed}, 1,
             base, one);
  // every frame's code
  int32_t* code = o.tmp<int32_t>("code", (size_t)F);
  double* dstab = o.out("stability", stability, 1);
  const bool want_mod = modulations || n_modulations;
  const int64_t nw = F > 20 ? F - 20 : 0;                   // positions 10 .. F - 11 (:634)
  int32_t* dmod = o.out("mod", modulations, (size_t)nw);
  int64_t* dnmod = o.out("nmod", n_modulations, 1);
  int32_t* wcode = want_mod && nw ? o.tmp<int32_t>("wcode", (size_t)nw) : nullptr;
  double* wconf = want_mod && nw ? o.tmp<double>("wconf", (size_t)nw) : nullptr;
  rc = o.ready("device allocation failed");
  if (rc != SONAR_OK) return rc;
  hipEvent_t tend = timed_begin(c, s);
  if (sonar::launch_key_colsum(din, F, dim, avg, s) != 0) return fail(c, SONAR_ERR_DEVICE, "key average launch failed");
  rc = launch_rows(c, one);
  if (rc != SONAR_OK) return rc;
  sonar::KeyArgs all = base;
  all.F = F;
  all.code = code;
  rc = launch_rows(c, all);                                 // also the non-finite test of every row
  if (rc != SONAR_OK) return rc;
  if (dstab && sonar::launch_key_stability(code, F, dstab, s) != 0)
    return fail(c, SONAR_ERR_DEVICE, "key stability launch failed");
  if (want_mod) {
    if (nw) {
      sonar::KeyArgs w = base;
      w.F = nw;
      w.window = 10;
      w.code = wcode;
      w.conf = wconf;
      rc = launch_rows(c, w);
      if (rc != SONAR_OK) return rc;
      sonar::KeyCompactArgs k{};
      k.code = wcode; k.conf = wconf; k.n = nw; k.transitions = 0; k.frame = dmod; k.count = dnmod;
      if (sonar::launch_key_compact(k, s) != 0) return fail(c, SONAR_ERR_DEVICE, "key modulation launch failed");
    } else if (dnmod) {
      HIP_TRY(c, hipMemsetAsync(dnmod, 0, 8, s));
    }
  }
  timed_end(c, s, tend);
  return done(c, o);
}

int sonar_key_batch(sonar_ctx* c, const double* chroma, int64_t F, int32_t dim, const sonar_key_params* params,
                    int32_t* key, int32_t* mode, int32_t* known, double* confidence, double* strength, double* clarity,
                    double* ambiguity, double* tonality, double* scores, int32_t* candidates, double* processed,
                    int32_t* global_code, double* global_confidence, double* global_strength, double* votes,
                    int32_t* t_frame, int32_t* t_from, int32_t* t_to, double* t_confidence, int32_t* t_type,
                    int64_t* n_transitions, int32_t device_ptrs) {
  if (!c) return SONAR_ERR_INVALID;
  int rc = common_checks(c, chroma, F, dim, params);
  if (rc != SONAR_OK) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  Staging o{c, "key.", device_ptrs != 0};
  if (F == 0) {                                             // :924-926, :963-965
    const int32_t none = -1;
    if ((rc = o.put(global_code, &none, 4)) != SONAR_OK) return rc;
    return o.zero({{global_confidence, 8}, {global_strength, 8}, {votes, 24 * 8}, {n_transitions, 8}});
  }
  sonar::KeyArgs a{};
  base_args(*params, dim, a);
  rc = device_tables(c, *params, dim, &a);
  if (rc != SONAR_OK) return rc;
  stage_input(o, chroma, F, dim, a);
  a.F = F;
  frame_outs(o, {key, mode, known, confidence, strength, clarity, ambiguity, tonality, scores, candidates, processed},
             (size_t)F, a, a);
  const bool want_global = global_code || global_confidence || global_strength || votes;
  const bool want_trans = t_frame || t_from || t_to || t_confidence || t_type || n_transitions;
  if (want_global || want_trans) {
    a.code = o.tmp<int32_t>("code", (size_t)F);
    if (!a.conf) a.conf = o.tmp<double>("fconf", (size_t)F);
  }
  int32_t* dg = o.out("gcode", global_code, 1);
  double* dgc = o.out("gconf", global_confidence, 1);
  double* dgs = o.out("gstrength", global_strength, 1);
  double* dv = o.out("votes", votes, 24);
  const size_t cap = (size_t)(F - 1);
  sonar::KeyCompactArgs k{};
  k.frame = o.out("tframe", t_frame, cap);
  k.from = o.out("tfrom", t_from, cap);
  k.to = o.out("tto", t_to, cap);
  k.tconf = o.out("tconf", t_confidence, cap);
  k.type = o.out("ttype", t_type, cap);
  k.count = o.out("ntrans", n_transitions, 1);
  rc = o.ready("device allocation failed");
  if (rc != SONAR_OK) return rc;
  hipEvent_t tend = timed_begin(c, s);
  rc = launch_rows(c, a);
  if (rc != SONAR_OK) return rc;
  if (want_global && sonar::launch_key_votes(a.code, a.conf, F, dv, dg, dgc, dgs, s) != 0)
    return fail(c, SONAR_ERR_DEVICE, "key vote launch failed");
  if (want_trans) {
    k.code = a.code; k.conf = a.conf; k.n = F; k.transitions = 1;
    if (sonar::launch_key_compact(k, s) != 0) return fail(c, SONAR_ERR_DEVICE, "key progression launch failed");
  }
  timed_end(c, s, tend);
  return done(c, o);
}

}  // extern "C"
