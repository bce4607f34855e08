// chord_api.cpp -- sonar_chord_frames, sonar_chord_sequence, sonar_chord_detect, sonar_chord_progression
// and the host-only sonar_chord_params_default: ChordDetector and ChordProgressionAnalyzer
// (algorithms/tonal/chord_detection.go).  The host side: the argument checks in Go's order, the launch
// sequences over the staged arrays (staging.h) and what the device flags mean.  The templates are
// constants of the reference that no parameter changes; they are compiled into chord_kernels.hip, so
// there is no device table to cache.  sonar_chord_detect composes the float64 STFT magnitudes, the
// mirror kernel and sonar_hpcp_from_spectrum's path in chunks, and leaves the chromagram on the device.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "ctx.h"
#include "kernels.h"
#include "magnitude_walk.h"
#include "staging.h"

using sonar::detail::fail;
using sonar::detail::Staging;
using sonar::detail::timed_begin;
using sonar::detail::timed_end;

namespace {

constexpr int64_t kDetectChunkBytes = 32ll << 20;   // full-length magnitude rows per chunk of sonar_chord_detect

int check_params(const sonar_chord_params& p, int64_t F, int32_t dim, std::string& msg) {
  if (dim != 12 && dim != 24 && dim != 36) {                 // :416-419 over :559-560
    msg = "failed to extract chroma features: unsupported chroma size: " + std::to_string(dim);
    return SONAR_ERR_INVALID;
  }
  if (p.max_candidates < 0) {                                // :458-460: len(candidates) >= 0 > MaxCandidates
    msg = "runtime error: slice bounds out of range [:" + std::to_string(p.max_candidates) + "]";
    return SONAR_ERR_PANIC;
  }
  if (!std::isfinite(p.min_chord_strength) || !std::isfinite(p.bass_weight)) {
    msg = "chord detection: a non-finite min_chord_strength or bass_weight is not reproduced";
    return SONAR_ERR_UNSUPPORTED;
  }
  if (p.temporal_window > sonar::CHORD_MAX_WINDOW) {
    msg = "chord detection: temporal_window above " + std::to_string(sonar::CHORD_MAX_WINDOW) + " is not supported";
    return SONAR_ERR_UNSUPPORTED;
  }
  if (F > INT32_MAX) { msg = "chord detection: more than 2^31 - 1 frames are not supported"; return SONAR_ERR_UNSUPPORTED; }
  return SONAR_OK;
}

void base_args(const sonar_chord_params& p, int32_t dim, sonar::ChordArgs& a) {
  a.dim = dim;
  // DetectChord (:421-445): no bass without UseBassDetection; harmonicAnalysis, cqtBasedDetection and
  // statisticalAnalysis hand templateMatching (0, 0.0)
  a.match_bass = p.use_bass_detection != 0 && !(p.method >= 1 && p.method <= 3);
  a.normalize = p.normalize_templates != 0;
  a.use_inversions = p.use_inversions != 0;
  a.detect_ext = p.detect_extensions != 0;
  a.max_ext = p.max_extension;
  a.functional = p.use_functional_analysis != 0;
  a.smoothing = p.use_temporal_smoothing != 0;
  a.max_cand = p.max_candidates;
  a.min_strength = p.min_chord_strength;
  a.bass_weight = p.bass_weight;
}

template <typename T>
T* out_if(Staging& o, const char* name, T* user, size_t count) {
  return count ? o.out(name, user, count) : nullptr;
}

void frame_outs(Staging& o, const sonar_chord_out& u, size_t F, size_t mc, sonar::ChordArgs& a) {
  a.root = o.out("root", u.root, F);
  a.quality = o.out("quality", u.quality, F);
  a.inversion = o.out("inversion", u.inversion, F);
  a.n_found = o.out("nfound", u.n_found, F);
  a.conf = o.out("conf", u.confidence, F);
  a.strength = o.out("strength", u.strength, F);
  a.clarity = o.out("clarity", u.clarity, F);
  a.ambiguity = o.out("ambiguity", u.ambiguity, F);
  a.consonance = o.out("consonance", u.consonance, F);
  a.tension = o.out("tension", u.tension, F);
  a.stability = o.out("stability", u.stability, F);
  a.ext = o.out("ext", u.extensions, F);
  a.role = o.out("role", u.role, F);
  a.scores = o.out("scores", u.template_scores, F * sonar::CHORD_SLOTS);
  a.cand = out_if(o, "cand", u.candidates, F * mc);
  a.cand_inv = out_if(o, "candinv", u.cand_inversion, F * mc);
  a.cand_conf = out_if(o, "candconf", u.cand_confidence, F * mc);
  a.cand_strength = out_if(o, "candstrength", u.cand_strength, F * mc);
}

int launch_rows(sonar_ctx* c, const sonar::ChordArgs& a) {
  const int rc = sonar::launch_chord_rows(a, c->stream);
  if (rc == -1) return fail(c, SONAR_ERR_UNSUPPORTED, "chord detection: a shape the kernel does not take");
  if (rc != 0) return fail(c, SONAR_ERR_DEVICE, "chord detection launch failed");
  return SONAR_OK;
}

// The launches of one entry over staged arrays: a holds the inputs, the parameters and the outputs.
// sequence: the record pass, the chain, the output pass and the stability pass; else the output pass alone.
int run(sonar_ctx* c, Staging& o, sonar::ChordArgs& a, const sonar_chord_params& p, bool sequence) {
  hipStream_t s = c->stream;
  const int64_t F = a.F;
  const bool smoothing = a.smoothing != 0;
  const bool history = a.stability != nullptr && p.temporal_window > 0 && p.max_candidates > 0;
  const bool chain = sequence && (smoothing || history);
  int32_t *rec = nullptr, *hstate = nullptr, *kidx = nullptr;
  double* kconf = nullptr;
  if (chain) {
    rec = o.tmp<int32_t>("rec", (size_t)F * 4);
    hstate = o.tmp<int32_t>("hstate", (size_t)F);
    kidx = o.tmp<int32_t>("kidx", (size_t)F + 1);
    if (history) kconf = o.tmp<double>("kconf", (size_t)F);
  }
  a.flags = o.flag();
  int rc = o.ready("device allocation failed");
  if (rc != SONAR_OK) return rc;
  hipEvent_t tend = timed_begin(c, s);
  if (chain) {
    sonar::ChordArgs r = a;
    r.record = 1;
    r.rec = rec;
    rc = launch_rows(c, r);
    if (rc != SONAR_OK) return rc;
    if (sonar::launch_chord_chain(rec, F, smoothing, p.temporal_window, p.max_candidates > 0, hstate, kidx, a.flags, s) != 0)
      return fail(c, SONAR_ERR_DEVICE, "chord chain launch failed");
    a.hstate = hstate;
    a.kidx = kidx;
    a.kconf = kconf;
  }
  a.record = 0;
  rc = launch_rows(c, a);
  if (rc != SONAR_OK) return rc;
  if (kconf && sonar::launch_chord_stability(kidx, kconf, F, p.temporal_window, a.stability, s) != 0)
    return fail(c, SONAR_ERR_DEVICE, "chord stability launch failed");
  timed_end(c, s, tend);
  rc = o.finish();
  if (rc != SONAR_OK) return rc;
  const int32_t flags = o.flags();
  if (flags & sonar::CHORD_FLAG_BASS_NOTE) return fail(c, SONAR_ERR_INVALID, "chord detection: a bass note outside 0..11");
  if (flags & sonar::CHORD_FLAG_NONFINITE)
    return fail(c, SONAR_ERR_UNSUPPORTED,
                "chord detection: a non-finite chroma value or bass confidence is not reproduced (a NaN "
                "confidence leaves the order of sort.Slice undefined)");
  if (flags & sonar::CHORD_FLAG_SLICE_PANIC) return fail(c, SONAR_ERR_PANIC, "runtime error: slice bounds out of range [1:0]");
  return SONAR_OK;
}

int rows_entry(sonar_ctx* c, const double* chroma, int64_t F, int32_t dim, const int32_t* bass_note,
               const double* bass_confidence, const sonar_chord_params* params, const sonar_chord_out* out,
               int32_t device_ptrs, bool sequence) {
  if (!c) return SONAR_ERR_INVALID;
  if (F < 0 || !params || !out)
    return fail(c, SONAR_ERR_INVALID, "chord detection: negative frame count, null params or null outputs");
  if (F == 0) return SONAR_OK;
  std::string msg;
  int rc = check_params(*params, F, dim, msg);
  if (rc != SONAR_OK) return fail(c, rc, msg);
  if (!chroma) return fail(c, SONAR_ERR_INVALID, "chord detection: null chroma pointer");
  HIP_TRY(c, hipSetDevice(c->device));
  Staging o{c, "chord.", device_ptrs != 0};
  sonar::ChordArgs a{};
  base_args(*params, dim, a);
  a.F = F;
  a.chroma = o.in("in", chroma, (size_t)F * (size_t)dim);
  a.bass_note = o.in("bassnote", bass_note, (size_t)F);
  a.bass_conf = o.in("bassconf", bass_confidence, (size_t)F);
  frame_outs(o, *out, (size_t)F, (size_t)params->max_candidates, a);
  return run(c, o, a, *params, sequence);
}

bool power_of_two(int32_t w) { return w > 0 && (w & (w - 1)) == 0; }

}  // namespace

extern "C" {

void sonar_chord_params_default(sonar_chord_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->method = SONAR_CHORD_TEMPLATE_MATCHING;
  p->normalize_templates = 1;
  p->use_inversions = 1;
  p->max_candidates = 5;
  p->use_bass_detection = 1;
  p->detect_extensions = 1;
  p->max_extension = 13;
  p->use_temporal_smoothing = 1;
  p->temporal_window = 5;
  p->min_chord_strength = 0.2;
  p->bass_weight = 0.3;
}

int sonar_chord_frames(sonar_ctx* c, const double* chroma, int64_t F, int32_t dim, const int32_t* bass_note,
                       const double* bass_confidence, const sonar_chord_params* params, const sonar_chord_out* out,
                       int32_t device_ptrs) {
  return rows_entry(c, chroma, F, dim, bass_note, bass_confidence, params, out, device_ptrs, false);
}

int sonar_chord_sequence(sonar_ctx* c, const double* chroma, int64_t F, int32_t dim, const int32_t* bass_note,
                         const double* bass_confidence, const sonar_chord_params* params, const sonar_chord_out* out,
                         int32_t device_ptrs) {
  return rows_entry(c, chroma, F, dim, bass_note, bass_confidence, params, out, device_ptrs, true);
}

int sonar_chord_detect(sonar_ctx* c, const double* pcm, int64_t n, int32_t sample_rate, int32_t frame_len, int32_t hop,
                       const int32_t* bass_note, const double* bass_confidence, const sonar_chord_params* params,
                       const sonar_chord_out* out, double* hpcp, int64_t* frames, int32_t device_ptrs) {
  if (!c) return SONAR_ERR_INVALID;
  if (!params || !out) return fail(c, SONAR_ERR_INVALID, "chord detection: null params or null outputs");
  if (frame_len <= 0 || hop <= 0 || n < 0)
    return fail(c, SONAR_ERR_INVALID, "chord detection: frame length and hop must be positive");
  if (n < frame_len) return fail(c, SONAR_ERR_TOO_SHORT, "signal too short for given frame length");
  const sonar_chord_params& p = *params;
  const int64_t F = (n - frame_len) / hop + 1;
  const int32_t W = frame_len < 2048 ? frame_len : 2048;    // :512-519
  std::string msg;
  int rc = check_params(p, F, 12, msg);
  if (rc != SONAR_OK) return fail(c, rc, msg);
  if (p.method == SONAR_CHORD_CQT_BASED)
    return fail(c, SONAR_ERR_UNSUPPORTED, "chord detection: method cqt_based is not supported on PCM");
  if (!power_of_two(W))
    return fail(c, SONAR_ERR_UNSUPPORTED, "chord detection: the frame's window must be a power of two");
  const bool bass_frames = frame_len == 1024;               // DetectPitch takes no other length (F53)
  if (bass_frames && p.use_bass_detection && (!bass_note || !bass_confidence))
    return fail(c, SONAR_ERR_UNSUPPORTED,
                "chord detection: at frame length 1024 with use_bass_detection the bass arrays must be given "
                "(the pitch detector's state is not reproduced)");
  const int64_t used = (F - 1) * (int64_t)hop + W;          // every frame's first W samples lie inside it
  sonar::detail::MagnitudeWalk walk;
  rc = walk.plan(sample_rate, W, hop, SONAR_WIN_RECTANGULAR, used, pcm != nullptr, &msg);
  if (rc != SONAR_OK) return fail(c, rc, msg);
  if (walk.F != F) return fail(c, SONAR_ERR_UNSUPPORTED, "chord detection: the STFT path frames this signal differently");
  walk.chunk_frames = std::max<int64_t>(kDetectChunkBytes / ((int64_t)W * 8), 1);
  if (frames) *frames = F;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  Staging o{c, "chord.", device_ptrs != 0};
  const double* dx = o.in("pcm", pcm, (size_t)n);
  double* dh = hpcp ? o.out("hpcp", hpcp, (size_t)F * 12) : o.tmp<double>("hpcp", (size_t)F * 12);
  walk.alloc(o, 0, "half");
  double* full = o.tmp<double>("full", (size_t)std::min(walk.chunk_frames, F) * (size_t)W);
  sonar::ChordArgs a{};
  base_args(p, 12, a);
  a.F = F;
  a.chroma = dh;
  if (bass_frames) {
    a.bass_note = o.in("bassnote", bass_note, (size_t)F);
    a.bass_conf = o.in("bassconf", bass_confidence, (size_t)F);
  }
  frame_outs(o, *out, (size_t)F, (size_t)p.max_candidates, a);
  rc = o.ready("device allocation failed");
  if (rc != SONAR_OK) return rc;
  sonar_hpcp_params hp;
  sonar_hpcp_params_default(&hp);                           // NewHPCP(sampleRate) (:255)
  rc = walk.each(c, dx, used, false, [&](const double* half, int64_t f0, int64_t nf) {
    if (sonar::launch_chord_mirror(half, nf, W, full, s) != 0) return fail(c, SONAR_ERR_DEVICE, "chord mirror launch failed");
    return sonar_hpcp_from_spectrum(c, full, nf, W, W, sample_rate, &hp, dh + f0 * 12, nullptr, nullptr, 1);
  });
  if (rc != SONAR_OK) return rc;
  return run(c, o, a, p, true);
}

int sonar_chord_progression(sonar_ctx* c, const int32_t* root, const int32_t* quality, const int32_t* inversion,
                            const double* confidence, int64_t F, int64_t* num_chords, int32_t* insufficient_data,
                            double* average_confidence, int32_t* most_common_quality, int32_t device_ptrs) {
  (void)root;
  (void)inversion;
  if (F < 0) return c ? fail(c, SONAR_ERR_INVALID, "chord progression: negative chord count") : SONAR_ERR_INVALID;
  const int32_t insufficient = F < 2 ? 1 : 0;               // :1129-1134
  if (!device_ptrs) {
    if (num_chords) *num_chords = F;
    if (insufficient_data) *insufficient_data = insufficient;
    if (insufficient) return SONAR_OK;
  }
  if (!c) return SONAR_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  Staging o{c, "chordprog.", device_ptrs != 0};
  if (device_ptrs) {
    int rc = o.put(num_chords, &F, 8);
    if (rc == SONAR_OK) rc = o.put(insufficient_data, &insufficient, 4);
    if (rc != SONAR_OK) return rc;
    if (insufficient) return o.finish();                    // nothing to copy back: the wait for the two uploads
  }
  if (F > INT32_MAX) return fail(c, SONAR_ERR_UNSUPPORTED, "chord progression: more than 2^31 - 1 chords are not supported");
  if (!quality || !confidence) return fail(c, SONAR_ERR_INVALID, "chord progression: null quality or confidence pointer");
  const int32_t* dq = o.in("quality", quality, (size_t)F);
  const double* dc = o.in("conf", confidence, (size_t)F);
  double* davg = o.out("avg", average_confidence, 1);
  int32_t* dmost = o.out("most", most_common_quality, 1);
  int32_t* dflags = o.flag();
  int rc = o.ready("device allocation failed");
  if (rc != SONAR_OK) return rc;
  hipEvent_t tend = timed_begin(c, s);
  if (sonar::launch_chord_progression(dq, dc, F, davg, dmost, dflags, s) != 0)
    return fail(c, SONAR_ERR_DEVICE, "chord progression launch failed");
  timed_end(c, s, tend);
  rc = o.finish();
  if (rc != SONAR_OK) return rc;
  const int32_t flags = o.flags();
  if (flags & sonar::CHORD_FLAG_QUALITY) return fail(c, SONAR_ERR_UNSUPPORTED, "chord progression: a quality code outside 0..31");
  if (flags & sonar::CHORD_FLAG_NONFINITE) return fail(c, SONAR_ERR_UNSUPPORTED, "chord progression: a non-finite confidence");
  return SONAR_OK;
}

}  // extern "C"
