// speech_api.cpp -- C++ restatement of the Go orchestration above the GPU seams, speech half.
//
//   sonar_generate_fingerprint      FingerprintGenerator.GenerateFingerprint
//                                   (fingerprint/fingerprint.go:137-236) with the
//                                   ContentAwareConfigManager tables (content_config.go:54-278)
//   sonar_extract_speech_features   SpeechFeatureExtractor.ExtractFeatures
//                                   (fingerprint/extractors/speech.go:135-550)
//
// Every per-frame array is produced by a HIP kernel (sonar_fingerprint, YIN, energy, tilt, stats);
// what the Go code runs sequentially on O(frames) data (YIN temporal tracking, the percentile
// threshold, pauses, onsets, attack times) is host_dsp.cpp's, and this file only calls it.  The
// extractor is: validate, plan (speech_layout.h), reserve, run the chunk pipeline, queue the copies
// back, track, finish on the host.  Formants (lpc_kernels.hip), voice quality (voice_api.cpp) and
// content detection (content_api.cpp) run on their own kernels; fingerprint ID/timestamp metadata is
// not produced.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "ctx.h"
#include "host_dsp.h"
#include "kernels.h"
#include "speech_layout.h"

using sonar::SpeechPlan;
using sonar::detail::dbuf;
using sonar::detail::fail;

namespace {

enum ContentType { CT_MUSIC = 0, CT_NEWS, CT_SPORTS, CT_TALK, CT_MIXED, CT_UNKNOWN };

int to_content_type(const char* s) {   // config.ToContentType (fingerprint/config/config.go:50-65)
  if (!s) return CT_UNKNOWN;
  const std::string v(s);
  if (v == "music") return CT_MUSIC;
  if (v == "news") return CT_NEWS;
  if (v == "sports") return CT_SPORTS;
  if (v == "talk") return CT_TALK;
  if (v == "mixed") return CT_MIXED;
  return CT_UNKNOWN;
}

struct Settings { bool mfcc, speech, temporal; };
// content_config.go:104-278 (sports has no entry -> unknown settings, :68-72)
Settings settings_for(int ct) {
  switch (ct) {
    case CT_MUSIC: return {true, false, false};
    case CT_NEWS: return {true, true, true};
    case CT_TALK: return {true, true, true};
    case CT_MIXED: return {true, true, true};
    default: return {true, false, true};
  }
}

// the extractor's device buffers (cached in the context under these names)
struct SpeechBufs {
  double *pcm, *pre, *mfcc, *spec, *zcr, *energy, *pitch, *conf, *env, *loud, *stats, *tilt, *ent;
};

// one call: its arguments, its plan, its device buffers and its pinned result block
struct SpeechRun {
  sonar_ctx* c;
  const double* pcm;
  int64_t n;
  int32_t sample_rate;
  const sonar_feature_config* fc;
  SpeechPlan p;
  SpeechBufs d;
  double* B;                       // the pinned block; its sections are p.sec
  int64_t CH, NCH;                 // samples per H2D chunk, chunks
  double *yin_pitch, *yin_conf;    // where YIN writes: d.pitch / d.conf, or the block's rows (early tracker)
  bool trk_early;
  std::vector<int64_t> p_end;      // pitch frames complete after chunk k
  double* sec(SpeechPlan::Section s) const { return p.at(B, s); }
  size_t cnt(SpeechPlan::Section s) const { return p.sec[s].cnt; }
};

int reserve(sonar_ctx* c, int64_t n, const SpeechPlan& p, SpeechBufs* b) {
  auto buf = [&](const char* name, int64_t doubles) {
    return (double*)dbuf(c, name, (size_t)std::max<int64_t>(doubles, 1) * 8);
  };
  b->pcm = (double*)dbuf(c, "sx.pcm", n * 8);
  b->pre = (double*)dbuf(c, "sx.pre", n * 8);
  if (!b->pcm || !b->pre) return fail(c, SONAR_ERR_NOMEM, "device allocation failed (pcm)");
  b->mfcc = buf("sx.mfcc", p.F * p.nm);
  b->spec = buf("sx.spec", p.F * 9);
  b->zcr = buf("sx.zcr", p.F);
  b->energy = buf("sx.energy", p.Fe);
  if (!b->mfcc || !b->spec || !b->zcr || !b->energy) return fail(c, SONAR_ERR_NOMEM, "device allocation failed (features)");
  b->pitch = buf("sx.pitch", p.Fp);
  b->conf = buf("sx.conf", p.Fp);
  if (!b->pitch || !b->conf) return fail(c, SONAR_ERR_NOMEM, "device allocation failed (pitch)");
  b->env = buf("sx.env", p.Fenv);
  b->loud = buf("sx.loud", p.Fl);
  if (!b->env || !b->loud) return fail(c, SONAR_ERR_NOMEM, "device allocation failed (envelope)");
  b->stats = buf("sx.stats", sonar::SPEECH_STAT_BLOCKS * 4);
  if (!b->stats) return fail(c, SONAR_ERR_NOMEM, "device allocation failed (stats)");
  b->tilt = buf("sx.tilt", p.Fp);
  if (!b->tilt) return fail(c, SONAR_ERR_NOMEM, "device allocation failed (tilt)");
  b->ent = buf("sx.ent", p.Fe);
  if (!b->ent) return fail(c, SONAR_ERR_NOMEM, "device allocation failed (entropy)");
  return SONAR_OK;
}

int grow_events(sonar_ctx* c, std::vector<hipEvent_t>& v, int64_t cnt) {
  while ((int64_t)v.size() < cnt) {
    hipEvent_t e;
    HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    v.push_back(e);
  }
  return SONAR_OK;
}

// The host PCM crosses PCIe in chunks on the copy stream; once chunk k has landed, every frame whose
// samples lie in [0, end of chunk k) is computed while the next chunk is in flight: pre-emphasis of the
// chunk, the fused STFT kernel + descriptors + ZCR over the frames it completes, the energy / envelope /
// loudness frames, and YIN (1024 / 512) on the side stream.  Frames are independent (the flux reads the
// previous frame's |X| row, already written in stream order), so the results equal the one-shot
// schedule's.  The fused kernel takes frame ranges on the per-frame path (W = 128 .. 2048); other W run
// it once after the last chunk.
int run_pipeline(SpeechRun& r) {
  sonar_ctx* c = r.c;
  const sonar_feature_config* fc = r.fc;
  const SpeechPlan& p = r.p;
  const SpeechBufs& d = r.d;
  const int64_t n = r.n;
  hipStream_t s = c->stream;
  const int W = fc->stft_window_size, H = fc->stft_hop_size, csr = fc->sample_rate;
  // the fused STFT kernel: MFCC + descriptors + ZCR (the energy frames are launched beside it)
  sonar_fp_cfg cfg;
  sonar_fp_cfg_default(&cfg);
  cfg.window_size = W; cfg.hop_size = H; cfg.window_type = fc->window_type;
  cfg.sample_rate = csr;                                          // NewMFCC(config.SampleRate, ...) etc.
  cfg.n_mfcc = p.nm; cfg.n_filters = 26; cfg.use_lifter = 1; cfg.lifter = 22.0;   // NewMFCC defaults (mfcc.go:44-54)
  cfg.low_freq = 0.0; cfg.high_freq = (double)csr / 2.0;
  cfg.preemph_alpha = 0.97;
  cfg.flags = SONAR_FP_SPECTRAL | SONAR_FP_ZCR | (fc->enable_mfcc ? SONAR_FP_MFCC : 0);
  cfg.precision = fc->precision; cfg.pcm_dtype = SONAR_F64; cfg.out_dtype = SONAR_F64; cfg.device_ptrs = 1;
  sonar_fp_out fo;
  std::memset(&fo, 0, sizeof(fo));
  const size_t Fz = (size_t)p.F;
  fo.mfcc = d.mfcc;
  fo.centroid = d.spec; fo.rolloff = d.spec + Fz; fo.bandwidth = d.spec + 2 * Fz; fo.flatness = d.spec + 3 * Fz;
  fo.crest = d.spec + 4 * Fz; fo.slope = d.spec + 5 * Fz; fo.flux = d.spec + 6 * Fz; fo.low_ratio = d.spec + 7 * Fz;
  fo.high_ratio = d.spec + 8 * Fz; fo.zcr = d.zcr;

  if (r.NCH > 1) {
    HIP_TRY(c, hipEventRecord(c->side_ev[0], s));                // the buffers' previous readers
    HIP_TRY(c, hipStreamWaitEvent(c->copy, c->side_ev[0], 0));
  }
  const bool fp_chunks = sonar::fingerprint_supported(W);
  // frames t < total whose samples [t hop, t hop + win) lie below sample b (all of them at the end)
  auto ready = [&](int64_t b, int64_t total, int64_t win, int64_t hop) -> int64_t {
    if (b >= n) return total;
    if (b < win || hop <= 0) return 0;
    return std::min<int64_t>(total, (b - win) / hop + 1);
  };
  // the three energy-type frame sets of the pre-emphasised PCM (the kernel pre-emphasises, alpha 0.97)
  struct EnergyRun { double* out; int64_t total; int win, hop; const char* err; int64_t done; };
  EnergyRun energies[3] = {{d.energy, p.Fe, fc->window_size, fc->hop_size, "energy launch failed", 0},
                           {d.env, p.Fenv, 512, 256, "envelope launch failed", 0},
                           {d.loud, p.Fl, p.lw, p.lh, "loudness launch failed", 0}};
  int64_t done_fp = 0, done_p = 0;
  for (int64_t k = 0; k < r.NCH; ++k) {
    const int64_t a = k * r.CH, b = std::min<int64_t>(n, a + r.CH);
    if (r.NCH > 1) {
      HIP_TRY(c, hipMemcpyAsync(d.pcm + a, r.pcm + a, (size_t)(b - a) * 8, hipMemcpyHostToDevice, c->copy));
      HIP_TRY(c, hipEventRecord(c->chunk_ev[k], c->copy));
      HIP_TRY(c, hipStreamWaitEvent(s, c->chunk_ev[k], 0));
    } else {
      HIP_TRY(c, hipMemcpyAsync(d.pcm, r.pcm, (size_t)n * 8, hipMemcpyHostToDevice, s));
    }
    // preprocessForSpeech: PreEmphasis("speech") alpha 0.97, fresh state (speech.go:238-245)
    if (sonar::launch_preemph(d.pcm, 1, n, 0.97, d.pre, s, a, b) != 0) return fail(c, SONAR_ERR_DEVICE, "preemph launch failed");
    // YIN raw results on the pre-emphasised PCM (extractHarmonicFeatures :464), side stream
    const int64_t pk = ready(b, p.Fp, 1024, 512);
    if (pk > done_p) {
      HIP_TRY(c, hipEventRecord(c->side_ev[0], s));
      HIP_TRY(c, hipStreamWaitEvent(c->side, c->side_ev[0], 0));
      if (sonar::launch_yin(d.pre, n, p.Fp, 512, csr, r.yin_pitch, r.yin_conf, nullptr, c->side, done_p, pk) != 0)
        return fail(c, SONAR_ERR_DEVICE, "yin launch failed");
      done_p = pk;
    }
    const int64_t fk = fp_chunks ? ready(b, p.F, W, H) : (b >= n ? p.F : 0);
    if (fk > done_fp) {
      const int rc = sonar::detail::fingerprint_impl(c, d.pcm, n, &cfg, &fo, true, done_fp, fk);
      if (rc != SONAR_OK) return rc;
      done_fp = fk;
    }
    for (EnergyRun& e : energies) {
      const int64_t ek = ready(b, e.total, e.win, e.hop);
      if (ek > e.done && sonar::launch_energy(d.pcm, 1, n, e.total, e.win, e.hop, 0.97, e.out, 1, s, e.done, ek) != 0)
        return fail(c, SONAR_ERR_DEVICE, e.err);
      e.done = std::max(e.done, ek);
    }
    // the tracker's input: with trk_early, YIN writes this chunk's pitch rows straight into the
    // pinned result block (mapped host memory) and the event marks them complete.  A DMA copy per
    // chunk instead queues behind the next chunk's H2D on the copy engine and serialises the
    // pipeline: 41-42 against 30 ms per hour (profiles/r06r_gf_early_ab.log)
    if (r.trk_early) HIP_TRY(c, hipEventRecord(c->back_ev[k], c->side));
    r.p_end[k] = done_p;
  }
  HIP_TRY(c, hipEventRecord(c->side_ev[1], c->side));
  HIP_TRY(c, hipStreamWaitEvent(s, c->side_ev[1], 0));
  return SONAR_OK;
}

// the whole-signal kernels after the last chunk, then every section the device fills, copied into the block
int queue_results(const SpeechRun& r) {
  sonar_ctx* c = r.c;
  const SpeechBufs& d = r.d;
  hipStream_t s = c->stream;
  // whole-signal statistics of the pre-emphasised PCM: read by detectSpeech and the temporal
  // block only (the music generation config enables neither, content_config.go:108-140)
  if (r.fc->enable_speech_features || r.fc->enable_temporal_features) {
    if (sonar::launch_stats(d.pre, r.n, d.stats, sonar::SPEECH_STAT_BLOCKS, s) != 0)
      return fail(c, SONAR_ERR_DEVICE, "stats launch failed");
  } else {
    HIP_TRY(c, hipMemsetAsync(d.stats, 0, sonar::SPEECH_STAT_BLOCKS * 4 * 8, s));
  }
  if (r.fc->enable_speech_features && sonar::launch_tilt(d.pre, r.n, r.p.Fp, d.tilt, s) != 0)
    return fail(c, SONAR_ERR_DEVICE, "tilt launch failed");
  if (r.p.Fe && sonar::launch_energy_entropy(d.energy, r.p.Fe, d.ent, s) != 0)
    return fail(c, SONAR_ERR_DEVICE, "entropy launch failed");
  // with the early tracker the pitch rows are in the block already
  const struct { SpeechPlan::Section sec; const double* src; bool skip; } copies[] = {
      {SpeechPlan::PITCH_RAW, d.pitch, r.trk_early}, {SpeechPlan::CONF_RAW, d.conf, r.trk_early},
      {SpeechPlan::MFCC, d.mfcc, false},     {SpeechPlan::SPEC, d.spec, false},     {SpeechPlan::ZCR, d.zcr, false},
      {SpeechPlan::ENERGY, d.energy, false}, {SpeechPlan::ENVELOPE, d.env, false},  {SpeechPlan::LOUDNESS, d.loud, false},
      {SpeechPlan::ENTROPY, d.ent, false},   {SpeechPlan::STATS, d.stats, false},   {SpeechPlan::TILT, d.tilt, false},
      {SpeechPlan::HEAD, d.pre, false}};
  for (const auto& cp : copies)
    if (!cp.skip && r.cnt(cp.sec))
      HIP_TRY(c, hipMemcpyAsync(r.sec(cp.sec), cp.src, r.cnt(cp.sec) * 8, hipMemcpyDeviceToHost, s));
  return SONAR_OK;
}

// extractHarmonicFeatures' rows (speech.go:464-509) up to pitch frame hi, from the raw YIN rows in the block
struct HarmonicTrack {
  sonar::host::YinTracker tracker;
  int64_t done = 0;
  void to(const SpeechRun& r, int64_t hi) {
    const int64_t Fp = r.p.Fp;
    double* pe = r.sec(SpeechPlan::TRACK);
    double *pc = pe + Fp, *vs = pc + Fp, *hr = vs + Fp, *ih = hr + Fp, *tcen = ih + Fp;
    sonar::host::track_rows(tracker, r.sec(SpeechPlan::PITCH_RAW), r.sec(SpeechPlan::CONF_RAW), done, hi, r.n, pe, pc, vs);
    for (int64_t i = done; i < hi; i++) {
      hr[i] = vs[i] * 10.0;
      ih[i] = 1.0 - vs[i];
      tcen[i] = pe[i] > 0 ? pe[i] : 0.0;
    }
    done = std::max(done, hi);
  }
};

// AnalyzeSpeech -> FormantAnalyzer.AnalyzeFormants(preprocessed PCM) (speech_analysis.go:70-74,
// format.go:85-124); a failed analysis leaves FormantResult nil (speech.go:297-303)
int formants(const SpeechRun& r, std::vector<double>* freqs, double* vtl) {
  sonar_ctx* c = r.c;
  hipStream_t s = c->stream;
  const int csr = r.fc->sample_rate;
  const int W = csr >= 16000 ? 2048 : 1024, p = 12 + csr / 1000;
  sonar_formant_frame* dfm = (sonar_formant_frame*)dbuf(c, "sx.formant", sizeof(sonar_formant_frame));
  double* dham = (double*)dbuf(c, "sx.ham", W * 8);
  if (!dfm || !dham) return fail(c, SONAR_ERR_NOMEM, "device allocation failed");
  std::vector<double> ham(W);
  for (int i = 0; i < W; i++) ham[i] = 0.54 - 0.46 * std::cos(2.0 * M_PI * (double)i / (double)(W - 1));
  sonar_formant_frame fm;
  if (hipMemcpyAsync(dham, ham.data(), W * 8, hipMemcpyHostToDevice, s) != hipSuccess ||
      p > 64 || sonar::launch_formants(r.d.pre, 1, 0, W, p, csr, r.n >= W ? 1 : 0, dham, dfm, nullptr, nullptr, s) != 0 ||
      hipMemcpyAsync(&fm, dfm, sizeof(fm), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return fail(c, SONAR_ERR_DEVICE, "formant launch failed");
  if (fm.status == 0) {
    freqs->assign(fm.frequency, fm.frequency + fm.n_formants);
    *vtl = fm.vocal_tract_length;
  }
  return SONAR_OK;
}

// what finish() reads more than once: the energy frames, their silence threshold and ratio (computed
// when a block asks for them), the whole-signal sums
struct Tail {
  const double* energy;
  size_t Fe;
  double silence = 0.0, thr10 = 0.0;
  double peak = 0, sabs = 0, ssq = 0, cross = 0;
};

// extractSpeechFeatures (speech.go:272-313); the tracker's voicing pass runs here, before the harmonic pass
int speech_block(const SpeechRun& r, const Tail& t, sonar::host::YinTracker& tracker, sonar_result* res) {
  const int csr = r.fc->sample_rate;
  const bool sp = sonar::host::detect_speech(r.n, csr, t.cross, t.ssq, r.sec(SpeechPlan::HEAD), (int64_t)r.cnt(SpeechPlan::HEAD));
  res->scalar("is_speech", sp ? 1.0 : 0.0);
  std::vector<double> freqs;
  double vtl = 17.5;
  if (sp) {
    const int rc = formants(r, &freqs, &vtl);
    if (rc != SONAR_OK) return rc;
  }
  res->put("formant_frequencies", freqs, freqs.empty() ? 0 : 1, (int64_t)freqs.size());   // convertFormantData
  res->scalar("vocal_tract_length", vtl);
  // AnalyzeSpeech -> VoiceQualityAnalyzer.AnalyzeVoiceQuality(preprocessed PCM) (speech_analysis.go:76-80);
  // a failed analysis leaves VoiceQualityResult nil and Jitter/Shimmer 0 (speech.go:287-288, 306-309)
  double jitter = 0.0, shimmer = 0.0;
  if (sp) {
    sonar_voice_quality_result vq;
    const int rc = sonar::detail::voice_quality(r.c, r.d.pre, r.n, csr, &vq);
    if (rc == SONAR_ERR_DEVICE || rc == SONAR_ERR_NOMEM) return rc;
    if (rc == SONAR_OK) { jitter = vq.jitter; shimmer = vq.shimmer; }
  }
  res->scalar("jitter", jitter);
  res->scalar("shimmer", shimmer);
  // estimateSpeechRate (speech.go:779-797) on the energy frames of the pre-emphasised PCM
  res->scalar("speech_rate", sp ? sonar::host::speech_rate(t.silence, r.n, csr) : 0.0);
  if (sp) {
    std::vector<double> voicing((size_t)r.p.Fp);                   // extractVoicingProbability (:530-550)
    sonar::host::track_rows(tracker, r.sec(SpeechPlan::PITCH_RAW), r.sec(SpeechPlan::CONF_RAW), 0, r.p.Fp, r.n, nullptr,
                            nullptr, voicing.data());
    res->vec("voicing_probability", voicing);
    res->put_ext("spectral_tilt", r.sec(SpeechPlan::TILT), (int64_t)r.cnt(SpeechPlan::TILT), 1);
    res->vec("pause_duration", t.Fe ? sonar::host::pause_durations(t.energy, t.Fe, t.thr10, r.fc->hop_size, csr)
                                    : std::vector<double>());
  }
  return SONAR_OK;
}

// extractTemporalFeatures (speech.go:370-409)
void temporal_block(const SpeechRun& r, const Tail& t, double lrange, sonar_result* res) {
  res->put_ext("rms_energy", t.energy, (int64_t)t.Fe, 1);
  res->scalar("dynamic_range", lrange);
  res->scalar("silence_ratio", t.silence);
  res->scalar("peak_amplitude", t.peak);
  res->scalar("average_amplitude", r.n > 0 ? t.sabs / (double)r.n : 0.0);
  const std::vector<int64_t> onsets = sonar::host::detect_onsets(t.energy, t.Fe);
  res->scalar("onset_density", (double)onsets.size() / ((double)r.n / (double)r.sample_rate));
  res->vec("attack_time", sonar::host::attack_times(onsets, t.energy, r.fc->hop_size, r.fc->sample_rate));
  res->put_ext("envelope_shape", r.sec(SpeechPlan::ENVELOPE), (int64_t)r.cnt(SpeechPlan::ENVELOPE), 1);
}

// everything after the stream synchronisation: the result's arrays over the block, and the sequential tail
int finish(const SpeechRun& r, HarmonicTrack& track, sonar_result* res) {
  const sonar_feature_config* fc = r.fc;
  const SpeechPlan& p = r.p;
  const int64_t F = p.F;
  const size_t Fz = (size_t)F;
  const double* spec = r.sec(SpeechPlan::SPEC);
  if (fc->enable_mfcc) res->put_ext("mfcc", r.sec(SpeechPlan::MFCC), F, p.nm);
  static const char* spec_names[7] = {"spectral_centroid", "spectral_rolloff", "spectral_bandwidth", "spectral_flatness",
                                      "spectral_crest", "spectral_slope", "spectral_flux"};
  for (int d = 0; d < 7; d++) {
    if (d == 6 && F <= 1) continue;                               // flux only when TimeFrames > 1 (:362-365)
    res->put_ext(spec_names[d], spec + d * Fz, d == 6 ? F - 1 : F, 1);
  }
  res->put_ext("zero_crossing_rate", r.sec(SpeechPlan::ZCR), (int64_t)r.cnt(SpeechPlan::ZCR), 1);

  Tail t{r.sec(SpeechPlan::ENERGY), r.cnt(SpeechPlan::ENERGY)};
  // whole-signal stats: partials reduced in block order (sign changes at block boundaries are counted
  // inside each block: i > 0 uses y[i-1])
  const double* part = r.sec(SpeechPlan::STATS);
  for (int b = 0; b < sonar::SPEECH_STAT_BLOCKS; b++) {
    t.peak = std::max(t.peak, part[4 * b]); t.sabs += part[4 * b + 1]; t.ssq += part[4 * b + 2]; t.cross += part[4 * b + 3];
  }
  if (t.Fe && (fc->enable_speech_features || fc->enable_temporal_features)) {
    t.thr10 = sonar::host::percentile10_threshold(t.energy, t.Fe);
    t.silence = sonar::host::silence_ratio(t.energy, t.Fe, t.thr10);
  }
  if (fc->enable_speech_features) {
    const int rc = speech_block(r, t, track.tracker, res);
    if (rc != SONAR_OK) return rc;
  }
  const double* loud = r.sec(SpeechPlan::LOUDNESS);
  const double lrange = fc->sample_rate > 0 ? sonar::host::loudness_range_from_rms(
                                                   std::vector<double>(loud, loud + r.cnt(SpeechPlan::LOUDNESS)))
                                             : 0.0;
  if (fc->enable_temporal_features) temporal_block(r, t, lrange, res);

  // ---- energy features (extractEnergyFeatures :411-461) -------------------------
  res->put_ext("short_time_energy", t.energy, (int64_t)t.Fe, 1);
  res->scalar("energy_variance", sonar::host::energy_variance(t.energy, t.Fe));
  res->scalar("loudness_range", lrange);
  res->put_ext("energy_entropy", r.sec(SpeechPlan::ENTROPY), (int64_t)r.cnt(SpeechPlan::ENTROPY), 1);
  if (!p.lohi_copy()) {                                           // every energy frame has a spectrogram row
    res->put_ext("low_energy_ratio", spec + 7 * Fz, (int64_t)t.Fe, 1);
    res->put_ext("high_energy_ratio", spec + 8 * Fz, (int64_t)t.Fe, 1);
  } else {
    double* lo = r.sec(SpeechPlan::LOHI);
    double* hi = lo + t.Fe;
    for (size_t i = 0; i < t.Fe; i++) {
      lo[i] = (int64_t)i < F ? spec[7 * Fz + i] : 0.0;
      hi[i] = (int64_t)i < F ? spec[8 * Fz + i] : 0.0;
    }
    res->put_ext("low_energy_ratio", lo, (int64_t)t.Fe, 1);
    res->put_ext("high_energy_ratio", hi, (int64_t)t.Fe, 1);
  }

  // ---- harmonic features (extractHarmonicFeatures :464-509) --------------------
  track.to(r, p.Fp);                                              // the rest (all of it after the speech block)
  static const char* track_names[6] = {"pitch_estimate", "pitch_confidence", "voicing_strength", "harmonic_ratio",
                                       "inharmonicity_ratio", "tonal_centroid"};
  for (int d = 0; d < 6; d++) res->put_ext(track_names[d], r.sec(SpeechPlan::TRACK) + d * p.Fp, p.Fp, 1);
  return SONAR_OK;
}

}  // namespace

extern "C" {

void sonar_fingerprint_config_default(sonar_fingerprint_config* c) {   // fingerprint.go:70-98
  std::memset(c, 0, sizeof(*c));
  c->window_size = 2048;
  c->hop_size = 512;
  c->feature_window_size = 0;    // FeatureConfig.WindowSize is unset in the default config (F13)
  c->feature_hop_size = 0;
  c->enable_content_detect = 1;
  c->window_type = SONAR_WIN_HANN;
  c->precision = SONAR_F64;
  c->acoustic_detection = 1;     // ContentConfig (fingerprint.go:92-96)
  c->default_content_type = SONAR_CT_UNKNOWN;
  c->auto_detect_threshold = 2.0;
}

void sonar_feature_config_default(sonar_feature_config* c) {
  std::memset(c, 0, sizeof(*c));
  c->stft_window_size = 1024;
  c->stft_hop_size = 256;
  c->window_type = SONAR_WIN_HANN;
  c->enable_mfcc = 1;
  c->mfcc_coefficients = 13;
  c->is_news = 1;
  c->precision = SONAR_F64;
}

// ------------------------------------------------ SpeechFeatureExtractor ----
int sonar_extract_speech_features(sonar_ctx* c, const double* pcm, int64_t n, int32_t sample_rate,
                                  const sonar_feature_config* fc, sonar_result** out) {
  if (!c || !fc || !out) return fail(c, SONAR_ERR_INVALID, "null argument");
  *out = nullptr;
  if (n <= 0 || !pcm) return fail(c, SONAR_ERR_EMPTY, "PCM data cannot be empty");
  if (sample_rate <= 0) return fail(c, SONAR_ERR_INVALID, "sample rate must be positive");
  const int W = fc->stft_window_size, H = fc->stft_hop_size;
  const int64_t F = sonar_stft_frames(n, W, H);
  if (F == SONAR_ERR_EMPTY) return fail(c, SONAR_ERR_EMPTY, "empty signal");
  if (F == SONAR_ERR_INVALID) return fail(c, SONAR_ERR_INVALID, W <= 0 ? "window size must be positive" : "hop size must be positive");
  if (F < 0) return fail(c, SONAR_ERR_TOO_SHORT, "signal too short for given window size and hop size");
  HIP_TRY(c, hipSetDevice(c->device));

  SpeechRun r{c, pcm, n, sample_rate, fc,
              SpeechPlan(n, F, fc->sample_rate, fc->window_size, fc->hop_size, fc->mfcc_coefficients, fc->enable_mfcc != 0,
                         fc->enable_speech_features != 0)};
  if (const int rc = reserve(c, n, r.p, &r.d)) return rc;
  if (const int rc = sonar::detail::ensure_side(c)) return rc;
  // results: ONE pinned block from the pool, every array copied into it by DMA; the result's large
  // arrays point into the block (no host copy, no page faults on fresh vectors)
  std::shared_ptr<void> blk = sonar::detail::pinned_block(r.p.total * 8);
  if (!blk) return fail(c, SONAR_ERR_NOMEM, "pinned host allocation failed (results)");
  r.B = (double*)blk.get();

  r.CH = n > ((int64_t)24 << 20) ? ((int64_t)8 << 20) : n;                // 8 M samples (64 MB) per chunk
  if (const char* e = std::getenv("SONAR_PCM_CHUNK")) {                   // samples per chunk (tests)
    const long long v = std::atoll(e);
    if (v > 0) r.CH = std::min<int64_t>(n, v);
  }
  r.NCH = (n + r.CH - 1) / r.CH;
  r.p_end.assign(r.NCH, 0);
  if (grow_events(c, c->back_ev, r.NCH)) return SONAR_ERR_DEVICE;
  if (r.NCH > 1) {
    if (!c->copy) HIP_TRY(c, hipStreamCreateWithFlags(&c->copy, hipStreamNonBlocking));
    if (grow_events(c, c->chunk_ev, r.NCH)) return SONAR_ERR_DEVICE;
  }
  // Without the speech block (the GenerateFingerprint content configs for music / news / sports,
  // content_config.go:108-140) the harmonic features' sequential tracker is the only consumer of the
  // pitch frames before the end: it runs chunk by chunk as each chunk's pitch rows land in the block
  // (mapped pinned memory; no device address -> the late order), while the device and PCIe work on.
  // With the speech block its voicing pass must see the tracker first, so the tracker runs after the
  // sync.  SONAR_GF_EARLY=0: after the last chunk in either case.
  const char* gf_env = std::getenv("SONAR_GF_EARLY");
  r.yin_pitch = r.d.pitch; r.yin_conf = r.d.conf;
  r.trk_early = false;
  if (!fc->enable_speech_features && (gf_env ? std::atoi(gf_env) : 1) != 0 && r.p.Fp) {
    void* dB = nullptr;
    if (hipHostGetDevicePointer(&dB, r.B, 0) == hipSuccess && dB) {
      r.yin_pitch = r.p.at((double*)dB, SpeechPlan::PITCH_RAW);
      r.yin_conf = r.p.at((double*)dB, SpeechPlan::CONF_RAW);
      r.trk_early = true;
    } else {
      (void)hipGetLastError();
    }
  }
  // copies into the block are queued on c->stream, and with the early tracker YIN writes into it on the
  // side stream: an early exit drains them before the block goes back to the pool
  sonar::detail::DrainOnExit drain{c, r.NCH > 1, true};
  std::unique_ptr<sonar_result> res(new sonar_result());
  res->hold(blk);

  if (const int rc = run_pipeline(r)) return rc;
  if (const int rc = queue_results(r)) return rc;
  HarmonicTrack track;
  if (r.trk_early) {
    for (int64_t k = 0; k < r.NCH; ++k) {
      HIP_TRY(c, hipEventSynchronize(c->back_ev[k]));
      track.to(r, r.p_end[k]);
    }
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (const int rc = finish(r, track, res.get())) return rc;
  drain.armed = false;             // every stream's work ended with the synchronisations above
  *out = res.release();
  return SONAR_OK;
}

// ------------------------------------------ FingerprintGenerator ------------
int sonar_generate_fingerprint(sonar_ctx* c, const double* pcm, int64_t n, int32_t sample_rate, const char* content_type,
                               const sonar_fingerprint_config* cfg, sonar_result** out) {
  if (!c || !cfg || !out) return fail(c, SONAR_ERR_INVALID, "null argument");
  *out = nullptr;
  int ct = to_content_type(content_type);                         // fingerprint.go:155
  if (ct == CT_UNKNOWN && cfg->enable_content_detect) {           // fingerprint.go:156-158
    int32_t d = CT_UNKNOWN;
    const int rc = sonar::detail::detect_content_type(c, pcm, n, sample_rate, 1, content_type, cfg->genre,
                                                      cfg->station, cfg->url, cfg->acoustic_detection,
                                                      cfg->default_content_type, cfg->auto_detect_threshold, &d);
    if (rc != SONAR_OK) return rc;
    ct = d;
  }
  const Settings st = settings_for(ct);                           // GetGenerationConfig -> buildFeatureConfig
  sonar_feature_config fc;
  sonar_feature_config_default(&fc);
  fc.sample_rate = 0;                                             // F1: SampleRate is never copied (content_config.go:87-103)
  fc.window_size = cfg->feature_window_size;                      // base FeatureConfig.WindowSize/HopSize
  fc.hop_size = cfg->feature_hop_size;
  fc.stft_window_size = cfg->window_size;                         // generationConfig.WindowSize/HopSize (:174-179)
  fc.stft_hop_size = cfg->hop_size;
  fc.window_type = cfg->window_type;
  fc.enable_mfcc = st.mfcc; fc.enable_speech_features = st.speech; fc.enable_temporal_features = st.temporal;
  fc.mfcc_coefficients = 13;
  fc.is_news = ct != CT_TALK;                                     // CreateExtractor (feature_extractor.go:38-62)
  fc.precision = cfg->precision;
  const int rc = sonar_extract_speech_features(c, pcm, n, sample_rate, &fc, out);
  if (rc != SONAR_OK) return rc;
  (*out)->scalar("content_type", (double)ct);
  (*out)->scalar("sample_rate", (double)sample_rate);
  (*out)->scalar("hop_size", (double)cfg->feature_hop_size);       // AudioFingerprint.HopSize (fingerprint.go:215)
  (*out)->scalar("duration_seconds", (double)n / (double)sample_rate);
  return SONAR_OK;
}

}  // extern "C"
