// music_api.cpp -- MusicFeatureExtractor.ExtractFeatures (fingerprint/extractors/music.go:178-583)
// as one C entry: NewMusicFeatureExtractor(cfg) (:70-137) + ExtractFeatures(STFT(pcm, W, H), pcm,
// sample_rate); and its energy + chroma alone (sonar_music_alignment_features), which the alignment
// entries run on both streams of a pair.  Every per-sample and per-frame pass runs on the device (the
// fused STFT kernel for the spectrogram's descriptors and |X|^4 MFCC, music_kernels.hip for the spectral
// contrast and the band energy ratios, the DC / pre-emphasis scan, chroma and energy kernels of the
// alignment path); the host runs only Go's O(frames) scalar tails, which are host_dsp.cpp's.  The entry is
// validate and plan (music_plan.h) / reserve / launches / copies back / result assembly.
//
// The reference panics inside extractTemporalFeatures for almost every input (DESIGN.md F15 and
// Kernel 10): music.go:403 passes the percentiles 10 and 90 where
// DynamicRange.calculatePercentileRange (temporal/dynamic_range.go:58-76) expects fractions, so
// int(10 * (L - 1)) indexes past the L RMS frames (1024 / 512) of any signal with L >= 2
// (n >= 1536 samples); and a signal with no energy frame divides by zero at music.go:383.  Such a
// call returns SONAR_ERR_PANIC with Go's runtime message, and *out holds the arrays the Go call
// had computed before the panic (spectral features, MFCC, chroma, rms_energy, envelope_shape,
// peak / average amplitude); Go itself returns nothing.  A FeatureConfig hop above the
// spectrogram's panics earlier, in extractChromaFeatures (slice bounds, :348-352), after the
// spectral features and the MFCC.  Below 1536 samples every group is
// computed as in Go, the harmonic block zero by F7 unless the frame is exactly 1024 samples.
#include "../../include/sonar_gpu.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "ctx.h"
#include "host_dsp.h"
#include "kernels.h"
#include "music_plan.h"
#include "staging.h"

using sonar::MusicPlan;
using sonar::kContrastBands;
using sonar::detail::fail;
using sonar::detail::Staging;

namespace {

// scratch of preprocessAudio under a Staging's prefix: the prefix is the call's tag, so two calls on
// different streams (sonar_align_pair_device) do not share it
struct PreScratch { double *y, *dcs; };
PreScratch reserve_pre(Staging& st, int64_t n) {
  PreScratch p;
  p.y = st.tmp<double>("pre", n);                                 // processedPCM
  p.dcs = (double*)st.tmp<char>("dcscratch", sonar::dc_preemph_scratch_bytes(n));
  return p;
}

// preprocessAudio (music.go:245-259: DC removal, pre-emphasis 0.95) of dp into p.y, then ShortTimeEnergy
// (:460-466, Fe frames of fw / fh into de) and the chroma (:327-376, F rows into dc at chroma_sr) of p.y,
// on c->stream.  dc null: no chroma.
int preprocess_energy_chroma(sonar_ctx* c, const double* dp, int64_t n, const PreScratch& p, int64_t F, int64_t Fe,
                             int32_t fw, int32_t fh, int32_t chroma_sr, double* de, double* dc) {
  if (sonar::launch_dc_preemph(dp, n, 0.995, 0.95, p.y, p.dcs, c->stream) != 0)
    return fail(c, SONAR_ERR_DEVICE, "dc launch failed");
  // ShortTimeEnergy of the already pre-emphasised signal: alpha 0 makes the kernel's
  // pre-emphasis the identity (x - 0 * x[n-1] == x exactly)
  if (Fe > 0 && sonar::launch_energy(p.y, 1, n, Fe, fw, fh, 0.0, de, 1, c->stream) != 0)
    return fail(c, SONAR_ERR_DEVICE, "energy launch failed");
  return dc ? sonar_chroma_stft(c, p.y, n, F, fh, chroma_sr, 0, dc, 1) : SONAR_OK;
}

// one call of the extractor: its arguments, its plan, its device buffers and what came back
struct MusicRun {
  sonar_ctx* c;
  int64_t n;
  const sonar_feature_config* fc;
  MusicPlan p;
  const double* pcm;               // on the device
  PreScratch pre;
  double *mag, *mfcc, *spec, *con, *lh, *chroma, *energy, *abs, *env, *peak, *yin;
  int* edges;
  struct { std::vector<double> mfcc, spec, con, lh, chroma, energy, env, abs, peak, yin; } h;
};

int reserve(MusicRun& r, const double* pcm) {
  const MusicPlan& p = r.p;
  const size_t F = (size_t)p.F, Fe1 = (size_t)std::max<int64_t>(p.Fe, 1);
  Staging st{r.c, "mx.", false};
  r.pcm = st.in("pcm", pcm, r.n);
  r.pre = reserve_pre(st, r.n);
  r.mag = st.tmp<double>("mag", F * p.K);
  r.mfcc = st.tmp<double>("mfcc", F * 13);
  r.spec = st.tmp<double>("spec", F * 9);
  r.edges = st.tmp<int>("edges", 16);
  r.con = st.tmp<double>("contrast", F * kContrastBands);
  r.lh = st.tmp<double>("lohi", F * 2);
  r.chroma = st.tmp<double>("chroma", F * 12);
  r.energy = st.tmp<double>("energy", Fe1);
  r.abs = st.tmp<double>("abs", 2);
  r.env = st.tmp<double>("env", (size_t)std::max<int64_t>(p.Fenv, 1));
  r.peak = st.tmp<double>("peak", Fe1);
  r.yin = st.tmp<double>("yin", 2);
  return st.ready("device allocation failed (music features)");
}

// the spectrogram's features in one fused launch: descriptors (:270-299), |X|^4 MFCC with 13
// coefficients over 26 mel filters (:105-114, :304-325, F5), and the magnitude rows; then the spectral
// contrast and extractEnergyFeatures' band ratios per magnitude row
int launch_spectral(MusicRun& r) {
  sonar_ctx* c = r.c;
  const sonar_feature_config* fc = r.fc;
  const int64_t F = r.p.F;
  sonar_fp_cfg cfg;
  sonar_fp_cfg_default(&cfg);
  cfg.window_size = fc->stft_window_size; cfg.hop_size = fc->stft_hop_size; cfg.window_type = fc->window_type;
  cfg.sample_rate = fc->sample_rate;                              // m.config.SampleRate
  cfg.n_mfcc = 13; cfg.n_filters = 26; cfg.use_lifter = 1; cfg.lifter = 22.0;
  cfg.low_freq = 0.0; cfg.high_freq = (double)fc->sample_rate / 2.0;
  cfg.mfcc_input_power = 1;                                       // MFCC.Compute fed |X|^2 (F5)
  cfg.flags = SONAR_FP_MFCC | SONAR_FP_SPECTRAL | SONAR_FP_MAGNITUDE;
  cfg.precision = fc->precision; cfg.pcm_dtype = SONAR_F64; cfg.out_dtype = SONAR_F64; cfg.device_ptrs = 1;
  sonar_fp_out fo;
  std::memset(&fo, 0, sizeof(fo));
  double* s = r.spec;
  fo.mfcc = r.mfcc; fo.magnitude = r.mag;
  fo.centroid = s; fo.rolloff = s + F; fo.bandwidth = s + 2 * F; fo.flatness = s + 3 * F;
  fo.crest = s + 4 * F; fo.slope = s + 5 * F; fo.flux = s + 6 * F; fo.low_ratio = s + 7 * F;
  fo.high_ratio = s + 8 * F;
  const int rc = sonar_fingerprint(c, r.pcm, r.n, &cfg, &fo);
  if (rc != SONAR_OK) return rc;
  HIP_TRY(c, hipMemcpyAsync(r.edges, r.p.edges, sizeof(r.p.edges), hipMemcpyHostToDevice, c->stream));
  if (sonar::launch_music_frames(r.mag, F, r.p.K, r.edges, kContrastBands, r.p.maxband, r.con, r.lh, r.lh + F,
                                 c->stream) != 0)
    return fail(c, SONAR_ERR_UNSUPPORTED, "spectral contrast launch failed (window too large for LDS?)");
  return SONAR_OK;
}

// chroma (:327-376) and the temporal group's arrays (:378-458) on the preprocessed PCM: ShortTimeEnergy
// (FeatureConfig W / H), envelope, amplitudes, frame peaks, and the one live pitch frame
int launch_temporal(MusicRun& r) {
  sonar_ctx* c = r.c;
  const MusicPlan& p = r.p;
  const sonar_feature_config* fc = r.fc;
  hipStream_t s = c->stream;
  // FeatureConfig.HopSize <= 0: the per-frame ChromaSTFT's STFT rejects it (stft.go:54-56), and
  // ExtractFeatures returns the wrapped error (music.go:218-221, :358-361)
  if (fc->hop_size <= 0)
    return fail(c, SONAR_ERR_INVALID,
                "chroma feature extraction failed: chroma computation failed at frame 0: hop size must be positive");
  // a chroma frame starting past the end is Go's slice-bounds panic; the spectral group and the MFCC
  // were computed before it, and nothing after it
  const bool live = p.chroma_bad < 0;
  const int rc = preprocess_energy_chroma(c, r.pcm, r.n, r.pre, p.F, p.Fe, fc->window_size, fc->hop_size,
                                          fc->sample_rate, r.energy, live ? r.chroma : nullptr);
  if (rc != SONAR_OK) return rc;
  if (p.Fenv > 0 && sonar::launch_energy(r.pre.y, 1, r.n, p.Fenv, (int)p.fse, fc->hop_size, 0.0, r.env, 1, s) != 0)
    return fail(c, SONAR_ERR_DEVICE, "envelope launch failed");
  if (live && sonar::launch_abs_stats(r.pre.y, r.n, r.abs, s) != 0)
    return fail(c, SONAR_ERR_DEVICE, "amplitude launch failed");
  if (p.Fe > 0 && sonar::launch_frame_peak(r.pre.y, r.n, p.Fe, p.fse, r.peak, s) != 0)
    return fail(c, SONAR_ERR_DEVICE, "peak launch failed");
  if (p.harmonic_live && sonar::launch_yin(r.pre.y, r.n, 1, 1024, fc->sample_rate, r.yin, r.yin + 1, nullptr, s) != 0)
    return fail(c, SONAR_ERR_DEVICE, "yin launch failed");
  return SONAR_OK;
}

// queues every array's copy to the host; the caller's guard drains the stream on a failure
int copy_back(MusicRun& r) {
  sonar_ctx* c = r.c;
  const MusicPlan& p = r.p;
  const size_t F = (size_t)p.F, Fe = (size_t)p.Fe;
  auto back = [&](std::vector<double>& v, const double* d, size_t count) {
    v.resize(count);
    if (count) HIP_TRY(c, hipMemcpyAsync(v.data(), d, count * 8, hipMemcpyDeviceToHost, c->stream));
    return (int)SONAR_OK;
  };
  auto& h = r.h;
  if (back(h.mfcc, r.mfcc, F * 13) || back(h.spec, r.spec, F * 9) || back(h.con, r.con, F * kContrastBands) ||
      back(h.lh, r.lh, F * 2) || back(h.chroma, r.chroma, p.chroma_bad < 0 ? F * 12 : 0) ||
      back(h.energy, r.energy, Fe) || back(h.env, r.env, (size_t)p.Fenv) || back(h.abs, r.abs, 2) ||
      back(h.peak, r.peak, Fe) || back(h.yin, r.yin, p.harmonic_live ? 2 : 0))
    return SONAR_ERR_DEVICE;
  return SONAR_OK;
}

// extractSpectralFeatures (:261-302): flux[0] = 0, flux[t] = flux(t-1, t); ZCR allocated and never
// filled (zeros); the contrast and the MFCC
void put_spectral(MusicRun& r, sonar_result* res) {
  const int64_t F = r.p.F;
  const std::vector<double>& spec = r.h.spec;
  static const char* names[6] = {"spectral_centroid", "spectral_rolloff", "spectral_bandwidth",
                                 "spectral_flatness", "spectral_crest", "spectral_slope"};
  for (int d = 0; d < 6; d++) res->put(names[d], std::vector<double>(spec.begin() + d * F, spec.begin() + (d + 1) * F), F, 1);
  std::vector<double> flux(F, 0.0);
  for (int64_t t = 1; t < F; t++) flux[t] = spec[6 * F + t - 1];
  res->put("spectral_flux", std::move(flux), F, 1);
  res->put("zero_crossing_rate", std::vector<double>(F, 0.0), F, 1);
  res->put("spectral_contrast", std::move(r.h.con), F, kContrastBands);
  res->put("mfcc", std::move(r.h.mfcc), F, 13);
}

// what follows the onsets: crest factors (:428-444), silence, extractEnergyFeatures (:460-525) and
// extractHarmonicFeatures (:528-583)
void put_energy_and_harmonic(MusicRun& r, sonar_result* res) {
  const int64_t F = r.p.F;
  const std::vector<double>& energy = r.h.energy;
  res->vec("crest_factor", sonar::host::crest_factors(r.h.peak.data(), energy.data(), energy.size()));
  // ComputeSilenceRatio(pcm, spectrogram.SampleRate, -40) (silence_detection.go:171-193): RMS of
  // 25 ms frames; an RMS is never below -40, so every frame is not silent
  const double sil = 0.0;
  res->scalar("silence_ratio", sil);
  res->vec("activity_level", std::vector<double>(energy.size(), 1.0 - sil));
  res->vec("short_time_energy", energy);
  res->scalar("energy_variance", sonar::host::gonum_variance(energy.data(), energy.size()));
  double lr = 0.0;
  res->vec("energy_entropy", sonar::host::energy_entropy(energy.data(), energy.size(), &lr));
  res->scalar("loudness_range", lr);
  res->vec("low_energy_ratio", std::vector<double>(r.h.lh.begin(), r.h.lh.begin() + F));
  res->vec("high_energy_ratio", std::vector<double>(r.h.lh.begin() + F, r.h.lh.end()));
  // DetectPitch takes only 1024-sample frames, the harmonic ratio 2048 and the inharmonicity 4096 (F7);
  // with a fresh detector the one live frame is the raw YIN result through the temporal tracking of
  // its first frame
  std::vector<double> pe(F, 0.0), pc(F, 0.0), vs(F, 0.0), zeros(F, 0.0), tc(F, 0.0);
  if (r.p.harmonic_live) {
    sonar::host::YinTracker tr;
    double p = r.h.yin[0], q = r.h.yin[1], v = 0.0;
    tr.step(p, q, v);
    pe[0] = p; pc[0] = q; vs[0] = v;
  }
  for (int64_t t = 0; t < F; t++) tc[t] = r.h.spec[t] * vs[t];    // centroid x voicing (:580-581)
  res->vec("pitch_estimate", pe);
  res->vec("pitch_confidence", pc);
  res->vec("voicing_strength", vs);
  res->vec("harmonic_ratio", zeros);
  res->vec("inharmonicity_ratio", zeros);
  res->vec("tonal_centroid", tc);
}

// The result in Go's order of computation.  Where Go panics, *out is what it had computed until then.
int assemble(MusicRun& r, sonar_result** out) {
  sonar_ctx* c = r.c;
  const MusicPlan& p = r.p;
  std::unique_ptr<sonar_result> res(new sonar_result());
  char msg[96];
  put_spectral(r, res.get());
  if (p.chroma_bad >= 0) {
    std::snprintf(msg, sizeof(msg), "runtime error: slice bounds out of range [%lld:%lld]",
                  (long long)(p.chroma_bad * r.fc->hop_size), (long long)r.n);
    *out = res.release();
    return fail(c, SONAR_ERR_PANIC, msg);
  }
  res->put("chroma", std::move(r.h.chroma), p.F, 12);
  res->vec("rms_energy", r.h.energy);
  // numFrames := len(RMSEnergy); frameSize := len(pcm) / numFrames (:382-383)
  if (p.Fe == 0) {
    *out = res.release();
    return fail(c, SONAR_ERR_PANIC, "runtime error: integer divide by zero");
  }
  res->vec("envelope_shape", r.h.env);
  res->scalar("peak_amplitude", r.h.abs[0]);                      // :386-397
  res->scalar("average_amplitude", r.h.abs[1] / (double)r.n);
  // DynamicRange.ComputeRange(pcm, 10.0, 90.0) (:401-403)
  if (p.L >= 2) {
    std::snprintf(msg, sizeof(msg), "runtime error: index out of range [%lld] with length %lld",
                  (long long)p.pct_index, (long long)p.L);
    *out = res.release();
    return fail(c, SONAR_ERR_PANIC, msg);
  }
  // L <= 1: the single value (or none) against itself -> 0 dB (dynamic_range.go:67-76)
  res->scalar("dynamic_range", 0.0);
  // onsets (:405-425): STFT 1024 / 512 of at most one frame -> no flux values -> no onsets;
  // a signal of at most 512 samples makes that STFT fail, and the extractor with it (:412-415)
  if (r.n <= 512)
    return fail(c, SONAR_ERR_TOO_SHORT, "temporal feature extraction failed: signal too short for given window size and hop size");
  res->scalar("onset_density", 0.0);
  res->vec("attack_time", {});
  put_energy_and_harmonic(r, res.get());
  *out = res.release();
  return SONAR_OK;
}

}  // namespace

namespace sonar {
namespace detail {

// MusicFeatureExtractor energy + chroma (music.go:245-259, :327-376, :460-466) on c->stream; `tag`
// prefixes the names of this call's scratch, so two calls on different streams do not share it
int music_features_impl(sonar_ctx* c, const double* pcm, int64_t n, int32_t sr, int32_t stft_w, int32_t stft_h,
                        int32_t fw, int32_t fh, double* energy, double* chroma, int32_t device_ptrs, const char* tag) {
  if (!c) return SONAR_ERR_INVALID;
  if (!pcm || n <= 0) return fail(c, SONAR_ERR_INVALID, "invalid input data");        // music.go:179-181
  if (stft_w <= 0 || stft_h <= 0) return fail(c, SONAR_ERR_INVALID, "window and hop size must be positive");
  const int64_t F = sonar_stft_frames(n, stft_w, stft_h);
  if (F <= 0) return fail(c, SONAR_ERR_TOO_SHORT, "signal too short for given window size and hop size");
  if (fh <= 0) return fail(c, SONAR_ERR_INVALID, "hop size must be positive");
  HIP_TRY(c, hipSetDevice(c->device));
  const int64_t Fe = sonar_energy_frames(n, fw, fh);
  Staging st{c, tag, device_ptrs != 0};
  const double* dp = st.in("pcm", pcm, n);
  const PreScratch pre = reserve_pre(st, n);
  double* de = device_ptrs ? energy : st.tmp<double>("energy", (size_t)std::max<int64_t>(Fe, 1));
  double* dc = device_ptrs ? chroma : st.tmp<double>("chroma", (size_t)F * 12);
  if (const int rc = st.ready("device allocation failed")) return rc;
  if (!de || !dc) return fail(c, SONAR_ERR_NOMEM, "device allocation failed");   // a null device output
  if (const int rc = preprocess_energy_chroma(c, dp, n, pre, F, Fe, fw, fh, sr, de, dc)) return rc;
  if (device_ptrs) return SONAR_OK;
  // the copies land in the caller's own arrays
  if (const int rc = st.give(energy, de, (size_t)Fe * 8)) return rc;
  if (const int rc = st.give(chroma, dc, (size_t)F * 12 * 8)) return rc;
  return st.finish();
}

}  // namespace detail
}  // namespace sonar

extern "C" {

int sonar_music_alignment_features(sonar_ctx* c, const double* pcm, int64_t n, int32_t sr, int32_t stft_w,
                                   int32_t stft_h, int32_t fw, int32_t fh, double* energy, double* chroma,
                                   int32_t device_ptrs) {
  return sonar::detail::music_features_impl(c, pcm, n, sr, stft_w, stft_h, fw, fh, energy, chroma, device_ptrs, "mf.");
}

int sonar_extract_music_features(sonar_ctx* c, const double* pcm, int64_t n, int32_t sample_rate,
                                 const sonar_feature_config* fc, sonar_result** out) {
  if (!c || !fc || !out) return fail(c, SONAR_ERR_INVALID, "null argument");
  *out = nullptr;
  (void)sample_rate;   // spectrogram.SampleRate: only ComputeSilenceRatio reads it, and its answer is a constant
  if (!pcm || n <= 0) return fail(c, SONAR_ERR_INVALID, "invalid input data");        // music.go:179-181
  const int W = fc->stft_window_size, H = fc->stft_hop_size;    // the spectrogram handed in
  const int64_t F = sonar_stft_frames(n, W, H);
  if (F == SONAR_ERR_INVALID) return fail(c, SONAR_ERR_INVALID, W <= 0 ? "window size must be positive" : "hop size must be positive");
  if (F < 0) return fail(c, SONAR_ERR_TOO_SHORT, "signal too short for given window size and hop size");
  HIP_TRY(c, hipSetDevice(c->device));
  MusicRun r{};
  r.c = c; r.n = n; r.fc = fc;
  r.p = MusicPlan(n, F, W, fc->sample_rate, fc->window_size, fc->hop_size);
  if (const int rc = reserve(r, pcm)) return rc;
  if (const int rc = launch_spectral(r)) return rc;
  if (const int rc = launch_temporal(r)) return rc;
  // from the first queued copy on, an early exit waits for the stream before r's host arrays go
  sonar::detail::DrainOnExit drain{c};
  if (const int rc = copy_back(r)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  drain.armed = false;
  return assemble(r, out);
}

}  // extern "C"
