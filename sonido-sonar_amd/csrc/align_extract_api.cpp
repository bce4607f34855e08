// align_extract_api.cpp -- the alignment extractor: C++ restatement of the Go orchestration above the
// GPU seams (the speech extractor and GenerateFingerprint are speech_api.cpp's, the music extractor
// and its energy + chroma music_api.cpp's).
//
//   sonar_align_features            AlignmentExtractor.ExtractAlignmentFeatures
//                                   (fingerprint/extractors/alignment.go:139-476)
//   sonar_align_pair_device         the same from device-resident PCM, with the
//                                   MusicFeatureExtractor energy + chroma of both streams
//
// Every per-cell array is produced by a HIP kernel (NCC, DTW, energy, chroma); this
// file only runs what the Go code runs sequentially on O(lags) / O(path) data: the
// scorer formulas, selectBestAlignment and the time-stretch estimate.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "ctx.h"
#include "host_dsp.h"
#include "kernels.h"

using sonar::detail::dbuf;
using sonar::detail::fail;
using sonar::detail::music_features_impl;

namespace sonar {
namespace detail {

// ExtractAlignmentFeatures after the GPU work (alignment.go:139-476): the candidates' scorers,
// selectBestAlignment (:412-446) and estimateTimeStretch (:448-476)
void align_finish(const AlignIn& in, sonar_result* res, sonar_pair_record* rec) {
  const double qlen = (double)in.q_pcm_len / (double)in.sample_rate, rlen = (double)in.r_pcm_len / (double)in.sample_rate;
  if (res) {
    res->scalar("query_length", qlen);
    res->scalar("reference_length", rlen);
  }
  if (rec) {
    std::memset(rec, 0, sizeof(*rec));
    rec->temporal_offset = rec->offset_confidence = rec->alignment_similarity = rec->alignment_quality = NAN;
    rec->corr_offset_seconds = rec->dtw_distance = rec->peak_lag = NAN;
  }
  struct Cand { bool ok = false; int type = 0; sonar::host::AlignScores s; bool dtw = false;
                int64_t p0q = 0, p0r = 0, p1q = 0, p1r = 0, plen = 0; };
  Cand corr, chroma;
  if (in.corr || in.corr_sums) {   // alignWithFeatures (:357-410) on the energy correlation
    const auto m = in.corr_sums ? sonar::host::ncc_metrics(*in.corr_sums, in.L, in.nqe, in.nre)
                                : sonar::host::ncc_metrics(in.corr, 2 * in.L + 1, in.L, in.nqe, in.nre);
    corr.ok = true; corr.type = 1;
    corr.s = sonar::host::xcorr_scores(m, in.hop, in.sample_rate, (int)in.mlf);
    if (rec) { rec->peak_lag = (double)m.peak_lag; rec->corr_offset_seconds = corr.s.offset_seconds; }
    if (res && in.corr) {
      res->vec("correlations", std::vector<double>(in.corr, in.corr + 2 * in.L + 1));
      res->scalar("peak_lag", (double)m.peak_lag);
      res->scalar("peak_correlation", m.peak_corr);
      res->scalar("corr_snr", m.snr);
      res->scalar("corr_sharpness", m.sharpness);
      res->scalar("corr_peak_to_sidelobe", m.psl);
      res->scalar("corr_offset", (double)corr.s.offset);
      res->scalar("corr_offset_seconds", corr.s.offset_seconds);
      res->scalar("corr_similarity", corr.s.similarity);
      res->scalar("corr_confidence", corr.s.confidence);
      res->scalar("corr_quality", corr.s.quality);
      res->scalar("corr_noise_level", corr.s.noise_level);
    }
  }
  if (in.has_dtw) {  // alignWithDTW (:129-148)
    const int64_t P = in.P;
    chroma.ok = true; chroma.type = 2; chroma.dtw = true;
    const sonar::host::PathSums ps = in.path_sums ? *in.path_sums : sonar::host::path_sums(in.pq, in.pr, in.pc, P);
    chroma.s = sonar::host::dtw_scores(ps, in.nqc, in.nrc, in.dist, in.sample_rate);
    chroma.plen = P;
    if (P > 0) { chroma.p0q = ps.p0q; chroma.p0r = ps.p0r; chroma.p1q = ps.p1q; chroma.p1r = ps.p1r; }
    if (rec) rec->dtw_distance = in.dist;
    if (res && in.pq) {
      std::vector<double> vq(P), vr(P), vc(P);
      for (int64_t i = 0; i < P; i++) { vq[i] = in.pq[i]; vr[i] = in.pr[i]; vc[i] = in.pc[i]; }
      res->scalar("dtw_distance", in.dist);
      res->vec("dtw_path_query", vq);
      res->vec("dtw_path_reference", vr);
      res->vec("dtw_path_cost", vc);
      res->scalar("dtw_offset", (double)chroma.s.offset);
      res->scalar("dtw_offset_seconds", chroma.s.offset_seconds);
      res->scalar("dtw_similarity", chroma.s.similarity);
      res->scalar("dtw_confidence", chroma.s.confidence);
      res->scalar("dtw_quality", chroma.s.quality);
      res->scalar("dtw_stability", chroma.s.stability);
    }
  }
  // selectBestAlignment (:412-446); Go iterates a map (random order) with strict >:
  // here corr_energy is visited first, so exact ties go to it deterministically
  const Cand* best = nullptr;
  double best_score = 0.0;
  for (const Cand* cd : {&corr, &chroma}) {
    if (!cd->ok) continue;
    const double w = cd->type == 1 ? 1.0 : 0.7;
    const double sc = w * (0.4 * cd->s.confidence + 0.4 * cd->s.similarity + 0.2 * cd->s.quality);
    if (sc > best_score) { best_score = sc; best = cd; }
  }
  double stretch = 1.0;                                           // estimateTimeStretch (:448-476)
  if (best) {
    if (res) {
      res->scalar("temporal_offset", best->s.offset_seconds);
      res->scalar("offset_confidence", best->s.confidence);
      res->scalar("alignment_similarity", best->s.similarity);
      res->scalar("alignment_quality", best->s.quality);
      res->scalar("method", (double)best->type);
    }
    if (rec) {
      rec->temporal_offset = best->s.offset_seconds;
      rec->offset_confidence = best->s.confidence;
      rec->alignment_similarity = best->s.similarity;
      rec->alignment_quality = best->s.quality;
      rec->method = (double)best->type;
    }
    if (qlen > 0 && rlen > 0) {
      const double lr = qlen / rlen;
      stretch = lr;
      if (best->dtw && best->plen > 1) {
        const double qs = (double)(best->p1q - best->p0q + 1), rs = (double)(best->p1r - best->p0r + 1);
        if (rs > 0) stretch = 0.7 * (qs / rs) + 0.3 * lr;
      }
    }
  } else if (res) {
    res->scalar("method", 0.0);
  }
  if (res) {
    if (corr.ok) res->scalar("feature_similarity_corr_energy", corr.s.similarity);
    if (chroma.ok) res->scalar("feature_similarity_dtw_chroma", chroma.s.similarity);
    res->scalar("time_stretch", stretch);
  }
}

}  // namespace detail
}  // namespace sonar

namespace {

// AlignmentExtractor.ExtractAlignmentFeatures body; dev = the four feature arrays are device
// pointers on the ctx's device (no H2D), else host arrays
int align_impl(sonar_ctx* c, const double* qe, int64_t nqe, const double* re, int64_t nre, const double* qc,
               int64_t nqc, const double* rc_, int64_t nrc, int64_t q_pcm_len, int64_t r_pcm_len,
               int32_t sample_rate, int32_t feature_sample_rate, int32_t hop, int32_t win,
               double max_lag_seconds, int32_t dev, sonar_result** out) {
  if (!c || !out) return fail(c, SONAR_ERR_INVALID, "null argument");
  *out = nullptr;
  if (hop <= 0) return fail(c, SONAR_ERR_INVALID, "hop size must be positive (NewAlignmentExtractor divides by it)");
  (void)win;
  const int64_t max_lag_samples = (int64_t)(max_lag_seconds * (double)feature_sample_rate);   // alignment.go:104
  const bool want_corr = qe && re && nqe > 0 && nre > 0, want_dtw = qc && rc_ && nqc > 0 && nrc > 0;
  const int64_t mlf = want_corr ? std::min(max_lag_samples / hop, std::min(nqe, nre) - 1) : 0;
  // device arrays: the NCC and the DTW are both queued before one stream synchronisation; their
  // small results (correlation, path length, status words) arrive in pinned host memory
  double* hcorr = nullptr;
  int64_t hL = 0;
  sonar::detail::DtwPending pend;
  if (dev) {
    HIP_TRY(c, hipSetDevice(c->device));
    int st = SONAR_OK;
    if (want_corr && want_dtw) {
      // the NCC (energies) and the DTW (chroma) are independent: the NCC runs on the side stream
      // beside the band kernel (which leaves LDS and wave slots free on every CU), and the main
      // stream waits for it, so the one synchronisation below still covers both
      if (const int rc = sonar::detail::ensure_side(c)) return rc;
      HIP_TRY(c, hipEventRecord(c->side_ev[0], c->stream));
      HIP_TRY(c, hipStreamWaitEvent(c->side, c->side_ev[0], 0));
      {
        sonar::detail::OnSideStream on_side(c);
        st = sonar::detail::ncc_enqueue(c, qe, nqe, re, nre, (int32_t)mlf, &hcorr, &hL);
      }
      if (st != SONAR_OK) return st;
      HIP_TRY(c, hipEventRecord(c->side_ev[1], c->side));
      st = sonar::detail::dtw_enqueue(c, qc, nqc, rc_, nrc, 12, -1, &pend);
      if (st != SONAR_OK) return st;
      HIP_TRY(c, hipStreamWaitEvent(c->stream, c->side_ev[1], 0));
    } else {
      if (want_corr) st = sonar::detail::ncc_enqueue(c, qe, nqe, re, nre, (int32_t)mlf, &hcorr, &hL);
      if (st == SONAR_OK && want_dtw) st = sonar::detail::dtw_enqueue(c, qc, nqc, rc_, nrc, 12, -1, &pend);
      if (st != SONAR_OK) return st;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  sonar::detail::AlignIn in;
  in.q_pcm_len = q_pcm_len; in.r_pcm_len = r_pcm_len; in.sample_rate = sample_rate; in.hop = hop;
  std::vector<double> cr;
  if (want_corr) {   // 2. energy cross-correlation (performMultiFeatureAlignment :320-333)
    const int64_t L = std::max<int64_t>(0, std::min({mlf, nqe - 1, nre - 1}));
    if (dev) {
      cr.assign(hcorr, hcorr + 2 * hL + 1);
    } else {
      cr.resize(2 * L + 1);
      const int rc = sonar_ncc(c, qe, nqe, re, nre, (int32_t)mlf, cr.data(), nullptr, 0);
      if (rc != SONAR_OK) return rc;
    }
    in.corr = cr.data(); in.L = L; in.nqe = nqe; in.nre = nre; in.mlf = mlf;
  }
  std::vector<int32_t> vpq, vpr;
  std::vector<double> vpc;
  if (want_dtw) {    // 4. chroma DTW (:346-351)
    int rc;
    if (dev) {
      rc = sonar::detail::dtw_finish(c, &pend, &in.pq, &in.pr, &in.pc, &in.P, &in.dist);
    } else {
      const int64_t cap = nqc + nrc + 1;
      vpq.resize(cap); vpr.resize(cap); vpc.resize(cap);
      rc = sonar_dtw(c, qc, nqc, rc_, nrc, 12, -1, &in.dist, vpq.data(), vpr.data(), vpc.data(), &in.P, nullptr, 0);
      in.pq = vpq.data(); in.pr = vpr.data(); in.pc = vpc.data();
    }
    if (rc != SONAR_OK) return rc;
    in.has_dtw = true; in.nqc = nqc; in.nrc = nrc;
  }
  std::unique_ptr<sonar_result> res(new sonar_result());
  sonar::detail::align_finish(in, res.get(), nullptr);
  *out = res.release();
  return SONAR_OK;
}

}  // namespace

extern "C" {

int sonar_align_features(sonar_ctx* c, const double* qe, int64_t nqe, const double* re, int64_t nre, const double* qc,
                         int64_t nqc, const double* rc_, int64_t nrc, int64_t q_pcm_len, int64_t r_pcm_len,
                         int32_t sample_rate, int32_t feature_sample_rate, int32_t hop, int32_t win,
                         double max_lag_seconds, sonar_result** out) {
  return align_impl(c, qe, nqe, re, nre, qc, nqc, rc_, nrc, q_pcm_len, r_pcm_len, sample_rate, feature_sample_rate,
                    hop, win, max_lag_seconds, 0, out);
}

// One stream pair end to end from device-resident PCM: MusicFeatureExtractor energy + chroma of
// both streams (music.go:245-259, :327-376, :460-466) into ctx buffers, then
// ExtractAlignmentFeatures on those device arrays -- no feature round trip through the host.
int sonar_align_pair_device(sonar_ctx* c, const double* q_pcm, int64_t nq, const double* r_pcm, int64_t nr,
                            int32_t sample_rate, int32_t stft_window, int32_t hop, int32_t feature_window,
                            double max_lag_seconds, sonar_result** out) {
  if (!c || !out) return fail(c, SONAR_ERR_INVALID, "null argument");
  *out = nullptr;
  if (stft_window <= 0 || hop <= 0) return fail(c, SONAR_ERR_INVALID, "window and hop size must be positive");
  const int64_t Fq = sonar_stft_frames(nq, stft_window, hop), Fr = sonar_stft_frames(nr, stft_window, hop);
  if (Fq <= 0 || Fr <= 0) return fail(c, SONAR_ERR_TOO_SHORT, "signal too short for given window size and hop size");
  const int64_t Eq = sonar_energy_frames(nq, feature_window, hop), Er = sonar_energy_frames(nr, feature_window, hop);
  double* qe = (double*)dbuf(c, "ap.qe", std::max<int64_t>(Eq, 1) * 8);
  double* re = (double*)dbuf(c, "ap.re", std::max<int64_t>(Er, 1) * 8);
  double* qc = (double*)dbuf(c, "ap.qc", Fq * 12 * 8);
  double* rc = (double*)dbuf(c, "ap.rc", Fr * 12 * 8);
  if (!qe || !re || !qc || !rc) return fail(c, SONAR_ERR_NOMEM, "device allocation failed");
  // the two streams' features are independent: r's on the side stream (its own scratch) beside q's
  HIP_TRY(c, hipSetDevice(c->device));
  if (const int rc = sonar::detail::ensure_side(c)) return rc;
  HIP_TRY(c, hipEventRecord(c->side_ev[0], c->stream));        // the caller's PCM is ready on c->stream
  HIP_TRY(c, hipStreamWaitEvent(c->side, c->side_ev[0], 0));
  int st = music_features_impl(c, q_pcm, nq, sample_rate, stft_window, hop, feature_window, hop, qe, qc, 1, "mf.");
  if (st != SONAR_OK) return st;
  {
    sonar::detail::OnSideStream on_side(c);
    st = music_features_impl(c, r_pcm, nr, sample_rate, stft_window, hop, feature_window, hop, re, rc, 1, "mf.r.");
  }
  if (st != SONAR_OK) return st;
  HIP_TRY(c, hipEventRecord(c->side_ev[1], c->side));
  HIP_TRY(c, hipStreamWaitEvent(c->stream, c->side_ev[1], 0));
  return align_impl(c, Eq > 0 ? qe : nullptr, Eq, Er > 0 ? re : nullptr, Er, qc, Fq, rc, Fr, nq, nr, sample_rate,
                    sample_rate, hop, feature_window, max_lag_seconds, 1, out);
}

}  // extern "C"
