// chroma_sim_api.cpp -- sonar_chroma_frame_matrix / sonar_chroma_similarity / sonar_chroma_similarity_plan:
// ChromaSequenceSimilarity.ComputeSimilarity (algorithms/chroma/chroma_similarity.go:86-538).  The host
// side: Go's integer arithmetic (the sample step, the OTI column ranges, the DTW band rule), the choice
// of the transposition from the device's ordered sums, the empty-input results and the scratch; the
// sequences, the matrix and the path arrays are the caller's host or device arrays (staging.h).  The
// kernels are chroma_sim_kernels.hip's.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "ctx.h"
#include "kernels.h"
#include "staging.h"

namespace {
using namespace sonar::detail;

constexpr int64_t kMaxCells = int64_t(1) << 30;   // SW / DTW: one float64 DP matrix of 8 GiB
const char* const kPanicEmpty = "runtime error: index out of range [0] with length 0";

// sampleStep := math.Max(1, float64(len(queryChroma))/50), used as int(sampleStep) (:459-464)
int64_t sample_step(int64_t nq) {
  const double v = (double)nq / 50.0;
  return (int64_t)(v > 1.0 ? v : 1.0);
}
// the column range of OTI row i (:422): j from max(0, i - R) while j < min(nr, i + R + 1)
int64_t oti_row_cells(int64_t i, int64_t nr, int64_t R) {
  const int64_t lo = i - R > 0 ? i - R : 0, hi = i + R + 1 < nr ? i + R + 1 : nr;
  return hi > lo ? hi - lo : 0;
}
// the DTW band rule (:315-320): expectedJ := int(float64(j*nq) / float64(nr)); abs(j - expectedJ) > R
bool dtw_skips(int64_t j, int64_t nq, int64_t nr, int64_t R) {
  const int64_t e = (int64_t)((double)(j * nq) / (double)nr);
  return (j > e ? j - e : e - j) > R;
}
int norm_method(int method) {
  return method >= SONAR_CHROMA_SIM_DIRECT && method <= SONAR_CHROMA_SIM_OTI ? method : SONAR_CHROMA_SIM_DIRECT;
}

bool is_dev(const void* p) {
  if (!p) return false;
  hipPointerAttribute_t at{};
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return at.type == hipMemoryTypeDevice;
}

// the event pair of one kernel family around the launches between begin and end
struct Stages {
  sonar_ctx* c;
  hipStream_t s;
  bool used[4] = {false, false, false, false};
  bool ok = true;
  void begin(int k) {
    for (int e = 2 * k; e < 2 * k + 2; ++e)
      if (!c->csim_ev[e] && hipEventCreate(&c->csim_ev[e]) != hipSuccess) { ok = false; return; }
    ok = ok && hipEventRecord(c->csim_ev[2 * k], s) == hipSuccess;
  }
  void end(int k) { used[k] = ok && hipEventRecord(c->csim_ev[2 * k + 1], s) == hipSuccess; }
  void finish() {                                    // after the stream is synchronised
    for (int k = 0; k < 4; ++k) {
      float f = 0.f;
      if (used[k] && hipEventElapsedTime(&f, c->csim_ev[2 * k], c->csim_ev[2 * k + 1]) != hipSuccess) f = 0.f;
      c->csim_ms[k] = f;
    }
  }
};

// device copies of the two sequences (their own when they are device pointers)
int stage_inputs(Staging& o, const double* q, int64_t nq, const double* r, int64_t nr, int dim, const double** dq,
                 const double** dr) {
  *dq = o.in("q", q, (size_t)nq * dim);
  *dr = o.in("r", r, (size_t)nr * dim);
  return o.ready("device allocation failed (chroma sequences)");
}

int check_inputs(sonar_ctx* c, const double* q, int64_t nq, const double* r, int64_t nr, int32_t dim) {
  if (nq < 0 || nr < 0) return fail(c, SONAR_ERR_INVALID, "chroma similarity: negative frame count");
  if (dim < 1) return fail(c, SONAR_ERR_INVALID, "chroma similarity: dim must be >= 1");
  if ((nq > 0 && !q) || (nr > 0 && !r)) return fail(c, SONAR_ERR_INVALID, "chroma similarity: null sequence pointer");
  if (nq + nr > (int64_t)INT32_MAX) return fail(c, SONAR_ERR_UNSUPPORTED, "chroma similarity: sequences too long");
  return SONAR_OK;
}

}  // namespace

extern "C" {

int sonar_chroma_similarity_plan(int32_t method, int64_t nq, int64_t nr, int32_t dim, int32_t oti_radius,
                                 int32_t dtw_band_radius, int64_t* sample_step_out, int64_t* sampled_pairs,
                                 int64_t* oti_cells, int64_t* dtw_skipped_columns, int64_t* scratch_bytes) {
  if (nq < 0 || nr < 0 || dim < 1) return SONAR_ERR_INVALID;
  const int m = norm_method(method);
  const int64_t step = sample_step(nq);
  if (sample_step_out) *sample_step_out = step;
  if (sampled_pairs) *sampled_pairs = ((nq + step - 1) / step) * ((nr + step - 1) / step);
  if (oti_cells) {
    int64_t n = 0;
    for (int64_t i = 0; i < nq; ++i) n += oti_row_cells(i, nr, oti_radius);
    *oti_cells = n;
  }
  if (dtw_skipped_columns) {
    int64_t n = 0;
    if (dtw_band_radius > 0 && nq >= 2)
      for (int64_t j = 1; j < nr; ++j) n += dtw_skips(j, nq, nr, dtw_band_radius);
    *dtw_skipped_columns = n;
  }
  if (scratch_bytes) {
    // host-pointer call with a matrix: the sequences, their prepared rows (the query's 12 shifts), the
    // matrix, and for the two recurrences the DP matrix, the traceback bytes and the path
    const int64_t rl = sonar::chroma_row_len(dim), cells = nq * nr;
    int64_t b = (nq + nr) * dim * 8 + (12 * nq + nr) * rl * 8 + cells * 8;
    if (m == SONAR_CHROMA_SIM_DIRECT) b += sonar::chroma_matrix_blocks(nq, nr) * 8;
    if (m == SONAR_CHROMA_SIM_SMITH_WATERMAN)
      b += cells + sonar::chroma_matrix_blocks(nq, nr) * 16 + (nq + nr) * 16;
    if (m == SONAR_CHROMA_SIM_DTW) b += cells * 8 + nr + (nq + nr) * 16;
    *scratch_bytes = b;
  }
  return SONAR_OK;
}

int sonar_chroma_frame_matrix(sonar_ctx* c, const double* q, int64_t nq, const double* r, int64_t nr, int32_t dim,
                              int32_t metric, int32_t shift, int32_t as_similarity, double* out) {
  if (!c) return SONAR_ERR_INVALID;
  if (const int rc = check_inputs(c, q, nq, r, nr, dim)) return rc;
  // CircularShift indexes cv.Values[(i+shift)%len]: a negative shift indexes below 0
  if (shift < 0 && nq > 0)
    return fail(c, SONAR_ERR_PANIC, "runtime error: index out of range [" + std::to_string(shift % dim) + "]");
  if (nq == 0 || nr == 0) return SONAR_OK;
  if (!out) return fail(c, SONAR_ERR_INVALID, "chroma frame matrix: null output pointer");
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  Staging o{c, "csim.", is_dev(q)};
  const double *dq, *dr;
  if (const int rc = stage_inputs(o, q, nq, r, nr, dim, &dq, &dr)) return rc;
  const int64_t rl = sonar::chroma_row_len(dim);
  double* qp = o.tmp<double>("qp", (size_t)nq * rl);
  double* rp = o.tmp<double>("rp", (size_t)nr * rl);
  double* dout = o.out("out", out, (size_t)nq * nr);
  if (const int rc = o.ready("device allocation failed (chroma frame matrix)")) return rc;
  Stages st{c, s};
  st.begin(0);
  hipEvent_t tend = timed_begin(c, s);
  if (sonar::launch_chroma_prepare(dq, nq, dim, metric, shift, 1, qp, s) ||
      sonar::launch_chroma_prepare(dr, nr, dim, metric, 0, 1, rp, s))
    return fail(c, SONAR_ERR_DEVICE, "chroma prepare launch failed");
  sonar::ChromaMatArgs a{};
  a.qp = qp; a.rp = rp; a.nq = nq; a.nr = nr; a.dim = dim; a.metric = metric; a.mode = as_similarity ? 1 : 0;
  a.out = dout;
  const int lrc = sonar::launch_chroma_matrix(a, s);
  if (lrc == -1) return fail(c, SONAR_ERR_UNSUPPORTED, "chroma frame matrix: more query frames than one launch takes");
  if (lrc != 0) return fail(c, SONAR_ERR_DEVICE, "chroma frame matrix launch failed");
  timed_end(c, s, tend);
  st.end(0);
  if (const int rc = o.finish()) return rc;
  st.finish();
  return SONAR_OK;
}

int sonar_chroma_similarity(sonar_ctx* c, const double* q, int64_t nq, const double* r, int64_t nr, int32_t dim,
                            int32_t method, int32_t metric, double binary_threshold, int32_t oti_radius,
                            int32_t dtw_band_radius, int32_t transposition_invariant, double* matrix,
                            int32_t* matrix_is_nil, double* overall, int32_t* best_transposition, int32_t* path_q,
                            int32_t* path_r, double* path_score, int64_t* path_len) {
  if (!c) return SONAR_ERR_INVALID;
  if (const int rc = check_inputs(c, q, nq, r, nr, dim)) return rc;
  const int m = norm_method(method);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  int32_t nil = 0, best = 0;
  double ov = 0.0;
  int64_t P = 0;
  auto done = [&]() {
    if (matrix_is_nil) *matrix_is_nil = nil;
    if (overall) *overall = ov;
    if (best_transposition) *best_transposition = best;
    if (path_len) *path_len = P;
    return SONAR_OK;
  };
  const bool ti = transposition_invariant != 0;
  if (nq == 0 || nr == 0) {                          // nothing is launched
    switch (m) {
      case SONAR_CHROMA_SIM_DTW: return fail(c, SONAR_ERR_PANIC, kPanicEmpty);   // cost[0][0] (:301)
      case SONAR_CHROMA_SIM_DIRECT: ov = ti ? 0.0 : nan; break;   // maxSimilarity stays 0.0 | 0 / 0 (:146-149)
      case SONAR_CHROMA_SIM_BINARY: ov = nan; break;              // matches / total = 0 / 0 (:190)
      case SONAR_CHROMA_SIM_SMITH_WATERMAN: ov = nan; break;      // maxScore / len(path) = 0 / 0 (:261)
      case SONAR_CHROMA_SIM_QMAX: ov = 0.0; break;
      default: nil = 1; ov = 0.0; break;                          // OTI: every avg is NaN, bestMatrix stays nil
    }
    return done();
  }
  const bool dp = m == SONAR_CHROMA_SIM_SMITH_WATERMAN || m == SONAR_CHROMA_SIM_DTW;
  if (dp && nq > kMaxCells / nr)
    return fail(c, SONAR_ERR_UNSUPPORTED, "chroma similarity: Smith-Waterman and DTW take at most 2^30 cells (nq * nr)");
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  Staging o{c, "csim.", is_dev(q)};
  const double *dq, *dr;
  if (const int rc = stage_inputs(o, q, nq, r, nr, dim, &dq, &dr)) return rc;
  const int64_t rl = sonar::chroma_row_len(dim), cells = nq * nr, cap = nq + nr;
  const double total = (double)(nq * nr);            // float64(queryLen*refLen), float64(count)
  double* rp = (double*)dbuf(c, "csim.rp", (size_t)nr * rl * 8);
  unsigned long long* red = (unsigned long long*)dbuf(c, "csim.red", 32);   // sum | count | max bits | spare
  if (!rp || !red) return fail(c, SONAR_ERR_NOMEM, "device allocation failed (chroma similarity)");
  Stages st{c, s};
  const double* qp = nullptr;

  // the 12 ordered sums of findBestTransposition (banded = 0) or OTI (banded = 1) -> host
  const double* tot = nullptr;
  auto ordered = [&](int banded) -> int {
    double* q12 = (double*)dbuf(c, "csim.q12", (size_t)12 * nq * rl * 8);
    double* dt = (double*)dbuf(c, "csim.tot", 12 * 8);
    if (!q12 || !dt) return fail(c, SONAR_ERR_NOMEM, "device allocation failed (chroma transpositions)");
    st.begin(1);
    if (sonar::launch_chroma_prepare(dq, nq, dim, metric, 0, 12, q12, s) ||
        sonar::launch_chroma_prepare(dr, nr, dim, metric, 0, 1, rp, s))
      return fail(c, SONAR_ERR_DEVICE, "chroma prepare launch failed");
    sonar::ChromaOrdArgs a{};
    a.qp = q12; a.rp = rp; a.nq = nq; a.nr = nr; a.dim = dim; a.metric = metric;
    a.step = banded ? 1 : sample_step(nq); a.banded = banded; a.radius = oti_radius; a.totals = dt;
    if (sonar::launch_chroma_ordered(a, s) != 0) return fail(c, SONAR_ERR_DEVICE, "chroma ordered-sum launch failed");
    st.end(1);
    tot = o.back(dt, 12);
    qp = q12;
    return o.fetch();
  };
  // the first shift whose mean is strictly greater than the running best, from 0.0 (:471-475, :429-434)
  auto pick = [&](double count, double* mx) {
    int b = -1;
    *mx = 0.0;
    for (int sh = 0; sh < 12; ++sh) {
      const double avg = tot[sh] / count;
      if (avg > *mx) { *mx = avg; b = sh; }
    }
    return b;
  };
  auto prepare_shift0 = [&]() -> int {
    double* p = (double*)dbuf(c, "csim.qp", (size_t)nq * rl * 8);
    if (!p) return fail(c, SONAR_ERR_NOMEM, "device allocation failed (chroma similarity)");
    if (sonar::launch_chroma_prepare(dq, nq, dim, metric, 0, 1, p, s) ||
        sonar::launch_chroma_prepare(dr, nr, dim, metric, 0, 1, rp, s))
      return fail(c, SONAR_ERR_DEVICE, "chroma prepare launch failed");
    qp = p;
    return SONAR_OK;
  };
  auto launch_matrix = [&](sonar::ChromaMatArgs& a) -> int {
    a.rp = rp; a.nq = nq; a.nr = nr; a.dim = dim; a.metric = metric;
    const int lrc = sonar::launch_chroma_matrix(a, s);
    if (lrc == -1) return fail(c, SONAR_ERR_UNSUPPORTED, "chroma similarity: more query frames than one launch takes");
    if (lrc != 0) return fail(c, SONAR_ERR_DEVICE, "chroma frame matrix launch failed");
    return SONAR_OK;
  };
  // the device matrix the caller gets: its own device pointer, or scratch copied back at the end
  auto out_matrix = [&](const char* name) { return o.out(name, matrix, (size_t)cells); };

  if (m == SONAR_CHROMA_SIM_OTI) {                   // :400-445; ignores TranspositionInvariant
    if (const int rc = ordered(1)) return rc;
    double mx;
    const int b = pick(total, &mx);
    if (b < 0) {                                     // no shift won: bestMatrix is nil
      nil = 1;
      st.finish();
      return done();
    }
    best = b; ov = mx;
    if (matrix) {
      double* dout = out_matrix("out");
      if (!dout) return fail(c, SONAR_ERR_NOMEM, "device allocation failed (similarity matrix)");
      sonar::ChromaMatArgs a{};
      a.qp = qp + (int64_t)b * nq * rl; a.mode = 1; a.banded = 1; a.radius = oti_radius; a.out = dout;
      st.begin(0);
      if (const int rc = launch_matrix(a)) return rc;
      st.end(0);
    }
    if (const int rc = o.finish()) return rc;
    st.finish();
    return done();
  }

  if (!dp) {                                         // Direct, Binary, QMax (:106-194, :362-397)
    double maxsim = 0.0;
    if (ti) {                                        // findBestTransposition (:450-479)
      if (const int rc = ordered(0)) return rc;
      const int64_t step = sample_step(nq);
      const int b = pick((double)(((nq + step - 1) / step) * ((nr + step - 1) / step)), &maxsim);
      best = b < 0 ? 0 : b;
      qp = qp + (int64_t)best * nq * rl;
    }
    st.begin(0);
    hipEvent_t tend = timed_begin(c, s);
    if (!ti)
      if (const int rc = prepare_shift0()) return rc;
    double* dout = out_matrix("out");
    if (matrix && !dout) return fail(c, SONAR_ERR_NOMEM, "device allocation failed (similarity matrix)");
    const bool want_sum = m == SONAR_CHROMA_SIM_DIRECT && !ti;
    const int64_t nblk = sonar::chroma_matrix_blocks(nq, nr);
    double* partial = want_sum ? (double*)dbuf(c, "csim.partial", (size_t)nblk * 8) : nullptr;
    if (want_sum && !partial) return fail(c, SONAR_ERR_NOMEM, "device allocation failed (chroma similarity)");
    HIP_TRY(c, hipMemsetAsync(red, 0, 32, s));
    sonar::ChromaMatArgs a{};
    a.qp = qp; a.mode = 1; a.out = dout; a.partial = partial;
    a.binary = m == SONAR_CHROMA_SIM_BINARY; a.thr = binary_threshold;
    a.count = a.binary ? red + 1 : nullptr;
    a.maxbits = m == SONAR_CHROMA_SIM_QMAX ? red + 2 : nullptr;
    if (const int rc = launch_matrix(a)) return rc;
    if (want_sum && sonar::launch_chroma_sum_partials(partial, nblk, (double*)red, s) != 0)
      return fail(c, SONAR_ERR_DEVICE, "chroma reduction launch failed");
    timed_end(c, s, tend);
    st.end(0);
    const unsigned long long* h = o.back(red, 3);
    if (const int rc = o.finish()) return rc;
    st.finish();
    double sum, mx;
    std::memcpy(&sum, &h[0], 8);
    std::memcpy(&mx, &h[2], 8);
    if (m == SONAR_CHROMA_SIM_BINARY) ov = (double)h[1] / total;        // matches / total (:180-190)
    else if (m == SONAR_CHROMA_SIM_QMAX) ov = mx;
    else ov = ti ? maxsim : sum / total;                                // (:146-149)
    return done();
  }

  // Smith-Waterman (:197-271) and the file's DTW (:274-352): the frame matrix, then the recurrence in
  // place on it, then the walk back.  Neither applies a transposition.
  const bool dtw = m == SONAR_CHROMA_SIM_DTW;
  // SW: SimilarityMatrix is scores[1:][1:] (:252-258), so the recurrence runs in the caller's matrix
  double* M = (!dtw && matrix) ? out_matrix("M") : o.tmp<double>("M", (size_t)cells);
  int32_t* pq = (int32_t*)dbuf(c, "csim.pq", (size_t)cap * 4);
  int32_t* pr = (int32_t*)dbuf(c, "csim.pr", (size_t)cap * 4);
  double* ps = (double*)dbuf(c, "csim.ps", (size_t)cap * 8);
  if (!M || !pq || !pr || !ps) return fail(c, SONAR_ERR_NOMEM, "device allocation failed (DP matrix)");
  st.begin(0);
  if (const int rc = prepare_shift0()) return rc;
  {
    sonar::ChromaMatArgs a{};
    a.qp = qp; a.mode = dtw ? 0 : 1; a.out = M;
    if (const int rc = launch_matrix(a)) return rc;
  }
  double* dsim = nullptr;
  if (dtw && matrix) {                               // SimilarityMatrix = exp(-cost) (:332-338)
    dsim = out_matrix("out");
    if (!dsim) return fail(c, SONAR_ERR_NOMEM, "device allocation failed (similarity matrix)");
    if (sonar::launch_chroma_exp_neg(M, cells, dsim, s) != 0) return fail(c, SONAR_ERR_DEVICE, "chroma exp launch failed");
  }
  st.end(0);
  sonar::ChromaDpArgs d{};
  d.M = M; d.nq = nq; d.nr = nr; d.ntj = (nr + sonar::CHROMA_DP_T - 1) / sonar::CHROMA_DP_T; d.dtw = dtw;
  const int64_t ntiles = ((nq + sonar::CHROMA_DP_T - 1) / sonar::CHROMA_DP_T) * d.ntj;
  int64_t* dscal = (int64_t*)red;                    // [0] best score, [1] its index, [2] path length, [3] acc end
  if (dtw) {
    if (dtw_band_radius > 0 && nq >= 2) {
      std::vector<uint8_t> skip((size_t)nr, 0);
      bool any = false;
      for (int64_t j = 1; j < nr; ++j) any |= (skip[(size_t)j] = dtw_skips(j, nq, nr, dtw_band_radius));
      if (any) {                                     // the mask goes up from a copy of it that o keeps
        d.skip = o.in_host("skip", skip.data(), (size_t)nr);
        if (const int rc = o.ready("device allocation failed (band mask)")) return rc;
      }
    }
  } else {
    d.tb = (uint8_t*)dbuf(c, "csim.tb", (size_t)cells);
    d.tile_best = (double*)dbuf(c, "csim.tbest", (size_t)ntiles * 8);
    d.tile_idx = (int64_t*)dbuf(c, "csim.tidx", (size_t)ntiles * 8);
    if (!d.tb || !d.tile_best || !d.tile_idx) return fail(c, SONAR_ERR_NOMEM, "device allocation failed (traceback)");
  }
  st.begin(2);
  hipEvent_t tend = timed_begin(c, s);
  if (sonar::launch_chroma_dp(d, s) != 0) return fail(c, SONAR_ERR_DEVICE, "chroma DP launch failed");
  if (!dtw && sonar::launch_chroma_sw_best(d.tile_best, d.tile_idx, ntiles, (double*)dscal, dscal + 1, s) != 0)
    return fail(c, SONAR_ERR_DEVICE, "chroma DP launch failed");
  timed_end(c, s, tend);
  st.end(2);
  st.begin(3);
  if (sonar::launch_chroma_traceback(M, d.tb, nq, nr, dtw, dscal + 1, pq, pr, ps, cap, dscal + 2, s) != 0)
    return fail(c, SONAR_ERR_DEVICE, "chroma traceback launch failed");
  st.end(3);
  // SW: the best score; DTW: acc[nq-1][nr-1]
  const double* end = o.back(dtw ? M + cells - 1 : (const double*)dscal, 1);
  const int64_t* plen = o.back(dscal + 2, 1);
  if (const int rc = o.fetch()) return rc;
  P = *plen;
  if (P > 0) {                                       // written back to front: the path is the tail
    if (const int rc = o.give(path_q, pq + cap - P, (size_t)P * 4)) return rc;
    if (const int rc = o.give(path_r, pr + cap - P, (size_t)P * 4)) return rc;
    if (const int rc = o.give(path_score, ps + cap - P, (size_t)P * 8)) return rc;
  }
  if (const int rc = o.finish()) return rc;
  st.finish();
  // SW: maxScore / len(path) (:261); DTW: exp(-(acc[nq-1][nr-1] / len(path))) (:341-342)
  ov = dtw ? std::exp(-(*end / (double)P)) : *end / (double)P;
  return done();
}

int sonar_chroma_similarity_last_timing(sonar_ctx* c, double* ms4) {
  if (!c || !ms4) return SONAR_ERR_INVALID;
  for (int k = 0; k < 4; ++k) ms4[k] = c->csim_ms[k];
  return SONAR_OK;
}

}  // extern "C"
