// align_api.cpp -- the alignment entries of include/sonar_gpu.h: sonar_ncc and the sonar_dtw
// family (CrossCorrelation.Compute's NCC, correlation.go:131-409; DTWAlignment.Align, dtw.go:55-307),
// and their deferred-sync halves for one stream pair (ncc_enqueue, dtw_enqueue / dtw_finish: the
// device path of align_extract_api.cpp's align_impl).  The kernels are ncc_kernels.hip's and dtw_kernels.hip's.
#include "../../include/sonar_gpu.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "ctx.h"
#include "host_dsp.h"
#include "kernels.h"

namespace {
using namespace sonar::detail;

// The NCC of two device arrays over L lags: scratch, then the launch.  *dc null: the correlation goes
// to the cached "ncc.corr"; hc (nullable): a pinned host buffer of its size, allocated with the scratch
int ncc_launch(sonar_ctx* c, const double* da, int64_t na, const double* db, int64_t nb, int64_t L, double** dc,
               double** hc, bool timed, const char* nomem) {
  const int64_t nl = 2 * L + 1;
  hipStream_t s = c->stream;
  double* xa = (double*)dbuf(c, "ncc.xa", na * 8);
  double* xb = (double*)dbuf(c, "ncc.xb", nb * 8);
  double* st = (double*)dbuf(c, "ncc.stats", 64);
  if (!*dc) *dc = (double*)dbuf(c, "ncc.corr", nl * 8);
  if (hc) *hc = (double*)hbuf(c, "ncc.corr", nl * 8);
  if (!xa || !xb || !st || !*dc || (hc && !*hc)) return fail(c, SONAR_ERR_NOMEM, nomem);
  hipEvent_t tend = timed ? timed_begin(c, s) : nullptr;
  if (sonar::launch_ncc(da, na, db, nb, L, xa, xb, st, *dc, s) != 0) return fail(c, SONAR_ERR_DEVICE, "ncc launch failed");
  timed_end(c, s, tend);
  return SONAR_OK;
}

// Align's argument checks (dtw.go:55-78), then the GPU path's limits
int dtw_check(sonar_ctx* c, const double* q, int64_t nq, const double* r, int64_t nr, int32_t dim, int step) {
  if (nq <= 0 || nr <= 0 || !q || !r) return fail(c, SONAR_ERR_EMPTY, "empty sequences provided");
  // applyStepPattern's default case at the first filled cell (dtw.go:159-160), wrapped by Align (:76-78)
  if (step < sonar::DTW_STEP_SYMMETRIC2 || step > sonar::DTW_STEP_SYMMETRIC1)
    return fail(c, SONAR_ERR_INVALID, "failed to fill cost matrix: unknown step pattern: " + std::to_string(step));
  if (dim <= 0) return fail(c, SONAR_ERR_INVALID, "feature dimension must be positive");
  if (nq + nr > (int64_t)INT32_MAX) return fail(c, SONAR_ERR_UNSUPPORTED, "sequence too long");
  return SONAR_OK;
}

// The cached scratch of one nq x nr DTW on c, as the record the kernels take: the geometry and the
// buffers of the sweep, the walk and the tile pass (full: the whole cost store Cn; else CK + runs).
// The sequences, band and mode are the caller's to add, a missing buffer the caller's to report.
sonar::DtwArgs dtw_scratch(sonar_ctx* c, int64_t nq, int64_t nr, bool full) {
  const sonar::DtwGeom g = sonar::dtw_geom(nq, nr);
  sonar::DtwArgs a = sonar::dtw_args(g);
  if (full) a.Cn = (double*)dbuf(c, "dtw.Cn", sonar::dtw_cn_bytes(g));
  else a.CK = (double*)dbuf(c, "dtw.CK", sonar::dtw_ck_bytes(g));
  if (!full) a.runs = (int32_t*)dbuf(c, "dtw.runs", (size_t)sonar::dtw_run_words(g) * 4);
  a.cnm = (double*)dbuf(c, "dtw.cnm", 8);
  a.Dn = (uint32_t*)dbuf(c, "dtw.Dn", sonar::dtw_dn_bytes(g));
  a.E = (uint64_t*)dbuf(c, "dtw.E", sonar::dtw_edge_bytes(g));
  a.sync = (int32_t*)dbuf(c, "dtw.sync", sonar::DTW_SYNC_BYTES);
  a.codes = (uint32_t*)dbuf(c, "dtw.codes", sonar::dtw_codes_bytes(g.cap()));
  a.plen = (int64_t*)dbuf(c, "dtw.plen", 16);
  return a;
}

// the non-finite probe of both sequences into sync[2] (math.Min's NaN / -Inf / -0 rules only matter
// when an input is not finite)
int dtw_probe(sonar_ctx* c, const sonar::DtwArgs& a, hipStream_t s) {
  HIP_TRY(c, hipMemsetAsync(a.sync + 2, 0, 4, s));
  if (sonar::launch_nonfinite(a.q, a.nq * a.dim, a.sync + 2, s) || sonar::launch_nonfinite(a.r, a.nr * a.dim, a.sync + 2, s))
    return fail(c, SONAR_ERR_DEVICE, "dtw launch failed");
  return SONAR_OK;
}

// a finished DTW's status block on the host: its counters, and the failure when it timed out
int dtw_check_status(sonar_ctx* c, const void* sync_block) {
  const std::string why = dtw_status(c, sync_block);
  return why.empty() ? SONAR_OK : fail(c, SONAR_ERR_DEVICE, why);
}

// The warping path of a walked DTW (P points): the points from the move codes and, in checkpoint
// mode, the tile pass for their costs and C[nq][nr].  The path kernels always write all three arrays:
// a->pq / pr / pc, or the cached scratch for those left null (filled in on return).
int dtw_decode(sonar_ctx* c, sonar::DtwArgs* a, int64_t P, hipStream_t s, const char* nomem) {
  const int64_t cap = sonar::dtw_geom(*a).cap();
  if (!a->pq) a->pq = (int32_t*)dbuf(c, "dtw.pq", cap * 4);
  if (!a->pr) a->pr = (int32_t*)dbuf(c, "dtw.pr", cap * 4);
  if (!a->pc) a->pc = (double*)dbuf(c, "dtw.pc", cap * 8);
  a->wstart = (int2*)dbuf(c, "dtw.wstart", sonar::dtw_wstart_bytes(P));
  if (!a->pq || !a->pr || !a->pc || !a->wstart) return fail(c, SONAR_ERR_NOMEM, nomem);
  if (sonar::launch_dtw_path_cost(*a, P, s) != 0 || (!a->Cn && sonar::launch_dtw_path_tiles(*a, P, s) != 0))
    return fail(c, SONAR_ERR_DEVICE, "dtw path launch failed");
  return SONAR_OK;
}

// DTWAlignment.Align (dtw.go:55-103) for one step pattern and metric (the metric already validated;
// mode 0 = symmetric2 / Euclidean is sonar_dtw, unchanged)
int dtw_run(sonar_ctx* c, const double* q, int64_t nq, const double* r, int64_t nr, int32_t dim, int32_t band,
            double* distance, int32_t* path_q, int32_t* path_r, double* path_cost, int64_t* path_len, double* cost,
            int32_t device_ptrs, int step, int metric) {
  if (!c) return SONAR_ERR_INVALID;
  if (const int rc = dtw_check(c, q, nq, r, nr, dim, step)) return rc;
  const int mode = sonar::dtw_mode(step, metric);
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const double *dq = q, *dr = r;
  if (!device_ptrs) {
    double* pq = (double*)dbuf(c, "dtw.q", nq * dim * 8);
    double* pr = (double*)dbuf(c, "dtw.r", nr * dim * 8);
    if (!pq || !pr) return fail(c, SONAR_ERR_NOMEM, "device allocation failed");
    HIP_TRY(c, hipMemcpyAsync(pq, q, nq * dim * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(pr, r, nr * dim * 8, hipMemcpyHostToDevice, s));
    dq = pq; dr = pr;
  }
  if (metric >= sonar::DTW_METRIC_COSINE) {
    // Cosine / Pearson: the band kernel and the tile pass read prepared rows (launch_dtw_prepare)
    const int rl = sonar::dtw_row_len(dim, metric);
    double* qp = (double*)dbuf(c, "dtw.qp", (size_t)nq * rl * 8);
    double* rp = (double*)dbuf(c, "dtw.rp", (size_t)nr * rl * 8);
    if (!qp || !rp) return fail(c, SONAR_ERR_NOMEM, "device allocation failed");
    if (sonar::launch_dtw_prepare(dq, nq, dim, metric, qp, s) || sonar::launch_dtw_prepare(dr, nr, dim, metric, rp, s))
      return fail(c, SONAR_ERR_DEVICE, "dtw launch failed");
    dq = qp; dr = rp;
  }
  // the full cost store only when the caller asks for the cost matrix; otherwise every 64th
  // column (CK) and the path costs recomputed per visited tile
  const bool full = cost != nullptr;
  sonar::DtwArgs a = dtw_scratch(c, nq, nr, full);
  if ((full ? !a.Cn : (!a.CK || !a.runs)) || !a.cnm || !a.Dn || !a.E || !a.sync || !a.codes || !a.plen)
    return fail(c, SONAR_ERR_NOMEM, "device allocation failed (cost matrix)");
  a.q = dq; a.r = dr; a.dim = dim; a.band = band; a.mode = mode;
  const sonar::DtwGeom g = sonar::dtw_geom(a);
  // (the params family has no FAST instances: mode != 0 always runs the exact min)
  bool fast = mode == 0;
  if (fast && !device_ptrs) {
    for (int64_t i = 0; i < nq * dim && fast; ++i) fast = std::isfinite(q[i]);
    for (int64_t i = 0; i < nr * dim && fast; ++i) fast = std::isfinite(r[i]);
  } else if (fast) {
    if (const int rc = dtw_probe(c, a, s)) return rc;
    int32_t nf = 0;
    HIP_TRY(c, hipMemcpyAsync(&nf, a.sync + 2, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    fast = nf == 0;
  }
  // SONAR_DTW_TRACE=<file>: per-band timestamps of the sweep (diagnostics only)
  const char* trace_path = std::getenv("SONAR_DTW_TRACE");
  a.trace = trace_path ? (uint64_t*)dbuf(c, "dtw.trace", (size_t)g.nb * 64) : nullptr;
  for (auto& e : c->dtw_ev)
    if (!e) HIP_TRY(c, hipEventCreate(&e));
  hipEvent_t tend = timed_begin(c, s);
  HIP_TRY(c, hipEventRecord(c->dtw_ev[0], s));
  if (sonar::launch_dtw(a, fast, s, c->dtw_ev[1]) != 0) return fail(c, SONAR_ERR_DEVICE, "dtw launch failed");
  HIP_TRY(c, hipEventRecord(c->dtw_ev[2], s));
  timed_end(c, s, tend);
  if (a.trace) {
    std::vector<uint64_t> t((size_t)g.nb * 8);
    HIP_TRY(c, hipMemcpyAsync(t.data(), a.trace, t.size() * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (FILE* f = std::fopen(trace_path, "wb")) { std::fwrite(t.data(), 8, t.size(), f); std::fclose(f); }
  }
  int64_t P = 0;
  alignas(8) char sblk[sonar::DTW_SYNC_BYTES];
  HIP_TRY(c, hipMemcpyAsync(&P, a.plen, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(sblk, a.sync, sizeof(sblk), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (const int rc = dtw_check_status(c, sblk)) return rc;
  // the caller's device buffers, or scratch for host pointers and for any the caller left null
  // (sonar_dtw_optimize_step_pattern wants distances only)
  if (device_ptrs) { a.pq = path_q; a.pr = path_r; a.pc = path_cost; }
  if (const int rc = dtw_decode(c, &a, P, s, "device allocation failed (path)")) return rc;
  HIP_TRY(c, hipEventRecord(c->dtw_ev[3], s));
  double cNM = 0;
  HIP_TRY(c, hipMemcpyAsync(&cNM, full ? a.Cn + sonar::dtw_cn_index(g, nq, nr) : a.cnm, 8, hipMemcpyDeviceToHost, s));
  double* cost_dev = cost;
  if (cost && !device_ptrs) {
    cost_dev = (double*)dbuf(c, "dtw.cost", (size_t)nq * (nr + 1) * 8);
    if (!cost_dev) return fail(c, SONAR_ERR_NOMEM, "device allocation failed (cost output)");
  }
  if (cost && sonar::launch_dtw_cost_rowmajor(a.Cn, g, cost_dev, s) != 0)
    return fail(c, SONAR_ERR_DEVICE, "dtw cost launch failed");
  if (!device_ptrs) {
    if (path_q) HIP_TRY(c, hipMemcpyAsync(path_q, a.pq, P * 4, hipMemcpyDeviceToHost, s));
    if (path_r) HIP_TRY(c, hipMemcpyAsync(path_r, a.pr, P * 4, hipMemcpyDeviceToHost, s));
    if (path_cost) HIP_TRY(c, hipMemcpyAsync(path_cost, a.pc, P * 8, hipMemcpyDeviceToHost, s));
    if (cost) HIP_TRY(c, hipMemcpyAsync(cost, cost_dev, (size_t)nq * (nr + 1) * 8, hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(c, hipStreamSynchronize(s));
  for (int i = 0; i < 3; ++i) {
    float f = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&f, c->dtw_ev[i], c->dtw_ev[i + 1]));
    c->dtw_ms[i] = f;
  }
  if (path_len) *path_len = P;
  if (distance) *distance = cNM / (double)P;                      // dtw.go:88-91
  return SONAR_OK;
}

// GetDistanceFunction (distance.go:10-26): Mahalanobis and every unknown value are Euclidean
int dtw_metric(int32_t m) {
  return m >= SONAR_DTW_METRIC_EUCLIDEAN && m <= SONAR_DTW_METRIC_PEARSON ? m : sonar::DTW_METRIC_EUCLIDEAN;
}

}  // namespace

extern "C" {

// ================================================================ NCC ====
int sonar_ncc(sonar_ctx* c, const double* a, int64_t na, const double* b, int64_t nb, int32_t max_lag, double* corr,
              double* metrics, int32_t device_ptrs) {
  if (!c) return SONAR_ERR_INVALID;
  if (na <= 0 || nb <= 0 || !a || !b) return fail(c, SONAR_ERR_EMPTY, "empty signals provided");
  const int64_t L = ncc_max_lag(max_lag, na, nb), nl = 2 * L + 1;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const double *da = a, *db = b;
  if (!device_ptrs) {
    double* pa = (double*)dbuf(c, "ncc.a", na * 8);
    double* pb = (double*)dbuf(c, "ncc.b", nb * 8);
    if (!pa || !pb) return fail(c, SONAR_ERR_NOMEM, "device allocation failed");
    HIP_TRY(c, hipMemcpyAsync(pa, a, na * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(pb, b, nb * 8, hipMemcpyHostToDevice, s));
    da = pa; db = pb;
  }
  double* dc = device_ptrs ? corr : nullptr;
  if (const int rc = ncc_launch(c, da, na, db, nb, L, &dc, nullptr, true, "device allocation failed")) return rc;
  std::vector<double> hc(nl);
  HIP_TRY(c, hipMemcpyAsync(hc.data(), dc, nl * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (corr && !device_ptrs) std::memcpy(corr, hc.data(), nl * 8);
  if (metrics) ncc_metrics_host(hc.data(), L, na, nb, metrics);
  return SONAR_OK;
}

// ================================================================ DTW ====
int sonar_dtw(sonar_ctx* c, const double* q, int64_t nq, const double* r, int64_t nr, int32_t dim, int32_t band,
              double* distance, int32_t* path_q, int32_t* path_r, double* path_cost, int64_t* path_len, double* cost,
              int32_t device_ptrs) {
  return dtw_run(c, q, nq, r, nr, dim, band, distance, path_q, path_r, path_cost, path_len, cost, device_ptrs,
                 sonar::DTW_STEP_SYMMETRIC2, sonar::DTW_METRIC_EUCLIDEAN);
}

int sonar_dtw_params(sonar_ctx* c, const double* q, int64_t nq, const double* r, int64_t nr, int32_t dim,
                     int32_t band, int32_t step_pattern, int32_t metric, double* distance, int32_t* path_q,
                     int32_t* path_r, double* path_cost, int64_t* path_len, double* cost, int32_t device_ptrs) {
  return dtw_run(c, q, nq, r, nr, dim, band, distance, path_q, path_r, path_cost, path_len, cost, device_ptrs,
                 step_pattern, dtw_metric(metric));
}

int sonar_dtw_quality(const int32_t* path_q, const int32_t* path_r, const double* path_cost, int64_t path_len,
                      int64_t nq, int64_t nr, double distance, double* out4) {
  if (path_len <= 0) return SONAR_ERR_EMPTY;                      // dtw.go:254-256 (an empty map there)
  if (!path_q || !path_r || !path_cost || !out4) return SONAR_ERR_INVALID;
  const double P = (double)path_len;
  out4[0] = (double)std::max(nq, nr) / P;                         // :261-262
  int64_t diag = 0;
  for (int64_t k = 1; k < path_len; ++k)                          // :265-271
    if (path_q[k] > path_q[k - 1] && path_r[k] > path_r[k - 1]) ++diag;
  out4[1] = (double)diag / (double)(path_len - 1);                // :272 (one point: 0 / 0)
  double total = 0.0;
  for (int64_t k = 0; k < path_len; ++k) total += path_cost[k];   // :275-278, in path order
  out4[2] = total / P;                                            // :279
  out4[3] = distance;                                             // :282
  return SONAR_OK;
}

int sonar_dtw_optimize_step_pattern(sonar_ctx* c, const double* q, int64_t nq, const double* r, int64_t nr,
                                    int32_t dim, int32_t band, int32_t metric, int32_t device_ptrs, int32_t* best,
                                    double* distances3) {
  if (!c) return SONAR_ERR_INVALID;
  if (!best) return fail(c, SONAR_ERR_INVALID, "best must not be null");
  // dtw.go:290-307: symmetric2, asymmetric, symmetric1; a failing Align is skipped; strict <
  const int patterns[3] = {SONAR_DTW_STEP_SYMMETRIC2, SONAR_DTW_STEP_ASYMMETRIC, SONAR_DTW_STEP_SYMMETRIC1};
  int32_t best_pattern = patterns[0];
  double best_distance = std::numeric_limits<double>::infinity();
  for (int k = 0; k < 3; ++k) {
    double d = 0.0;
    const int rc = dtw_run(c, q, nq, r, nr, dim, band, &d, nullptr, nullptr, nullptr, nullptr, nullptr, device_ptrs,
                           patterns[k], dtw_metric(metric));
    if (distances3) distances3[k] = rc == SONAR_OK ? d : std::numeric_limits<double>::quiet_NaN();
    if (rc != SONAR_OK) continue;
    if (d < best_distance) {
      best_distance = d;
      best_pattern = patterns[k];
    }
  }
  *best = best_pattern;
  return SONAR_OK;
}

}  // extern "C"

// ============================================= deferred-sync pair pieces ====
namespace sonar::detail {

std::string dtw_status(sonar_ctx* c, const void* sync_block) {
  int32_t sync[4];
  uint64_t d[sonar::DTW_DIAG_WORDS];
  std::memcpy(sync, sync_block, 16);
  std::memcpy(d, static_cast<const char*>(sync_block) + 16, sizeof(d));
  c->dtw_ctr[0] += (long long)d[13];
  c->dtw_ctr[1] += (long long)d[14];
  c->dtw_ctr[3] += (long long)d[15];
  if (!sync[1]) return std::string();
  c->dtw_ctr[2] += 1;
  static const char* roles[] = {"?", "edge", "feeder", "sweep", "code", "distance", "loader"};
  std::string roles_hit;
  for (int k = 0; k < 6; ++k)
    if (sync[1] & (1 << k)) roles_hit += std::string(roles_hit.empty() ? "" : "+") + roles[k + 1];
  char buf[768];
  if (!(d[0] >> 63)) {
    std::snprintf(buf, sizeof(buf), "dtw band pipeline timed out (roles %s; no diagnostic record)", roles_hit.c_str());
    return buf;
  }
  const int role = (int)((d[0] >> 56) & 0x7F);
  const uint64_t ticks = d[11] & 0xFFFFFFFFFFull;
  std::snprintf(buf, sizeof(buf),
                "dtw band pipeline timed out (roles %s): first %s wave, band %u ticket %u, no progress for %.3f s "
                "(%llu k polls); prog %u cprog %u efill %u rdy %d dchunk %u/%u/%u/%u edge target %u of %u; "
                "E[efill+1] sc1 %016llx after-acquire %016llx system %016llx rmw-agent %016llx rmw-system %016llx; "
                "first sentinel column %lld; xcc %u hw_id %08x; waves timed out %llu; refresh fences %llu (%llu hit)",
                roles_hit.c_str(), roles[role >= 1 && role <= 6 ? role : 0], (unsigned)(d[0] & 0xFFFFFFFF),
                (unsigned)((d[0] >> 32) & 0xFFFFFF), ticks * 1e-8, (unsigned long long)(d[11] >> 40),
                (unsigned)(d[1] & 0xFFFFFFFF), (unsigned)(d[1] >> 32), (unsigned)(d[2] & 0xFFFFFFFF),
                (int)(int32_t)(d[2] >> 32), (unsigned)(d[3] & 0xFFFF), (unsigned)((d[3] >> 16) & 0xFFFF),
                (unsigned)((d[3] >> 32) & 0xFFFF), (unsigned)((d[3] >> 48) & 0xFFFF), (unsigned)(d[4] & 0xFFFFFFFF),
                (unsigned)(d[4] >> 32), (unsigned long long)d[5], (unsigned long long)d[6], (unsigned long long)d[7],
                (unsigned long long)d[8], (unsigned long long)d[9], (long long)(int64_t)d[10], (unsigned)(d[12] & 0xFF),
                (unsigned)(d[12] >> 32), (unsigned long long)d[15], (unsigned long long)d[13],
                (unsigned long long)d[14]);
  return buf;
}

void ncc_metrics_host(const double* corr, int64_t L, int64_t na, int64_t nb, double* metrics) {
  const auto m = sonar::host::ncc_metrics(corr, 2 * L + 1, L, na, nb);
  const double v[10] = {m.peak_corr, (double)m.peak_lag, (double)m.peak_index, m.p_value, m.snr, m.sharpness,
                        m.second_peak, m.psl, (double)m.overlap, (double)m.num_lags};
  std::memcpy(metrics, v, sizeof(v));
}

// sonar_ncc's launch half: the correlation lands in pinned host memory once the stream drains
int ncc_enqueue(sonar_ctx* c, const double* da, int64_t na, const double* db, int64_t nb, int32_t max_lag,
                double** hcorr, int64_t* Lout) {
  if (na <= 0 || nb <= 0 || !da || !db) return fail(c, SONAR_ERR_EMPTY, "empty signals provided");
  const int64_t L = ncc_max_lag(max_lag, na, nb);
  double* dc = nullptr;
  if (const int rc = ncc_launch(c, da, na, db, nb, L, &dc, hcorr, false, "allocation failed (ncc)")) return rc;
  HIP_TRY(c, hipMemcpyAsync(*hcorr, dc, (2 * L + 1) * 8, hipMemcpyDeviceToHost, c->stream));
  *Lout = L;
  return SONAR_OK;
}

// sonar_dtw's launch half for device sequences: the non-finite probe runs on the device and the
// FAST (finite-input) pipeline is launched without waiting for it; dtw_finish re-runs the exact
// math.Min pipeline in the rare case the probe fired
int dtw_enqueue(sonar_ctx* c, const double* dq, int64_t nq, const double* dr, int64_t nr, int32_t dim, int32_t band,
                DtwPending* p) {
  if (const int rc = dtw_check(c, dq, nq, dr, nr, dim, sonar::DTW_STEP_SYMMETRIC2)) return rc;
  hipStream_t s = c->stream;
  sonar::DtwArgs a = dtw_scratch(c, nq, nr, false);
  int64_t* st = (int64_t*)hbuf(c, "dtw.status", 8 + sonar::DTW_SYNC_BYTES);
  if (!a.CK || !a.Dn || !a.E || !a.sync || !a.codes || !a.plen || !st)
    return fail(c, SONAR_ERR_NOMEM, "allocation failed (dtw)");
  a.q = dq; a.r = dr; a.dim = dim; a.band = band;
  if (const int rc = dtw_probe(c, a, s)) return rc;
  if (sonar::launch_dtw(a, true, s) != 0) return fail(c, SONAR_ERR_DEVICE, "dtw launch failed");
  HIP_TRY(c, hipMemcpyAsync(st, a.plen, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(st + 1, a.sync, sonar::DTW_SYNC_BYTES, hipMemcpyDeviceToHost, s));
  *p = DtwPending{a, st};
  return SONAR_OK;
}

// after the caller's stream sync: decode the path into pinned host arrays (one more sync)
int dtw_finish(sonar_ctx* c, DtwPending* p, const int32_t** hq, const int32_t** hr, const double** hc, int64_t* Pout,
               double* distance) {
  hipStream_t s = c->stream;
  sonar::DtwArgs& a = p->a;
  const int64_t cap = sonar::dtw_geom(a).cap();
  if (!a.runs || !a.cnm) return fail(c, SONAR_ERR_NOMEM, "allocation failed (dtw path)");
  int32_t nfw[3];
  std::memcpy(nfw, p->st + 1, 12);
  if (nfw[2] != 0) {                                              // non-finite input: exact math.Min rules
    if (sonar::launch_dtw(a, false, s)) return fail(c, SONAR_ERR_DEVICE, "dtw launch failed");
    HIP_TRY(c, hipMemcpyAsync(p->st, a.plen, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(p->st + 1, a.sync, sonar::DTW_SYNC_BYTES, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
  }
  if (const int rc = dtw_check_status(c, p->st + 1)) return rc;
  const int64_t P = p->st[0];
  // one pinned block: cost(N,M), path costs, then the two index arrays
  char* h = (char*)hbuf(c, "dtw.path", 8 + sonar::dtw_path_bytes(cap));
  if (!h) return fail(c, SONAR_ERR_NOMEM, "allocation failed (dtw path)");
  if (const int rc = dtw_decode(c, &a, P, s, "allocation failed (dtw path)")) return rc;
  double* hcnm = (double*)h;
  double* hcost = hcnm + 1;
  int32_t* hpq = (int32_t*)(hcost + cap);
  int32_t* hpr = hpq + cap;
  HIP_TRY(c, hipMemcpyAsync(hcnm, a.cnm, 8, hipMemcpyDeviceToHost, s));
  if (P > 0) {
    HIP_TRY(c, hipMemcpyAsync(hcost, a.pc, P * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(hpq, a.pq, P * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(hpr, a.pr, P * 4, hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(c, hipStreamSynchronize(s));
  *hq = hpq; *hr = hpr; *hc = hcost;
  *Pout = P;
  *distance = *hcnm / (double)P;                                  // dtw.go:88-91
  return SONAR_OK;
}

}  // namespace sonar::detail
