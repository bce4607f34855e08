// pairs_api.cpp -- sonar_align_pairs: the C5 unit (sonar_align_pair_device) over many stream pairs on
// one device.  Worker contexts on the caller's device, one HIP stream + host thread
// each.  Batched (default): a worker takes batches of pairs and runs each batch's chroma DTWs in ONE
// band-kernel launch with one host synchronisation, in four steps: plan (host arithmetic: every
// region and buffer size, pair_batch_layout.h), reserve (the worker's named buffers, or
// SONAR_ERR_NOMEM), enqueue (the launches and the two copies) and decode (status block -> record).
// Pairs are independent (extractors/alignment.go:139), so records equal the single-pair calls.
#include "../../include/sonar_gpu.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "ctx.h"
#include "kernels.h"
#include "pair_batch_layout.h"

using sonar::al256;
using sonar::PairBatchLayout;
using sonar::PairStatus;
using sonar::detail::dbuf;
using sonar::detail::fail;

static_assert(sonar::PAIR_DIAG_BYTES == 8 * sonar::DTW_DIAG_WORDS, "diagnostic record of a pair");

namespace {

// what is fixed across one sonar_align_pairs call
struct PairCall {
  const double* const* q_pcm; const int64_t* nq; const double* const* r_pcm; const int64_t* nr;
  int32_t sr, sw, hop, fw; double max_lag; int32_t device_ptrs; sonar_pair_record* out;
};

// the environment switches, read once at the top of each call (never kept across calls)
struct PairEnv {
  bool batched;             // SONAR_PAIR_BATCH=0: one pair at a time per worker stream (the unbatched path, for A/B)
  int streams;              // SONAR_PAIR_STREAMS: worker streams of the batched path (16)
  double batch_gb;          // SONAR_PAIR_BATCH_GB: device memory one stream's batch may hold (24)
  bool retry;               // SONAR_PAIR_RETRY=0: a pair whose band pipeline timed out is an error (the bench's setting);
                            // default: it is redone once on the single-pair path and flagged SONAR_PAIR_REDONE_TIMEOUT
  const char* dump_dir;     // SONAR_PAIR_DUMP=<dir> (tests only): the batched DTW's raw outputs of every pair
  bool host_scores;         // SONAR_PAIR_HOST_SCORES=1 (A/B, tests) or a dump: correlations and paths are copied
                            // back and the scorers' O(path) loops run on the host, not in pair_score_kernel
  bool feat_batch;          // SONAR_FEAT_BATCH=0: the pair-by-pair feature launches inside a batch (A/B)
  const char* trace_path;   // SONAR_DTW_TRACE=<file> (diagnostics): every band's sweep timestamps, appended
};
PairEnv read_env() {
  auto get = [](const char* name) { return std::getenv(name); };
  auto off = [&](const char* name) { const char* v = get(name); return v && v[0] == '0'; };
  const char *b = get("SONAR_PAIR_BATCH"), *s = get("SONAR_PAIR_STREAMS"), *gb = get("SONAR_PAIR_BATCH_GB"),
             *hs = get("SONAR_PAIR_HOST_SCORES"), *dump = get("SONAR_PAIR_DUMP");
  return {!(b && std::atoi(b) == 0), s ? std::atoi(s) : 16, gb ? std::atof(gb) : 24.0, !off("SONAR_PAIR_RETRY"), dump,
          dump || (hs && std::atoi(hs) != 0), !off("SONAR_FEAT_BATCH"), get("SONAR_DTW_TRACE")};
}

// the call's first error: its code, and "pair <k>: <text>" in the caller's context
struct CallError {
  sonar_ctx* c;
  std::atomic<int> first{SONAR_OK};
  void note(int r, int64_t k, sonar_ctx* w) {
    int expect = SONAR_OK;
    if (r != SONAR_OK && first.compare_exchange_strong(expect, r)) c->err = "pair " + std::to_string(k) + ": " + w->err;
  }
};

double scalar_of(const sonar_result* r, const char* name) {
  const double* d = nullptr;
  int64_t rows = 0, cols = 0;
  if (sonar_result_get(r, name, &d, &rows, &cols) != SONAR_OK || !d || rows * cols < 1) return NAN;
  return d[0];
}

// worker contexts of sonar_align_pairs, created once per parent context and kept
std::vector<sonar_ctx*>& workers_of(sonar_ctx* c, int n, int* rc) {
  *rc = SONAR_OK;
  while ((int)c->workers.size() < n) {
    sonar_ctx* w = nullptr;
    const int r = sonar_create(c->device, &w);
    if (r != SONAR_OK) { *rc = r; break; }
    c->workers.push_back(w);
  }
  return c->workers;
}

// pair k on the single-pair path (sonar_align_pair_device), into its record
int align_one(sonar_ctx* w, const PairCall& call, int64_t k) {
  sonar_pair_record* out = &call.out[k];
  const double *q = call.q_pcm[k], *r = call.r_pcm[k];
  const int64_t nq = call.nq[k], nr = call.nr[k];
  std::memset(out, 0, sizeof(*out));
  out->temporal_offset = out->offset_confidence = out->alignment_similarity = out->alignment_quality = NAN;
  out->method = out->corr_offset_seconds = out->dtw_distance = out->peak_lag = NAN;
  if (!call.device_ptrs) {
    if (!q || !r || nq <= 0 || nr <= 0) return out->status = fail(w, SONAR_ERR_EMPTY, "empty signal");
    double* bq = (double*)dbuf(w, "pairs.q", (size_t)nq * 8);
    double* br = (double*)dbuf(w, "pairs.r", (size_t)nr * 8);
    if (!bq || !br) return out->status = fail(w, SONAR_ERR_NOMEM, "device allocation failed");
    if (hipSetDevice(w->device) != hipSuccess ||
        hipMemcpyAsync(bq, q, (size_t)nq * 8, hipMemcpyHostToDevice, w->stream) != hipSuccess ||
        hipMemcpyAsync(br, r, (size_t)nr * 8, hipMemcpyHostToDevice, w->stream) != hipSuccess)
      return out->status = fail(w, SONAR_ERR_DEVICE, "pair upload failed");
    q = bq; r = br;
  }
  sonar_result* res = nullptr;
  const int rc = sonar_align_pair_device(w, q, nq, r, nr, call.sr, call.sw, call.hop, call.fw, call.max_lag, &res);
  out->status = rc;
  if (rc != SONAR_OK) return rc;
  out->temporal_offset = scalar_of(res, "temporal_offset");
  out->offset_confidence = scalar_of(res, "offset_confidence");
  out->alignment_similarity = scalar_of(res, "alignment_similarity");
  out->alignment_quality = scalar_of(res, "alignment_quality");
  out->method = scalar_of(res, "method");
  out->corr_offset_seconds = scalar_of(res, "corr_offset_seconds");
  out->dtw_distance = scalar_of(res, "dtw_distance");
  out->peak_lag = scalar_of(res, "peak_lag");
  sonar_result_free(res);
  return SONAR_OK;
}

// Where a pair's regions start in the batch's buffers, every region 256-byte aligned: "pb.chroma",
// "pb.CK", ...; correlations and paths inside "pb.small"; the batched features' scratch "fb.y",
// "fb.dc", "fb.energy" per signal (query, reference) and "fb.ncc" (both z-scored energies, then 256
// bytes of statistics).  As a batch's running totals (index 0): the bytes of those buffers so far.
struct PairRegions {
  size_t chroma = 0, ck = 0, runs = 0, dn = 0, e = 0, codes = 0, wst = 0, path = 0, corr = 0;
  size_t y[2] = {}, dc[2] = {}, energy[2] = {}, ncc = 0, stats = 0;
};
struct PairGeo {
  int64_t k = 0, nq = 0, nr = 0, Fq = 0, Fr = 0, Eq = 0, Er = 0, L = 0, mlf = 0;
  bool corr = false;
  sonar::DtwGeom g{};
  PairRegions at;
};

// places p's regions at the running totals t and advances them: the one definition of their sizes
void place_pair(PairGeo& p, PairRegions& t) {
  auto take = [](size_t& total, size_t bytes) { const size_t off = total; total += al256(bytes); return off; };
  p.at.chroma = take(t.chroma, (size_t)(p.Fq + p.Fr) * 96);
  p.at.ck = take(t.ck, sonar::dtw_ck_bytes(p.g));
  p.at.runs = take(t.runs, (size_t)sonar::dtw_run_words(p.g) * 4);
  p.at.dn = take(t.dn, sonar::dtw_dn_bytes(p.g));
  p.at.e = take(t.e, sonar::dtw_edge_bytes(p.g));
  p.at.codes = take(t.codes, sonar::dtw_codes_bytes(p.g.cap()));
  p.at.wst = take(t.wst, sonar::dtw_wstart_bytes(p.g.cap()));
  p.at.path = take(t.path, sonar::dtw_path_bytes(p.g.cap()));
  p.at.corr = take(t.corr, (size_t)(2 * p.L + 1) * 8);
  for (int side = 0; side < 2; ++side) {
    const int64_t ns = side ? p.nr : p.nq;
    p.at.y[side] = take(t.y[0], (size_t)ns * 8);
    p.at.dc[side] = take(t.dc[0], sonar::dc_preemph_scratch_bytes(ns));
    p.at.energy[side] = take(t.energy[0], (size_t)std::max<int64_t>(side ? p.Er : p.Eq, 1) * 8);
  }
  if (p.corr) { p.at.ncc = take(t.ncc, (size_t)(p.Eq + p.Er) * 8); p.at.stats = take(t.ncc, 256); }
}
// a path block (dtw_path_bytes): cap costs, then cap query and cap reference indices
struct PathBlock { double* pc; int32_t *pq, *pr; };
PathBlock path_block(char* paths, const PairGeo& p) {
  double* pc = (double*)(paths + p.at.path);
  int32_t* pq = (int32_t*)(pc + p.g.cap());
  return {pc, pq, pq + p.g.cap()};
}

// the named buffers of a worker context a batch runs in (the by-name cache: sonar_trim and the NOMEM
// ladder release them); from F_Y on, the batched features'; B_HOST and F_HJOBS are pinned host memory
enum Buf { B_CHROMA, B_CK, B_RUNS, B_DN, B_E, B_CODES, B_WSTART, B_SMALL, B_HOST, B_EQ, B_ER, B_XA, B_XB, B_STATS,
           B_UPQ, B_UPR, B_TRACE, F_Y, F_DC, F_ENERGY, F_NCC, F_JOBS, F_HJOBS, NBUF };
const char* const kBufName[NBUF] = {"pb.chroma", "pb.CK", "pb.runs", "pb.Dn", "pb.E", "pb.codes", "pb.wstart", "pb.small",
                                    "pb.host", "pb.eq", "pb.er", "ncc.xa", "ncc.xb", "ncc.stats", "pairs.q", "pairs.r",
                                    "pb.trace", "fb.y", "fb.dc", "fb.energy", "fb.ncc", "fb.jobs", "fb.hjobs"};
bool pinned(int b) { return b == B_HOST || b == F_HJOBS; }

// A batch, planned: its pairs placed, the layout of "pb.small" (device) and "pb.host" (pinned), and
// the bytes of every buffer it needs (use[b]: whether it needs b at all).  Pure host arithmetic.
struct BatchPlan {
  std::vector<PairGeo> pg;
  int64_t max_cap = 1, max_nb = 0, total_bands = 0, max_el = 0;
  PairBatchLayout lay;
  // the batch's music features and NCCs go in batched launches (feat_batch): the inputs are on the
  // device, the switch is on and every signal's chroma frames are fs = 256 or 512 samples
  bool feat = false;
  int fs = -1, ncorr = 0;
  size_t mf_bytes = 0;   // "fb.jobs" / "fb.hjobs": the MfJobs, then the NccJobs
  size_t bytes[NBUF] = {};
  bool use[NBUF] = {};
};

BatchPlan plan_batch(std::vector<PairGeo> pairs, const PairCall& call, const PairEnv& env) {
  BatchPlan b;
  b.pg = std::move(pairs);
  const int n = (int)b.pg.size();
  PairRegions tot;
  int64_t maxE = 1, maxn = 1;
  b.feat = call.device_ptrs && env.feat_batch && call.fw > 0 && call.hop > 0;
  for (auto& p : b.pg) {
    place_pair(p, tot);
    maxE = std::max({maxE, p.Eq, p.Er});
    maxn = std::max({maxn, p.nq, p.nr});
    b.max_cap = std::max(b.max_cap, p.g.cap());
    b.max_nb = std::max(b.max_nb, p.g.nb);
    b.total_bands += p.g.nb;   // band-kernel tickets
    b.ncorr += p.corr;
    // the non-finite probe's reach: a pair's chroma values, and the words of its band-edge rows
    b.max_el = std::max({b.max_el, (p.Fq + p.Fr) * 12, (int64_t)(sonar::dtw_edge_bytes(p.g) / 8)});
    if (b.fs < 0) b.fs = (int)(p.nq / p.Fq);   // music.go:331
    b.feat = b.feat && p.nq / p.Fq == b.fs && p.nr / p.Fr == b.fs;
  }
  b.feat = b.feat && (b.fs == 256 || b.fs == 512);
  b.lay = PairBatchLayout(n, b.total_bands, tot.corr, tot.path, sizeof(sonar::DtwArgs), sizeof(sonar::ScoreJob),
                          sizeof(sonar::host::PathSums), sizeof(sonar::host::CorrSums));
  b.mf_bytes = al256((size_t)2 * n * sizeof(sonar::MfJob));
  const size_t jobs = b.mf_bytes + al256((size_t)std::max(b.ncorr, 1) * sizeof(sonar::NccJob));
  // B_EQ .. B_STATS: the per-pair feature launches' scratch; B_UPQ, B_UPR: where host signals go up
  const size_t bytes[NBUF] = {tot.chroma, tot.ck, tot.runs, tot.dn, tot.e, tot.codes, tot.wst, b.lay.total, b.lay.total,
                              (size_t)maxE * 8, (size_t)maxE * 8, (size_t)maxE * 8, (size_t)maxE * 8, 64,
                              (size_t)maxn * 8, (size_t)maxn * 8, (size_t)b.total_bands * 64,
                              tot.y[0], tot.dc[0], tot.energy[0], std::max<size_t>(tot.ncc, 256), jobs, jobs};
  for (int i = 0; i < NBUF; ++i) {
    b.bytes[i] = bytes[i];
    b.use[i] = i >= F_Y ? b.feat : i == B_TRACE ? env.trace_path != nullptr : !(i == B_UPQ || i == B_UPR) || !call.device_ptrs;
  }
  return b;
}

// Device bytes one pair of a batch holds: the pair planned alone.  The batch cut's estimate; a
// batch's buffers are never larger than the sum over its pairs.
size_t pair_bytes(const PairGeo& p, const PairCall& call, const PairEnv& env) {
  const BatchPlan b = plan_batch({p}, call, env);
  size_t sum = 0;
  for (int i = 0; i < NBUF; ++i)
    if (b.use[i] && !pinned(i)) sum += b.bytes[i];
  return sum;
}

// a batch's buffers in worker w, by Buf; and the chroma tables of the batched features
struct BatchBufs {
  char* p[NBUF] = {};
  const sonar_ctx::ChromaT* ct = nullptr;
};

// Every buffer of the batch in worker w, or SONAR_ERR_NOMEM (no launch has gone out: the retry
// ladder of batch_worker takes it).  The sizing pass of sonar_align_pairs is plan + reserve.
int reserve_batch(sonar_ctx* w, const BatchPlan& b, int32_t sr, BatchBufs* m) {
  HIP_TRY(w, hipSetDevice(w->device));
  if (b.feat) m->ct = sonar::detail::chroma_tables_for(w, b.fs, sr);
  bool ok = true, feat_ok = !b.feat || m->ct;
  for (int i = 0; i < NBUF; ++i) {
    if (!b.use[i]) continue;
    m->p[i] = (char*)(pinned(i) ? sonar::detail::hbuf(w, kBufName[i], b.bytes[i]) : dbuf(w, kBufName[i], b.bytes[i]));
    (i < F_Y ? ok : feat_ok) &= m->p[i] != nullptr;
  }
  if (!ok) return fail(w, SONAR_ERR_NOMEM, "allocation failed (pair batch)");
  return feat_ok ? SONAR_OK : fail(w, SONAR_ERR_NOMEM, "batch features: allocation failed");
}

// The batch's music features (music.go:245-376 per signal: DC removal + pre-emphasis, energy,
// chroma) and energy NCCs (correlation.go:131-409 per pair) in eight launches instead of 13 per pair
// (DESIGN.md 6): per-signal and per-pair regions of the worker's scratch, job tables staged through
// pinned memory.  Each signal / pair runs the same kernels' arithmetic in the same order as the
// per-pair path, so the outputs are bit-identical.  What became of them: NotApplicable (BatchPlan::feat
// is off: the switch, host inputs, signals of different chroma frame sizes or outside the batched
// kernels' shapes; nothing is launched), NoMem (their buffers are not there: reserve_batch answers
// SONAR_ERR_NOMEM for that before any launch), Failed (a copy or launch did not go out).
enum class Feat { Ran, NotApplicable, NoMem, Failed };
Feat feat_batch(const BatchPlan& b, const BatchBufs& m, const PairCall& call, hipStream_t s) {
  if (!b.feat) return Feat::NotApplicable;
  if (!m.ct || !m.p[F_HJOBS]) return Feat::NoMem;
  char *hj = m.p[F_HJOBS], *dj = m.p[F_JOBS], *corr = m.p[B_SMALL] + b.lay.corr;
  auto* mj = (sonar::MfJob*)hj;
  auto* nj = (sonar::NccJob*)(hj + b.mf_bytes);
  int k = 0, c = 0;
  for (const auto& p : b.pg) {
    for (int side = 0; side < 2; ++side) {
      sonar::MfJob& j = mj[k++];
      j.x = side ? call.r_pcm[p.k] : call.q_pcm[p.k];
      j.n = side ? p.nr : p.nq;
      j.y = (double*)(m.p[F_Y] + p.at.y[side]);
      j.T = sonar::dc_chunks(j.n);
      j.ends = (double*)(m.p[F_DC] + p.at.dc[side]);
      j.ystart = j.ends + j.T;
      j.Fe = side ? p.Er : p.Eq;
      j.energy = (double*)(m.p[F_ENERGY] + p.at.energy[side]);
      j.F = side ? p.Fr : p.Fq;
      j.chroma = (double*)(m.p[B_CHROMA] + p.at.chroma) + (side ? p.Fq * 12 : 0);
    }
    if (p.corr) {
      sonar::NccJob& j = nj[c++];
      j.a = mj[k - 2].energy; j.na = p.Eq; j.b = mj[k - 1].energy; j.nb = p.Er; j.L = p.L;
      j.xa = (double*)(m.p[F_NCC] + p.at.ncc);
      j.xb = j.xa + p.Eq;
      j.stats = (double*)(m.p[F_NCC] + p.at.stats);
      j.corr = (double*)(corr + p.at.corr);
    }
  }
  if (hipMemcpyAsync(dj, hj, b.bytes[F_JOBS], hipMemcpyHostToDevice, s) != hipSuccess) return Feat::Failed;
  if (sonar::launch_music_features_batch(mj, (const sonar::MfJob*)dj, k, call.fw, call.hop, b.fs, (const double*)m.ct->win,
                                         (const double*)m.ct->trig, (const int*)m.ct->cls, s) != 0)
    return Feat::Failed;
  if (c && sonar::launch_ncc_batch(nj, (const sonar::NccJob*)(dj + b.mf_bytes), c, s) != 0) return Feat::Failed;
  return Feat::Ran;
}

// Everything of the batch on worker w's stream up to its one host synchronisation, in this order:
// every pair's music features and energy NCC, the argument fill and its ONE upload, the non-finite
// probe, ONE launch_dtw_batch over all the chroma DTWs, the scorers, and ONE copy back (each
// runtime copy is a blit kernel that needs a CU beside the band blocks).  htrace: the bands' trace
// words when tracing.
int enqueue_batch(sonar_ctx* w, const BatchPlan& b, const BatchBufs& m, const PairCall& call, const PairEnv& env,
                  std::vector<uint64_t>* htrace) {
  const int n = (int)b.pg.size();
  const PairBatchLayout& L = b.lay;
  hipStream_t s = w->stream;
  char *small = m.p[B_SMALL], *h = m.p[B_HOST], *corr = small + L.corr, *trb = m.p[B_TRACE];
  PairStatus* dstat = L.at<PairStatus>(small, L.status);
  sonar::DtwArgs *dargs = L.at<sonar::DtwArgs>(small, L.args), *hargs = L.at<sonar::DtwArgs>(h, L.args);
  int64_t* hstart = L.at<int64_t>(h, L.starts);
  HIP_TRY(w, hipMemsetAsync(small, 0, L.clear_bytes(), s));
  // batched launches over the whole batch when it qualifies, else pair by pair on the worker's scratch;
  // after Feat::Failed too: the per-pair launches write the same regions (again)
  const Feat fr = feat_batch(b, m, call, s);
  if (fr == Feat::NoMem) return fail(w, SONAR_ERR_NOMEM, "batch features: allocation failed");
  const bool fb = fr == Feat::Ran;
  double *eq = (double*)m.p[B_EQ], *er = (double*)m.p[B_ER], *up_q = (double*)m.p[B_UPQ], *up_r = (double*)m.p[B_UPR];
  int64_t acc = 0;
  for (int i = 0; i < n; ++i) {
    const PairGeo& p = b.pg[i];
    const double *dq = call.q_pcm[p.k], *dr = call.r_pcm[p.k];
    double* cq = (double*)(m.p[B_CHROMA] + p.at.chroma);
    double* cr = cq + p.Fq * 12;
    if (!fb) {
      if (!call.device_ptrs) {
        HIP_TRY(w, hipMemcpyAsync(up_q, dq, (size_t)p.nq * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(w, hipMemcpyAsync(up_r, dr, (size_t)p.nr * 8, hipMemcpyHostToDevice, s));
        dq = up_q; dr = up_r;
      }
      int rc = sonar_music_alignment_features(w, dq, p.nq, call.sr, call.sw, call.hop, call.fw, call.hop, eq, cq, 1);
      if (rc == SONAR_OK)
        rc = sonar_music_alignment_features(w, dr, p.nr, call.sr, call.sw, call.hop, call.fw, call.hop, er, cr, 1);
      if (rc != SONAR_OK) return rc;
      if (p.corr && sonar::launch_ncc(eq, p.Eq, er, p.Er, p.L, (double*)m.p[B_XA], (double*)m.p[B_XB],
                                      (double*)m.p[B_STATS], (double*)(corr + p.at.corr), s) != 0)
        return fail(w, SONAR_ERR_DEVICE, "ncc launch failed");
    }
    const PathBlock pb = path_block(small + L.path, p);
    sonar::DtwArgs& a = hargs[i];
    a = sonar::dtw_args(p.g);
    a.q = cq; a.r = cr; a.dim = 12; a.band = -1;
    a.Cn = nullptr; a.CK = (double*)(m.p[B_CK] + p.at.ck); a.runs = (int32_t*)(m.p[B_RUNS] + p.at.runs);
    a.Dn = (uint32_t*)(m.p[B_DN] + p.at.dn); a.E = (uint64_t*)(m.p[B_E] + p.at.e);
    a.codes = (uint32_t*)(m.p[B_CODES] + p.at.codes); a.wstart = (int2*)(m.p[B_WSTART] + p.at.wst);
    a.sync = dstat[i].sync; a.plen = &dstat[i].plen; a.cnm = &dstat[i].cnm;
    a.pc = pb.pc; a.pq = pb.pq; a.pr = pb.pr;
    a.diag = L.at<uint64_t>(small, L.diag) + (size_t)i * sonar::DTW_DIAG_WORDS;
    a.trace = trb ? (uint64_t*)(trb + (size_t)acc * 64) : nullptr;
    a.dbg_stall = sonar::dtw_dbg_stall_band(true);
    L.at<sonar::ScoreJob>(h, L.jobs)[i] = sonar::ScoreJob{
        a.pq, a.pr, a.pc, a.plen, p.corr ? (const double*)(corr + p.at.corr) : nullptr, 2 * p.L + 1,
        L.at<sonar::host::PathSums>(small, L.path_sums) + i, L.at<sonar::host::CorrSums>(small, L.corr_sums) + i};
    hstart[i] = acc;
    acc += p.g.nb;
  }
  hstart[n] = acc;
  // band-major tickets across the batch: band b of every DTW before band b+1 of any, so a block
  // waits about one hand-off for its predecessor band rather than b of them while holding its slot
  int2* hmap = L.at<int2>(h, L.map);
  for (int64_t band = 0; band < b.max_nb; ++band)
    for (int i = 0; i < n; ++i)
      if (band < b.pg[i].g.nb) *hmap++ = make_int2(i, (int)band);
  HIP_TRY(w, hipMemcpyAsync(small + L.upload_offset(), h + L.upload_offset(), L.upload_bytes(), hipMemcpyHostToDevice, s));
  // the non-finite probe of every pair's chroma in one launch (flags in each pair's sync[2]); the
  // same launch fills every pair's band-edge rows E with the band kernel's sentinel
  if (sonar::launch_nonfinite_batch(dargs, n, b.max_el, s) != 0) return fail(w, SONAR_ERR_DEVICE, "dtw launch failed");
  if (sonar::launch_dtw_batch(hargs, dargs, L.at<int64_t>(small, L.starts), n, b.total_bands, b.max_cap,
                              L.at<int32_t>(small, L.ticket), s, L.at<int2>(small, L.map)) != 0)
    return fail(w, SONAR_ERR_DEVICE, "dtw batch launch failed");
  if (!env.host_scores && sonar::launch_pair_scores(L.at<sonar::ScoreJob>(small, L.jobs), n, s) != 0)
    return fail(w, SONAR_ERR_DEVICE, "score launch failed");
  HIP_TRY(w, hipMemcpyAsync(h, small, env.host_scores ? L.total : L.head_bytes(), hipMemcpyDeviceToHost, s));
  htrace->resize(trb ? (size_t)b.total_bands * 8 : 0);
  if (trb) HIP_TRY(w, hipMemcpyAsync(htrace->data(), trb, htrace->size() * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(w, hipStreamSynchronize(s));
  return SONAR_OK;
}

// SONAR_DTW_TRACE: the batch's bands appended to the file as {pair, band, 8 trace words} records
void append_trace(const char* file, const BatchPlan& b, const std::vector<uint64_t>& htrace) {
  static std::mutex trace_mu;
  std::lock_guard<std::mutex> lk(trace_mu);
  FILE* f = std::fopen(file, "ab");
  if (!f) return;
  const uint64_t* words = htrace.data();
  for (const auto& p : b.pg)
    for (int64_t band = 0; band < p.g.nb; ++band, words += 8) {
      const uint64_t hdr[2] = {(uint64_t)p.k, (uint64_t)band};
      std::fwrite(hdr, 8, 2, f);
      std::fwrite(words, 8, 8, f);
    }
  std::fclose(f);
}

// SONAR_PAIR_DUMP: the batched DTW's raw outputs of pair k (path length, C[nq][nr], path costs, query
// and reference indices) into <dir>/pair_<k>.bin, to be checked against the oracle
void dump_pair(const char* dir, int64_t k, const PairStatus& st, const PathBlock& pb) {
  FILE* f = std::fopen((std::string(dir) + "/pair_" + std::to_string(k) + ".bin").c_str(), "wb");
  if (!f) return;
  std::fwrite(&st.plen, 8, 1, f);
  std::fwrite(&st.cnm, 8, 1, f);
  std::fwrite(pb.pc, 8, (size_t)st.plen, f);
  std::fwrite(pb.pq, 4, (size_t)st.plen, f);
  std::fwrite(pb.pr, 4, (size_t)st.plen, f);
  std::fclose(f);
}

// of one worker: pairs to be redone on the single-pair path (with the record flag that says why), and
// pairs whose band pipeline failed (with the diagnostic text)
struct WorkerLists {
  std::vector<std::pair<int64_t, int32_t>> redo;
  std::vector<std::pair<int64_t, std::string>> errs;
};

// The copied-back status block, pair by pair: the record, or an entry of the redo list
// (SONAR_PAIR_REDONE_NONFINITE: the chroma is not finite, the batch ran the finite-input kernel and
// the exact math.Min rules are on the single-pair path; SONAR_PAIR_REDONE_TIMEOUT: the band pipeline
// timed out and the retry is on; the timeout stays counted in sonar_dtw_counters), or of the error list.
void decode_batch(sonar_ctx* w, const BatchPlan& b, const BatchBufs& m, const PairCall& call, const PairEnv& env,
                  WorkerLists* lists) {
  const PairBatchLayout& L = b.lay;
  char* h = m.p[B_HOST];
  for (int i = 0; i < (int)b.pg.size(); ++i) {
    const PairGeo& p = b.pg[i];
    const PairStatus& st = L.at<PairStatus>(h, L.status)[i];
    sonar_pair_record* rec = &call.out[p.k];
    if (st.sync[2]) { lists->redo.emplace_back(p.k, SONAR_PAIR_REDONE_NONFINITE); continue; }
    alignas(8) char sblk[sonar::DTW_SYNC_BYTES];
    std::memcpy(sblk, st.sync, 16);
    std::memcpy(sblk + 16, L.at<char>(h, L.diag) + (size_t)i * sonar::PAIR_DIAG_BYTES, sonar::PAIR_DIAG_BYTES);
    const std::string why = sonar::detail::dtw_status(w, sblk);
    if (!why.empty() && env.retry) { lists->redo.emplace_back(p.k, SONAR_PAIR_REDONE_TIMEOUT); continue; }
    if (!why.empty()) {
      std::memset(rec, 0, sizeof(*rec));
      rec->status = fail(w, SONAR_ERR_DEVICE, why);
      lists->errs.emplace_back(p.k, why);
      continue;
    }
    const PathBlock pb = path_block(h + L.path, p);   // copied back with host scoring only
    if (env.dump_dir) dump_pair(env.dump_dir, p.k, st, pb);
    sonar::detail::AlignIn ai;
    ai.q_pcm_len = p.nq; ai.r_pcm_len = p.nr; ai.sample_rate = call.sr; ai.hop = call.hop;
    if (p.corr) {
      if (env.host_scores) ai.corr = (const double*)(h + L.corr + p.at.corr);
      else ai.corr_sums = L.at<sonar::host::CorrSums>(h, L.corr_sums) + i;
      ai.L = p.L; ai.nqe = p.Eq; ai.nre = p.Er; ai.mlf = p.mlf;
    }
    ai.has_dtw = true;
    if (env.host_scores) { ai.pc = pb.pc; ai.pq = pb.pq; ai.pr = pb.pr; }
    else ai.path_sums = L.at<sonar::host::PathSums>(h, L.path_sums) + i;
    ai.P = st.plen; ai.nqc = p.Fq; ai.nrc = p.Fr; ai.dist = st.cnm / (double)st.plen;   // dtw.go:88-91
    sonar::detail::align_finish(ai, nullptr, rec);
    rec->status = SONAR_OK;
    rec->flags = 0;
  }
}

// one planned batch on worker w's stream: reserve, enqueue, decode
int align_batch(sonar_ctx* w, const BatchPlan& b, const PairCall& call, const PairEnv& env, WorkerLists* lists) {
  BatchBufs m;
  std::vector<uint64_t> htrace;
  int rc = reserve_batch(w, b, call.sr, &m);
  if (rc == SONAR_OK) rc = enqueue_batch(w, b, m, call, env, &htrace);
  if (rc != SONAR_OK) return rc;
  if (env.trace_path) append_trace(env.trace_path, b, htrace);
  decode_batch(w, b, m, call, env, lists);
  return SONAR_OK;
}

// what the workers of one call share: the planned batches, the next one to take, the sizing barrier
struct BatchQueue {
  std::vector<BatchPlan> plans;
  std::atomic<size_t> next{0};
  std::mutex mu;
  std::condition_variable cv;
  int sized = 0, nworkers = 0;
};

void batch_worker(sonar_ctx* w, BatchQueue& q, const PairCall& call, const PairEnv& env, CallError& err,
                  WorkerLists* lists) {
  // sizing pass: every worker reserves its buffers for the largest of all batches before any
  // worker launches, so no device or pinned allocation (which synchronises the device) happens
  // while other workers' band pipelines run
  for (const auto& b : q.plans) {
    BatchBufs m;
    if (reserve_batch(w, b, call.sr, &m) != SONAR_OK) break;   // NOMEM: the batch loop's retry path handles it
  }
  // one small fill on the worker's stream: HIP gives a stream its hardware queue at its first
  // command, so every worker's queue exists before any worker's DTW pipeline runs
  if (hipSetDevice(w->device) == hipSuccess) {
    if (void* z = dbuf(w, "pb.touch", 256)) (void)hipMemsetAsync(z, 0, 256, w->stream);
    (void)hipStreamSynchronize(w->stream);
  }
  {
    std::unique_lock<std::mutex> lk(q.mu);
    if (++q.sized == q.nworkers) q.cv.notify_all();
    else q.cv.wait(lk, [&] { return q.sized == q.nworkers; });
  }
  for (size_t bi = q.next.fetch_add(1); bi < q.plans.size(); bi = q.next.fetch_add(1)) {
    const BatchPlan& b = q.plans[bi];
    int r = align_batch(w, b, call, env, lists);
    if (r == SONAR_ERR_NOMEM) {
      // the worker's cached buffers are sized by earlier batches, name by name: release them
      // and retry the batch once; then pair by pair on the unbatched path
      sonar::detail::trim_buffers(w);
      r = align_batch(w, b, call, env, lists);
      if (r == SONAR_ERR_NOMEM) {
        sonar::detail::trim_buffers(w);
        r = SONAR_OK;
        for (const auto& p : b.pg) err.note(align_one(w, call, p.k), p.k, w);
      }
    }
    if (r != SONAR_OK)
      for (const auto& p : b.pg) { call.out[p.k].status = r; err.note(r, p.k, w); }
  }
  for (const auto& [k, why] : lists->redo) {       // exact single-pair path, flagged in the record
    err.note(align_one(w, call, k), k, w);
    call.out[k].flags |= why;
  }
}

// the pairs the batched path takes, validated and sized; any other pair gets its status here
std::vector<PairGeo> size_pairs(sonar_ctx* c, int64_t npairs, const PairCall& call, CallError& err) {
  const int64_t max_lag_samples = (int64_t)(call.max_lag * (double)call.sr);   // alignment.go:104
  std::vector<PairGeo> geo;
  for (int64_t k = 0; k < npairs; ++k) {
    sonar_pair_record* rec = &call.out[k];
    std::memset(rec, 0, sizeof(*rec));
    int st = SONAR_OK;
    PairGeo p;
    p.k = k; p.nq = call.nq[k]; p.nr = call.nr[k];
    if (!call.q_pcm[k] || !call.r_pcm[k] || p.nq <= 0 || p.nr <= 0) st = fail(c, SONAR_ERR_EMPTY, "empty signal");
    else if (call.sw <= 0 || call.hop <= 0) st = fail(c, SONAR_ERR_INVALID, "window and hop size must be positive");
    if (st == SONAR_OK) {
      p.Fq = sonar_stft_frames(p.nq, call.sw, call.hop);
      p.Fr = sonar_stft_frames(p.nr, call.sw, call.hop);
      if (p.Fq <= 0 || p.Fr <= 0) st = fail(c, SONAR_ERR_TOO_SHORT, "signal too short for given window size and hop size");
      else if (p.Fq + p.Fr > (int64_t)INT32_MAX) st = fail(c, SONAR_ERR_UNSUPPORTED, "sequence too long");
    }
    if (st != SONAR_OK) { rec->status = st; err.note(st, k, c); continue; }
    p.Eq = sonar_energy_frames(p.nq, call.fw, call.hop);
    p.Er = sonar_energy_frames(p.nr, call.fw, call.hop);
    p.corr = p.Eq > 0 && p.Er > 0;
    if (p.corr) {
      p.mlf = std::min(max_lag_samples / call.hop, std::min(p.Eq, p.Er) - 1);
      p.L = std::max<int64_t>(0, std::min({p.mlf, p.Eq - 1, p.Er - 1}));
    }
    p.g = sonar::dtw_geom(p.Fq, p.Fr);
    geo.push_back(p);
  }
  return geo;
}

// The pairs in batches of up to `per`, cut further by a device-memory budget per stream:
// SONAR_PAIR_BATCH_GB, and ~70 % of the device memory free now over the streams (each holds one batch)
void cut_batches(sonar_ctx* c, const std::vector<PairGeo>& geo, int64_t per, int nstreams, const PairCall& call,
                 const PairEnv& env, std::vector<BatchPlan>* plans) {
  size_t budget = (size_t)(env.batch_gb * (1ull << 30)), fr = 0, tot = 0;
  if (hipSetDevice(c->device) == hipSuccess && hipMemGetInfo(&fr, &tot) == hipSuccess && fr > 0)
    budget = std::min(budget, (size_t)(0.7 * (double)fr / (double)nstreams));
  for (size_t i = 0; i < geo.size();) {
    std::vector<PairGeo> b;
    size_t bytes = 0;
    while (i < geo.size() && (int64_t)b.size() < per && (b.empty() || bytes + pair_bytes(geo[i], call, env) <= budget)) {
      bytes += pair_bytes(geo[i], call, env);
      b.push_back(geo[i++]);
    }
    plans->push_back(plan_batch(std::move(b), call, env));
  }
}

}  // namespace

extern "C" int sonar_align_pairs(sonar_ctx* c, int64_t npairs, const double* const* q_pcm, const int64_t* nq,
                                 const double* const* r_pcm, const int64_t* nr, int32_t sample_rate,
                                 int32_t stft_window, int32_t hop, int32_t feature_window, double max_lag_seconds,
                                 int32_t workers, int32_t device_ptrs, sonar_pair_record* out) {
  if (!c) return SONAR_ERR_INVALID;
  if (npairs < 0 || (npairs > 0 && (!q_pcm || !nq || !r_pcm || !nr || !out)))
    return fail(c, SONAR_ERR_INVALID, "null pair arrays");
  if (npairs == 0) return SONAR_OK;
  const PairCall call{q_pcm, nq, r_pcm, nr, sample_rate, stft_window, hop, feature_window, max_lag_seconds,
                      device_ptrs, out};
  const PairEnv env = read_env();
  const int64_t inflight = workers > 0 ? workers : 128;   // pairs in flight (measured: C5 rises to ~128)
  const int nstreams = env.batched ? (int)std::max<int64_t>(1, std::min<int64_t>(env.streams, npairs))
                                   : (int)std::min<int64_t>(std::min<int64_t>(inflight, 16), npairs);
  int rc = SONAR_OK;
  std::vector<sonar_ctx*>& ws = workers_of(c, nstreams, &rc);
  if (rc != SONAR_OK) return fail(c, rc, "worker context creation failed");
  CallError err{c};
  std::vector<std::thread> th;
  if (!env.batched) {
    std::atomic<int64_t> next{0};
    for (int t = 0; t < nstreams; ++t)
      th.emplace_back([&, t] {
        for (int64_t k = next.fetch_add(1); k < npairs; k = next.fetch_add(1)) err.note(align_one(ws[t], call, k), k, ws[t]);
      });
    for (auto& x : th) x.join();
    return err.first.load();
  }
  // batched: each stream takes batches of up to the in-flight count split over the streams
  BatchQueue q;
  q.nworkers = nstreams;
  cut_batches(c, size_pairs(c, npairs, call, err), std::max<int64_t>(1, (inflight + nstreams - 1) / nstreams), nstreams,
              call, env, &q.plans);
  std::vector<WorkerLists> lists(nstreams);
  for (int t = 0; t < nstreams; ++t) th.emplace_back([&, t] { batch_worker(ws[t], q, call, env, err, &lists[t]); });
  for (auto& x : th) x.join();
  for (sonar_ctx* w : ws)                            // band-kernel liveness counters to the caller's ctx
    for (int k = 0; k < 4; ++k) { c->dtw_ctr[k] += w->dtw_ctr[k]; w->dtw_ctr[k] = 0; }
  // per-pair device failures (the band pipeline's diagnostic text), lowest pair first; an error
  // noted while the call ran comes before them
  std::vector<std::pair<int64_t, std::string>> all;
  for (auto& l : lists) all.insert(all.end(), l.errs.begin(), l.errs.end());
  if (!all.empty() && err.first.load() == SONAR_OK) {
    std::sort(all.begin(), all.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
    err.first = call.out[all[0].first].status;
    c->err = "pair " + std::to_string(all[0].first) + ": " + all[0].second;
    if (all.size() > 1) c->err += " (" + std::to_string(all.size() - 1) + " more pairs failed)";
  }
  return err.first.load();
}
