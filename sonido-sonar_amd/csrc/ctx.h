// ctx.h -- internal state behind the opaque sonar_ctx / sonar_result handles,
// shared by the kernel-level entries (sonar_api.cpp, fp_api.cpp, align_api.cpp, ...) and the Go-API mirrors
// (speech_api.cpp, align_extract_api.cpp).
#pragma once
#include "../../include/sonar_gpu.h"

#include <hip/hip_runtime.h>

#include "kernels.h"

#include <algorithm>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

struct DevBuf {
  void* ptr = nullptr;
  size_t cap = 0;
  // cached tables only (sonar::detail::cached_table): the upload completed, and what the builder
  // wants kept with the entry (the HPCP table's entry count)
  bool ready = false;
  int64_t tag = 0;
};

// Cached tables of the fingerprint paths and the chroma kernel: ONE device allocation each (base, the
// upload of a host image of fp_tables.h; sonar_destroy frees it) and typed views into it.
struct FpTables {
  void* base = nullptr;
  void* window = nullptr;
  int *mel_lo = nullptr, *mel_hi = nullptr, *mel_woff = nullptr, *grp_off = nullptr, *grp_mels = nullptr;
  void *mel_w = nullptr, *dct = nullptr, *lift = nullptr;
  void* trig = nullptr;   // generic-W path: (cos, -sin) of 2 pi m / W
  int n_mels = 0, n_mfcc = 0, nnz = 0;
};

// tables of the headline kernel (mfcc_pair.hip); ok = false -> configuration unsupported there
struct PairTables {
  bool ok = false;
  void* base = nullptr;
  // [0] float32 tables (the headline), [1] float64 (the same bank at the reference's precision; its
  // own chunk lane order, searched for its 16-byte power-row reads)
  void *window[2] = {}, *tw1[2] = {}, *tw2[2] = {}, *chunk_w[2] = {}, *dct[2] = {};
  int* chunk_ks[2] = {};
  uint16_t* mel_src[2] = {};
  void* zeros = nullptr;    // 1024 zero samples of either PCM type (8 KB)
  int JS[2] = {};           // chunk_w row stride per precision (mfcc_pair_w_stride)
  int J = 0, NMP = 0, n_mels = 0, n_mfcc = 0, max_src = 0;
};

struct IngestState;  // pinned slots + host pool of sonar_ingest_f64le (ingest_api.cpp)

struct sonar_ctx {
  int device = 0;
  int cus = 256;   // the device's compute units (sonar_create); the launch geometry of the fused kernels
  hipStream_t own = nullptr;
  hipStream_t stream = nullptr;
  std::string err;
  std::map<std::string, DevBuf> bufs;
  std::map<std::string, DevBuf> hbufs;   // pinned host staging (hipHostMalloc)
  std::map<std::string, FpTables> fp_tables;
  std::map<std::string, PairTables> pair_tables;
  struct ChromaT { void* base; void* win; void* trig; void* map; void* cls; };
  std::map<std::string, ChromaT> chroma_tables;
  bool timing = false;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;   // spare pair (kept for ABI simplicity)
  // one event pair per timed launch since the last sonar_last_kernel_ms query
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
  size_t ev_used = 0;
  double last_ms = 0.0;
  const char* last_fp_kernel = "";
  hipEvent_t dtw_ev[4] = {nullptr, nullptr, nullptr, nullptr};   // band | walk | decode boundaries
  double dtw_ms[3] = {0.0, 0.0, 0.0};
  IngestState* ingest = nullptr;
  std::vector<sonar_ctx*> workers;   // sonar_align_pairs' worker contexts (pairs_api.cpp)
  // a second stream for the NCC while the chroma DTW runs on `stream` (align_impl), and the two
  // events that order it: features done -> side, NCC done -> stream
  hipStream_t side = nullptr;
  hipEvent_t side_ev[2] = {nullptr, nullptr};
  // the host-PCM pipeline of sonar_extract_speech_features: H2D chunks on `copy`, one event per
  // chunk the compute streams wait on (speech_api.cpp)
  hipStream_t copy = nullptr;
  std::vector<hipEvent_t> chunk_ev;
  // ... and chunk k's pitch rows on the host (side stream), for the early tracker
  std::vector<hipEvent_t> back_ev;
  // band-kernel liveness counters (sonar_dtw_counters): edge refresh fences, those followed by new
  // edge values, DTWs that timed out, waves that timed out
  long long dtw_ctr[4] = {0, 0, 0, 0};
  // sonar_fingerprint_batch: its segment table's pinned staging is rewritten only after the previous
  // call's upload of it has completed (this event)
  hipEvent_t fpb_ev = nullptr;
  // sonar_chroma_similarity's kernel families (chroma_sim_api.cpp): an event pair each for the frame
  // matrix, the ordered sums, the DP fill and the traceback, and the last call's times
  hipEvent_t csim_ev[8] = {};
  double csim_ms[4] = {0.0, 0.0, 0.0, 0.0};
};

// Named float64 arrays + scalars.  An array either owns its values (v) or points into a block the
// result holds a reference to (ext + owners: pinned host memory the device copied into directly,
// sonar::detail::pinned_block), so large outputs reach the caller without a host copy.
struct sonar_result {
  struct Arr {
    std::string name;
    std::vector<double> v;
    int64_t rows = 0, cols = 0;
    const double* ext = nullptr;
    const double* data() const { return ext ? ext : v.data(); }
  };
  std::vector<Arr> arrays;
  std::vector<std::shared_ptr<void>> owners;
  Arr& slot(const std::string& name) {
    for (auto& a : arrays)
      if (a.name == name) return a;
    arrays.push_back({name, {}, 0, 0, nullptr});
    return arrays.back();
  }
  void put(const std::string& name, std::vector<double> v, int64_t rows, int64_t cols) {
    Arr& a = slot(name);
    a.v = std::move(v); a.rows = rows; a.cols = cols; a.ext = nullptr;
  }
  // rows x cols values at p, inside a block this result holds (see hold)
  void put_ext(const std::string& name, const double* p, int64_t rows, int64_t cols) {
    Arr& a = slot(name);
    a.v.clear(); a.rows = rows; a.cols = cols; a.ext = p;
  }
  void hold(std::shared_ptr<void> block) { owners.push_back(std::move(block)); }
  void scalar(const std::string& name, double x) { put(name, {x}, 1, 1); }
  void vec(const std::string& name, const std::vector<double>& v) { put(name, v, (int64_t)v.size(), 1); }
  double get(const std::string& name, double dflt = 0.0) const {
    for (auto& a : arrays)
      if (a.name == name && a.rows * a.cols > 0) return a.data()[0];
    return dflt;
  }
};

namespace sonar {
namespace detail {
int fail(sonar_ctx* c, int code, const std::string& msg);
void* dbuf(sonar_ctx* c, const std::string& name, size_t bytes);
// The device table `name`, cached in c->bufs until sonar_trim.  When it is not there, build fills the
// host image (and may set the tag kept with the entry); the image is uploaded on c->stream and the
// stream synchronised, and only then does the entry become servable.  A failed build returns its own
// code (it sets the error text), a failed allocation SONAR_ERR_NOMEM "device allocation failed
// (<what>)", a failed upload SONAR_ERR_DEVICE; each of them leaves no entry behind.
using TableBuilder = std::function<int(std::vector<unsigned char>& image, int64_t& tag)>;
int cached_table(sonar_ctx* c, const std::string& name, const char* what, const TableBuilder& build,
                 const unsigned char** table, int64_t* tag = nullptr);
// frees every cached device / pinned host buffer of c (sonar_trim; the batch path's NOMEM retry)
void trim_buffers(sonar_ctx* c);
void* hbuf(sonar_ctx* c, const std::string& name, size_t bytes);
// A block of `bytes` of pinned host memory from a process-wide pool (hipHostMalloc'd once, reused):
// device-to-host copies land in it at DMA speed and result arrays can point into it; the block
// returns to the pool when the last shared_ptr to it goes.  Null on allocation failure.
std::shared_ptr<void> pinned_block(size_t bytes);
// frees the pool's idle blocks (sonar_trim)
void pinned_pool_trim();
// A host image of tables (fp_tables.h) as one device allocation: one hipMalloc and one blocking
// hipMemcpy; null, with nothing left allocated, when either fails (fp_api.cpp)
void* upload_image(const std::vector<unsigned char>& image);
// chroma tables of frame size fs at sample rate sr, built once per context (sonar_api.cpp); null on
// allocation failure
const sonar_ctx::ChromaT* chroma_tables_for(sonar_ctx* c, int fs, int sr);
// calculateActualMaxLag (correlation.go:452-461): the lags an NCC of na and nb samples computes
inline int64_t ncc_max_lag(int64_t max_lag, int64_t na, int64_t nb) {
  return std::max<int64_t>(std::min({max_lag, na - 1, nb - 1}), 0);
}
// NCC + chroma DTW of one stream pair with two stream synchronisations (the device path of
// align_extract_api.cpp's align_impl; defined in align_api.cpp): ncc_enqueue and dtw_enqueue only
// launch and queue their small results into pinned host memory; after one hipStreamSynchronize,
// ncc_metrics_host reads the correlation and dtw_finish decodes the warping path into pinned host
// arrays (second sync).
struct DtwPending {
  sonar::DtwArgs a{};      // the queued DTW: its sequences, geometry and scratch (dtw_scratch)
  int64_t* st = nullptr;   // pinned: [0] path length, [1] sync words 0..1, [2] non-finite flag
};
int ncc_enqueue(sonar_ctx* c, const double* da, int64_t na, const double* db, int64_t nb, int32_t max_lag,
                double** hcorr, int64_t* L);
void ncc_metrics_host(const double* corr, int64_t L, int64_t na, int64_t nb, double* metrics);
// the band kernel's status block of one DTW (int32 sync[4] + the DtwArgs::diag record): adds its
// counters to c->dtw_ctr and, when the DTW timed out, returns the failure text with the record
std::string dtw_status(sonar_ctx* c, const void* sync_block);
int dtw_enqueue(sonar_ctx* c, const double* dq, int64_t nq, const double* dr, int64_t nr, int32_t dim, int32_t band,
                DtwPending* p);
int dtw_finish(sonar_ctx* c, DtwPending* p, const int32_t** hq, const int32_t** hr, const double** hc, int64_t* P,
               double* distance);
// ExtractAlignmentFeatures' host tail over the GPU results of one pair (align_extract_api.cpp): the scorers,
// selectBestAlignment and the time-stretch estimate, into a result handle and/or a pair record
struct AlignIn {
  const double* corr = nullptr;   // energy correlation, 2L+1 lags (null: no correlation candidate)
  const host::CorrSums* corr_sums = nullptr;   // or its reductions (the device scorer's), no array
  int64_t L = 0, nqe = 0, nre = 0, mlf = 0;
  bool has_dtw = false;           // chroma DTW candidate
  const int32_t *pq = nullptr, *pr = nullptr;
  const double* pc = nullptr;
  const host::PathSums* path_sums = nullptr;   // or the path's reductions, no arrays
  int64_t P = 0, nqc = 0, nrc = 0;
  double dist = 0.0;
  int64_t q_pcm_len = 0, r_pcm_len = 0;
  int32_t sample_rate = 0, hop = 0;
};
void align_finish(const AlignIn& in, sonar_result* res, sonar_pair_record* rec);
// sonar_music_alignment_features (music_api.cpp); `tag` prefixes the names of the call's scratch, so the
// two streams of sonar_align_pair_device keep their own
int music_features_impl(sonar_ctx* c, const double* pcm, int64_t n, int32_t sr, int32_t stft_w, int32_t stft_h,
                        int32_t fw, int32_t fh, double* energy, double* chroma, int32_t device_ptrs, const char* tag);
hipEvent_t timed_begin(sonar_ctx* c, hipStream_t s);
// the context a comparator gallery lives on (compare_api.cpp)
sonar_ctx* gallery_ctx(const sonar_gallery* g);
// ContentDetector (content_api.cpp)
int detect_from_audio(sonar_ctx* c, const double* pcm, int64_t n, int32_t sr, double thr, int32_t* out,
                      sonar_acoustic_features* feat);
int detect_content_type(sonar_ctx* c, const double* pcm, int64_t n, int32_t sr, int32_t has_md, const char* ct,
                        const char* genre, const char* station, const char* url, int32_t acoustic,
                        int32_t dflt, double thr, int32_t* out);
void timed_end(sonar_ctx* c, hipStream_t s, hipEvent_t end);
// frees the ingest ring and joins its host threads (ingest_api.cpp)
void ingest_release(sonar_ctx* c);
// sonar_fingerprint with the PCM already on the device and host outputs (fp_api.cpp)
// [f_lo, f_hi): only those frames of the whole signal's STFT (device outputs, per-frame kernel)
// raw_window: the window table is not energy-normalised (HarmonicProduct.applyWindow, sonar_hps); a
// table of its own under its own cache key, the kernels are the same
int fingerprint_impl(sonar_ctx* c, const void* pcm, int64_t n, const sonar_fp_cfg* cfg, sonar_fp_out* out,
                     bool pcm_dev, int64_t f_lo = 0, int64_t f_hi = -1, bool raw_window = false);
// sonar_fingerprint's argument checks in its order: SONAR_OK and the frame count, or the code and text
int fp_check(const sonar_fp_cfg* cfg, int64_t n, bool have_pcm, int64_t* F, std::string* msg);
// VoiceQualityAnalyzer.AnalyzeVoiceQuality on device-resident float64 samples (voice_api.cpp)
int voice_quality(sonar_ctx* c, const double* dsig, int64_t n, int32_t sr, sonar_voice_quality_result* out);
}  // namespace detail
}  // namespace sonar

#define HIP_TRY(ctx, call)                                                                   \
  do {                                                                                       \
    hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess)                                                                    \
      return ::sonar::detail::fail(ctx, SONAR_ERR_DEVICE, std::string(#call ": ") + hipGetErrorString(e_)); \
  } while (0)

namespace sonar {
namespace detail {
// c->side and its two events, created on first use (the context's device is current)
inline int ensure_side(sonar_ctx* c) {
  if (c->side) return SONAR_OK;
  HIP_TRY(c, hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
  for (auto& e : c->side_ev) HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  return SONAR_OK;
}
// While one lives, c->stream is the side stream, so a callee that works on c->stream works there.
// Scope it to the call: the caller's stream is back before the callee's status is looked at.
struct OnSideStream {
  sonar_ctx* c;
  hipStream_t main;
  explicit OnSideStream(sonar_ctx* ctx) : c(ctx), main(ctx->stream) { c->stream = c->side; }
  ~OnSideStream() { c->stream = main; }
  OnSideStream(const OnSideStream&) = delete;
  OnSideStream& operator=(const OnSideStream&) = delete;
};
// On any early exit the streams a call queued work on are drained before the host memory its copies land
// in goes away (a pinned block on its way back to the pool, a local vector).  Declare it after that
// memory, so it runs first; disarm it after the synchronisation that ends the call's device work.
struct DrainOnExit {
  sonar_ctx* c;
  bool copy = false, side = false;   // this call also used c->copy / c->side
  bool armed = true;
  ~DrainOnExit() {
    if (!armed) return;
    if (copy) (void)hipStreamSynchronize(c->copy);
    if (side) (void)hipStreamSynchronize(c->side);
    (void)hipStreamSynchronize(c->stream);
  }
};
}  // namespace detail
}  // namespace sonar
