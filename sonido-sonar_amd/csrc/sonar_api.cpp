// sonar_api.cpp -- the C ABI of include/sonar_gpu.h: the context, its device-buffer and pinned pools,
// YIN, STFT chroma, formants and the result object.
//
// Low-level entries (sonar_pitch_yin, sonar_chroma_stft, sonar_formants; sonar_fingerprint is
// fp_api.cpp's, sonar_ncc and sonar_dtw align_api.cpp's) validate exactly like the Go functions they replace,
// stage host buffers when device_ptrs == 0, and launch the HIP kernels.
// High-level entries (sonar_generate_fingerprint, sonar_align_features) are
// the C++ restatement of the Go orchestration above those seams
// (fingerprint/fingerprint.go:137-236, fingerprint/extractors/speech.go:135-550,
// fingerprint/extractors/alignment.go:139-476).  There is no CPU fallback:
// every numeric array comes from a GPU kernel; the host only builds tables
// and runs the O(frames) sequential epilogues the Go code runs.
#include "../../include/sonar_gpu.h"

#include <hip/hip_runtime.h>

#include <mutex>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "ctx.h"
#include "fp_tables.h"
#include "host_dsp.h"
#include "kernels.h"
#include "speech_layout.h"

namespace sonar {
namespace detail {

int fail(sonar_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}

void* dbuf(sonar_ctx* c, const std::string& name, size_t bytes) {
  if (bytes == 0) bytes = 16;
  DevBuf& b = c->bufs[name];
  if (b.cap < bytes) {
    if (b.ptr) { hipStreamSynchronize(c->stream); hipFree(b.ptr); b.ptr = nullptr; b.cap = 0; }
    if (hipMalloc(&b.ptr, bytes) != hipSuccess) { b.ptr = nullptr; return nullptr; }
    b.cap = bytes;
  }
  return b.ptr;
}

int cached_table(sonar_ctx* c, const std::string& name, const char* what, const TableBuilder& build,
                 const unsigned char** table, int64_t* tag) {
  auto it = c->bufs.find(name);
  if (it == c->bufs.end() || !it->second.ptr || !it->second.ready) {
    auto drop = [&]() {                                      // an unfilled buffer is never served later
      auto e = c->bufs.find(name);
      if (e == c->bufs.end()) return;
      if (e->second.ptr) hipFree(e->second.ptr);
      c->bufs.erase(e);
    };
    drop();
    std::vector<unsigned char> image;
    int64_t t = 0;
    const int rc = build(image, t);
    if (rc != SONAR_OK) return rc;
    void* d = dbuf(c, name, image.size());
    if (!d) {
      drop();
      return fail(c, SONAR_ERR_NOMEM, std::string("device allocation failed (") + what + ")");
    }
    hipError_t e = image.empty() ? hipSuccess
                                 : hipMemcpyAsync(d, image.data(), image.size(), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // the image goes out of scope
    if (e != hipSuccess) {
      drop();
      return fail(c, SONAR_ERR_DEVICE, std::string(what) + " upload: " + hipGetErrorString(e));
    }
    it = c->bufs.find(name);
    it->second.tag = t;
    it->second.ready = true;                                 // the one place an entry becomes servable
  }
  *table = (const unsigned char*)it->second.ptr;
  if (tag) *tag = it->second.tag;
  return SONAR_OK;
}

void* hbuf(sonar_ctx* c, const std::string& name, size_t bytes) {
  if (bytes == 0) bytes = 16;
  DevBuf& b = c->hbufs[name];
  if (b.cap < bytes) {
    if (b.ptr) { hipStreamSynchronize(c->stream); hipHostFree(b.ptr); b.ptr = nullptr; b.cap = 0; }
    if (hipHostMalloc(&b.ptr, bytes, hipHostMallocDefault) != hipSuccess) { b.ptr = nullptr; return nullptr; }
    b.cap = bytes;
  }
  return b.ptr;
}

// brackets the dominant kernel of a call with a HIP event pair on its stream
hipEvent_t timed_begin(sonar_ctx* c, hipStream_t s) {
  if (!c->timing) return nullptr;
  if (c->ev_used == c->ev_pool.size()) {
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return nullptr;
    c->ev_pool.emplace_back(a, b);
  }
  auto& e = c->ev_pool[c->ev_used];
  hipEventRecord(e.first, s);
  return e.second;
}
void timed_end(sonar_ctx* c, hipStream_t s, hipEvent_t end) {
  if (!end) return;
  hipEventRecord(end, s);
  c->ev_used++;
}

// the cached buffers of one context (not its workers')
namespace {
// idle pinned blocks by capacity; at most kPinnedCache bytes stay cached
struct PinnedPool {
  std::mutex m;
  std::multimap<size_t, void*> idle;
  size_t cached = 0;
};
PinnedPool& pinned_pool() {
  static PinnedPool* p = new PinnedPool();   // never destroyed: blocks may outlive static teardown
  return *p;
}
constexpr size_t kPinnedCache = size_t(8) << 30;
void pinned_release(void* ptr, size_t cap) {
  PinnedPool& pp = pinned_pool();
  std::lock_guard<std::mutex> g(pp.m);
  if (pp.cached + cap > kPinnedCache) { hipHostFree(ptr); return; }
  pp.idle.emplace(cap, ptr);
  pp.cached += cap;
}
}  // namespace

std::shared_ptr<void> pinned_block(size_t bytes) {
  if (bytes == 0) bytes = 64;
  PinnedPool& pp = pinned_pool();
  void* ptr = nullptr;
  size_t cap = 0;
  {
    std::lock_guard<std::mutex> g(pp.m);
    auto it = pp.idle.lower_bound(bytes);
    if (it != pp.idle.end() && it->first <= 2 * bytes + (size_t(64) << 20)) {
      ptr = it->second; cap = it->first;
      pp.cached -= cap;
      pp.idle.erase(it);
    }
  }
  if (!ptr) {
    cap = (bytes + (size_t(2) << 20) - 1) & ~((size_t(2) << 20) - 1);
    if (hipHostMalloc(&ptr, cap, hipHostMallocPortable) != hipSuccess) return nullptr;
  }
  return std::shared_ptr<void>(ptr, [cap](void* q) { pinned_release(q, cap); });
}

void pinned_pool_trim() {
  PinnedPool& pp = pinned_pool();
  std::lock_guard<std::mutex> g(pp.m);
  for (auto& kv : pp.idle) hipHostFree(kv.second);
  pp.idle.clear();
  pp.cached = 0;
}

void trim_buffers(sonar_ctx* c) {
  hipSetDevice(c->device);
  hipStreamSynchronize(c->stream);
  for (auto& kv : c->bufs) if (kv.second.ptr) hipFree(kv.second.ptr);
  for (auto& kv : c->hbufs) if (kv.second.ptr) hipHostFree(kv.second.ptr);
  c->bufs.clear();
  c->hbufs.clear();
}
}  // namespace detail
}  // namespace sonar

namespace {
using namespace sonar::detail;
}  // namespace

// ============================================================ context ====
extern "C" {

int sonar_abi_version(void) { return SONAR_ABI_VERSION; }

int sonar_create(int device, sonar_ctx** out) {
  if (!out) return SONAR_ERR_INVALID;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return SONAR_ERR_DEVICE;
  if (device < 0 || device >= n) return SONAR_ERR_INVALID;
  auto* c = new sonar_ctx();
  c->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return SONAR_ERR_DEVICE;
  }
  c->stream = c->own;
  hipDeviceGetAttribute(&c->cus, hipDeviceAttributeMultiprocessorCount, device);   // 256 stays when it fails
  hipEventCreate(&c->ev0);
  hipEventCreate(&c->ev1);
  *out = c;
  return SONAR_OK;
}

void sonar_destroy(sonar_ctx* c) {
  if (!c) return;
  for (sonar_ctx* w : c->workers) sonar_destroy(w);
  c->workers.clear();
  hipSetDevice(c->device);
  hipStreamSynchronize(c->stream);
  sonar::detail::ingest_release(c);
  for (auto& kv : c->bufs) if (kv.second.ptr) hipFree(kv.second.ptr);
  for (auto& kv : c->hbufs) if (kv.second.ptr) hipHostFree(kv.second.ptr);
  // cached tables: one allocation per entry (null for a pair bank remembered as unsupported)
  for (auto& kv : c->fp_tables) hipFree(kv.second.base);
  for (auto& kv : c->pair_tables) hipFree(kv.second.base);
  for (auto& kv : c->chroma_tables) hipFree(kv.second.base);
  for (auto& e : c->ev_pool) { hipEventDestroy(e.first); hipEventDestroy(e.second); }
  if (c->ev0) hipEventDestroy(c->ev0);
  if (c->fpb_ev) hipEventDestroy(c->fpb_ev);
  if (c->ev1) hipEventDestroy(c->ev1);
  for (auto& e : c->dtw_ev)
    if (e) hipEventDestroy(e);
  for (auto& e : c->csim_ev)
    if (e) hipEventDestroy(e);
  for (auto& e : c->side_ev)
    if (e) hipEventDestroy(e);
  if (c->side) hipStreamDestroy(c->side);
  for (auto e : c->chunk_ev)
    if (e) hipEventDestroy(e);
  if (c->copy) hipStreamDestroy(c->copy);
  for (auto e : c->back_ev)
    if (e) hipEventDestroy(e);
  if (c->own) hipStreamDestroy(c->own);
  delete c;
}

const char* sonar_last_error(const sonar_ctx* c) { return c ? c->err.c_str() : "null context"; }

int sonar_set_stream(sonar_ctx* c, void* s) {
  if (!c) return SONAR_ERR_INVALID;
  c->stream = s ? reinterpret_cast<hipStream_t>(s) : c->own;
  return SONAR_OK;
}

int sonar_synchronize(sonar_ctx* c) {
  if (!c) return SONAR_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SONAR_OK;
}

int sonar_enable_kernel_timing(sonar_ctx* c, int on) {
  if (!c) return SONAR_ERR_INVALID;
  c->timing = on != 0;
  return SONAR_OK;
}

const char* sonar_last_fp_kernel(sonar_ctx* c) { return c ? c->last_fp_kernel : ""; }


int sonar_trim(sonar_ctx* c) {
  if (!c) return SONAR_ERR_INVALID;
  for (sonar_ctx* w : c->workers) sonar::detail::trim_buffers(w);
  sonar::detail::trim_buffers(c);
  sonar::detail::pinned_pool_trim();
  return SONAR_OK;
}

int sonar_dtw_counters(sonar_ctx* c, int64_t* out4, int32_t reset) {
  if (!c || !out4) return SONAR_ERR_INVALID;
  for (int k = 0; k < 4; ++k) {
    long long v = c->dtw_ctr[k];
    for (sonar_ctx* w : c->workers) v += w->dtw_ctr[k];
    out4[k] = v;
  }
  if (reset) {
    for (int k = 0; k < 4; ++k) c->dtw_ctr[k] = 0;
    for (sonar_ctx* w : c->workers)
      for (int k = 0; k < 4; ++k) w->dtw_ctr[k] = 0;
  }
  return SONAR_OK;
}

int sonar_dtw_last_timing(sonar_ctx* c, double* ms3) {
  if (!c || !ms3) return SONAR_ERR_INVALID;
  for (int k = 0; k < 3; ++k) ms3[k] = c->dtw_ms[k];
  return SONAR_OK;
}

int sonar_last_kernel_ms(sonar_ctx* c, double* ms) {
  if (!c || !ms) return SONAR_ERR_INVALID;
  if (c->ev_used > 0) {   // average over every timed launch since the last query
    HIP_TRY(c, hipEventSynchronize(c->ev_pool[c->ev_used - 1].second));
    double sum = 0.0;
    for (size_t i = 0; i < c->ev_used; ++i) {
      float f = 0.f;
      HIP_TRY(c, hipEventElapsedTime(&f, c->ev_pool[i].first, c->ev_pool[i].second));
      sum += f;
    }
    c->last_ms = sum / (double)c->ev_used;
    c->ev_used = 0;
  }
  *ms = c->last_ms;
  return SONAR_OK;
}

int64_t sonar_energy_frames(int64_t n, int32_t W, int32_t H) { return sonar::energy_frames(n, W, H); }

int64_t sonar_pitch_frames(int64_t n) { return sonar::pitch_frames(n); }

// ========================================================= YIN, chroma ====
int sonar_pitch_yin(sonar_ctx* c, const double* pcm, int64_t n, int32_t sr, double* pitch, double* conf, int32_t* tau,
                    int32_t device_ptrs) {
  if (!c) return SONAR_ERR_INVALID;
  const int64_t F = sonar_pitch_frames(n);
  if (F == 0) return SONAR_OK;
  if (!pcm || !pitch || !conf) return fail(c, SONAR_ERR_INVALID, "null buffer");
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const double* dp = pcm;
  double *dpi = pitch, *dco = conf;
  int32_t* dta = tau;
  if (!device_ptrs) {
    void* b = dbuf(c, "yin.pcm", n * 8);
    dpi = (double*)dbuf(c, "yin.p", F * 8);
    dco = (double*)dbuf(c, "yin.c", F * 8);
    dta = tau ? (int32_t*)dbuf(c, "yin.t", F * 4) : nullptr;
    if (!b || !dpi || !dco) return fail(c, SONAR_ERR_NOMEM, "device allocation failed");
    HIP_TRY(c, hipMemcpyAsync(b, pcm, n * 8, hipMemcpyHostToDevice, s));
    dp = (const double*)b;
  }
  if (sonar::launch_yin(dp, n, F, 512, sr, dpi, dco, dta, s) != 0) return fail(c, SONAR_ERR_DEVICE, "yin launch failed");
  if (!device_ptrs) {
    HIP_TRY(c, hipMemcpyAsync(pitch, dpi, F * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(conf, dco, F * 8, hipMemcpyDeviceToHost, s));
    if (tau) HIP_TRY(c, hipMemcpyAsync(tau, dta, F * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
  }
  return SONAR_OK;
}

int sonar_chroma_stft(sonar_ctx* c, const double* pcm, int64_t n, int64_t F, int32_t hop, int32_t sr, int32_t preprocess,
                      double* chroma, int32_t device_ptrs) {
  if (!c) return SONAR_ERR_INVALID;
  if (!pcm || n <= 0 || F <= 0) return fail(c, SONAR_ERR_INVALID, "invalid input data");
  if (hop <= 0) return fail(c, SONAR_ERR_INVALID, "hop size must be positive");
  const int fs = (int)(n / F);                                    // music.go:331
  if (fs <= 0) return fail(c, SONAR_ERR_INVALID, "window size must be positive");
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const double* dp = pcm;
  double* dout = chroma;
  if (!device_ptrs) {
    void* b = dbuf(c, "chroma.pcm", n * 8);
    dout = (double*)dbuf(c, "chroma.out", F * 12 * 8);
    if (!b || !dout) return fail(c, SONAR_ERR_NOMEM, "device allocation failed");
    HIP_TRY(c, hipMemcpyAsync(b, pcm, n * 8, hipMemcpyHostToDevice, s));
    dp = (const double*)b;
  }
  const double* y = dp;
  if (preprocess) {
    double* yb = (double*)dbuf(c, "chroma.y", n * 8);
    if (!yb) return fail(c, SONAR_ERR_NOMEM, "device allocation failed");
    double* dcs = (double*)dbuf(c, "chroma.dcscratch", sonar::dc_preemph_scratch_bytes(n));
    if (!dcs) return fail(c, SONAR_ERR_NOMEM, "device allocation failed");
    if (sonar::launch_dc_preemph(dp, n, 0.995, 0.95, yb, dcs, s) != 0) return fail(c, SONAR_ERR_DEVICE, "dc launch failed");
    y = yb;
  }
  const sonar_ctx::ChromaT* ct = sonar::detail::chroma_tables_for(c, fs, sr);
  if (!ct) return fail(c, SONAR_ERR_NOMEM, "device allocation failed");
  const int* cls = (const int*)ct->cls;
  if (sonar::launch_chroma(y, n, F, hop, fs, (const double*)ct->win, (const double*)ct->trig,
                           (const int*)ct->map, cls, dout, s) != 0)
    return fail(c, SONAR_ERR_UNSUPPORTED, "chroma launch failed (frame size too large for LDS?)");
  if (!device_ptrs) {
    HIP_TRY(c, hipMemcpyAsync(chroma, dout, F * 12 * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
  }
  return SONAR_OK;
}

}  // extern "C"

namespace sonar {
namespace detail {
// the chroma tables of frame size fs at sample rate sr (ChromaSTFT, chroma_stft.go:45-138), built
// once per context: Hann window, the bin -> class map, the FFT twiddles, per-class bin lists
const sonar_ctx::ChromaT* chroma_tables_for(sonar_ctx* c, int fs, int sr) {
  namespace host = sonar::host;
  const std::string key = std::to_string(fs) + "|" + std::to_string(sr);
  auto it = c->chroma_tables.find(key);
  if (it == c->chroma_tables.end()) {
    std::vector<double> win;
    host::make_window(SONAR_WIN_HANN, fs, true, true, host::kStftBeta, host::kStftAlpha, win);
    std::vector<int> map = host::chroma_map(fs, sr);
    // per chroma class, its bins in ascending order (the fold order of music.go:366-372)
    std::vector<int> cls(13 + map.size());
    int e = 0;
    for (int b = 0; b < 12; ++b) {
      cls[b] = e;
      for (size_t k = 0; k < map.size(); ++k)
        if (map[k] == b) cls[13 + e++] = (int)k;
    }
    cls[12] = e;
    host::Image im;
    const size_t o_win = host::put_section(im, win), o_trig = host::put_section(im, host::trig_table(fs)),
                 o_map = host::put_section(im, map), o_cls = host::put_section(im, cls);
    unsigned char* base = (unsigned char*)upload_image(im);
    if (!base) return nullptr;
    const sonar_ctx::ChromaT t{base, base + o_win, base + o_trig, base + o_map, base + o_cls};
    it = c->chroma_tables.emplace(key, t).first;
  }
  return &it->second;
}
}  // namespace detail
}  // namespace sonar

extern "C" {

// ========================================================= formants ====
namespace {
int formant_geometry(int sr, int* W, int* p) {
  *W = sr >= 16000 ? 2048 : 1024;                    // NewFormantAnalyzer (format.go:48-69)
  *p = 12 + sr / 1000;
  return 0;
}
int run_formants(sonar_ctx* c, const double* pcm, int64_t n, int sr, int64_t frames, int64_t hop, bool ok_len,
                 sonar_formant_frame* out, double* coeffs, double* refl, int device_ptrs) {
  int W, p;
  formant_geometry(sr, &W, &p);
  if (p > 64) return fail(c, SONAR_ERR_UNSUPPORTED, "LPC order above 64 (sample rate > 52 kHz)");
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  std::vector<double> ham(W);
  for (int i = 0; i < W; ++i) ham[i] = 0.54 - 0.46 * std::cos(2.0 * M_PI * (double)i / (double)(W - 1));
  double* dham = (double*)dbuf(c, "lpc.ham", W * 8);
  if (!dham) return fail(c, SONAR_ERR_NOMEM, "device allocation failed");
  HIP_TRY(c, hipMemcpyAsync(dham, ham.data(), W * 8, hipMemcpyHostToDevice, s));
  const double* dp = pcm;
  sonar_formant_frame* dout = out;
  double *dco = coeffs, *dre = refl;
  if (!device_ptrs) {
    double* b = (double*)dbuf(c, "lpc.pcm", std::max<int64_t>(n, 1) * 8);
    dout = (sonar_formant_frame*)dbuf(c, "lpc.out", std::max<int64_t>(frames, 1) * sizeof(sonar_formant_frame));
    dco = coeffs ? (double*)dbuf(c, "lpc.coeffs", std::max<int64_t>(frames, 1) * (p + 1) * 8) : nullptr;
    dre = refl ? (double*)dbuf(c, "lpc.refl", std::max<int64_t>(frames, 1) * p * 8) : nullptr;
    if (!b || !dout || (coeffs && !dco) || (refl && !dre)) return fail(c, SONAR_ERR_NOMEM, "device allocation failed");
    HIP_TRY(c, hipMemcpyAsync(b, pcm, n * 8, hipMemcpyHostToDevice, s));
    dp = b;
  }
  hipEvent_t tend = timed_begin(c, s);
  if (sonar::launch_formants(dp, frames, hop, W, p, sr, ok_len ? 1 : 0, dham, dout, dco, dre, s) != 0)
    return fail(c, SONAR_ERR_DEVICE, "formant launch failed");
  timed_end(c, s, tend);
  if (!device_ptrs) {
    HIP_TRY(c, hipMemcpyAsync(out, dout, frames * sizeof(sonar_formant_frame), hipMemcpyDeviceToHost, s));
    if (coeffs) HIP_TRY(c, hipMemcpyAsync(coeffs, dco, frames * (p + 1) * 8, hipMemcpyDeviceToHost, s));
    if (refl) HIP_TRY(c, hipMemcpyAsync(refl, dre, frames * p * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
  }
  return SONAR_OK;
}
}  // namespace

extern "C" {

int64_t sonar_formant_frame_count(int64_t n, int32_t sample_rate, int32_t frame_size, int32_t hop_size) {
  int W, p;
  formant_geometry(sample_rate, &W, &p);
  if (frame_size <= 0) frame_size = W;
  if (hop_size <= 0) hop_size = frame_size / 2;
  if (hop_size <= 0) return 0;
  return n > frame_size ? (n - frame_size - 1) / hop_size + 1 : 0;   // for i := 0; i < n-frameSize; i += hop
}

int sonar_formants(sonar_ctx* c, const double* pcm, int64_t n, int32_t sample_rate, int32_t frame_size,
                   int32_t hop_size, sonar_formant_frame* out, double* lpc_coeffs, double* reflection,
                   int32_t device_ptrs) {
  if (!c) return SONAR_ERR_INVALID;
  if (sample_rate <= 0) return fail(c, SONAR_ERR_INVALID, "sample rate must be positive");
  int W, p;
  formant_geometry(sample_rate, &W, &p);
  if (frame_size <= 0) frame_size = W;
  if (hop_size <= 0) hop_size = frame_size / 2;
  if (hop_size <= 0) return fail(c, SONAR_ERR_INVALID, "hop size must be positive");
  const int64_t frames = sonar_formant_frame_count(n, sample_rate, frame_size, hop_size);
  if (frames == 0) return SONAR_OK;
  if (!pcm || !out) return fail(c, SONAR_ERR_INVALID, "null buffer");
  return run_formants(c, pcm, n, sample_rate, frames, hop_size, frame_size >= W, out, lpc_coeffs, reflection,
                      device_ptrs);
}

}  // extern "C"

int sonar_analyze_formants_host(sonar_ctx* c, const double* pcm, int64_t n, int sample_rate, sonar_formant_frame* out) {
  int W, p;
  formant_geometry(sample_rate, &W, &p);
  return run_formants(c, pcm, n, sample_rate, 1, 0, n >= W, out, nullptr, nullptr, 0);
}

// ====================================================== result object ====
int sonar_result_get(const sonar_result* r, const char* name, const double** data, int64_t* rows, int64_t* cols) {
  if (!r || !name) return SONAR_ERR_INVALID;
  for (const auto& a : r->arrays)
    if (a.name == name) {
      if (data) *data = a.data();
      if (rows) *rows = a.rows;
      if (cols) *cols = a.cols;
      return SONAR_OK;
    }
  return SONAR_ERR_INVALID;
}
int sonar_result_count(const sonar_result* r) { return r ? (int)r->arrays.size() : 0; }
const char* sonar_result_name(const sonar_result* r, int i) {
  return (r && i >= 0 && i < (int)r->arrays.size()) ? r->arrays[i].name.c_str() : nullptr;
}
void sonar_result_free(sonar_result* r) { delete r; }

}  // extern "C"
