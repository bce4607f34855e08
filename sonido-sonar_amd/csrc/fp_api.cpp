// fp_api.cpp -- the fingerprint entries of include/sonar_gpu.h: sonar_fingerprint, its batch form and
// fingerprint_impl, which every spectral entry runs through (stream, ingest, speech extractor, HPCP,
// HPS, onsets, chords).  A call is: validate and plan; resolve the outputs (the caller's device arrays
// or staging); one of three transform paths -- run_dft (any W <= 8192, float64 DFT), run_pair
// (mfcc_pair_kernel, MFCC only at W = 1024) or run_wave (fp_wave_kernel, the other fused window
// sizes); ZCR and energy; copy back.  The tables of each path are built on the host as one image
// (fp_tables.h), uploaded once per configuration and context, and survive sonar_trim; the LDS carves
// of the two fused kernels are fp_layout.h's.
#include "../../include/sonar_gpu.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"
#include "fp_layout.h"
#include "fp_tables.h"
#include "kernels.h"
#include "staging.h"

namespace {
using namespace sonar::detail;
namespace host = sonar::host;

int64_t go_frames(int64_t n, int W, int H) { return (n - W) / H + 1; }

// ------------------------------------------------------------------ tables ----
template <typename T>
T* view(void* base, size_t off) { return reinterpret_cast<T*>(static_cast<unsigned char*>(base) + off); }

// the part of a table key that names the window and the MFCC bank
std::string bank_key(const sonar_fp_cfg* cfg) {
  char key[384];
  std::snprintf(key, sizeof(key), "%d|%d|%d|%d|%d|%.17g|%.17g|%d|%.17g", cfg->window_type, cfg->sample_rate,
                cfg->n_mfcc, cfg->n_filters, cfg->filterbank, cfg->low_freq, cfg->high_freq, cfg->use_lifter,
                cfg->lifter);
  return key;
}

// the cached FpTables under `key`; built by build(image, descriptor) and uploaded when not there.  A
// failed build or upload leaves no entry and no allocation behind.
template <typename Build>
int fp_tables_for(sonar_ctx* c, const std::string& key, Build build, const FpTables** out) {
  auto it = c->fp_tables.find(key);
  if (it == c->fp_tables.end()) {
    host::Image im;
    host::FpTableDesc d;
    const int rc = build(im, d);
    if (rc == host::TABLES_BAD_WINDOW)
      return fail(c, SONAR_ERR_INVALID, "failed to generate window: unsupported window type");
    if (rc != host::TABLES_OK)
      return fail(c, SONAR_ERR_INVALID, "failed to initialize MFCC: failed to create mel filter bank");
    FpTables t;
    t.base = upload_image(im);
    if (!t.base) return fail(c, SONAR_ERR_NOMEM, "table upload failed");
    t.window = view<void>(t.base, d.window);
    t.trig = d.trig ? view<void>(t.base, d.trig) : nullptr;   // the DFT path's (the window comes first)
    if (d.has_mfcc) {
      t.mel_lo = view<int>(t.base, d.mel_lo); t.mel_hi = view<int>(t.base, d.mel_hi);
      t.mel_woff = view<int>(t.base, d.mel_woff);
      t.grp_off = view<int>(t.base, d.grp_off); t.grp_mels = view<int>(t.base, d.grp_mels);
      t.mel_w = view<void>(t.base, d.mel_w); t.dct = view<void>(t.base, d.dct); t.lift = view<void>(t.base, d.lift);
      t.n_mels = d.n_mels; t.n_mfcc = d.n_mfcc; t.nnz = d.nnz;
    }
    it = c->fp_tables.emplace(key, t).first;
  }
  *out = &it->second;
  return SONAR_OK;
}

// the headline kernel's tables for a configuration, built once per context; a bank the builder
// refuses (or a failed upload) is remembered as ok = false
const PairTables& pair_tables_for(sonar_ctx* c, const sonar_fp_cfg* cfg) {
  char key[512];
  std::snprintf(key, sizeof(key), "%d|%d|%d|%d|%.17g|%.17g|%d|%.17g|%d|%d", cfg->window_type, cfg->sample_rate,
                cfg->n_mfcc, cfg->n_filters, cfg->low_freq, cfg->high_freq, cfg->use_lifter, cfg->lifter,
                cfg->filterbank, cfg->mfcc_input_power);
  auto it = c->pair_tables.find(key);
  if (it == c->pair_tables.end()) {
    PairTables t;
    host::Image im;
    host::PairTableDesc d;
    if (host::build_pair_tables(cfg, im, d) && (t.base = upload_image(im)) != nullptr) {
      for (int e = 0; e < 2; e++) {
        t.window[e] = view<void>(t.base, d.window[e]); t.tw1[e] = view<void>(t.base, d.tw1[e]);
        t.tw2[e] = view<void>(t.base, d.tw2[e]); t.chunk_w[e] = view<void>(t.base, d.chunk_w[e]);
        t.dct[e] = view<void>(t.base, d.dct[e]); t.chunk_ks[e] = view<int>(t.base, d.chunk_ks[e]);
        t.mel_src[e] = view<uint16_t>(t.base, d.mel_src[e]);
        t.JS[e] = d.JS[e];
      }
      t.zeros = view<void>(t.base, d.zeros);
      t.J = d.J; t.NMP = d.NMP; t.n_mels = d.n_mels; t.n_mfcc = d.n_mfcc; t.max_src = d.max_src;
      t.ok = true;
    }
    it = c->pair_tables.emplace(key, t).first;
  }
  return it->second;
}

// ------------------------------------------------------------ plan, checks ----
// The transform kernel of a validated sonar_fingerprint call over F frames (sonar_fp_kernel_plan):
// mfcc_pair_kernel for the float32 MFCC-only configuration at W = 1024 while its 32-bit frame
// indices hold (t = 2 pair + 1 <= F), the general fused kernel for the other fused window sizes,
// the float64 DFT path for any other W.
int fp_plan(const sonar_fp_cfg* cfg, int64_t F) {
  const uint32_t flags = cfg->flags;
  if (!(flags & (SONAR_FP_MFCC | SONAR_FP_MAGNITUDE | SONAR_FP_SPECTRAL | SONAR_FP_COMPLEX | SONAR_FP_PHASE)))
    return SONAR_PLAN_NONE;
  if (!sonar::fingerprint_supported(cfg->window_size)) return SONAR_PLAN_DFT;
  // the pair kernel computes in float32 with float32 PCM and output, or in float64 with float64
  // output (PCM of either type)
  const bool types = cfg->precision == SONAR_F64 ? cfg->out_dtype == SONAR_F64
                                                  : cfg->pcm_dtype != SONAR_F64 && cfg->out_dtype != SONAR_F64;
  const bool pair = types && cfg->window_size == 1024 && (flags & SONAR_FP_MFCC) &&
                    !(flags & (SONAR_FP_MAGNITUDE | SONAR_FP_SPECTRAL | SONAR_FP_COMPLEX | SONAR_FP_PHASE |
                               SONAR_FP_GENERIC | 0x80000000u)) &&
                    F <= SONAR_PAIR_MAX_FRAMES;
  return pair ? SONAR_PLAN_PAIR : SONAR_PLAN_WAVE;
}

// spec_rows_kernel over F float64 |X| rows of K bins into the descriptor outputs (nullable each)
int launch_spec(const double* mag, int64_t F, int K, int sample_rate, bool o64, void* const* d_spec, hipStream_t s,
                int64_t f_lo, int64_t f_hi) {
  sonar::SpecParams sp{};
  sp.mag = mag; sp.F = F; sp.K = K; sp.sample_rate = sample_rate; sp.out_f64 = o64 ? 1 : 0;
  sp.f_first = f_lo; sp.f_last = f_hi;
  for (int d = 0; d < 9; d++) sp.out_spec[d] = d_spec[d];
  // ~24 resident waves per CU over 256 CUs, a contiguous frame run each
  const int64_t target = 256 * 24;
  sp.frames_per_wave = std::max<int64_t>(1, (f_hi - f_lo + target - 1) / target);
  return sonar::launch_spec_rows(sp, s);
}

// ComputeSTFTWithWindow's argument checks (spectral.go:386-412) and the GPU path's own limits, in the
// order sonar_fingerprint applies them: SONAR_OK and the frame count, or the error code + message
int fp_validate(const sonar_fp_cfg* cfg, int64_t n, bool have_pcm, int64_t* F, std::string* msg) {
  if (n <= 0 || !have_pcm) { *msg = "empty signal"; return SONAR_ERR_EMPTY; }
  const int W = cfg->window_size, H = cfg->hop_size;
  if (W <= 0) { *msg = "window size must be positive"; return SONAR_ERR_INVALID; }
  if (H <= 0) { *msg = "hop size must be positive"; return SONAR_ERR_INVALID; }
  *F = go_frames(n, W, H);
  if (*F <= 0) { *msg = "signal too short for given window size and hop size"; return SONAR_ERR_TOO_SHORT; }
  if (fp_plan(cfg, *F) == SONAR_PLAN_DFT) {
    // other window lengths (go-dsp takes any W, spectral.go:131) run the generic DFT path (its
    // |X| scratch feeds spec_rows_kernel for the spectral descriptors)
    if (W > 8192) {
      *msg = "window size " + std::to_string(W) + " above 8192 (generic STFT path)";
      return SONAR_ERR_UNSUPPORTED;
    }
  }
  return SONAR_OK;
}

// ------------------------------------------------------------ one call ----
// what the steps of one fingerprint_impl call share
struct FpCall {
  sonar_ctx* c;
  const sonar_fp_cfg* cfg;
  hipStream_t s;
  const void* dpcm;         // the PCM on the device
  int64_t n, F, f_lo, f_hi;
  int W, H, K;
  uint32_t flags;
  bool f64, pcm64, o64, raw_window;
  void *mfcc, *mag, *cplx, *phase, *spec[9];   // resolved outputs (device), null when not asked for
};

// an output of `bytes`: the caller's device array, or staging that is copied back at the end
void* staged(Staging& st, void* user, const char* name, size_t bytes) {
  return st.out<unsigned char>(name, static_cast<unsigned char*>(user), bytes);
}

// the transform's outputs; a flagged output that is null is reported in the order mfcc, magnitude,
// complex, phase (the descriptors are optional each)
int resolve_outputs(FpCall& k, Staging& st, const sonar_fp_out* out) {
  sonar_ctx* c = k.c;
  const uint32_t flags = k.flags;
  const size_t esz = k.o64 ? 8 : 4, F = (size_t)k.F, K = (size_t)k.K;
  const size_t n_mfcc = k.cfg->n_mfcc > 0 ? k.cfg->n_mfcc : 13;
  k.mfcc = (flags & SONAR_FP_MFCC) ? staged(st, out->mfcc, "mfcc", F * n_mfcc * esz) : nullptr;
  k.mag = (flags & SONAR_FP_MAGNITUDE) ? staged(st, out->magnitude, "mag", F * K * esz) : nullptr;
  if ((flags & SONAR_FP_MFCC) && !k.mfcc) return fail(c, SONAR_ERR_INVALID, "out->mfcc is null or allocation failed");
  if ((flags & SONAR_FP_MAGNITUDE) && !k.mag) return fail(c, SONAR_ERR_INVALID, "out->magnitude is null");
  k.cplx = (flags & SONAR_FP_COMPLEX) ? staged(st, out->complex, "cplx", F * K * 2 * esz) : nullptr;
  k.phase = (flags & SONAR_FP_PHASE) ? staged(st, out->phase, "phase", F * K * esz) : nullptr;
  if ((flags & SONAR_FP_COMPLEX) && !k.cplx) return fail(c, SONAR_ERR_INVALID, "out->complex is null");
  if ((flags & SONAR_FP_PHASE) && !k.phase) return fail(c, SONAR_ERR_INVALID, "out->phase is null");
  for (int d = 0; d < 9; d++) k.spec[d] = nullptr;
  if (flags & SONAR_FP_SPECTRAL) {
    void* user[9] = {out->centroid, out->rolloff, out->bandwidth, out->flatness, out->crest, out->slope,
                     out->flux, out->low_ratio, out->high_ratio};
    static const char* nm[9] = {"centroid", "rolloff", "bandwidth", "flatness", "crest", "slope", "flux", "low", "high"};
    for (int d = 0; d < 9; d++) {
      const size_t cnt = (d == 6) ? (size_t)std::max<int64_t>(k.F - 1, 0) : F;
      if (user[d] && cnt > 0) k.spec[d] = staged(st, user[d], nm[d], cnt * esz);
    }
  }
  return SONAR_OK;
}

// any W <= 8192: float64 DFT per frame into an |X| scratch, MFCC and descriptors from its rows
int run_dft(FpCall& k) {
  sonar_ctx* c = k.c;
  const sonar_fp_cfg* cfg = k.cfg;
  const bool want_mfcc = (k.flags & SONAR_FP_MFCC) != 0;
  // the MFCC tables are part of the entry only when asked for (their own key): a call without
  // MFCC succeeds with a bank that cannot be built
  const std::string key = "gen|" + std::to_string(k.W) + "|" + bank_key(cfg) + (k.raw_window ? "|raw" : "") +
                          (want_mfcc ? "|mfcc" : "");
  const FpTables* t = nullptr;
  const int rc = fp_tables_for(c, key, [&](host::Image& im, host::FpTableDesc& d) {
    return host::build_dft_tables(cfg, k.raw_window, want_mfcc, im, d);
  }, &t);
  if (rc != SONAR_OK) return rc;
  double* mag = (double*)dbuf(c, "fp.gen.mag", (size_t)k.F * k.K * 8);
  if (!mag) return fail(c, SONAR_ERR_NOMEM, "device allocation failed (spectrogram)");
  hipEvent_t tend = timed_begin(c, k.s);
  if (sonar::launch_stft_dft(k.dpcm, k.pcm64, k.n, k.F, k.W, k.H, (const double*)t->window, (const double*)t->trig,
                             mag, k.mag, k.cplx, k.phase, k.o64, k.s) != 0)
    return fail(c, SONAR_ERR_DEVICE, "stft launch failed");
  if (want_mfcc &&
      sonar::launch_mfcc_rows(mag, k.F, k.K, t->mel_lo, t->mel_hi, t->mel_woff, (const double*)t->mel_w, t->n_mels,
                              (const double*)t->dct, (const double*)t->lift, t->n_mfcc, cfg->mfcc_input_power, k.mfcc,
                              k.o64, k.s) != 0)
    return fail(c, SONAR_ERR_DEVICE, "mfcc launch failed");
  if ((k.flags & SONAR_FP_SPECTRAL) && launch_spec(mag, k.F, k.K, cfg->sample_rate, k.o64, k.spec, k.s, 0, k.F) != 0)
    return fail(c, SONAR_ERR_DEVICE, "spectral descriptor launch failed");
  timed_end(c, k.s, tend);
  c->last_fp_kernel = "stft_dft_kernel";
  return SONAR_OK;
}

#ifdef HL_STAMP
// diagnostics builds: every wave's {start, end, pairs} of a single-signal launch, appended to the file
// SONAR_HL_STAMP names.  stamp_begin returns the launch's wave count.
int64_t stamp_begin(sonar_ctx* c, int64_t NP, sonar::MfccPairParams& q) {
  if (!std::getenv("SONAR_HL_STAMP") || q.nseg > 0) return 0;
  const int64_t nw = (NP + q.pairs_per_block - 1) / q.pairs_per_block * q.waves_per_block;
  q.stamp = (uint64_t*)dbuf(c, "hl.stamp", (size_t)nw * 24);
  return nw;
}
int stamp_end(sonar_ctx* c, int64_t nw, const sonar::MfccPairParams& q, hipStream_t s) {
  if (!q.stamp) return SONAR_OK;
  std::vector<uint64_t> h((size_t)nw * 3);
  HIP_TRY(c, hipMemcpyAsync(h.data(), q.stamp, h.size() * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (FILE* f = std::fopen(std::getenv("SONAR_HL_STAMP"), "ab")) { std::fwrite(h.data(), 8, h.size(), f); std::fclose(f); }
  return SONAR_OK;
}
#else
inline int64_t stamp_begin(sonar_ctx*, int64_t, sonar::MfccPairParams&) { return 0; }
inline int stamp_end(sonar_ctx*, int64_t, const sonar::MfccPairParams&, hipStream_t) { return SONAR_OK; }
#endif

// One mfcc_pair_kernel launch over NP frame pairs.  q holds the call's own fields (PCM or segment
// table, n, F, H, out); the tables, the LDS carve and the work split are filled in here.  One block per
// CU (12 waves float32, 8 float64) over a contiguous range of pairs; a bank whose tables leave room for
// fewer waves runs more blocks.
int launch_pair(sonar_ctx* c, const PairTables& t, const sonar_fp_cfg* cfg, int64_t NP, bool f64, hipStream_t s,
                sonar::MfccPairParams& q) {
  const int e = f64 ? 1 : 0;
  q.f64 = e;
  q.window = t.window[e]; q.tw1 = t.tw1[e]; q.tw2 = t.tw2[e]; q.chunk_w = t.chunk_w[e]; q.dct = t.dct[e];
  q.chunk_ks = t.chunk_ks[e]; q.mel_src = t.mel_src[e]; q.zeros = t.zeros;
  q.J = t.J; q.JS = t.JS[e]; q.max_src = t.max_src; q.NMP = t.NMP; q.n_mels = t.n_mels; q.n_mfcc = t.n_mfcc;
  q.pow2 = cfg->mfcc_input_power != 0;
  const sonar::PairLdsLayout l = sonar::pair_lds_layout(t.J, t.JS[e], t.NMP, f64, sonar::mfcc_pair_wave_bytes(e),
                                                        sonar::mfcc_pair_waves_per_block(e));
  q.lds_src = l.lds_src; q.lds_dct = l.lds_dct; q.lds_ctr = l.lds_ctr; q.lds_tw2 = l.lds_tw2; q.lds_wave0 = l.lds_wave0;
  q.waves_per_block = l.waves_per_block; q.lds_bytes = l.lds_bytes;
  const int64_t blocks = (int64_t)c->cus * std::max(1, sonar::mfcc_pair_waves_per_cu(e) / q.waves_per_block);
  q.pairs_per_block = std::max<int64_t>(1, (NP + blocks - 1) / blocks);
  const int64_t stamped = stamp_begin(c, NP, q);
  hipEvent_t tend = timed_begin(c, s);
  const int lrc = sonar::launch_mfcc_pair(q, s);
  if (lrc == -4) return fail(c, SONAR_ERR_UNSUPPORTED, "too many frames for one mfcc_pair_kernel launch");
  if (lrc != 0)
    return fail(c, SONAR_ERR_DEVICE, std::string("mfcc kernel launch failed: ") + hipGetErrorString(hipGetLastError()));
  timed_end(c, s, tend);
  c->last_fp_kernel = "mfcc_pair_kernel";
  return stamp_end(c, stamped, q, s);
}

// headline path: MFCC only at W = 1024 (mfcc_pair.hip).  *done = false when the bank does not fit the
// kernel: the call falls to run_wave.
int run_pair(FpCall& k, bool* done) {
  const PairTables& t = pair_tables_for(k.c, k.cfg);
  *done = t.ok;
  if (!t.ok) return SONAR_OK;
  sonar::MfccPairParams q{};
  q.pcm = k.dpcm; q.pcm_f64 = k.pcm64 ? 1 : 0; q.n = k.n; q.F = k.F; q.H = k.H;
  q.out = k.mfcc;
  return launch_pair(k.c, t, k.cfg, (k.F + 1) / 2, k.f64, k.s, q);
}

// fp_wave_kernel (fp_kernel.hip) over frames [f_lo, f_hi).  Spectral descriptors: the transform writes
// float64 |X| rows to HBM (the caller's Magnitude output when it is float64, else a scratch of F x K
// doubles) and spec_rows_kernel reduces them.  The fused SPEC epilogue (one wave per SIMD) remains
// only for a float32 Magnitude output beside the descriptors, or when the scratch cannot be allocated.
int run_wave(FpCall& k) {
  sonar_ctx* c = k.c;
  const sonar_fp_cfg* cfg = k.cfg;
  const bool f64 = k.f64, spec_req = (k.flags & SONAR_FP_SPECTRAL) != 0;
  double* spec_mag = nullptr;
  if (spec_req && f64 && !(k.mag && !k.o64))
    spec_mag = k.mag ? (double*)k.mag : (double*)dbuf(c, "fp.specmag", (size_t)k.F * k.K * 8);
  const bool spec = spec_req && !spec_mag;            // the fused SPEC epilogue
  const int NB = sonar::fp_batch_frames(k.W, f64 ? 1 : 0, spec ? 1 : 0);
  const int PRE = sonar::fp_pre_rows(k.W, spec);
  sonar::FpParams p{};
  p.pcm = k.dpcm; p.n = k.n; p.pcm_f64 = k.pcm64; p.F = k.F; p.W = k.W; p.H = k.H;
  p.f_first = k.f_lo; p.f_last = k.f_hi;
  p.flags = spec ? k.flags : (k.flags & ~(uint32_t)SONAR_FP_SPECTRAL);
  p.input_power = cfg->mfcc_input_power;
  p.n_groups = 64 / NB;
  p.sample_rate = cfg->sample_rate;
  p.out_f64 = k.o64;
  p.out_mfcc = k.mfcc;
  p.out_mag = spec_mag ? (void*)spec_mag : k.mag;
  p.mag_f64 = spec_mag ? 1 : (int)k.o64;
  p.out_cplx = k.cplx;
  p.out_phase = k.phase;
  for (int d = 0; d < 9; d++) p.out_spec[d] = k.spec[d];
  // tables, cached per configuration
  const std::string key = std::to_string(k.W) + "|" + bank_key(cfg) + "|" + std::to_string((int)f64) + "|" +
                          std::to_string(NB) + (k.raw_window ? "|raw" : "");
  const FpTables* t = nullptr;
  const int trc = fp_tables_for(c, key, [&](host::Image& im, host::FpTableDesc& d) {
    return host::build_wave_tables(cfg, k.raw_window, f64, 64 / NB, im, d);
  }, &t);
  if (trc != SONAR_OK) return trc;
  p.window = t->window;
  p.n_mels = t->n_mels; p.n_mfcc = t->n_mfcc; p.nnz = t->nnz;
  p.mel_lo = t->mel_lo; p.mel_hi = t->mel_hi; p.mel_woff = t->mel_woff; p.mel_w = t->mel_w;
  p.grp_off = t->grp_off; p.grp_mels = t->grp_mels; p.dct = t->dct; p.lift = t->lift;
  // LDS carve: twiddle tables (shared), then one region per wave
  const sonar::FpLdsLayout l = sonar::fp_lds_layout(k.W, f64, NB, PRE, t->n_mels, t->n_mfcc, t->nnz, p.n_groups);
  p.lds_tab_t1 = l.lds_tab_t1; p.lds_tab_t2 = l.lds_tab_t2; p.lds_tab_t3 = l.lds_tab_t3; p.lds_tab_mel = l.lds_tab_mel;
  p.lds_tab_w = l.lds_tab_w; p.lds_tab_dct = l.lds_tab_dct; p.lds_wave0 = l.lds_wave0;
  p.lds_logmel = l.lds_logmel; p.lds_stage = l.lds_stage; p.lds_wave_stride = l.lds_wave_stride;
  p.waves_per_block = l.waves_per_block; p.lds_bytes = l.lds_bytes;
  if (p.lds_bytes > sonar::kLdsLimit) return fail(c, SONAR_ERR_UNSUPPORTED, "LDS budget exceeded");
  // frames per wave: about 12 resident waves per CU, equal shares, multiple of NB
  const int64_t target_waves = (int64_t)c->cus * 12;
  int64_t fpw = (k.f_hi - k.f_lo + target_waves - 1) / target_waves;
  p.frames_per_wave = std::max<int64_t>(NB, (fpw + NB - 1) / NB * NB);
  hipEvent_t tend = timed_begin(c, k.s);
  const int rc = sonar::launch_fingerprint(p, f64, k.s);
  c->last_fp_kernel = "fp_wave_kernel";
  if (rc != 0)
    return fail(c, SONAR_ERR_DEVICE, std::string("fingerprint kernel launch failed: ") + hipGetErrorString(hipGetLastError()));
  if (spec_mag && launch_spec(spec_mag, k.F, k.K, cfg->sample_rate, k.o64, k.spec, k.s, k.f_lo, k.f_hi) != 0)
    return fail(c, SONAR_ERR_DEVICE, "spectral descriptor launch failed");
  timed_end(c, k.s, tend);
  return SONAR_OK;
}

// the two time-domain outputs, resolved here: a null one is reported after the transform has run
int run_zcr_energy(FpCall& k, Staging& st, const sonar_fp_out* out) {
  sonar_ctx* c = k.c;
  const sonar_fp_cfg* cfg = k.cfg;
  const size_t esz = k.o64 ? 8 : 4;
  if (k.flags & SONAR_FP_ZCR) {
    void* d = staged(st, out->zcr, "zcr", (size_t)k.F * esz);
    if (!d) return fail(c, SONAR_ERR_INVALID, "out->zcr is null");
    if (sonar::launch_zcr(k.dpcm, k.pcm64, k.n, k.F, k.W, k.H, cfg->preemph_alpha, cfg->sample_rate, d, k.o64, k.s,
                          k.f_lo, k.f_hi) != 0)
      return fail(c, SONAR_ERR_DEVICE, "zcr launch failed");
  }
  if (k.flags & SONAR_FP_ENERGY) {
    const int64_t Fe = sonar_energy_frames(k.n, cfg->energy_window, cfg->energy_hop);
    if (Fe > 0) {
      void* d = staged(st, out->energy, "energy", (size_t)Fe * esz);
      if (!d) return fail(c, SONAR_ERR_INVALID, "out->energy is null");
      if (sonar::launch_energy(k.dpcm, k.pcm64, k.n, Fe, cfg->energy_window, cfg->energy_hop, cfg->preemph_alpha, d,
                               k.o64, k.s) != 0)
        return fail(c, SONAR_ERR_DEVICE, "energy launch failed");
    }
  }
  return SONAR_OK;
}
}  // namespace

namespace sonar {
namespace detail {
void* upload_image(const std::vector<unsigned char>& image) {
  void* p = nullptr;
  if (hipMalloc(&p, std::max<size_t>(16, image.size())) != hipSuccess) return nullptr;
  if (!image.empty() && hipMemcpy(p, image.data(), image.size(), hipMemcpyHostToDevice) != hipSuccess) {
    hipFree(p);
    return nullptr;
  }
  return p;
}

int fp_check(const sonar_fp_cfg* cfg, int64_t n, bool have_pcm, int64_t* F, std::string* msg) {
  return fp_validate(cfg, n, have_pcm, F, msg);
}

// pcm_dev: pcm is already device memory even though the outputs are host buffers
// (cfg->device_ptrs == 0) -- the sonar_fingerprint_f64le path (ingest_api.cpp)
int fingerprint_impl(sonar_ctx* c, const void* pcm, int64_t n, const sonar_fp_cfg* cfg, sonar_fp_out* out,
                     bool pcm_dev, int64_t f_lo, int64_t f_hi, bool raw_window) {
  if (!c || !cfg || !out) return fail(c, SONAR_ERR_INVALID, "null argument");
  // ComputeSTFTWithWindow validation order (spectral.go:386-412), then the GPU path's limits
  int64_t F = 0;
  {
    std::string msg;
    const int rc = fp_validate(cfg, n, pcm != nullptr, &F, &msg);
    if (rc != SONAR_OK) return fail(c, rc, msg);
  }
  const int plan = fp_plan(cfg, F);
  // a frame range [f_lo, f_hi) of the whole signal's STFT (the chunked host-PCM pipeline of the
  // speech extractor): device outputs, the per-frame fused kernel, no energy frames
  if (f_hi < 0 || f_hi > F) f_hi = F;
  if (f_lo < 0) f_lo = 0;
  const bool ranged = f_lo > 0 || f_hi < F;
  if (ranged && (cfg->device_ptrs == 0 || plan != SONAR_PLAN_WAVE || (cfg->flags & SONAR_FP_ENERGY)))
    return fail(c, SONAR_ERR_UNSUPPORTED, "frame ranges need device outputs and the per-frame fused kernel");
  if (f_hi <= f_lo) return SONAR_OK;
  FpCall k{};
  k.c = c; k.cfg = cfg; k.s = c->stream;
  k.n = n; k.F = F; k.f_lo = f_lo; k.f_hi = f_hi;
  k.W = cfg->window_size; k.H = cfg->hop_size; k.K = k.W / 2 + 1;
  k.flags = cfg->flags;
  // The spectral descriptors always take the float64 transform, whatever `precision` says: the
  // flatness (exp of the mean ln over every bin above 1e-10, spectral_flatness.go:31-73) and the
  // log-log slope (spectral_slope.go:24-63) read leakage bins that sit below an f32 FFT's rounding
  // floor, so an f32 transform cannot hold them to 1e-4.  ~10 % of the kernel.
  k.f64 = cfg->precision == SONAR_F64 || (k.flags & SONAR_FP_SPECTRAL) != 0;
  k.pcm64 = cfg->pcm_dtype == SONAR_F64;
  k.o64 = cfg->out_dtype == SONAR_F64;
  k.raw_window = raw_window;
  HIP_TRY(c, hipSetDevice(c->device));
  const bool dev = cfg->device_ptrs != 0;
  k.dpcm = pcm;
  if (!dev && !pcm_dev) {
    const size_t bytes = (size_t)n * (k.pcm64 ? 8 : 4);
    void* p = dbuf(c, "fp.pcm", bytes);
    if (!p) return fail(c, SONAR_ERR_NOMEM, "device allocation failed (pcm)");
    HIP_TRY(c, hipMemcpyAsync(p, pcm, bytes, hipMemcpyHostToDevice, k.s));
    k.dpcm = p;
  }
  Staging st{c, "fp.out.", dev};
  int rc = resolve_outputs(k, st, out);
  if (rc != SONAR_OK) return rc;
  c->last_fp_kernel = "";
  bool pair_done = false;
  if (plan == SONAR_PLAN_DFT) rc = run_dft(k);
  else if (plan == SONAR_PLAN_PAIR) rc = run_pair(k, &pair_done);
  if (rc == SONAR_OK && (plan == SONAR_PLAN_WAVE || (plan == SONAR_PLAN_PAIR && !pair_done))) rc = run_wave(k);
  if (rc != SONAR_OK) return rc;
  rc = run_zcr_energy(k, st, out);
  if (rc != SONAR_OK) return rc;
  return dev ? SONAR_OK : st.finish();   // device outputs stay queued on the stream
}
}  // namespace detail
}  // namespace sonar

extern "C" {

int64_t sonar_stft_frames(int64_t n, int32_t W, int32_t H) {
  if (n <= 0) return SONAR_ERR_EMPTY;
  if (W <= 0 || H <= 0) return SONAR_ERR_INVALID;
  const int64_t F = go_frames(n, W, H);
  return F <= 0 ? SONAR_ERR_TOO_SHORT : F;
}

void sonar_fp_cfg_default(sonar_fp_cfg* c) {
  std::memset(c, 0, sizeof(*c));
  c->window_size = 1024;
  c->hop_size = 256;
  c->window_type = SONAR_WIN_HANN;
  c->sample_rate = 44100;
  c->n_mfcc = 13;
  c->n_filters = 26;
  c->filterbank = SONAR_FB_MEL;
  c->use_lifter = 1;
  c->lifter = 22.0;
  c->preemph_alpha = 0.97;
  c->flags = SONAR_FP_MFCC;
  c->precision = SONAR_F32;
  c->pcm_dtype = SONAR_F64;
  c->out_dtype = SONAR_F64;
}

int32_t sonar_fp_kernel_plan(const sonar_fp_cfg* cfg, int64_t n) {
  if (!cfg) return SONAR_ERR_INVALID;
  int64_t F = 0;
  std::string msg;
  const int rc = fp_validate(cfg, n, true, &F, &msg);
  return rc != SONAR_OK ? rc : fp_plan(cfg, F);
}

int sonar_fingerprint(sonar_ctx* c, const void* pcm, int64_t n, const sonar_fp_cfg* cfg, sonar_fp_out* out) {
  return sonar::detail::fingerprint_impl(c, pcm, n, cfg, out, cfg && cfg->device_ptrs != 0);
}

}  // extern "C"

namespace {
// The segment table of a one-launch batch in pinned staging: {pcm address, frames inside the signal, F,
// out address, first pair}[count] and the pair total; the addresses are filled by the caller.  The
// staging is reused once the previous call's upload of it has completed.
int batch_segments(sonar_ctx* c, const int64_t* n, int32_t count, int W, int H, int64_t** seg_out, int64_t* NP,
                   int64_t* ns, int64_t* nf) {
  if (c->fpb_ev) HIP_TRY(c, hipEventSynchronize(c->fpb_ev));
  else HIP_TRY(c, hipEventCreateWithFlags(&c->fpb_ev, hipEventDisableTiming));
  int64_t* seg = (int64_t*)hbuf(c, "fpb.seg", (5 * (size_t)count + 1) * 8);
  if (!seg) return fail(c, SONAR_ERR_NOMEM, "pinned allocation failed (batch table)");
  *NP = *ns = *nf = 0;
  for (int i = 0; i < count; i++) {
    const int64_t F = go_frames(n[i], W, H);
    // frames whose W samples lie inside the signal (F itself unless n < W: Go's count truncates)
    seg[2 * (size_t)count + i] = F; seg[(size_t)count + i] = n[i] >= W ? std::min<int64_t>(F, (n[i] - W) / H + 1) : 0;
    seg[4 * (size_t)count + i] = *NP;
    *NP += (F + 1) / 2; *ns += n[i]; *nf += F;
  }
  seg[5 * (size_t)count] = *NP;
  *seg_out = seg;
  return SONAR_OK;
}
}  // namespace

// SpectralAnalyzer.ComputeSTFTBatch (fingerprint/analyzers/spectral.go:234-285): every signal through
// ComputeSTFTWithWindow with one configuration; the first failing signal (by index) reports
// "error processing signal i: <its error>" (:276-281).  The f32 MFCC configuration at W = 1024 runs
// all signals' frame pairs in ONE mfcc_pair_kernel launch (segment table, mfcc_pair.hip SEG); any
// other configuration runs sonar_fingerprint per signal on the context's stream.
extern "C" int sonar_fingerprint_batch(sonar_ctx* c, const void* const* pcm, const int64_t* n, int32_t count,
                                       const sonar_fp_cfg* cfg, sonar_fp_out* out) {
  if (!c) return SONAR_ERR_INVALID;
  if (count <= 0) return fail(c, SONAR_ERR_EMPTY, "no signals provided");
  if (!pcm || !n || !cfg || !out) return fail(c, SONAR_ERR_INVALID, "null argument");
  const int W = cfg->window_size, H = cfg->hop_size;
  auto sig_fail = [&](int i, int code, const std::string& msg) {
    return fail(c, code, "error processing signal " + std::to_string(i) + ": " + msg);
  };
  // ComputeSTFTWithWindow's checks per signal, in its order (spectral.go:386-412)
  for (int i = 0; i < count; i++) {
    if (n[i] <= 0 || !pcm[i]) return sig_fail(i, SONAR_ERR_EMPTY, "empty signal");
    if (W <= 0) return sig_fail(i, SONAR_ERR_INVALID, "window size must be positive");
    if (H <= 0) return sig_fail(i, SONAR_ERR_INVALID, "hop size must be positive");
    if (go_frames(n[i], W, H) <= 0)
      return sig_fail(i, SONAR_ERR_TOO_SHORT, "signal too short for given window size and hop size");
  }
  const bool dev = cfg->device_ptrs != 0;
  int64_t pairs_total = 0;                 // the one launch's 32-bit frame indices run over the whole batch
  for (int i = 0; i < count; i++) pairs_total += (go_frames(n[i], W, H) + 1) / 2;
  const bool one_launch = W == 1024 && cfg->flags == SONAR_FP_MFCC && cfg->precision == SONAR_F32 &&
                          cfg->pcm_dtype == SONAR_F32 && cfg->out_dtype == SONAR_F32 &&
                          2 * pairs_total <= SONAR_PAIR_MAX_FRAMES;
  const PairTables* tp = one_launch ? &pair_tables_for(c, cfg) : nullptr;
  if (!tp || !tp->ok) {
    for (int i = 0; i < count; i++) {
      const int rc = sonar::detail::fingerprint_impl(c, pcm[i], n[i], cfg, &out[i], dev);
      if (rc != SONAR_OK) return sig_fail(i, rc, c->err);
    }
    return SONAR_OK;
  }
  const PairTables& t = *tp;
  for (int i = 0; i < count; i++)
    if (!out[i].mfcc) return fail(c, SONAR_ERR_INVALID, "out[" + std::to_string(i) + "].mfcc is null");
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const size_t seg_n = 5 * (size_t)count + 1;
  int64_t *seg = nullptr, NP = 0, ns = 0, nf = 0;
  const int src = batch_segments(c, n, count, W, H, &seg, &NP, &ns, &nf);
  if (src != SONAR_OK) return src;
  float* dpcm = nullptr;
  float* dout = nullptr;
  if (!dev) {
    dpcm = (float*)dbuf(c, "fpb.pcm", (size_t)ns * 4);
    dout = (float*)dbuf(c, "fpb.mfcc", (size_t)nf * t.n_mfcc * 4);
    if (!dpcm || !dout) return fail(c, SONAR_ERR_NOMEM, "device allocation failed (batch)");
  }
  int64_t po = 0, fo = 0;
  for (int i = 0; i < count; i++) {
    if (dev) {
      seg[i] = (int64_t)(uintptr_t)pcm[i];
      seg[3 * (size_t)count + i] = (int64_t)(uintptr_t)out[i].mfcc;
    } else {
      HIP_TRY(c, hipMemcpyAsync(dpcm + po, pcm[i], (size_t)n[i] * 4, hipMemcpyHostToDevice, s));
      seg[i] = (int64_t)(uintptr_t)(dpcm + po);
      seg[3 * (size_t)count + i] = (int64_t)(uintptr_t)(dout + fo * t.n_mfcc);
    }
    po += n[i]; fo += seg[2 * (size_t)count + i];
  }
  int64_t* dseg = (int64_t*)dbuf(c, "fpb.seg", seg_n * 8);
  if (!dseg) return fail(c, SONAR_ERR_NOMEM, "device allocation failed (batch table)");
  HIP_TRY(c, hipMemcpyAsync(dseg, seg, seg_n * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(c, hipEventRecord(c->fpb_ev, s));
  sonar::MfccPairParams q{};
  q.F = 2 * NP; q.H = H;
  q.seg = dseg; q.nseg = count;
  const int lrc = launch_pair(c, t, cfg, NP, false, s, q);
  if (lrc != SONAR_OK) return lrc;
  if (!dev) {
    fo = 0;
    for (int i = 0; i < count; i++) {
      const int64_t F = seg[2 * (size_t)count + i];
      HIP_TRY(c, hipMemcpyAsync(out[i].mfcc, dout + fo * t.n_mfcc, (size_t)F * t.n_mfcc * 4, hipMemcpyDeviceToHost, s));
      fo += F;
    }
    HIP_TRY(c, hipStreamSynchronize(s));
  }
  return SONAR_OK;
}
