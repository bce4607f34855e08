// magnitude_walk.h -- the one chunked walk over rows of |X|, for the entries that run the float64 STFT
// magnitudes of a device signal through a bounded scratch (sonar_hpcp, sonar_hps, the flux onset
// detector, sonar_chord_detect): the transform of chunk_frames frames into the scratch, the entry's own
// work over those rows, the next chunk, all queued on the context's stream.
#pragma once
#include <algorithm>
#include <cstring>
#include <string>

#include "ctx.h"
#include "staging.h"

namespace sonar {
namespace detail {

struct MagnitudeWalk {
  sonar_fp_cfg cfg;   // SONAR_FP_MAGNITUDE only, float64 all through, device pointers
  int64_t F = 0, chunk_frames = 0;   // about 64 MiB of rows; the caller may set another count after plan
  int32_t W = 0, H = 0, K = 0;
  double* rows = nullptr;            // the chunk's rows; lead_rows rows of the scratch lie before them

  // the transform's own checks of a signal of n samples (fp_check: its code, its text), then F, K and chunk_frames
  int plan(int32_t sample_rate, int32_t window_size, int32_t hop_size, int32_t window_type, int64_t n, bool have_pcm,
           std::string* msg) {
    W = window_size;
    H = hop_size;
    sonar_fp_cfg_default(&cfg);
    cfg.window_size = W;
    cfg.hop_size = H;
    cfg.window_type = window_type;
    cfg.sample_rate = sample_rate;
    cfg.flags = SONAR_FP_MAGNITUDE;
    cfg.precision = cfg.pcm_dtype = cfg.out_dtype = SONAR_F64;
    cfg.device_ptrs = 1;
    const int rc = fp_check(&cfg, n, have_pcm, &F, msg);
    if (rc != SONAR_OK) return rc;
    K = W / 2 + 1;
    chunk_frames = std::max<int64_t>((int64_t(64) << 20) / (K * 8), 1);
    return SONAR_OK;
  }
  // before ready(): the scratch, so that its failure is the entry's one SONAR_ERR_NOMEM
  void alloc(Staging& o, int64_t lead_rows = 0, const char* name = "chunk") {
    double* scratch = o.tmp<double>(name, (size_t)(std::min(chunk_frames, F) + lead_rows) * (size_t)K);
    rows = scratch ? scratch + lead_rows * K : nullptr;
  }
  // fn(rows, f0, nf) over every chunk's nf rows from frame f0 on, until one does not return SONAR_OK.
  // Frame f of the signal is frame f - f0 of the samples from f0 * H on.  The transform sees the samples
  // there are, never more: Go's truncating frame count gives the flux detector's signal with n in
  // (W - H, W) one frame, left all zero (stft.go:59, :140).  In the other entries every frame lies inside
  // the signal, so the minimum is its first argument.
  template <typename Fn>
  int each(sonar_ctx* c, const double* dx, int64_t n, bool raw_window, Fn fn) const {
    for (int64_t f0 = 0; f0 < F; f0 += chunk_frames) {
      const int64_t nf = std::min(chunk_frames, F - f0);
      sonar_fp_out fo;
      std::memset(&fo, 0, sizeof fo);
      fo.magnitude = rows;
      int rc = fingerprint_impl(c, dx + f0 * H, std::min((nf - 1) * H + W, n - f0 * H), &cfg, &fo, true, 0, -1, raw_window);
      if (rc == SONAR_OK) rc = fn(rows, f0, nf);
      if (rc != SONAR_OK) return rc;
    }
    return SONAR_OK;
  }
};

}  // namespace detail
}  // namespace sonar
