// fp_layout.h -- the LDS carves of the two fused fingerprint kernels as functions of integers only:
// fp_wave_kernel's (fp_kernel.hip: shared twiddle / filterbank tables, then one region per wave) and
// mfcc_pair_kernel's (mfcc_pair.hip: tables, then one region per wave).  fp_api.cpp copies the results
// into FpParams / MfccPairParams; tests/c_abi/fp_layout_check.cpp holds them to the formulas they replaced.
// Plain C++: no HIP include.
#pragma once
#include <algorithm>

#include "mfcc_pair_layout.h"

namespace sonar {

constexpr int kLdsLimit = 160 * 1024;   // LDS bytes one block may use on gfx950
constexpr int lds_al16(int x) { return (x + 15) & ~15; }

// Byte offsets of fp_wave_kernel's block: lds_tab_* from the block's base, lds_logmel / lds_stage inside a
// wave's region (its FFT rows start at 0), waves of lds_wave_stride bytes from lds_wave0.  lds_bytes can
// exceed kLdsLimit (one wave does not fit): the caller refuses the launch.
struct FpLdsLayout {
  int lds_tab_t1, lds_tab_t2, lds_tab_t3, lds_tab_mel, lds_tab_w, lds_tab_dct, lds_wave0;
  int lds_logmel, lds_stage, lds_wave_stride, waves_per_block, lds_bytes;
};
inline FpLdsLayout fp_lds_layout(int W, bool f64, int NB, int PRE, int n_mels, int n_mfcc, int nnz, int n_groups) {
  const int esz = f64 ? 8 : 4, K = W / 2 + 1;
  const int R = W / 128, FR = R >= 8 ? 1 : 8 / R, G = R * FR / 8;
  FpLdsLayout l{};
  l.lds_tab_t1 = 0;
  l.lds_tab_t2 = lds_al16(R * 64 * 2 * esz);
  l.lds_tab_t3 = l.lds_tab_t2 + lds_al16(64 * 2 * esz);
  l.lds_tab_mel = l.lds_tab_t3 + lds_al16(G * 8 * 64 * 2 * esz);
  l.lds_tab_w = l.lds_tab_mel + lds_al16((4 * n_mels + n_groups + 1) * 4);
  l.lds_tab_dct = l.lds_tab_w + lds_al16(std::max(nnz, 1) * esz);
  l.lds_wave0 = l.lds_tab_dct + lds_al16((n_mfcc * n_mels + n_mfcc) * esz);
  l.lds_logmel = lds_al16((PRE + NB) * K * esz);
  l.lds_stage = l.lds_logmel + lds_al16(NB * (n_mels + 1) * esz);
  l.lds_wave_stride = l.lds_stage + lds_al16(NB * n_mfcc * esz);
  l.waves_per_block = 4;
  while (l.waves_per_block > 1 && l.lds_wave0 + l.waves_per_block * l.lds_wave_stride > kLdsLimit)
    l.waves_per_block--;
  l.lds_bytes = l.lds_wave0 + l.waves_per_block * l.lds_wave_stride;
  return l;
}

// Byte offsets of mfcc_pair_kernel's block.  wave_bytes and default_waves are mfcc_pair.hip's
// (mfcc_pair_wave_bytes, mfcc_pair_waves_per_block).  The float64 waves' 17.4 KB regions beside the
// largest tables (J = 16, NMP = 64: 29 KB) exceed the limit at 8 waves; such a bank runs 7 (or fewer).
struct PairLdsLayout {
  int lds_src, lds_dct, lds_ctr, lds_tw2, lds_wave0, waves_per_block, lds_bytes;   // lds_tw2: float64 only
};
inline PairLdsLayout pair_lds_layout(int J, int JS, int NMP, bool f64, int wave_bytes, int default_waves) {
  (void)J;   // the weight rows are JS (>= J) complex wide
  const int e = f64 ? 1 : 0, es = f64 ? 8 : 4;
  PairLdsLayout l{};
  l.lds_src = lds_al16(64 * JS * 2 * es);
  l.lds_dct = l.lds_src + 64 * 16 * 2;
  l.lds_ctr = l.lds_dct + lds_al16(16 * (NMP + mfcc_pair_dct_pad(e)) * es);
  l.lds_tw2 = l.lds_ctr + 16;
  l.lds_wave0 = l.lds_tw2 + (f64 ? 8 * kPairTw2Row * 16 : 0);   // float64: the stage-2 twiddle table
  l.waves_per_block = default_waves;
  while (l.waves_per_block > 1 && l.lds_wave0 + l.waves_per_block * wave_bytes > kLdsLimit) --l.waves_per_block;
  l.lds_bytes = l.lds_wave0 + l.waves_per_block * wave_bytes;
  return l;
}

}  // namespace sonar
