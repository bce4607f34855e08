// fp_layout_check -- csrc/fp_layout.h under a plain host compiler: the LDS carves of fp_wave_kernel and
// mfcc_pair_kernel are those of the inline formulas the header replaced (written out here), every region
// is 16-byte aligned and inside the 160 KiB of a block, and a float64 pair bank with the largest tables
// runs fewer waves than the default.  Prints one line per failure; exit status 1 if there is any.
#include <algorithm>
#include <cstdio>

#include "../../sonido-sonar_amd/csrc/fp_layout.h"
#include "../../sonido-sonar_amd/csrc/host_dsp.h"

static int failures = 0;
static void eq(const char* what, const char* tag, long long got, long long want) {
  if (got == want) return;
  std::printf("FAIL %s (%s): got %lld, want %lld\n", what, tag, got, want);
  failures++;
}
static void ok(bool cond, const char* what, const char* tag, long long v) {
  if (cond) return;
  std::printf("FAIL %s (%s): %lld\n", what, tag, v);
  failures++;
}
static int al(int x) { return (x + 15) & ~15; }

// fp_kernel.hip's fp_batch_frames / fp_pre_rows
static int batch_frames(int W, int f64, int spec) {
  const int R = W / 128, FR = R >= 8 ? 1 : 8 / R;
  return (f64 && !spec) ? FR : (FR > 4 ? FR : 4);
}
static int pre_rows(int W, int spec) {
  const int R = W / 128, FR = R >= 8 ? 1 : 8 / R;
  return spec ? FR : 0;
}

static void fused(int W, int f64, int spec, int n_filters) {
  sonar::host::MfccTables mt;
  if (!sonar::host::make_mfcc_tables(44100, 13, n_filters, 0, 0.0, 0.0, true, 22.0, W, mt)) {
    std::printf("FAIL bank of %d filters at W = %d\n", n_filters, W);
    failures++;
    return;
  }
  char tag[96];
  std::snprintf(tag, sizeof(tag), "fused W=%d f64=%d spec=%d filters=%d", W, f64, spec, n_filters);
  const int NB = batch_frames(W, f64, spec), PRE = pre_rows(W, spec), n_groups = 64 / NB;
  const int n_mels = mt.n_mels, n_mfcc = mt.n_mfcc, nnz = (int)mt.w.size(), K = W / 2 + 1;
  const sonar::FpLdsLayout l = sonar::fp_lds_layout(W, f64 != 0, NB, PRE, n_mels, n_mfcc, nnz, n_groups);
  // the formulas of fingerprint_impl's inline carve
  const int esz = f64 ? 8 : 4;
  const int R = W / 128, FR = R >= 8 ? 1 : 8 / R, G = R * FR / 8;
  const int t1 = 0, t2 = al(R * 64 * 2 * esz), t3 = t2 + al(64 * 2 * esz), mel = t3 + al(G * 8 * 64 * 2 * esz);
  const int w = mel + al((4 * n_mels + n_groups + 1) * 4), dct = w + al(std::max(nnz, 1) * esz);
  const int wave0 = dct + al((n_mfcc * n_mels + n_mfcc) * esz);
  const int logmel = al((PRE + NB) * K * esz), stage = logmel + al(NB * (n_mels + 1) * esz);
  const int stride = stage + al(NB * n_mfcc * esz);
  int waves = 4;
  while (waves > 1 && wave0 + waves * stride > 160 * 1024) waves--;
  eq("tab_t1", tag, l.lds_tab_t1, t1); eq("tab_t2", tag, l.lds_tab_t2, t2); eq("tab_t3", tag, l.lds_tab_t3, t3);
  eq("tab_mel", tag, l.lds_tab_mel, mel); eq("tab_w", tag, l.lds_tab_w, w); eq("tab_dct", tag, l.lds_tab_dct, dct);
  eq("wave0", tag, l.lds_wave0, wave0); eq("logmel", tag, l.lds_logmel, logmel); eq("stage", tag, l.lds_stage, stage);
  eq("wave_stride", tag, l.lds_wave_stride, stride); eq("waves_per_block", tag, l.waves_per_block, waves);
  eq("bytes", tag, l.lds_bytes, wave0 + waves * stride);
  const int offs[10] = {l.lds_tab_t1, l.lds_tab_t2, l.lds_tab_t3, l.lds_tab_mel, l.lds_tab_w, l.lds_tab_dct, l.lds_wave0, l.lds_logmel, l.lds_stage,
                        l.lds_wave_stride};
  for (int o : offs) ok(o % 16 == 0, "16-byte aligned", tag, o);
  ok(l.waves_per_block >= 1 && l.waves_per_block <= 4, "waves", tag, l.waves_per_block);
  ok(l.lds_bytes <= sonar::kLdsLimit, "inside the LDS", tag, l.lds_bytes);   // every case of this table fits
}

// One wave's region of mfcc_pair_kernel and its waves per block, read in mfcc_pair.hip: Lay<T>::WaveBytes
// = 64 * T2Stride + 16 with T2Stride = 17 * 2 * sizeof(T), and mfcc_pair_waves_per_block (12 / 8).
static const int kWaveBytes[2] = {64 * 17 * 2 * 4 + 16, 64 * 17 * 2 * 8 + 16};   // 8720, 17424
static const int kWaves[2] = {12, 8};

static sonar::PairLdsLayout pair(int J, int NMP, int f64) {
  char tag[96];
  std::snprintf(tag, sizeof(tag), "pair J=%d NMP=%d f64=%d", J, NMP, f64);
  const int JS = sonar::mfcc_pair_w_stride(J, f64);
  const sonar::PairLdsLayout l = sonar::pair_lds_layout(J, JS, NMP, f64 != 0, kWaveBytes[f64], kWaves[f64]);
  // the formulas of fill_pair_params
  const int es = f64 ? 8 : 4;
  const int src = al(64 * JS * 2 * es), dct = src + 64 * 16 * 2;
  const int ctr = dct + al(16 * (NMP + (f64 ? 2 : 4)) * es), tw2 = ctr + 16;
  const int wave0 = tw2 + (f64 ? 8 * 9 * 16 : 0);
  int waves = kWaves[f64];
  while (waves > 1 && wave0 + waves * kWaveBytes[f64] > 160 * 1024) --waves;
  eq("src", tag, l.lds_src, src); eq("dct", tag, l.lds_dct, dct); eq("ctr", tag, l.lds_ctr, ctr); eq("tw2", tag, l.lds_tw2, tw2);
  eq("wave0", tag, l.lds_wave0, wave0); eq("waves_per_block", tag, l.waves_per_block, waves);
  eq("bytes", tag, l.lds_bytes, wave0 + waves * kWaveBytes[f64]);
  for (int o : {l.lds_src, l.lds_dct, l.lds_ctr, l.lds_tw2, l.lds_wave0}) ok(o % 16 == 0, "16-byte aligned", tag, o);
  ok(l.lds_bytes <= sonar::kLdsLimit, "inside the LDS", tag, l.lds_bytes);
  return l;
}

int main() {
  const int Ws[5] = {128, 256, 512, 1024, 2048}, banks[3] = {26, 40, 64};
  for (int W : Ws)
    for (int f64 = 0; f64 < 2; f64++)
      for (int spec = 0; spec < 2; spec++)
        for (int nf : banks) fused(W, f64, spec, nf);
  for (int f64 = 0; f64 < 2; f64++)
    for (int J = 1; J <= 16; J++)
      for (int NMP = 8; NMP <= 64; NMP += 8) pair(J, NMP, f64);
  // the headline bank (44.1 kHz, 40 filters: J = 12) keeps the default waves in both precisions
  eq("headline float32 waves", "pair", pair(12, 40, 0).waves_per_block, 12);
  eq("headline float64 waves", "pair", pair(12, 40, 1).waves_per_block, 8);
  // the largest float64 tables: 8 waves of 17,424 bytes beside them exceed 160 KiB
  const sonar::PairLdsLayout big = pair(16, 64, 1);
  ok(big.waves_per_block < kWaves[1], "float64 J=16 NMP=64 runs fewer waves than the default", "pair", big.waves_per_block);
  eq("float64 J=16 NMP=64 waves", "pair", big.waves_per_block, 7);
  ok(big.lds_bytes <= 160 * 1024, "float64 J=16 NMP=64 inside 160 KiB", "pair", big.lds_bytes);
  eq("LDS limit", "constant", sonar::kLdsLimit, 163840);
  if (failures) return 1;
  std::printf("fp_layout ok\n");
  return 0;
}
