// fp_tables.h -- the device tables of the three fingerprint paths, built on the host as ONE image
// each: a byte vector whose sections start at multiples of 256 bytes (the kernels' 16-byte weight reads
// need 16), and a descriptor with the section offsets and the integers.  fp_api.cpp uploads an image
// with one allocation and one copy and keeps typed views into it.  Plain C++: no HIP include
// (tests/c_abi/fp_tables_check.cpp runs the builders on a CPU).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/sonar_gpu.h"

namespace sonar {
namespace host {

// The WindowConfig literals of ComputeSTFTWithWindow / ComputeSTFTStreaming (spectral.go:290-295,
// :415-420) and extractChromaFeatures (music.go:335-340) set only Type, Size, Normalize and Symmetric:
// Beta and Alpha keep Go's zero value, not DefaultWindowConfig's 8.6 / 0.5 (windowing.go:66-73).  So a
// Kaiser STFT window is I0(0)/I0(0) = 1 everywhere and a Tukey one has no taper (int(0 * N / 2) = 0):
// both are rectangular.
constexpr double kStftBeta = 0.0, kStftAlpha = 0.0;

using Image = std::vector<unsigned char>;
constexpr size_t kSectionAlign = 256;

// appends v as a new section (at least 16 bytes, as each table's own allocation had); its offset
template <typename T>
size_t put_section(Image& im, const std::vector<T>& v) {
  const size_t off = (im.size() + kSectionAlign - 1) / kSectionAlign * kSectionAlign;
  const size_t bytes = v.size() * sizeof(T);
  im.resize(off + (bytes < 16 ? 16 : bytes), 0);
  if (bytes) std::memcpy(im.data() + off, v.data(), bytes);
  return off;
}
// float64 values as they are, or rounded once to float32
size_t put_real(Image& im, const std::vector<double>& v, bool f64);

// (cos, -sin) of 2 pi m / n, m < n: the DFT path's and the chroma kernel's twiddles
std::vector<double> trig_table(int n);

enum { TABLES_OK = 0, TABLES_BAD_WINDOW = 1, TABLES_BAD_BANK = 2 };

// DFT path (float64 all through) and fp_wave_kernel (T = double or float; grp_*: the filters of each
// epilogue group).  has_mfcc = false: window and trig only, the rest is unset.
struct FpTableDesc {
  size_t window = 0, trig = 0;
  bool has_mfcc = false;
  size_t mel_lo = 0, mel_hi = 0, mel_woff = 0, grp_off = 0, grp_mels = 0, mel_w = 0, dct = 0, lift = 0;
  int n_mels = 0, n_mfcc = 0, nnz = 0;
};
// window (not energy-normalised when raw_window), trig, and with want_mfcc the filterbank / DCT / lifter
int build_dft_tables(const sonar_fp_cfg* cfg, bool raw_window, bool want_mfcc, Image& im, FpTableDesc& d);
// window and MFCC tables in the kernel's precision, the filters balanced over `groups` epilogue groups
int build_wave_tables(const sonar_fp_cfg* cfg, bool raw_window, bool f64, int groups, Image& im, FpTableDesc& d);

// mfcc_pair_kernel (W = 1024): [0] float32 tables (the headline), [1] float64 (the same bank at the
// reference's precision; its own chunk lane order, searched for its 16-byte power-row reads)
struct PairTableDesc {
  bool ok = false;
  size_t window[2] = {}, tw1[2] = {}, tw2[2] = {}, chunk_w[2] = {}, dct[2] = {}, chunk_ks[2] = {}, mel_src[2] = {};
  size_t zeros = 0;         // 1024 zero samples of either PCM type (8 KB)
  int JS[2] = {};           // chunk_w row stride per precision (mfcc_pair_w_stride)
  int J = 0, NMP = 0, n_mels = 0, n_mfcc = 0, max_src = 0;
};
// false (d.ok = false, the image unspecified) when the bank does not fit the kernel
bool build_pair_tables(const sonar_fp_cfg* cfg, Image& im, PairTableDesc& d);

}  // namespace host
}  // namespace sonar
