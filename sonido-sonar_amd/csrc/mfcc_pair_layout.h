// mfcc_pair_layout.h -- the per-instance LDS layout constants of mfcc_pair_kernel that the kernel
// (mfcc_pair.hip, through kernels.h) shares with the host table builder (fp_tables.cpp) and the LDS carve
// (fp_layout.h).  Plain C++: no HIP include.
#pragma once

namespace sonar {

// Bank-conflict-free strides for the kernel's 8-B float32 and 16-B float64 accesses
// (tools/pair_lds_model.py):
//   pad rows after every 16 power rows: float32 2 (18 rows x 8 B = 36 dwords per 16 bins), float64
//   1 (17 x 16 B = 68 dwords: 8-lane ds_write_b128 groups of rows 18 apart collide mod 32);
//   DCT row stride NMP + 4 (float32) / NMP + 2 (float64), stage-2 twiddle rows of 9 complex (float64).
constexpr int mfcc_pair_pad_rows(int f64) { return f64 ? 1 : 2; }
constexpr int mfcc_pair_dct_pad(int f64) { return f64 ? 2 : 4; }
constexpr int kPairTw2Row = 9;
// chunk_w row stride (complex per lane).  float32: the filterbank reads two bins' weights as one
// ds_read_b128, so the stride is the smallest even JS >= J (J + 1 for odd J) with JS = 2 mod 4:
// rows stay 16-byte aligned and the lane stride is an odd number of 16-byte units, which spreads
// each 16-lane group of the read over all 64 banks.  float64 (16-byte reads of one bin): J | 1.
#ifndef HL_W128
#define HL_W128 1
#endif
constexpr int mfcc_pair_w128(int f64) { return HL_W128 && !f64; }
constexpr int mfcc_pair_w_stride(int J, int f64) {
  if (!mfcc_pair_w128(f64)) return J | 1;
  const int m = J + (J & 1);
  return (m & 3) == 2 ? m : m + 2;
}

}  // namespace sonar
