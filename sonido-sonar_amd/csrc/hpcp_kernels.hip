// hpcp_kernels.hip -- SpectralPeaks.DetectPeaks (algorithms/harmonic/spectral_peaks.go:36-100) and
// HPCP.ComputeFromSpectralPeaks (algorithms/chroma/hpcp.go:147-202) per spectrum row, float64 like the
// Go reference.
//
// One wave (one block) per row.  A peak's frequency is bin * freq_res, so everything transcendental
// in the profile is the host's table (hpcp_api.cpp, sonar_hpcp_table); the device compares, selects
// and adds (magnitude * factor) * window_weight in the reference's program order.  Every comparison
// and every sum here decides an output bit, so this file is built without FMA contraction.
//
//  1. candidates: 64 bins per step, ballot + prefix -> the row's strict local maxima >= min_height,
//     compacted in bin order into LDS as (ordered key of the magnitude, bin).
//  2. the distance rule (:56-73), only when min_distance_bins >= 3: "compare with the
//     last kept peak" (F35), a serial chain walked by lane 0, compacting in place.
//  3. the max_peaks largest by (magnitude descending, bin ascending) in that order: when there are
//     more kept peaks than slots, a bitwise search for the max_peaks-th largest key and a compaction
//     leave exactly max_peaks of them; then every peak counts the peaks that precede it, and that
//     rank is its output slot.
//  4. the profile: lane b (and b + 64) owns hpcp[b] and walks the sorted peaks' table rows, adding
//     the entries of its bin; then NonLinear, the energy normalisation, MaxShifted, energy, entropy.
#include <cstdint>

#include "kernels.h"

namespace sonar {

namespace {

// Larger magnitude <-> larger key; -0.0 and +0.0 share a key (Go's > does not tell them apart).
// Candidates are never NaN: a NaN fails its own comparisons.
__device__ inline uint64_t order_key(double m) {
  const uint64_t u = (uint64_t)__double_as_longlong(m + 0.0);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

constexpr int kProfSlots = 128;   // >= HPCP_MAX_SIZE

}  // namespace

// LDS: keys[cmax] | prof[2][kProfSlots] | nkept | cbin[cmax, padded to 4] | sbin[P]
__global__ __launch_bounds__(64) void hpcp_rows_kernel(HpcpArgs a) {
  extern __shared__ unsigned char smem[];
  const int lane = threadIdx.x;
  const int K = a.K, P = a.P;
  const int cmax = K > 2 ? (K - 1) / 2 : 0;
  uint64_t* keys = (uint64_t*)smem;
  double* prof = (double*)(keys + cmax);
  int* nkept = (int*)(prof + 2 * kProfSlots);
  uint16_t* cbin = (uint16_t*)(nkept + 2);
  uint16_t* sbin = cbin + ((cmax + 3) & ~3);
  const uint64_t below = lane == 0 ? 0ull : (~0ull >> (64 - lane));   // the lanes before this one

  for (int64_t f = blockIdx.x; f < a.F; f += gridDim.x) {
    const double* row = a.mag + f * (int64_t)K;
    // 1. candidates, in bin order
    int C = 0;
    for (int base = 1; base < K - 1; base += 64) {
      const int i = base + lane;
      bool cand = false;
      double m = 0.0;
      if (i < K - 1) {
        m = row[i];
        cand = m > row[i - 1] && m > row[i + 1] && m >= a.min_height;
      }
      const uint64_t b = __ballot(cand);
      if (cand) {
        const int pos = C + __popcll(b & below);   // < cmax: strict maxima are 2 bins apart
        keys[pos] = order_key(m);
        cbin[pos] = (uint16_t)i;
      }
      C += __popcll(b);
    }
    __syncthreads();
    // 2. the distance rule
    if (a.min_dist >= 3 && C > 1) {
      if (lane == 0) {
        int n = 1;
        uint64_t lk = keys[0];
        int lb = cbin[0];
        for (int j = 1; j < C; ++j) {
          const uint64_t k = keys[j];
          const int b = cbin[j];
          if (b - lb < a.min_dist) {
            if (k > lk) { keys[n - 1] = k; cbin[n - 1] = (uint16_t)b; lk = k; lb = b; }   // replaces it (:60-67)
          } else {
            keys[n] = k; cbin[n] = (uint16_t)b; ++n; lk = k; lb = b;
          }
        }
        nkept[0] = n;
      }
      __syncthreads();
      C = nkept[0];
    }
    const int nsel = C < P ? C : P;
    // 3a. more kept peaks than slots: keep the P that come first in (magnitude descending, bin
    // ascending).  T, the P-th largest key, is found bit by bit (the largest T that P keys reach);
    // the keys above T and the first P - #above of the keys equal to T, in bin order, are compacted
    // in place (a peak moves to an index not above its own, and a step reads before it writes).
    int R = P == 0 ? 0 : C;
    if (P > 0 && P < C) {
      constexpr int kRegSlots = 8;                 // up to 512 kept peaks: the lane's keys stay in registers
      uint64_t mine[kRegSlots];
      const bool in_regs = C <= 64 * kRegSlots;
#pragma unroll
      for (int q = 0; q < kRegSlots; ++q) mine[q] = (in_regs && q * 64 + lane < C) ? keys[q * 64 + lane] : 0ull;
      auto reach = [&](uint64_t t, bool strictly) {   // keys >= t (t >= 1), or > t
        int cnt = 0;
        if (in_regs) {
#pragma unroll
          for (int q = 0; q < kRegSlots; ++q) cnt += __popcll(__ballot(strictly ? mine[q] > t : mine[q] >= t));
        } else {
          for (int s0 = 0; s0 < C; s0 += 64) {
            const uint64_t k = s0 + lane < C ? keys[s0 + lane] : 0ull;
            cnt += __popcll(__ballot(strictly ? k > t : k >= t));
          }
        }
        return cnt;
      };
      uint64_t T = 0;
      for (int bit = 63; bit >= 0; --bit) {
        const uint64_t trial = T | (1ull << bit);
        if (reach(trial, false) >= P) T = trial;
      }
      const int ties = P - reach(T, true);         // >= 1 of the keys equal to T are kept
      int n = 0, neq = 0;
      for (int s0 = 0; s0 < C; s0 += 64) {
        const int s = s0 + lane;
        const uint64_t k = s < C ? keys[s] : 0ull;
        const uint16_t b = s < C ? cbin[s] : (uint16_t)0;
        const bool eq = s < C && k == T;
        const uint64_t beq = __ballot(eq);
        const bool sel = s < C && (k > T || (eq && neq + __popcll(beq & below) < ties));
        const uint64_t bsel = __ballot(sel);
        if (sel) {
          const int pos = n + __popcll(bsel & below);
          keys[pos] = k;
          cbin[pos] = b;
        }
        n += __popcll(bsel);
        neq += __popcll(beq);
      }
      __syncthreads();
      R = P;
    }
    // 3b. ranks: the peaks before s in (magnitude descending, bin ascending); the list is in bin order
    for (int s0 = 0; s0 < R; s0 += 64) {
      const int s = s0 + lane;
      const uint64_t k = s < R ? keys[s] : 0ull;
      int rank = 0;
#pragma unroll 4
      for (int j = 0; j < R; ++j) {
        const uint64_t kj = keys[j];
        rank += (kj > k || (kj == k && j < s)) ? 1 : 0;
      }
      if (s < R) sbin[rank] = cbin[s];
    }
    __syncthreads();
    if (a.count && lane == 0) a.count[f] = nsel;
    if (a.bin) {
      for (int r = lane; r < P; r += 64) {
        const int b = r < nsel ? sbin[r] : 0;
        const int64_t o = f * (int64_t)P + r;
        a.bin[o] = b;
        if (a.pmag) a.pmag[o] = r < nsel ? row[b] : 0.0;
        if (a.pfreq) a.pfreq[o] = r < nsel ? (double)b * a.freq_res : 0.0;
      }
    }
    if (a.hpcp) {
      // 4. hpcp[b] += weight * windowWeight, peak by peak, main then harmonics, bins ascending
      const int size = a.size;
      double h0 = 0.0, h1 = 0.0;
      for (int r = 0; r < nsel; ++r) {
        const int b = __builtin_amdgcn_readfirstlane((int)sbin[r]);
        const double m = row[b];
        const int e1 = a.row_start[b + 1];
        for (int e = a.row_start[b]; e < e1; ++e) {
          const int w = a.wbin[e];
          const double v = (m * a.factor[e]) * a.weight[e];
          if (w == lane) h0 = h0 + v;
          else if (w == lane + 64) h1 = h1 + v;
        }
      }
      if (a.non_linear) {   // applyNonLinearTransform (:330-336)
        if (h0 > 0.0) h0 = log(1.0 + h0);
        if (h1 > 0.0) h1 = log(1.0 + h1);
      }
      double* cur = prof;
      double* alt = prof + kProfSlots;
      cur[lane] = h0;
      cur[lane + 64] = h1;
      __syncthreads();
      if (a.normalized) {   // EnergyNormalize (common/math.go:116-137)
        double e = 0.0;
        for (int i = 0; i < size; ++i) e = e + cur[i] * cur[i];
        if (!(e < 1e-10) && size > 0) {
          const double nrm = __dsqrt_rn(e);
          h0 = __ddiv_rn(h0, nrm);
          h1 = __ddiv_rn(h1, nrm);
        }
        alt[lane] = h0;
        alt[lane + 64] = h1;
        __syncthreads();
        double* t = cur; cur = alt; alt = t;
      }
      if (a.max_shifted) {   // applyMaxShifted (:339-373)
        for (int sh = lane; sh < size; sh += 64) {
          double corr = 0.0;
          for (int i = 0; i < size; ++i) corr = corr + cur[i] * cur[(i + sh) % size];
          alt[sh] = corr;
        }
        __syncthreads();
        double best = 0.0;
        int shift = 0;
        for (int sh = 0; sh < size; ++sh)
          if (alt[sh] > best) { best = alt[sh]; shift = sh; }
        if (lane < size) h0 = cur[(lane + shift) % size];
        if (lane + 64 < size) h1 = cur[(lane + 64 + shift) % size];
        __syncthreads();
        alt[lane] = h0;
        alt[lane + 64] = h1;
        __syncthreads();
        double* t = cur; cur = alt; alt = t;
      }
      if (lane < size) a.hpcp[f * (int64_t)size + lane] = h0;
      if (lane + 64 < size) a.hpcp[f * (int64_t)size + lane + 64] = h1;
      if (lane == 0 && (a.energy || a.entropy)) {
        double e = 0.0, sum = 0.0;   // computeEnergy (:376-382), computeEntropy (:385-405)
        for (int i = 0; i < size; ++i) { e = e + cur[i] * cur[i]; sum = sum + cur[i]; }
        double ent = 0.0;
        if (sum != 0.0)
          for (int i = 0; i < size; ++i)
            if (cur[i] > 0.0) {
              const double p = __ddiv_rn(cur[i], sum);
              ent = ent - p * log2(p);
            }
        if (a.energy) a.energy[f] = __dsqrt_rn(e);
        if (a.entropy) a.entropy[f] = ent;
      }
    }
    __syncthreads();   // the next row rewrites the lists
  }
}

int launch_hpcp(const HpcpArgs& a, hipStream_t s) {
  if (a.F < 1) return 0;
  const int cmax = a.K > 2 ? (a.K - 1) / 2 : 0;
  if (a.K < 1 || a.K > HPCP_MAX_K || a.P < 0 || a.P > cmax || a.min_dist < 1) return -1;
  if (a.hpcp && (a.size < 1 || a.size > HPCP_MAX_SIZE || !a.row_start)) return -1;
  const size_t lds = (size_t)cmax * 8 + 2 * kProfSlots * 8 + 8 + (size_t)((cmax + 3) & ~3) * 2 + (size_t)a.P * 2 + 8;
  const unsigned grid = (unsigned)(a.F < (int64_t)(1 << 20) ? a.F : (int64_t)(1 << 20));
  hipLaunchKernelGGL(hpcp_rows_kernel, dim3(grid), dim3(64), lds, s, a);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // namespace sonar
