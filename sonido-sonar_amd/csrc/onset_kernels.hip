// onset_kernels.hip -- OnsetDetection and TempoEstimation (algorithms/temporal/onset_detection.go,
// tempo_estimation.go) over spectral/spectral_flux.go and temporal/envelope.go, float64 like the Go
// reference.  Every value here feeds a comparison (a strict local maximum, a threshold, a vote), so
// every sum keeps the reference's order and this file is built without FMA contraction.
//
//  1. onset_flux_kernel: SpectralFlux.Compute / ComputeAllChanges (spectral_flux.go:17-56).  A wave owns
//     64 consecutive outputs, that is 65 consecutive rows; tiles of 65 rows x 32 columns go through LDS
//     and lane r adds the squared differences of rows r and r + 1 in bin order.  Every row is read from
//     memory once by its wave, except the one row two neighbouring waves share (an L2 hit).  It is
//     hps_energy_kernel's row-per-lane layout, which was the faster of the two measured there from two
//     waves per CU on; an onset curve is wanted for whole recordings, not for a handful of rows.
//  2. onset_rms_kernel: Envelope.ComputeRMS (envelope.go:18-43), the same layout with rows that overlap
//     in memory (row f starts at f * hop): a half wave loads 32 consecutive samples of one frame.
//  3. onset_candidates_kernel + onset_pick_kernel: findFluxPeaks (onset_detection.go:97-120).  The
//     candidates (strict local maximum, >= threshold) are a bit per frame, one 64-bit word per wave, all
//     CUs.  One block then takes the words through LDS a tile at a time.  Below 3 frames of minimum
//     interval the greedy never rejects and nothing walks.  From 3 to 16 every thread tabulates what its
//     256 frames do to the chain for each state the chain can arrive in, and one thread threads the
//     state through the tables; above 16 one thread walks the set bits with find-first-set (a word that
//     lies wholly inside the dead interval costs one comparison).  The kept bits are compacted in order
//     by a block scan over the words' population counts.
//  4. onset_threshold_kernel: AdaptiveThreshold (:200-222), two ordered passes, one lane adding out of LDS.
//  5. onset_autocorr_kernel: calculateAutocorrelation (tempo_estimation.go:121-150), a lag per lane, the
//     sum in ascending i as ncc_lags_kernel (ncc_kernels.hip) does it; onset_autocorr_norm_kernel is
//     the reference's in-place "normalisation" (:143-147) written out.
#include <cstdint>

#include "kernels.h"

namespace sonar {

namespace {

constexpr int kTileRows = 64, kTileCols = 32;   // outputs per wave, columns per tile
constexpr int kPickThreads = 1024, kPickWordsPerThread = 4;
constexpr int kPickTileWords = kPickThreads * kPickWordsPerThread;   // 4,096 words: 262,144 frames, 32 KB
constexpr int kPickTableMif = 16;   // the largest minimum interval the tabled greedy takes
constexpr int kSumTile = 2048;
constexpr int kLagBatch = 16;   // products of one lag whose loads are issued together

}  // namespace

__global__ __launch_bounds__(64) void onset_flux_kernel(const double* mag, int64_t F, int K, int all_changes, double* flux) {
  __shared__ double tile[kTileRows + 1][kTileCols + 1];
  const int lane = threadIdx.x;
  const int half = lane >> 5, col = lane & 31;
  const int64_t nout = F - 1;
  for (int64_t r0 = (int64_t)blockIdx.x * kTileRows; r0 < nout; r0 += (int64_t)gridDim.x * kTileRows) {
    const int outs = nout - r0 < kTileRows ? (int)(nout - r0) : kTileRows;   // rows r0 .. r0 + outs
    double t = 0.0;
    for (int c0 = 0; c0 < K; c0 += kTileCols) {
      const double* src = mag + (r0 + half) * (int64_t)K + c0 + col;
      const bool in_row = c0 + col < K;
      double v[kTileRows / 2 + 1];
#pragma unroll
      for (int j = 0; j <= kTileRows / 2; ++j) v[j] = (in_row && 2 * j + half <= outs) ? src[(int64_t)(2 * j) * K] : 0.0;
      __syncthreads();   // the previous tile's chains are done
#pragma unroll
      for (int j = 0; j <= kTileRows / 2; ++j)
        if (2 * j + half <= kTileRows) tile[2 * j + half][col] = v[j];
      __syncthreads();
      const int w = K - c0 < kTileCols ? K - c0 : kTileCols;
      for (int c = 0; c < w; ++c) {
        const double d = tile[lane + 1][c] - tile[lane][c];
        if (all_changes || d > 0.0) t = t + d * d;   // a NaN difference is not > 0 (:28)
      }
    }
    if (lane < outs) flux[r0 + lane] = __dsqrt_rn(t);
  }
}

__global__ __launch_bounds__(64) void onset_rms_kernel(const double* x, int64_t frames, int frame, int hop, double* env) {
  __shared__ double tile[kTileRows][kTileCols + 1];
  const int lane = threadIdx.x;
  const int half = lane >> 5, col = lane & 31;
  for (int64_t r0 = (int64_t)blockIdx.x * kTileRows; r0 < frames; r0 += (int64_t)gridDim.x * kTileRows) {
    const int rows = frames - r0 < kTileRows ? (int)(frames - r0) : kTileRows;
    double t = 0.0;
    for (int c0 = 0; c0 < frame; c0 += kTileCols) {
      const double* src = x + (r0 + half) * (int64_t)hop + c0 + col;
      const bool in_row = c0 + col < frame;
      double v[kTileRows / 2];
#pragma unroll
      for (int j = 0; j < kTileRows / 2; ++j) v[j] = (in_row && 2 * j + half < rows) ? src[(int64_t)(2 * j) * hop] : 0.0;
      __syncthreads();
#pragma unroll
      for (int j = 0; j < kTileRows / 2; ++j) tile[2 * j + half][col] = v[j] * v[j];
      __syncthreads();
      const int w = frame - c0 < kTileCols ? frame - c0 : kTileCols;
      for (int c = 0; c < w; ++c) t = t + tile[lane][c];
    }
    if (lane < rows) env[r0 + lane] = __dsqrt_rn(__ddiv_rn(t, (double)frame));
  }
}

// energyDiff of DetectOnsetsEnergy (:74-82): the `if`, so a NaN difference gives 0
__global__ __launch_bounds__(256) void onset_posdiff_kernel(const double* env, int64_t n, double* diff) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const double d = env[i + 1] - env[i];
    diff[i] = d > 0.0 ? d : 0.0;
  }
}

// bit i of the mask: 1 <= i <= n - 2, v[i] > v[i-1], v[i] > v[i+1], v[i] >= thr.  A wave per word.
__global__ __launch_bounds__(256) void onset_candidates_kernel(const double* v, int64_t n, double thr, uint64_t* mask,
                                                                int64_t nwords) {
  const int lane = threadIdx.x & 63;
  for (int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); w < nwords; w += (int64_t)gridDim.x * 4) {
    const int64_t i = w * 64 + lane;
    bool cand = false;
    if (i >= 1 && i < n - 1) {
      const double a = v[i];
      cand = a > v[i - 1] && a > v[i + 1] && a >= thr;
    }
    const uint64_t b = __ballot(cand);
    if (lane == 0) mask[w] = b;
  }
}

// The greedy over one thread's run of kPickWordsPerThread words.  `dead` is how many frames at the start
// of the run are still closer than mif to the last frame kept before it (0 .. mif - 1); the result is
// the same number for the run after it.  With write, m becomes the kept bits.
__device__ inline int pick_walk_run(uint64_t (&m)[kPickWordsPerThread], int dead, int mif, bool write) {
  int next = dead;   // the first offset in the run that can be kept
#pragma unroll
  for (int q = 0; q < kPickWordsPerThread; ++q) {
    uint64_t mm = m[q], keep = 0;
    while (true) {
      const int sh = next - q * 64;
      if (sh >= 64) mm = 0;
      else if (sh > 0) mm &= ~0ull << sh;
      if (!mm) break;
      const int b = __ffsll((unsigned long long)mm) - 1;
      keep |= 1ull << b;
      next = q * 64 + b + mif;
    }
    if (write) m[q] = keep;
  }
  return next > kPickWordsPerThread * 64 ? next - kPickWordsPerThread * 64 : 0;
}

// One block.  index[k] = frame * scale for the kept frames in ascending order (k < width), *count = how many.
// The greedy has two forms.  Up to kPickTableMif frames of minimum interval, what a run of 256 frames
// does to the chain depends only on `dead` above, so every thread tabulates its run for each of the mif
// possible values, thread 0 threads the true value through the 1,024 tables (one LDS lookup per run
// instead of one step per candidate), and every thread then walks its run once more with its value.
// Above it, thread 0 walks the words itself: most of them lie inside a dead interval and cost one
// comparison.
__global__ __launch_bounds__(kPickThreads) void onset_pick_kernel(const uint64_t* mask, int64_t nwords, int32_t mif,
                                                                  int64_t scale, int64_t* index, int64_t width,
                                                                  int64_t* count) {
  __shared__ uint64_t words[kPickTileWords];
  __shared__ int scan[kPickThreads];
  __shared__ unsigned char table[kPickThreads * kPickTableMif];
  __shared__ unsigned char dead_in[kPickThreads];
  const int tid = threadIdx.x;
  const bool tabled = mif > 2 && mif <= kPickTableMif;
  int64_t last = -(int64_t)mif;   // lastPeakFrame (:106); thread 0's, the serial form
  int carry = 0;                  // `dead` of the tile's first run; thread 0's, the tabled form
  int64_t kept = 0;
  for (int64_t w0 = 0; w0 < nwords; w0 += kPickTileWords) {
    const int nw = nwords - w0 < kPickTileWords ? (int)(nwords - w0) : kPickTileWords;
    for (int j = tid; j < kPickTileWords; j += kPickThreads) words[j] = j < nw ? mask[w0 + j] : 0;
    __syncthreads();
    if (mif > kPickTableMif && tid == 0) {   // strict maxima are 2 apart: the rule acts from 3 on
      for (int w = 0; w < nw; ++w) {
        uint64_t m = words[w];
        if (!m) continue;
        const int64_t b0 = (w0 + w) * 64;
        if (b0 + 63 - last < mif) { words[w] = 0; continue; }
        uint64_t keep = 0;
        while (m) {
          const int b = __ffsll((unsigned long long)m) - 1;
          if (b0 + b - last >= mif) {
            keep |= 1ull << b;
            last = b0 + b;
            const int64_t nb = (int64_t)b + mif;   // the next frame that can be kept
            m = nb >= 64 ? 0 : m & (~0ull << nb);
          } else {
            m &= m - 1;
          }
        }
        words[w] = keep;
      }
    }
    __syncthreads();
    uint64_t m[kPickWordsPerThread];
    int cnt = 0;
#pragma unroll
    for (int q = 0; q < kPickWordsPerThread; ++q) {
      m[q] = words[tid * kPickWordsPerThread + q];
    }
    if (tabled) {
      for (int d = 0; d < mif; ++d) table[tid * kPickTableMif + d] = (unsigned char)pick_walk_run(m, d, mif, false);
      __syncthreads();
      if (tid == 0) {
        const int runs = (nw + kPickWordsPerThread - 1) / kPickWordsPerThread;   // the runs after them are empty
        int d = carry;
        for (int t = 0; t < runs; ++t) {
          dead_in[t] = (unsigned char)d;
          d = table[t * kPickTableMif + d];
        }
        for (int t = runs; t < kPickThreads; ++t) dead_in[t] = 0;
        carry = d;
      }
      __syncthreads();
      pick_walk_run(m, dead_in[tid], mif, true);
    }
#pragma unroll
    for (int q = 0; q < kPickWordsPerThread; ++q) cnt += __popcll(m[q]);
    scan[tid] = cnt;
    __syncthreads();
    for (int off = 1; off < kPickThreads; off <<= 1) {
      const int a = tid >= off ? scan[tid - off] : 0;
      __syncthreads();
      scan[tid] += a;
      __syncthreads();
    }
    int64_t pos = kept + scan[tid] - cnt;
    kept += scan[kPickThreads - 1];
#pragma unroll
    for (int q = 0; q < kPickWordsPerThread; ++q) {
      uint64_t mm = m[q];
      while (mm) {
        const int b = __ffsll((unsigned long long)mm) - 1;
        mm &= mm - 1;
        if (pos < width) index[pos] = ((w0 + tid * kPickWordsPerThread + q) * 64 + b) * scale;
        ++pos;
      }
    }
    __syncthreads();   // the next tile rewrites words and scan
  }
  if (tid == 0) *count = kept;
}

// mean + 2 * population standard deviation, both sums in index order (:206-221); n >= 1
__global__ __launch_bounds__(256) void onset_threshold_kernel(const double* v, int64_t n, double* out) {
  __shared__ double t[kSumTile];
  __shared__ double mean_s;
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int pass = 0; pass < 2; ++pass) {
    const double mean = pass ? mean_s : 0.0;
    acc = 0.0;
    for (int64_t i0 = 0; i0 < n; i0 += kSumTile) {
      const int w = n - i0 < kSumTile ? (int)(n - i0) : kSumTile;
      for (int j = tid; j < w; j += 256) t[j] = v[i0 + j];
      __syncthreads();
      if (tid == 0) {
        if (pass == 0) {
          for (int j = 0; j < w; ++j) acc = acc + t[j];
        } else {
          for (int j = 0; j < w; ++j) {
            const double d = t[j] - mean;
            acc = acc + d * d;
          }
        }
      }
      __syncthreads();
    }
    if (tid == 0) {
      if (pass == 0) mean_s = __ddiv_rn(acc, (double)n);
      else *out = mean + 2.0 * __dsqrt_rn(__ddiv_rn(acc, (double)n));
    }
    __syncthreads();
  }
}

// raw[t] = (sum over i < L - lag of e[i] * e[i + lag]) / float64(L - lag); lag = lag_lo + t, or with
// zero_first lag 0 for t == 0 and lag_lo + t - 1 after it.  Every lag is below L.
__global__ __launch_bounds__(64) void onset_autocorr_kernel(const double* e, int64_t L, int64_t lag_lo, int64_t nlags,
                                                            int zero_first, double* raw) {
  const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (t >= nlags) return;
  const int64_t lag = zero_first ? (t == 0 ? 0 : lag_lo + t - 1) : lag_lo + t;
  const int64_t m = L - lag;
  double s = 0.0;
  int64_t i = 0;
  for (; i + kLagBatch <= m; i += kLagBatch) {   // the loads of a batch first, then its links of the chain
    double a[kLagBatch], b[kLagBatch];
#pragma unroll
    for (int u = 0; u < kLagBatch; ++u) {
      a[u] = e[i + u];
      b[u] = e[i + u + lag];
    }
#pragma unroll
    for (int u = 0; u < kLagBatch; ++u) s = s + a[u] * b[u];
  }
  for (; i < m; ++i) s = s + e[i] * e[i + lag];
  raw[t] = __ddiv_rn(s, (double)m);
}

// `for i := range autocorr { autocorr[i] /= autocorr[0] }` when autocorr[0] > 0 (:143-147): the first
// step makes autocorr[0] its own quotient and every later step divides by that
__global__ __launch_bounds__(256) void onset_autocorr_norm_kernel(const double* raw, int64_t n, double* ac) {
  const double a0 = raw[0];
  const bool norm = a0 > 0.0;
  const double q = __ddiv_rn(a0, a0);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    ac[i] = !norm ? raw[i] : i == 0 ? q : __ddiv_rn(raw[i], q);
}

namespace {
unsigned blocks_for(int64_t items, int per_block) {
  const int64_t b = (items + per_block - 1) / per_block;
  return (unsigned)(b < 1 ? 1 : b < (int64_t)(1 << 20) ? b : (int64_t)(1 << 20));
}
int launched() { return hipGetLastError() == hipSuccess ? 0 : -5; }
}  // namespace

int launch_onset_flux(const double* mag, int64_t F, int K, bool all_changes, double* flux, hipStream_t s) {
  if (F < 2) return 0;
  if (K < 0 || K > ONSET_MAX_K || !flux || (K > 0 && !mag)) return -1;
  hipLaunchKernelGGL(onset_flux_kernel, dim3(blocks_for(F - 1, kTileRows)), dim3(64), 0, s, mag, F, K,
                     all_changes ? 1 : 0, flux);
  return launched();
}

int launch_onset_rms(const double* x, int64_t frames, int frame, int hop, double* env, hipStream_t s) {
  if (frames < 1) return 0;
  if (frame < 1 || hop < 1 || !x || !env) return -1;
  hipLaunchKernelGGL(onset_rms_kernel, dim3(blocks_for(frames, kTileRows)), dim3(64), 0, s, x, frames, frame, hop, env);
  return launched();
}

int launch_onset_posdiff(const double* env, int64_t n, double* diff, hipStream_t s) {
  if (n < 1) return 0;
  if (!env || !diff) return -1;
  hipLaunchKernelGGL(onset_posdiff_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, s, env, n, diff);
  return launched();
}

int64_t onset_mask_words(int64_t n) { return n > 0 ? (n + 63) / 64 : 0; }

int launch_onset_peaks(const double* v, int64_t n, double threshold, int32_t min_interval_frames, int64_t scale,
                       uint64_t* mask, int64_t* index, int64_t width, int64_t* count, hipStream_t s) {
  if (!count || (width > 0 && !index)) return -1;
  const int64_t nwords = n >= 3 ? onset_mask_words(n) : 0;   // fewer than 3 values give nothing (:98-100)
  if (nwords > 0) {
    if (!v || !mask) return -1;
    hipLaunchKernelGGL(onset_candidates_kernel, dim3(blocks_for(nwords, 4)), dim3(256), 0, s, v, n, threshold, mask, nwords);
    if (launched() != 0) return -5;
  }
  hipLaunchKernelGGL(onset_pick_kernel, dim3(1), dim3(kPickThreads), 0, s, mask, nwords, min_interval_frames, scale, index,
                     width, count);
  return launched();
}

int launch_onset_threshold(const double* v, int64_t n, double* value, hipStream_t s) {
  if (n < 1 || !v || !value) return -1;
  hipLaunchKernelGGL(onset_threshold_kernel, dim3(1), dim3(256), 0, s, v, n, value);
  return launched();
}

int launch_onset_autocorr(const double* e, int64_t L, int64_t lag_lo, int64_t nlags, bool zero_first, double* raw,
                          hipStream_t s) {
  if (nlags < 1) return 0;
  const int64_t top = zero_first ? lag_lo + nlags - 2 : lag_lo + nlags - 1;   // the largest lag
  if (!e || !raw || lag_lo < 0 || top >= L || L < 1 || nlags > (int64_t)64 * (1 << 20)) return -1;
  hipLaunchKernelGGL(onset_autocorr_kernel, dim3(blocks_for(nlags, 64)), dim3(64), 0, s, e, L, lag_lo, nlags,
                     zero_first ? 1 : 0, raw);
  return launched();
}

int launch_onset_autocorr_norm(const double* raw, int64_t n, double* ac, hipStream_t s) {
  if (n < 1) return 0;
  if (!raw || !ac) return -1;
  hipLaunchKernelGGL(onset_autocorr_norm_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, s, raw, n, ac);
  return launched();
}

}  // namespace sonar
