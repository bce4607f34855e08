// chroma_sim_kernels.hip -- ChromaSequenceSimilarity.ComputeSimilarity on the device
// (algorithms/chroma/chroma_similarity.go:86-538) over ChromaVectorAnalyzer.Distance / Similarity /
// CircularShift (chroma_vector.go:145-216) and the seven frame metrics (stats/distance.go:28-108,
// 247-294, 341-369).  All float64, built with -ffp-contract=off: the transposition, the Smith-Waterman
// traceback codes and the DTW path hang on unfused roundings.
//
//   chroma_prepare_kernel        per-row values and scalars, once per call and per circular shift
//   chroma_frame_matrix_kernel   Distance / Similarity of every (query, reference) pair + the epilogues
//   chroma_ordered_sum_kernel    the sampled means of findBestTransposition and the OTI totals, Go's order
//   chroma_dp_kernel             Smith-Waterman or the file's own DTW, one launch per tile anti-diagonal
//   chroma_sw_best_kernel        first row-major maximum of the score matrix
//   chroma_traceback_kernel      tracebackAlignment / tracebackDTW
#include <hip/hip_runtime.h>

#include <cstdint>

#include "go_math.h"
#include "kernels.h"
#include "wave.h"

namespace sonar {

namespace {

constexpr int T = CHROMA_DP_T;

// normalizeToProbability (distance.go:341-369) of v[0..dim) read through `at`, written to o
template <typename F>
__device__ __forceinline__ void normalize_prob(F at, int dim, double* o) {
  double sum = 0.0;
  for (int k = 0; k < dim; ++k) {
    const double v = at(k);
    if (v > 0) sum = sum + v;
  }
  const double uniform = 1.0 / (double)dim;
  for (int k = 0; k < dim; ++k) {
    const double v = at(k);
    o[k] = sum == 0 ? uniform : (v > 0 ? v / sum : 0.0);
  }
}

// A prepared row is 2 dim + 2 doubles: [0, dim) the metric's per-row values, [dim, 2 dim) JS's second
// normalisation, then two scalars.  Every entry is what Go recomputes per pair from that row alone, in
// Go's index order, so it has Go's bits:
//   Euclidean / Manhattan  the shifted values
//   Cosine                 the shifted values; normA, sqrt(normA)                  (distance.go:49-63)
//   Pearson                a[k] - meanA; sumSqA                                    (:80-99)
//   KL                     normalizeToProbability(a)                               (:250)
//   Hellinger              sqrt of it                                              (:284-289)
//   JS                     pNorm (for m) and normalizeToProbability(pNorm), what KLDivergenceFunc makes
//                          of its already normalised argument                      (:266, :276, :250)
// CircularShift (chroma_vector.go:207-216): value k of the shifted row is a[(k + shift) % dim].
__global__ __launch_bounds__(256) void chroma_prepare_kernel(const double* x, int64_t n, int dim, int metric, int shift0,
                                                             int nshift, double* out) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * nshift) return;
  const int shift = shift0 + (int)(idx / n);
  const double* a = x + (idx % n) * dim;
  double* o = out + idx * (2 * dim + 2);
  auto at = [&](int k) { return a[(k + shift) % dim]; };
  for (int k = dim; k < 2 * dim + 2; ++k) o[k] = 0.0;
  if (metric == CHROMA_COSINE) {
    double s = 0.0;
    for (int k = 0; k < dim; ++k) { const double v = at(k); o[k] = v; s = s + v * v; }
    o[2 * dim] = s;
    o[2 * dim + 1] = sqrt(s);
  } else if (metric == CHROMA_PEARSON) {
    double mean = 0.0, s = 0.0;
    for (int k = 0; k < dim; ++k) mean = mean + at(k);
    mean = mean / (double)dim;
    for (int k = 0; k < dim; ++k) { const double df = at(k) - mean; o[k] = df; s = s + df * df; }
    o[2 * dim] = s;
  } else if (metric == CHROMA_KL) {
    normalize_prob(at, dim, o);
  } else if (metric == CHROMA_HELLINGER) {
    normalize_prob(at, dim, o);
    for (int k = 0; k < dim; ++k) o[k] = sqrt(o[k]);
  } else if (metric == CHROMA_JS) {
    normalize_prob(at, dim, o);
    normalize_prob([&](int k) { return o[k]; }, dim, o + dim);
  } else {
    for (int k = 0; k < dim; ++k) o[k] = at(k);
  }
}

// ChromaVectorAnalyzer.Distance of two prepared rows (any address space), sums in Go's index order
template <int METRIC, typename QP, typename RP>
__device__ __forceinline__ double chroma_dist(QP qa, RP rb, int dim) {
  if constexpr (METRIC == CHROMA_MANHATTAN) {                     // distance.go:39-45
    double sum = 0.0;
    for (int k = 0; k < dim; ++k) sum = sum + __builtin_fabs(qa[k] - rb[k]);
    return sum;
  } else if constexpr (METRIC == CHROMA_COSINE) {                 // :48-65
    double dot = 0.0;
    for (int k = 0; k < dim; ++k) dot = dot + qa[k] * rb[k];
    if (qa[2 * dim] == 0 || rb[2 * dim] == 0) return 1.0;
    return 1.0 - dot / (qa[2 * dim + 1] * rb[2 * dim + 1]);
  } else if constexpr (METRIC == CHROMA_PEARSON) {                // :73-108, 1 - |corr|
    double num = 0.0;
    for (int k = 0; k < dim; ++k) num = num + qa[k] * rb[k];
    if (qa[2 * dim] == 0 || rb[2 * dim] == 0) return 1.0;
    return 1.0 - __builtin_fabs(num / sqrt(qa[2 * dim] * rb[2 * dim]));
  } else if constexpr (METRIC == CHROMA_KL) {                     // :248-261
    double kl = 0.0;
    for (int k = 0; k < dim; ++k) {
      const double p = qa[k], q = rb[k];
      if (p > 0 && q > 0) kl = kl + p * log(p / q);
    }
    return kl;
  } else if constexpr (METRIC == CHROMA_JS) {                     // :264-280
    // m = (pNorm + qNorm) / 2, then KLDivergenceFunc(pNorm, m) normalises both arguments again: the
    // row's second normalisation is prepared, m's is this pair's
    double msum = 0.0;
    for (int k = 0; k < dim; ++k) {
      const double m = (qa[k] + rb[k]) / 2.0;
      if (m > 0) msum = msum + m;
    }
    const double uniform = 1.0 / (double)dim;
    double kl1 = 0.0, kl2 = 0.0;
    for (int k = 0; k < dim; ++k) {
      const double m = (qa[k] + rb[k]) / 2.0;
      const double m2 = msum == 0 ? uniform : (m > 0 ? m / msum : 0.0);
      const double p = qa[dim + k], q = rb[dim + k];
      if (p > 0 && m2 > 0) kl1 = kl1 + p * log(p / m2);
      if (q > 0 && m2 > 0) kl2 = kl2 + q * log(q / m2);
    }
    return sqrt(0.5 * kl1 + 0.5 * kl2);
  } else if constexpr (METRIC == CHROMA_HELLINGER) {              // :283-294, math.Sqrt(2) rounded
    double sum = 0.0;
    for (int k = 0; k < dim; ++k) { const double df = qa[k] - rb[k]; sum = sum + df * df; }
    return sqrt(sum) / 1.4142135623730951;
  } else {                                                        // :29-36
    double sum = 0.0;
    for (int k = 0; k < dim; ++k) { const double df = qa[k] - rb[k]; sum = sum + df * df; }
    return sqrt(sum);
  }
}
// ChromaVectorAnalyzer.Similarity (chroma_vector.go:172-186)
template <int METRIC>
__device__ __forceinline__ double chroma_sim(double d) {
  if constexpr (METRIC == CHROMA_COSINE || METRIC == CHROMA_PEARSON) return 1.0 - (d / 2.0);
  else return exp(-d);
}

// A block computes 64 query rows x 64 reference rows: lane = reference row (column), each of the 4
// waves 16 query rows.  D = 12: both row tiles are staged in LDS (each frame is read from HBM once per
// tile), the lane's reference row then sits in registers and the query row is an LDS broadcast.  D = 0:
// the runtime dimension, rows straight from global memory (they stay in L2).
// Epilogue: band mask (OTI: zero outside |i - j| <= R), threshold (Binary) with an exact count, the
// NaN-skipping maximum from 0 (QMax), the block's tree sum (Direct's overall), the store when out != 0.
template <int METRIC, int D>
__global__ __launch_bounds__(256) void chroma_frame_matrix_kernel(ChromaMatArgs a) {
  constexpr int RL = 2 * D + 2, P = RL + 1;          // odd pitch: the lanes' row reads spread over the banks
  __shared__ double qs[D > 0 ? 64 * P : 1], rs[D > 0 ? 64 * P : 1];
  __shared__ double red[256];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t i0 = (int64_t)blockIdx.y * 64, j0 = (int64_t)blockIdx.x * 64;
  const int dim = D > 0 ? D : a.dim;
  const int rl = 2 * dim + 2;
  double rv[D > 0 ? RL : 1];
  if constexpr (D > 0) {
    for (int idx = tid; idx < 64 * RL; idx += 256) {
      const int row = idx / RL, k = idx % RL;
      qs[row * P + k] = i0 + row < a.nq ? a.qp[(i0 + row) * RL + k] : 0.0;
      rs[row * P + k] = j0 + row < a.nr ? a.rp[(j0 + row) * RL + k] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RL; ++k) rv[k] = rs[lane * P + k];
  }
  const int64_t j = j0 + lane;
  double sum = 0.0, mx = 0.0;
  unsigned long long cnt = 0;
  for (int u = 0; u < 16; ++u) {
    const int row = w * 16 + u;
    const int64_t i = i0 + row;
    if (i >= a.nq || j >= a.nr) continue;
    double v = 0.0;
    if (!a.banded || (j >= i - a.radius && j < i + a.radius + 1)) {
      double d;
      if constexpr (D > 0) d = chroma_dist<METRIC>(qs + row * P, rv, D);
      else d = chroma_dist<METRIC>(a.qp + i * rl, a.rp + j * rl, dim);
      v = a.mode ? chroma_sim<METRIC>(d) : d;
    }
    if (a.binary) {                                  // chroma_similarity.go:171-175
      const bool hit = v > a.thr;
      cnt += hit;
      v = hit ? 1.0 : 0.0;
    }
    if (v > mx) mx = v;                              // :382-390: strict, from 0; a NaN never wins
    sum = sum + v;
    if (a.out) a.out[i * a.nr + j] = v;
  }
  if (a.partial) {                                   // fixed tree: the same bits on every call
    red[tid] = sum;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
      if (tid < h) red[tid] = red[tid] + red[tid + h];
      __syncthreads();
    }
    if (tid == 0) a.partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = red[0];
  }
  for (int off = 32; off > 0; off >>= 1) {
    const double o = __shfl_xor(mx, off);
    if (o > mx) mx = o;
    cnt += __shfl_xor(cnt, off);
  }
  if (lane == 0) {
    // mx >= 0 and never NaN: its bit pattern orders as an unsigned integer
    if (a.maxbits && mx > 0) atomicMax(a.maxbits, (unsigned long long)__double_as_longlong(mx));
    if (a.count && cnt) atomicAdd(a.count, cnt);
  }
}

// sum of n partials by one block, fixed order
__global__ __launch_bounds__(256) void chroma_sum_partials_kernel(const double* p, int64_t n, double* out) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int64_t k = tid; k < n; k += 256) s = s + p[k];
  red[tid] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) red[tid] = red[tid] + red[tid + h];
    __syncthreads();
  }
  if (tid == 0) *out = red[0];
}

// The sums that decide BestTransposition, added in Go's order: one block of 16 waves per shift.
//   findBestTransposition (:450-479): rows i = 0, step, ...; columns j = 0, step, ...
//   OTI (:409-427):                   every row i; columns max(0, i - R) .. min(nr, i + R + 1) - 1
// A row's terms are cut into segments of Wc = min(widest row, 1024) slots and a round takes the next
// 1024 / Wc segments of the chain, one slot per thread in chain order: all 16 waves compute their
// similarities at once (the loads of a round overlap), then wave 0 adds the valid ones in order through
// lane broadcasts, every lane running the same chain.
template <int METRIC>
__global__ __launch_bounds__(1024) void chroma_ordered_sum_kernel(ChromaOrdArgs a) {
  __shared__ double vals[1024];
  __shared__ unsigned long long masks[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, shift = blockIdx.x;
  const int rl = 2 * a.dim + 2;
  const double* qp = a.qp + (int64_t)shift * a.nq * rl;
  int64_t W;                                          // the widest row, in terms
  if (a.banded) W = a.radius < 0 ? 0 : (2 * a.radius + 1 < a.nr ? 2 * a.radius + 1 : a.nr);
  else W = (a.nr + a.step - 1) / a.step;
  const int64_t nrows = (a.nq + a.step - 1) / a.step;
  double acc = 0.0;
  if (W > 0 && nrows > 0) {
    const int64_t Wc = W < 1024 ? W : 1024, cpr = (W + Wc - 1) / Wc, RR = 1024 / Wc, nseg = nrows * cpr;
    const int64_t g = tid / Wc, b = tid % Wc;
    for (int64_t s0 = 0; s0 < nseg; s0 += RR) {
      const int64_t sidx = s0 + g;
      bool valid = false;
      double v = 0.0;
      if (g < RR && sidx < nseg) {
        const int64_t i = (sidx / cpr) * a.step, bb = (sidx % cpr) * Wc + b;
        int64_t j;
        if (a.banded) {
          const int64_t lo = i - a.radius > 0 ? i - a.radius : 0;
          const int64_t hi = i + a.radius + 1 < a.nr ? i + a.radius + 1 : a.nr;
          j = lo + bb;
          valid = j < hi;
        } else {
          j = bb * a.step;
          valid = j < a.nr;
        }
        if (valid) v = chroma_sim<METRIC>(chroma_dist<METRIC>(qp + i * rl, a.rp + j * rl, a.dim));
      }
      vals[tid] = v;
      const unsigned long long m = __ballot(valid);
      if (lane == 0) masks[wave] = m;
      __syncthreads();
      if (wave == 0) {
        for (int k = 0; k < 16; ++k) {
          const unsigned long long mv = masks[k];
          const unsigned lo32 = __builtin_amdgcn_readfirstlane((unsigned)mv);
          const unsigned hi32 = __builtin_amdgcn_readfirstlane((unsigned)(mv >> 32));
          if ((lo32 | hi32) == 0) continue;
          const double x = vals[64 * k + lane];
#pragma unroll
          for (int t = 0; t < 32; ++t)
            if ((lo32 >> t) & 1) acc = acc + readlane_f64(x, t);
#pragma unroll
          for (int t = 0; t < 32; ++t)
            if ((hi32 >> t) & 1) acc = acc + readlane_f64(x, 32 + t);
        }
      }
      __syncthreads();
    }
  }
  if (tid == 0) a.totals[shift] = acc;
}

__global__ __launch_bounds__(256) void chroma_exp_neg_kernel(const double* in, int64_t n, double* out) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) out[k] = exp(-in[k]);
}

// One 64 x 64 tile of the recurrence per block (one wave), in place on M: a cell holds its frame
// similarity (SW) or distance (DTW) until the sweep replaces it by its score / accumulated cost.
// Lane l owns tile row l and at step s the column s - l, so the wave runs along the tile's
// anti-diagonal: `left` is the lane's previous value, `up` and `diag` come from lane l - 1 by a
// shuffle.  The tile, the row above it and the column left of it are read before the sweep (tiles of
// earlier launches: the kernel boundary is the only hand-off, no block waits on another).
//   SW  (:217-246): max(0, max(diag + sim, max(up - 0.1, left - 0.1))) with math.Max, the traceback
//        code by float equality in the order match, delete, insert (0 when none is equal), the
//        tile's best (score, first row-major index) with strict >.
//   DTW (:301-326): acc[0][0] = cost, first row / column cumulative, interior cost + min(up, min(left,
//        diag)) with math.Min; a column j >= 1 the band rule skips stays 0 in every row i >= 1.
template <bool DTW>
__global__ __launch_bounds__(64) void chroma_dp_kernel(ChromaDpArgs a, int64_t d, int64_t ti0) {
  __shared__ double tile[T][T + 2];
  __shared__ double top[T + 1];
  __shared__ uint8_t tbs[T][T];
  __shared__ uint8_t sk[T];
  const int l = threadIdx.x;
  const int64_t ti = ti0 + blockIdx.x, tj = d - ti;
  const int64_t a0 = ti * T, b0 = tj * T;
  const int rows = a.nq - a0 < T ? (int)(a.nq - a0) : T, cols = a.nr - b0 < T ? (int)(a.nr - b0) : T;
  const double edge = DTW ? __builtin_inf() : 0.0;   // outside the matrix
  if (l < cols)
    for (int rr = 0; rr < rows; ++rr) tile[rr][l] = a.M[(a0 + rr) * a.nr + b0 + l];
  for (int k = l; k <= cols; k += 64) {              // top[k] = value at (a0 - 1, b0 - 1 + k)
    const int64_t jj = b0 - 1 + k;
    top[k] = (a0 > 0 && jj >= 0) ? a.M[(a0 - 1) * a.nr + jj] : edge;
  }
  sk[l] = (DTW && a.skip && l < cols) ? a.skip[b0 + l] : 0;
  const double leftb = (b0 > 0 && l < rows) ? a.M[(a0 + l) * a.nr + b0 - 1] : edge;
  __syncthreads();
  const double left_above = __shfl_up(leftb, 1);
  double cur = 0.0, upn_prev = 0.0, bestv = 0.0;
  int bestc = -1;
  const int steps = rows + cols - 1;
  for (int s = 0; s < steps; ++s) {
    const double upn = __shfl_up(cur, 1);
    const int c = s - l;
    if (c >= 0 && c < cols && l < rows) {
      const double up = l == 0 ? top[c + 1] : upn;
      const double dg = l == 0 ? top[c] : (c == 0 ? left_above : upn_prev);
      const double lf = c == 0 ? leftb : cur;
      const double x = tile[l][c];
      double v;
      if constexpr (DTW) {
        const int64_t i = a0 + l, j = b0 + c;
        if (i == 0 && j == 0) v = x;
        else if (i > 0 && j > 0 && sk[c]) v = 0.0;
        else v = x + go_min(up, go_min(lf, dg));
      } else {
        const double match = dg + x, del = up - 0.1, ins = lf - 0.1;
        v = go_max(0.0, go_max(match, go_max(del, ins)));
        tbs[l][c] = v == match ? 1 : (v == del ? 2 : (v == ins ? 3 : 0));
        if (v > bestv) { bestv = v; bestc = c; }
      }
      tile[l][c] = v;
      cur = v;
    }
    upn_prev = upn;
  }
  __syncthreads();
  if (l < cols)
    for (int rr = 0; rr < rows; ++rr) {
      a.M[(a0 + rr) * a.nr + b0 + l] = tile[rr][l];
      if constexpr (!DTW) a.tb[(a0 + rr) * a.nr + b0 + l] = tbs[rr][l];
    }
  if constexpr (!DTW) {
    long long idx = bestc >= 0 ? (long long)((a0 + l) * a.nr + b0 + bestc) : INT64_MAX;
    for (int off = 32; off > 0; off >>= 1) {
      const double ov = __shfl_xor(bestv, off);
      const long long oi = __shfl_xor(idx, off);
      if (ov > bestv || (ov == bestv && oi < idx)) { bestv = ov; idx = oi; }
    }
    if (l == 0) {
      const int64_t t = ti * a.ntj + tj;
      a.tile_best[t] = bestv;
      a.tile_idx[t] = idx;
    }
  }
}

// the first cell in row-major order that holds the matrix maximum, when that is > 0 (:231-234);
// idx = -1 when nothing scores
__global__ __launch_bounds__(256) void chroma_sw_best_kernel(const double* tb, const int64_t* ti, int64_t n, double* best,
                                                            int64_t* idx) {
  __shared__ double bv[256];
  __shared__ long long bi[256];
  const int tid = threadIdx.x;
  double v = 0.0;
  long long x = INT64_MAX;
  for (int64_t k = tid; k < n; k += 256) {
    const double ov = tb[k];
    const long long oi = ti[k];
    if (ov > v || (ov == v && oi < x)) { v = ov; x = oi; }
  }
  bv[tid] = v; bi[tid] = x;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h && (bv[tid + h] > bv[tid] || (bv[tid + h] == bv[tid] && bi[tid + h] < bi[tid]))) {
      bv[tid] = bv[tid + h]; bi[tid] = bi[tid + h];
    }
    __syncthreads();
  }
  if (tid == 0) { *best = bv[0]; *idx = bv[0] > 0 ? bi[0] : -1; }
}

// tracebackAlignment (:482-507) / tracebackDTW (:510-538): one thread walks back from the end cell
// and writes the points back to front into arrays of `cap` entries; the path is their last *plen.
__global__ void chroma_traceback_kernel(const double* M, const uint8_t* tb, int64_t nq, int64_t nr, int dtw,
                                        const int64_t* start, int32_t* pq, int32_t* pr, double* ps, int64_t cap,
                                        int64_t* plen) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int64_t k = 0;
  if (dtw) {
    int64_t i = nq - 1, j = nr - 1;
    while ((i > 0 || j > 0) && k < cap) {
      const int64_t pos = cap - 1 - k;
      pq[pos] = (int32_t)i; pr[pos] = (int32_t)j; ps[pos] = M[i * nr + j];
      ++k;
      if (i == 0) --j;
      else if (j == 0) --i;
      else {
        const double dg = M[(i - 1) * nr + j - 1], up = M[(i - 1) * nr + j], lf = M[i * nr + j - 1];
        if (dg <= up && dg <= lf) { --i; --j; }
        else if (up <= lf) --i;
        else --j;
      }
    }
  } else if (*start >= 0) {
    int64_t i = *start / nr, j = *start % nr;        // the cell of scores[i + 1][j + 1]
    while (i >= 0 && j >= 0 && k < cap) {
      const double s = M[i * nr + j];
      if (!(s > 0)) break;
      const int64_t pos = cap - 1 - k;
      pq[pos] = (int32_t)i; pr[pos] = (int32_t)j; ps[pos] = s;
      ++k;
      const int code = tb[i * nr + j];
      if (code == 1) { --i; --j; }
      else if (code == 2) --i;
      else if (code == 3) --j;
      else break;
    }
  }
  *plen = k;
}

template <int D>
int launch_matrix_d(const ChromaMatArgs& a, dim3 grid, hipStream_t s) {
  switch (a.metric) {
#define SONAR_CM(M) case M: hipLaunchKernelGGL((chroma_frame_matrix_kernel<M, D>), grid, dim3(256), 0, s, a); break
    SONAR_CM(CHROMA_MANHATTAN); SONAR_CM(CHROMA_COSINE); SONAR_CM(CHROMA_PEARSON); SONAR_CM(CHROMA_KL);
    SONAR_CM(CHROMA_JS); SONAR_CM(CHROMA_HELLINGER);
    default: hipLaunchKernelGGL((chroma_frame_matrix_kernel<CHROMA_EUCLIDEAN, D>), grid, dim3(256), 0, s, a); break;
#undef SONAR_CM
  }
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace

int launch_chroma_prepare(const double* x, int64_t n, int dim, int metric, int shift0, int nshift, double* out,
                          hipStream_t s) {
  if (n <= 0 || nshift <= 0) return 0;
  const int64_t total = n * nshift;
  if ((total + 255) / 256 > INT32_MAX) return -1;
  hipLaunchKernelGGL(chroma_prepare_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, n, dim, metric,
                     shift0, nshift, out);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int64_t chroma_matrix_blocks(int64_t nq, int64_t nr) { return ((nq + 63) / 64) * ((nr + 63) / 64); }

int launch_chroma_matrix(const ChromaMatArgs& a, hipStream_t s) {
  if (a.nq <= 0 || a.nr <= 0) return 0;
  const int64_t gy = (a.nq + 63) / 64, gx = (a.nr + 63) / 64;
  if (gy > 65535 || gx > INT32_MAX) return -1;
  const dim3 grid((unsigned)gx, (unsigned)gy);
  return a.dim == 12 ? launch_matrix_d<12>(a, grid, s) : launch_matrix_d<0>(a, grid, s);
}

int launch_chroma_sum_partials(const double* p, int64_t n, double* out, hipStream_t s) {
  hipLaunchKernelGGL(chroma_sum_partials_kernel, dim3(1), dim3(256), 0, s, p, n, out);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_chroma_ordered(const ChromaOrdArgs& a, hipStream_t s) {
  switch (a.metric) {
#define SONAR_CO(M) case M: hipLaunchKernelGGL((chroma_ordered_sum_kernel<M>), dim3(12), dim3(1024), 0, s, a); break
    SONAR_CO(CHROMA_MANHATTAN); SONAR_CO(CHROMA_COSINE); SONAR_CO(CHROMA_PEARSON); SONAR_CO(CHROMA_KL);
    SONAR_CO(CHROMA_JS); SONAR_CO(CHROMA_HELLINGER);
    default: hipLaunchKernelGGL((chroma_ordered_sum_kernel<CHROMA_EUCLIDEAN>), dim3(12), dim3(1024), 0, s, a); break;
#undef SONAR_CO
  }
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_chroma_exp_neg(const double* in, int64_t n, double* out, hipStream_t s) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(chroma_exp_neg_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, n, out);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_chroma_dp(const ChromaDpArgs& a, hipStream_t s) {
  const int64_t nti = (a.nq + T - 1) / T, ntj = (a.nr + T - 1) / T;
  if (nti <= 0 || ntj <= 0 || a.ntj != ntj) return -1;
  for (int64_t d = 0; d < nti + ntj - 1; ++d) {
    const int64_t lo = d - (ntj - 1) > 0 ? d - (ntj - 1) : 0, hi = d < nti - 1 ? d : nti - 1;
    const dim3 grid((unsigned)(hi - lo + 1));
    if (a.dtw) hipLaunchKernelGGL((chroma_dp_kernel<true>), grid, dim3(64), 0, s, a, d, lo);
    else hipLaunchKernelGGL((chroma_dp_kernel<false>), grid, dim3(64), 0, s, a, d, lo);
  }
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_chroma_sw_best(const double* tile_best, const int64_t* tile_idx, int64_t ntiles, double* best, int64_t* idx,
                          hipStream_t s) {
  hipLaunchKernelGGL(chroma_sw_best_kernel, dim3(1), dim3(256), 0, s, tile_best, tile_idx, ntiles, best, idx);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_chroma_traceback(const double* M, const uint8_t* tb, int64_t nq, int64_t nr, int dtw, const int64_t* start,
                            int32_t* pq, int32_t* pr, double* ps, int64_t cap, int64_t* plen, hipStream_t s) {
  hipLaunchKernelGGL(chroma_traceback_kernel, dim3(1), dim3(64), 0, s, M, tb, nq, nr, dtw, start, pq, pr, ps, cap, plen);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace sonar
