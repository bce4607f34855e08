// key_kernels.hip -- KeyEstimator (algorithms/tonal/key_estimation.go) over a device chromagram:
// EstimateKey per row (:196-233), and the order-dependent parts of EstimateKeySequence (:250-270) and
// KeyEstimationBatch (:896-1005).  All float64 like the Go reference; every key, mode, threshold and
// modulation is decided from a rounding here, so this file is built without FMA contraction.
//
//   key_rows_kernel       one lane per row: the row is staged through LDS (the global reads of a block's
//                         64 rows are contiguous), resized, preprocessed, correlated with the 24 shifted
//                         profiles, ranked and thresholded.  With window == 10 the staged row is the
//                         in-order mean of ten chroma rows (detectModulations' window).
//   key_colsum_kernel     computeAverageChroma: one block; waves 1..15 stage the next tile of rows while
//                         wave 0 runs one serial chain per bin over the current one
//   key_votes_kernel      GetGlobalKey: the same shape, 24 vote chains and the total's
//   key_stability_kernel  findMode's histogram (integer, order-free) and the share of the mode
//   key_compact_kernel    the modulation positions / the transition records, compacted in ascending
//                         order by one block (ballot + wave counts)
// No kernel waits on another block.
#include <cstdint>
#include <type_traits>

#include "go_math.h"
#include "kernels.h"

namespace sonar {

namespace {

// The row-to-result computation: p holds the resized row (hs values, a lane's own LDS) and leaves it
// preprocessed; s receives the 24 scores [12 major | 12 minor].
struct KeyRowOut {
  int code;            // key * 2 + mode of the first candidate
  double best;         // its score: Strength, and Confidence before the threshold
  double clarity, ambiguity, tonality;
};

__device__ __forceinline__ void key_estimate_row(const KeyArgs& a, double* p, double (&s)[24], int32_t* cand,
                                                 KeyRowOut& o) {
  const int hs = a.hs;
  if (a.normalize) {   // energyNormalize (common/normalization.go:113-134)
    double e = 0.0;
    for (int i = 0; i < hs; ++i) e = e + p[i] * p[i];
    if (!(e < 1e-10)) {
      const double nrm = __dsqrt_rn(e);
      for (int i = 0; i < hs; ++i) p[i] = __ddiv_rn(p[i], nrm);
    }
  }
  if (a.remove_mean) {   // removeMean (:487-498)
    double sum = 0.0;
    for (int i = 0; i < hs; ++i) sum = sum + p[i];
    const double mean = __ddiv_rn(sum, (double)hs);
    for (int i = 0; i < hs; ++i) p[i] = p[i] - mean;
  }
  if (a.binary) {   // applyBinaryThreshold (:500-515)
    double sum = 0.0;
    for (int i = 0; i < hs; ++i) sum = sum + p[i];
    const double thr = __ddiv_rn(sum, (double)hs);
    for (int i = 0; i < hs; ++i) p[i] = p[i] > thr ? 1.0 : 0.0;
  }
  // estimateKeyProfile (:300-370) over PearsonCorrelationFunc (stats/distance.go:111-145): meanA, diffA
  // and sumSqA are the row's own, the same for all 24 keys
  if (hs == 12) {
    double mean_a = 0.0;
#pragma unroll
    for (int i = 0; i < 12; ++i) mean_a = mean_a + p[i];
    mean_a = __ddiv_rn(mean_a, 12.0);
    double da[12];
    double ssa = 0.0;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      da[i] = p[i] - mean_a;
      ssa = ssa + da[i] * da[i];
    }
#pragma unroll
    for (int j = 0; j < 24; ++j) {
      const double* t = a.tab + j * KEY_TAB_ROW;
      double num = 0.0;
#pragma unroll
      for (int i = 0; i < 12; ++i) num = num + da[i] * t[i];
      const double ssb = t[12];
      s[j] = (ssa == 0.0 || ssb == 0.0) ? 0.0 : __ddiv_rn(num, __dsqrt_rn(ssa * ssb));
    }
  } else {   // correlateWithProfile's length test (:388-390)
#pragma unroll
    for (int j = 0; j < 24; ++j) s[j] = 0.0;
  }
  // the candidates in creation order c = key * 2 + mode; rank = those that sort before c
  int best = 0;
  double s0 = 0.0, s1 = 0.0;
#pragma unroll
  for (int c = 0; c < 24; ++c) {
    const double sc = s[(c & 1) * 12 + (c >> 1)];
    int rank = 0;
#pragma unroll
    for (int d = 0; d < 24; ++d) {
      const double sd = s[(d & 1) * 12 + (d >> 1)];
      rank += (sd > sc || (sd == sc && d < c)) ? 1 : 0;
    }
    if (rank == 0) { best = c; s0 = sc; }
    if (rank == 1) s1 = sc;
    if (cand && rank < a.ncand) cand[rank] = c;
  }
  o.code = best;
  o.best = s0;
  o.clarity = s0 > 0.0 ? __ddiv_rn(s0 - s1, s0) : 0.0;   // calculateClarity (:517-533)
  double sum = 0.0;                                       // calculateAmbiguity (:535-559)
#pragma unroll
  for (int j = 0; j < 24; ++j)
    if (s[j] > 0.0) sum = sum + s[j];
  double amb = 0.0;
  if (sum != 0.0) {
    double ent = 0.0;
#pragma unroll
    for (int j = 0; j < 24; ++j)
      if (s[j] > 0.0) {
        const double prob = __ddiv_rn(s[j], sum);
        ent = ent - prob * go_log2(prob);
      }
    amb = __ddiv_rn(ent, a.log2_24);
  }
  o.ambiguity = amb;
  // calculateTonality (:688-692) over computeUniformity (chroma_vector.go:385-408)
  double tot = 0.0;
  for (int i = 0; i < hs; ++i) tot = tot + p[i];
  double uni = 1.0;
  if (tot != 0.0) {
    const double expected = __ddiv_rn(tot, (double)hs);
    double var = 0.0;
    for (int i = 0; i < hs; ++i) {
      const double d = p[i] - expected;
      var = var + d * d;
    }
    var = __ddiv_rn(var, (double)hs);
    uni = __ddiv_rn(1.0, 1.0 + var);
  }
  o.tonality = 1.0 - uni;
}

}  // namespace

// LDS: 64 rows of sd = max(hs | 1, 25) doubles (an odd stride; 25 holds a row's scores on the way out)
__global__ __launch_bounds__(64) void key_rows_kernel(KeyArgs a) {
  extern __shared__ double tile[];
  const int lane = threadIdx.x;
  const int hs = a.hs, dim = a.dim;
  const int sd = (hs | 1) > 25 ? (hs | 1) : 25;
  const int64_t f0 = (int64_t)blockIdx.x * 64;
  const int nrows = a.F - f0 < 64 ? (int)(a.F - f0) : 64;
  bool bad = false;
  for (int t = lane; t < nrows * hs; t += 64) {
    const int r = t / hs, i = t - r * hs;
    const int src = a.ridx ? a.ridx[i] : i;
    double v = 0.0;
    if (src >= 0) {
      if (a.window) {   // computeAverageChroma of rows f + 5 .. f + 14 (:636-641)
        const double* q = a.chroma + (f0 + r + 5) * (int64_t)dim + src;
        double sum = 0.0;
        for (int w = 0; w < 10; ++w) sum = sum + q[(int64_t)w * dim];
        v = __ddiv_rn(sum, 10.0);
      } else {
        v = a.chroma[(f0 + r) * (int64_t)dim + src];
      }
      bad = bad || !(fabs(v) <= 1.79769313486231570815e+308);
    }
    tile[r * sd + i] = v;
  }
  if (bad && a.nonfinite) atomicOr(a.nonfinite, 1);
  __syncthreads();
  const bool active = lane < nrows;
  const int64_t f = f0 + lane;
  double s[24];
  if (active) {
    KeyRowOut o;
    key_estimate_row(a, tile + lane * sd, s, a.cand ? a.cand + f * a.ncand : nullptr, o);
    const bool below = o.best < a.min_conf;   // postProcessResult (:675-686)
    if (a.key) a.key[f] = o.code >> 1;
    if (a.mode) a.mode[f] = o.code & 1;
    if (a.code) a.code[f] = o.code;
    if (a.known) a.known[f] = below ? 0 : 1;
    if (a.conf) a.conf[f] = below ? 0.0 : o.best;
    if (a.strength) a.strength[f] = o.best;
    if (a.clarity) a.clarity[f] = o.clarity;
    if (a.ambiguity) a.ambiguity[f] = o.ambiguity;
    if (a.tonality) a.tonality[f] = o.tonality;
  }
  if (a.processed) {
    __syncthreads();
    for (int t = lane; t < nrows * hs; t += 64) {
      const int r = t / hs, i = t - r * hs;
      a.processed[f0 * hs + t] = tile[r * sd + i];
    }
  }
  if (a.scores) {
    __syncthreads();
    if (active) {
#pragma unroll
      for (int j = 0; j < 24; ++j) tile[lane * sd + j] = s[j];
    }
    __syncthreads();
    for (int t = lane; t < nrows * 24; t += 64) {
      const int r = t / 24, j = t - r * 24;
      a.scores[f0 * 24 + t] = tile[r * sd + j];
    }
  }
}

// computeAverageChroma (:575-596).  One block of 16 waves; a tile is tf = KEY_TILE_ELEMS / dim rows.
__global__ __launch_bounds__(1024) void key_colsum_kernel(const double* x, int64_t F, int dim, double* avg) {
  __shared__ double buf[2][KEY_TILE_ELEMS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t tf = KEY_TILE_ELEMS / dim;
  const int64_t ntiles = (F + tf - 1) / tf;
  auto stage = [&](int64_t t, int first, int nthreads) {
    const int64_t r0 = t * tf;
    const int64_t n = (F - r0 < tf ? F - r0 : tf) * dim;
    const double* src = x + r0 * dim;
    double* dst = buf[t & 1];
    constexpr int kPer = (KEY_TILE_ELEMS + 959) / 960;   // all of a thread's loads are issued before its stores
    double v[kPer];
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int64_t k = tid - first + (int64_t)u * nthreads;
      v[u] = k < n ? src[k] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int64_t k = tid - first + (int64_t)u * nthreads;
      if (k < n) dst[k] = v[u];
    }
  };
  stage(0, 0, 1024);
  __syncthreads();
  double acc0 = 0.0, acc1 = 0.0;
  for (int64_t t = 0; t < ntiles; ++t) {
    if (wave != 0) {
      if (t + 1 < ntiles) stage(t + 1, 64, 960);
    } else {
      const int64_t r0 = t * tf;
      const int n = (int)(F - r0 < tf ? F - r0 : tf);
      const double* b = buf[t & 1];
      // eight LDS reads in flight, then the eight additions in row order
      // (a compile-time stride for 12 bins: the reads then differ by immediate offsets only)
      auto chain = [&](const double* col, double acc, auto stride) {
        const int st = stride ? (int)stride : dim;
        int r = 0;
        for (; r + 8 <= n; r += 8) {
          double v[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) v[u] = col[(r + u) * st];
#pragma unroll
          for (int u = 0; u < 8; ++u) acc = acc + v[u];
        }
        for (; r < n; ++r) acc = acc + col[r * st];
        return acc;
      };
      if (dim == 12) {
        if (lane < 12) acc0 = chain(b + lane, acc0, std::integral_constant<int, 12>{});
      } else {
        if (lane < dim) acc0 = chain(b + lane, acc0, std::integral_constant<int, 0>{});
        if (lane + 64 < dim) acc1 = chain(b + lane + 64, acc1, std::integral_constant<int, 0>{});
      }
    }
    __syncthreads();
  }
  if (wave == 0) {
    if (lane < dim) avg[lane] = __ddiv_rn(acc0, (double)F);
    if (lane + 64 < dim) avg[lane + 64] = __ddiv_rn(acc1, (double)F);
  }
}

// GetGlobalKey (:923-959).  Lane c < 24 owns the vote of code c, lane 24 the total.
__global__ __launch_bounds__(1024) void key_votes_kernel(const int32_t* code, const double* conf, int64_t F,
                                                         double* votes, int32_t* gcode, double* gconf,
                                                         double* gstrength) {
  __shared__ __attribute__((aligned(16))) double cbuf[2][KEY_TILE_FRAMES];
  __shared__ __attribute__((aligned(16))) int kbuf[2][KEY_TILE_FRAMES];
  __shared__ double fin[25];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t tf = KEY_TILE_FRAMES;
  const int64_t ntiles = (F + tf - 1) / tf;
  auto stage = [&](int64_t t, int first, int nthreads) {
    const int64_t r0 = t * tf;
    const int64_t n = F - r0 < tf ? F - r0 : tf;
    constexpr int kPer = (KEY_TILE_FRAMES + 959) / 960;   // all of a thread's loads are issued before its stores
    double cf[kPer];
    int kc[kPer];
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int64_t k = tid - first + (int64_t)u * nthreads;
      cf[u] = k < n ? conf[r0 + k] : 0.0;
      kc[u] = k < n ? code[r0 + k] : 0;
    }
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int64_t k = tid - first + (int64_t)u * nthreads;
      if (k < n) {
        cbuf[t & 1][k] = cf[u] > 0.5 ? cf[u] : 0.0;   // :933; a vote is >= 0, so adding 0.0 leaves its bits
        kbuf[t & 1][k] = kc[u];
      }
    }
  };
  stage(0, 0, 1024);
  __syncthreads();
  double acc = 0.0;
  for (int64_t t = 0; t < ntiles; ++t) {
    if (wave != 0) {
      if (t + 1 < ntiles) stage(t + 1, 64, 960);
    } else if (lane < 25) {
      const int64_t r0 = t * tf;
      const int n = (int)(F - r0 < tf ? F - r0 : tf);
      const double* cb = cbuf[t & 1];
      const int* kb = kbuf[t & 1];
      int r = 0;
      for (; r + 8 <= n; r += 8) {   // eight LDS reads in flight, then the eight additions in frame order
        const int4 k0 = *(const int4*)(kb + r), k1 = *(const int4*)(kb + r + 4);
        const double2 c0 = *(const double2*)(cb + r), c1 = *(const double2*)(cb + r + 2);
        const double2 c2 = *(const double2*)(cb + r + 4), c3 = *(const double2*)(cb + r + 6);
        const int k[8] = {k0.x, k0.y, k0.z, k0.w, k1.x, k1.y, k1.z, k1.w};
        const double c[8] = {c0.x, c0.y, c1.x, c1.y, c2.x, c2.y, c3.x, c3.y};
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = acc + ((lane == 24 || k[u] == lane) ? c[u] : 0.0);
      }
      for (; r < n; ++r) acc = acc + ((lane == 24 || kb[r] == lane) ? cb[r] : 0.0);
    }
    __syncthreads();
  }
  if (wave == 0 && lane < 25) fin[lane] = acc;
  __syncthreads();
  if (tid < 24 && votes) votes[tid] = fin[tid];
  if (tid == 0) {
    int best = -1;
    double score = 0.0;
    for (int c = 0; c < 24; ++c)
      if (fin[c] > score) { score = fin[c]; best = c; }
    if (gcode) *gcode = best;
    if (gconf) *gconf = __ddiv_rn(score, fin[24]);
    if (gstrength) *gstrength = __ddiv_rn(score, (double)F);
  }
}

// analyzeTemporalStability's tail (:611-621) with findMode (:657-673): a wave counts 64 codes per step
// with one ballot per code (the counters are wave-uniform), the waves meet in LDS.
__global__ __launch_bounds__(1024) void key_stability_kernel(const int32_t* code, int64_t F, double* stability) {
  __shared__ unsigned int hist[24];
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < 24) hist[tid] = 0u;
  __syncthreads();
  unsigned int cnt[24];
#pragma unroll
  for (int c = 0; c < 24; ++c) cnt[c] = 0u;
  for (int64_t e0 = 0; e0 < F; e0 += 1024) {
    const int64_t e = e0 + tid;
    const int k = e < F ? code[e] : -1;
#pragma unroll
    for (int c = 0; c < 24; ++c) cnt[c] += (unsigned int)__popcll(__ballot(k == c));
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 24; ++c)
      if (cnt[c]) atomicAdd(&hist[c], cnt[c]);
  }
  __syncthreads();
  if (tid == 0) {
    unsigned int max_count = 0u;
    for (int c = 0; c < 24; ++c)
      if (hist[c] > max_count) max_count = hist[c];   // the first (lowest) code of that count is the mode
    *stability = F < 3 ? 0.0 : __ddiv_rn((double)max_count, (double)F);
  }
}

// One block walks the entries 1024 at a time; a flagged entry's slot is the flags before it.
__global__ __launch_bounds__(1024) void key_compact_kernel(KeyCompactArgs a) {
  __shared__ int wcount[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  int64_t total = 0;
  for (int64_t e0 = 0; e0 < a.n; e0 += 1024) {
    const int64_t e = e0 + tid;
    bool flag = false;
    int k0 = 0, k1 = 0;
    double c0 = 0.0, c1 = 0.0;
    if (e >= 1 && e < a.n) {
      k0 = a.code[e - 1]; k1 = a.code[e];
      c0 = a.conf[e - 1]; c1 = a.conf[e];
      flag = a.transitions ? (c0 > 0.5 && c1 > 0.5)    // GetKeyProgression (:973)
                           : (k1 != k0 && c1 > 0.7);   // detectModulations (:646)
    }
    const uint64_t b = __ballot(flag);
    if (lane == 0) wcount[wave] = __popcll(b);
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < 16; ++w) {
      const int n = wcount[w];
      if (w < wave) before += n;
      all += n;
    }
    if (flag) {
      const int64_t pos = total + before + __popcll(b & below);
      if (a.transitions) {
        if (a.frame) a.frame[pos] = (int32_t)e;
        if (a.from) a.from[pos] = k0;
        if (a.to) a.to[pos] = k1;
        if (a.tconf) a.tconf[pos] = __ddiv_rn(c0 + c1, 2.0);
        if (a.type) a.type[pos] = key_transition_type(k0 >> 1, k0 & 1, k1 >> 1, k1 & 1);
      } else if (a.frame) {
        a.frame[pos] = (int32_t)(e + 10);
      }
    }
    total += all;
    __syncthreads();
  }
  if (tid == 0 && a.count) *a.count = total;
}

int launch_key_rows(const KeyArgs& a, hipStream_t s) {
  if (a.F < 1) return 0;
  if (a.hs < 1 || a.hs > KEY_MAX_SIZE || a.dim < 0 || a.dim > KEY_MAX_SIZE || a.ncand < 1 || a.ncand > 24) return -1;
  if ((a.dim != a.hs && !a.ridx) || (a.hs == 12 && !a.tab) || (a.window != 0 && a.window != 10)) return -1;
  const int64_t blocks = (a.F + 63) / 64;
  if (blocks > INT32_MAX) return -1;
  const int sd = (a.hs | 1) > 25 ? (a.hs | 1) : 25;
  hipLaunchKernelGGL(key_rows_kernel, dim3((unsigned)blocks), dim3(64), (size_t)64 * sd * 8, s, a);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

int launch_key_colsum(const double* chroma, int64_t F, int dim, double* avg, hipStream_t s) {
  if (F < 1 || dim < 1) return 0;
  if (dim > KEY_MAX_SIZE) return -1;
  hipLaunchKernelGGL(key_colsum_kernel, dim3(1), dim3(1024), 0, s, chroma, F, dim, avg);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

int launch_key_stability(const int32_t* code, int64_t F, double* stability, hipStream_t s) {
  hipLaunchKernelGGL(key_stability_kernel, dim3(1), dim3(1024), 0, s, code, F, stability);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

int launch_key_votes(const int32_t* code, const double* conf, int64_t F, double* votes, int32_t* gcode, double* gconf,
                     double* gstrength, hipStream_t s) {
  if (F < 1) return 0;
  hipLaunchKernelGGL(key_votes_kernel, dim3(1), dim3(1024), 0, s, code, conf, F, votes, gcode, gconf, gstrength);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

int launch_key_compact(const KeyCompactArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(key_compact_kernel, dim3(1), dim3(1024), 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // namespace sonar
