// chord_kernels.hip -- ChordDetector (algorithms/tonal/chord_detection.go) over a device chromagram:
// DetectChord from templateMatching on (:428-502) per row, the frame-to-frame chain of
// applyTemporalSmoothing (:783-806) and updateTemporalTracking (:919-926), and AnalyzeProgression
// (:1128-1173).  All float64 like the Go reference; every candidate, rank and clip is decided from a
// rounding here, so this file is built without FMA contraction.  Nothing here calls a transcendental.
//
//   chord_rows_kernel         one lane per row, 64 rows staged through LDS of which the block reports the
//                             last 63: lane 0 holds the row before them, whose candidate set is the
//                             history the block's first row meets.  A lane keeps its 120 strengths in its
//                             own LDS row.  record == 1 writes the chain's record (n, topN, top0, top1),
//                             else the lane applies the boosts the chain resolved, ranks, cuts and writes.
//   chord_chain_kernel        the integer recurrence over the records: one lane walks a tile of 1024 that
//                             the block staged, the block writes the states out
//   chord_stability_kernel    the variance of the last <= temporal_window first confidences, per frame
//   chord_progression_kernel  the ordered confidence sum and the quality histogram
//   chord_mirror_kernel       the full-length magnitude row DetectChord hands to the HPCP (F37)
// No kernel waits on another block.
#include <cstdint>

#include "kernels.h"

namespace sonar {

namespace {

// initializeTemplates (:268-367) in ascending quality code: Major, Minor, Diminished, Augmented, Sus2, Sus4,
// Maj7, Min7, Dom7, PowerChord.  A pattern is 1.0 at its intervals and 0.0 elsewhere.
__host__ __device__ constexpr int chord_ntones(int t) {
  constexpr int n[10] = {3, 3, 3, 3, 3, 3, 4, 4, 4, 2};
  return n[t];
}
__host__ __device__ constexpr int chord_interval(int t, int k) {
  constexpr int iv[10][4] = {{0, 4, 7, 0}, {0, 3, 7, 0}, {0, 3, 6, 0}, {0, 4, 8, 0},  {0, 2, 7, 0},
                             {0, 5, 7, 0}, {0, 4, 7, 11}, {0, 3, 7, 10}, {0, 4, 7, 10}, {0, 7, 0, 0}};
  return iv[t][k];
}
__host__ __device__ constexpr unsigned chord_tones(int t) {   // bit i: interval i is a chord tone
  unsigned m = 0;
  for (int k = 0; k < chord_ntones(t); ++k) m |= 1u << chord_interval(t, k);
  return m;
}
__host__ __device__ constexpr double chord_weight(int t) {
  constexpr double w[10] = {1.0, 1.0, 0.8, 0.7, 0.7, 0.7, 0.85, 0.85, 0.9, 0.6};
  return w[t];
}
__host__ __device__ constexpr double chord_consonance(int t) {
  constexpr double c[10] = {0.9, 0.85, 0.3, 0.4, 0.6, 0.6, 0.8, 0.75, 0.7, 0.8};
  return c[t];
}
__host__ __device__ constexpr int chord_quality(int t) { return t < 9 ? t : 23; }

constexpr int kStride = CHORD_SLOTS + 13;   // doubles per lane: the 120 slots, the 12 normalised bins, odd

__device__ __forceinline__ bool slot_bit(uint64_t m0, uint64_t m1, int s) {
  return ((s < 64 ? m0 >> s : m1 >> (s - 64)) & 1ull) != 0;
}

// Confidence = math.Min(score, 1.0) (:619), boosted math.Min(c * 1.1, 1.0) (:794)
__device__ __forceinline__ double chord_conf(double strength, bool boost) {
  double c = strength < 1.0 ? strength : 1.0;
  if (boost) {
    const double b = c * 1.1;
    c = b < 1.0 ? b : 1.0;
  }
  return c;
}

// The candidate a stable descending sort puts right after (pc, ps); pc = +inf, ps = -1 gives the first.
__device__ __forceinline__ int chord_next(const double* st, uint64_t c0, uint64_t c1, uint64_t b0, uint64_t b1,
                                          double pc, int ps, double* conf) {
  int best = -1;
  double bc = 0.0;
  // no branch in the body, so that the unrolled loop has eight LDS reads in flight
#pragma unroll 8
  for (int s = 0; s < 64; ++s) {
    const double c = chord_conf(st[s], (b0 >> s & 1ull) != 0);
    const bool take = (c0 >> s & 1ull) != 0 && (c < pc || (c == pc && s > ps)) && (best < 0 || c > bc);
    best = take ? s : best;
    bc = take ? c : bc;
  }
#pragma unroll 8
  for (int s = 64; s < CHORD_SLOTS; ++s) {
    const double c = chord_conf(st[s], (b1 >> (s - 64) & 1ull) != 0);
    const bool take = (c1 >> (s - 64) & 1ull) != 0 && (c < pc || (c == pc && s > ps)) && (best < 0 || c > bc);
    best = take ? s : best;
    bc = take ? c : bc;
  }
  *conf = bc;
  return best;
}

}  // namespace

// LDS: 64 lanes x 133 doubles.  First the staged rows (stride dim | 1), then each lane's 120 raw template
// scores (copied out from there) and its normalised row, then its candidates' strengths.
__global__ __launch_bounds__(64) void chord_rows_kernel(ChordArgs a) {
  extern __shared__ double tile[];
  __shared__ uint64_t pm[64][2];
  const int lane = threadIdx.x;
  const int dim = a.dim, sd = dim | 1;
  const int64_t f0 = (int64_t)blockIdx.x * CHORD_ROWS - 1;   // lane 0's row, -1 in the first block
  const int nrows = a.F - f0 < 64 ? (int)(a.F - f0) : 64;
  int flag = 0;
  for (int t = lane; t < nrows * dim; t += 64) {
    const int r = t / dim, i = t - r * dim;
    double v = 0.0;
    if (f0 + r >= 0) {
      v = a.chroma[(f0 + r) * (int64_t)dim + i];
      if (!(fabs(v) <= 1.79769313486231570815e+308)) flag |= CHORD_FLAG_NONFINITE;
    }
    tile[r * sd + i] = v;
  }
  const int64_t f = f0 + lane;
  const bool active = lane < nrows && f >= 0;
  int bn = 0;
  double bc = 0.0;
  if (active) {
    if (a.bass_note) {
      const int note = a.bass_note[f];
      if (note < 0 || note > 11) flag |= CHORD_FLAG_BASS_NOTE;
      if (a.match_bass) bn = note;
    }
    if (a.bass_conf) {
      const double v = a.bass_conf[f];
      if (!(fabs(v) <= 1.79769313486231570815e+308)) flag |= CHORD_FLAG_NONFINITE;
      if (a.match_bass) bc = v;
    }
  }
  if (flag && a.flags) atomicOr(a.flags, flag);
  __syncthreads();
  double c[12], nc[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) c[i] = active ? tile[lane * sd + i] : 0.0;
  __syncthreads();
  // calculateHarmonicTension (:1012-1035) and analyzeExtensions' threshold (:868), both on the raw row
  double tension = 0.0;
  unsigned hot = 0;
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    if (c[i] > 0.3) hot |= 1u << i;
#pragma unroll
    for (int j = i + 1; j < 12; ++j) {
      if ((j - i == 1 || j - i == 6 || j - i == 11) && c[i] > 0.2 && c[j] > 0.2) tension = tension + c[i] * c[j];
    }
  }
  tension = tension < 1.0 ? tension : 1.0;
  // normalizeChroma (:703-710); a row of another length scores 0 whatever it holds (:722)
#pragma unroll
  for (int i = 0; i < 12; ++i) nc[i] = c[i];
  if (a.normalize && dim == 12) {
    double e = 0.0;
#pragma unroll
    for (int i = 0; i < 12; ++i) e = e + c[i] * c[i];
    if (!(e < 1e-10)) {
      const double nrm = __dsqrt_rn(e);
#pragma unroll
      for (int i = 0; i < 12; ++i) nc[i] = __ddiv_rn(c[i], nrm);
    }
  }
  double* st = tile + lane * kStride;
  double* ncl = st + CHORD_SLOTS;   // the lane's normalised row, where a loop over the roots can index it
#pragma unroll
  for (int i = 0; i < 12; ++i) ncl[i] = nc[i];
  // calculateTemplateScore (:721-733).  The pattern's zeros add +-0 to a sum that starts at +0 (and so
  // never becomes -0) and its ones multiply by 1.0, so the sum over the chord tones in ascending index
  // order is the reference's sum bit for bit (the input is finite): the tones that wrap past pitch class
  // 11 come first, then the others, each group in interval order; a tone of the other group adds 0.0.
  if (dim == 12) {
#pragma unroll 1
    for (int root = 0; root < 12; ++root) {
#pragma unroll
      for (int t = 0; t < 10; ++t) {
        double sum = 0.0;
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (k < chord_ntones(t)) {
              const int p = root + chord_interval(t, k);
              const double v = ncl[p >= 12 ? p - 12 : p];
              sum = sum + ((p >= 12) == (pass == 0) ? v : 0.0);
            }
          }
        }
        st[t * 12 + root] = sum * chord_weight(t);
      }
    }
  } else {
    for (int s = 0; s < CHORD_SLOTS; ++s) st[s] = 0.0;
  }
  if (a.scores && !a.record) {   // TemplateScores: rows f0 + 1 .. of the block, 120 each
    __syncthreads();
    const int64_t base = (f0 + 1) * CHORD_SLOTS;
    for (int t = lane; t < (nrows - 1) * CHORD_SLOTS; t += 64) {
      const int r = t / CHORD_SLOTS, j = t - r * CHORD_SLOTS;
      a.scores[base + t] = tile[(r + 1) * kStride + j];
    }
    __syncthreads();
  }
  // the bass bonus (:735-750), the threshold (:612) and detectInversion (:752-781); bc > 0.3 only with
  // use_bass_detection, since the bass is (0, 0.0) without it
  uint64_t c0 = 0ull, c1 = 0ull;
  uint64_t inv0 = 0ull, inv1 = 0ull, inv2 = 0ull, inv3 = 0ull;   // two bits per slot, 32 slots a word
  if (active) {
    const bool bass_on = bc > 0.3;
    const double bonus = a.bass_weight * bc;
#pragma unroll 1
    for (int root = 0; root < 12; ++root) {
      const int rel = ((bn - root) % 12 + 12) % 12;   // the bass as an interval above this root
#pragma unroll
      for (int t = 0; t < 10; ++t) {
        const int s = t * 12 + root;
        const double raw = st[s];
        double score = raw;
        int inv = 0;
        const bool tone = bass_on && (chord_tones(t) >> rel & 1u) != 0;
        if (bass_on) score = score + (tone ? bonus : 0.0);
        const bool is_cand = score >= a.min_strength;
        if (is_cand && tone && a.use_inversions) {
          int k = 0;
#pragma unroll
          for (int q = 1; q < 4; ++q)
            if (q < chord_ntones(t) && chord_interval(t, q) == rel) k = q;
          double x = raw;   // inversion 0 is the pattern itself
          if (k != 0) {     // 1.5 at the bass tone (:397)
            double sum = 0.0;
#pragma unroll
            for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                if (q < chord_ntones(t)) {
                  const int p = root + chord_interval(t, q);
                  const int i = p >= 12 ? p - 12 : p;
                  const double v = i == bn ? ncl[i] * 1.5 : ncl[i];
                  sum = sum + ((p >= 12) == (pass == 0) ? v : 0.0);
                }
              }
            }
            x = dim == 12 ? sum * chord_weight(t) : 0.0;
          }
          // bestScore starts at 0.0 and only a higher score replaces it (:757-776)
          const double best_score = x > 0.0 ? x : 0.0;
          if (best_score > score) { inv = x > 0.0 ? k : 0; score = best_score; }
        } else if (is_cand && bass_on && a.use_inversions) {
          if (0.0 > score) score = 0.0;   // no inversion matches the bass: (ChordRoot, 0.0) against a negative score
        }
        if (is_cand) {
          st[s] = score;
          if (s < 64) c0 |= 1ull << s; else c1 |= 1ull << (s - 64);
          const uint64_t ib = (uint64_t)inv << ((s & 31) * 2);
          if (s < 32) inv0 |= ib; else if (s < 64) inv1 |= ib; else if (s < 96) inv2 |= ib; else inv3 |= ib;
        }
      }
    }
  }
  pm[lane][0] = c0;
  pm[lane][1] = c1;
  __syncthreads();
  if (!active || lane == 0) return;
  const uint64_t p0 = pm[lane - 1][0], p1 = pm[lane - 1][1];   // the previous frame's candidate set
  const int n = __popcll(c0) + __popcll(c1);
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  if (a.record) {
    int top_n = -1, top0 = -1, top1 = -1;
    if (a.smoothing && n > 0) {
      double cf;
      top_n = chord_next(st, c0, c1, 0ull, 0ull, inf, -1, &cf);
      top0 = chord_next(st, c0, c1, p0, p1, inf, -1, &cf);
      const uint64_t q0 = top0 < 64 ? p0 & ~(1ull << top0) : p0;
      const uint64_t q1 = top0 < 64 ? p1 : p1 & ~(1ull << (top0 - 64));
      top1 = chord_next(st, c0, c1, q0, q1, inf, -1, &cf);
    }
    int32_t* r = a.rec + f * 4;
    r[0] = n; r[1] = top_n; r[2] = top0; r[3] = top1;
    return;
  }
  // the boosts the chain resolved (:790-797)
  uint64_t b0 = 0ull, b1 = 0ull;
  if (a.hstate) {
    const int h = a.hstate[f];
    if (h != CHORD_HIST_EMPTY) {
      b0 = p0; b1 = p1;
      if (h >= 0 && h < 64) b0 &= ~(1ull << h);
      if (h >= 64 && h < CHORD_SLOTS) b1 &= ~(1ull << (h - 64));
    }
  }
  // sort.Slice (:453) as a stable sort, the cut (:458-460), and the primary chord (:475-484)
  const int64_t mc = a.max_cand;
  const int kept = n < mc ? n : (int)mc;
  double conf0 = 0.0, conf1 = 0.0, strength0 = 0.0;
  int first = -1, inv_first = 0;
  {
    double pc = inf;
    int ps = -1;
    for (int k = 0; k < kept; ++k) {
      double cf;
      const int s = chord_next(st, c0, c1, b0, b1, pc, ps, &cf);
      const uint64_t w = s < 32 ? inv0 : s < 64 ? inv1 : s < 96 ? inv2 : inv3;
      const int inv = (int)(w >> ((s & 31) * 2) & 3ull);
      const double sg = st[s];
      if (k == 0) { first = s; conf0 = cf; strength0 = sg; inv_first = inv; }
      if (k == 1) conf1 = cf;
      if (a.cand) a.cand[f * mc + k] = s;
      if (a.cand_inv) a.cand_inv[f * mc + k] = inv;
      if (a.cand_conf) a.cand_conf[f * mc + k] = cf;
      if (a.cand_strength) a.cand_strength[f * mc + k] = sg;
      pc = cf;
      ps = s;
    }
    for (int64_t k = kept; k < mc; ++k) {
      if (a.cand) a.cand[f * mc + k] = -1;
      if (a.cand_inv) a.cand_inv[f * mc + k] = 0;
      if (a.cand_conf) a.cand_conf[f * mc + k] = 0.0;
      if (a.cand_strength) a.cand_strength[f * mc + k] = 0.0;
    }
  }
  const bool have = kept > 0;
  const int t_first = have ? first / 12 : 0, root = have ? first - t_first * 12 : 0;
  const int quality = have ? chord_quality(t_first) : 0;
  const double clarity = have ? (kept > 1 ? conf0 - conf1 : conf0) : 0.0;   // :813-821
  int ext = 0;
  if (have && a.detect_ext) {   // analyzeExtensions (:840-894) as a mask of 1 << interval
    const unsigned tones = chord_tones(t_first);
    const int ivs[5] = {10, 11, 2, 5, 9}, num[5] = {7, 7, 9, 11, 13};
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      const int iv = ivs[q];
      if ((hot >> ((root + iv) % 12) & 1u) && !(tones >> iv & 1u) && (q < 2 || a.max_ext >= num[q])) ext |= 1 << iv;
    }
  }
  int role = 0;
  if (have && a.functional)   // analyzeFunctionalRole (:896-917)
    role = quality == 0 ? 1 : quality == 1 ? 2 : quality == 8 ? 3 : quality == 2 ? 4 : 5;
  if (a.root) a.root[f] = root;
  if (a.quality) a.quality[f] = quality;
  if (a.inversion) a.inversion[f] = have ? inv_first : 0;
  if (a.n_found) a.n_found[f] = n;
  if (a.ext) a.ext[f] = ext;
  if (a.role) a.role[f] = role;
  if (a.conf) a.conf[f] = have ? conf0 : 0.0;
  if (a.strength) a.strength[f] = have ? strength0 : 0.0;
  if (a.clarity) a.clarity[f] = clarity;
  if (a.ambiguity) a.ambiguity[f] = have ? 1.0 - clarity : 0.0;
  if (a.consonance) a.consonance[f] = have ? chord_consonance(t_first) : 0.0;
  if (a.tension) a.tension[f] = have ? tension : 0.0;
  if (a.stability) a.stability[f] = have ? conf0 : 0.0;   // an empty confidenceHistory (:832-834)
  if (a.kconf && have) a.kconf[a.kidx[f]] = conf0;
}

// The state of chordHistory before every frame, from the records alone (DESIGN.md Kernel 4f).  While a
// tile is staged every thread turns its record into the frame's transition, which needs no state:
//   the state after the frame = e when the state before it is empty, else (state == key ? v1 : v0)
// (a frame that does not drop its winner has v0 = v1), so the walking lane's step is two compares and
// two selects.  The count of frames that kept a candidate is a prefix sum and is not on the chain.
__global__ __launch_bounds__(1024) void chord_chain_kernel(const int32_t* rec, int64_t F, int smoothing, int window,
                                                           int keeps, int32_t* hstate, int32_t* kidx, int32_t* flags) {
  __shared__ int4 tr[CHORD_TILE_FRAMES];   // e, key, v0, v1
  __shared__ int hs[CHORD_TILE_FRAMES], pf[CHORD_TILE_FRAMES];
  __shared__ int wcount[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  int state = CHORD_HIST_EMPTY, panic = 0;
  int64_t kept = 0;
  for (int64_t r0 = 0; r0 < F; r0 += CHORD_TILE_FRAMES) {
    const int n_tile = F - r0 < CHORD_TILE_FRAMES ? (int)(F - r0) : CHORD_TILE_FRAMES;
    bool keep = false;
    if (tid < n_tile) {
      const int4 q = ((const int4*)rec)[r0 + tid];   // n, topN, top0, top1
      const int n = q.x;
      const int some = n > 0 ? CHORD_HIST_FULL : CHORD_HIST_EMPTY;
      int4 t;
      t.x = smoothing ? some : CHORD_HIST_EMPTY;                       // :784-787
      if (!smoothing) { t.y = -3; t.z = t.w = CHORD_HIST_EMPTY; }
      else if (n > window && n > 1) { t.y = q.z; t.z = q.z; t.w = q.w; }   // the winner leaves the history (:801-803)
      else { t.y = -3; t.z = t.w = n > window ? CHORD_HIST_EMPTY : some; }
      tr[tid] = t;
      keep = n > 0 && keeps;
      pf[tid] = (smoothing && n == 0 && window < 0) ? 1 : 0;           // history[1:] of an empty slice (:802)
    }
    const uint64_t b = __ballot(keep);
    if (lane == 0) wcount[wave] = __popcll(b);
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < 16; ++w) {
      const int c = wcount[w];
      if (w < wave) before += c;
      all += c;
    }
    if (tid < n_tile) kidx[r0 + tid] = (int32_t)(kept + before + __popcll(b & below));
    kept += all;
    if (tid == 0) {
      auto step = [&](const int4 t, int bad, int r) {
        panic |= (state != CHORD_HIST_EMPTY) ? bad : 0;
        hs[r] = state;
        const int full = state == t.y ? t.w : t.z;
        state = state == CHORD_HIST_EMPTY ? t.x : full;
      };
      int r = 0;
      for (; r + 8 <= n_tile; r += 8) {   // the LDS reads of eight frames in flight, then their steps in frame order
        int4 t[8];
        int bad[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { t[u] = tr[r + u]; bad[u] = pf[r + u]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) step(t[u], bad[u], r + u);
      }
      for (; r < n_tile; ++r) step(tr[r], pf[r], r);
    }
    __syncthreads();
    if (tid < n_tile) hstate[r0 + tid] = hs[tid];
    __syncthreads();
  }
  if (tid == 0) {
    kidx[F] = (int32_t)kept;
    if (panic && flags) atomicOr(flags, CHORD_FLAG_SLICE_PANIC);
  }
}

// calculateVariance (:991-1010) of confidenceHistory, math.Max(0.0, 1.0 - variance) (:829-831)
__global__ __launch_bounds__(256) void chord_stability_kernel(const int32_t* kidx, const double* kconf, int64_t F,
                                                              int window, double* stability) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  const int k0 = kidx[f], k1 = kidx[f + 1];
  if (k1 == k0 || k0 == 0 || window <= 0) return;
  const int n = k0 < window ? k0 : window;
  const double* h = kconf + (k0 - n);
  double mean = 0.0;
  for (int i = 0; i < n; ++i) mean = mean + h[i];
  mean = __ddiv_rn(mean, (double)n);
  double var = 0.0;
  for (int i = 0; i < n; ++i) {
    const double d = h[i] - mean;
    var = var + d * d;
  }
  var = __ddiv_rn(var, (double)n);
  const double s = 1.0 - var;
  stability[f] = s > 0.0 ? s : 0.0;
}

// AnalyzeProgression (:1149-1170): totalConfidence in frame order / F; the quality counts are integers
__global__ __launch_bounds__(1024) void chord_progression_kernel(const int32_t* quality, const double* conf, int64_t F,
                                                                 double* avg, int32_t* most, int32_t* flags) {
  __shared__ double cb[CHORD_TILE_FRAMES];
  __shared__ unsigned int hist[32];
  const int tid = threadIdx.x;
  if (tid < 32) hist[tid] = 0u;
  __syncthreads();
  double acc = 0.0;
  int bad = 0;
  for (int64_t r0 = 0; r0 < F; r0 += CHORD_TILE_FRAMES) {
    const int n_tile = F - r0 < CHORD_TILE_FRAMES ? (int)(F - r0) : CHORD_TILE_FRAMES;
    if (tid < n_tile) {
      const double v = conf[r0 + tid];
      if (!(fabs(v) <= 1.79769313486231570815e+308)) bad |= CHORD_FLAG_NONFINITE;
      cb[tid] = v;
      const int q = quality[r0 + tid];
      if (q < 0 || q > 31) bad |= CHORD_FLAG_QUALITY;
      else atomicAdd(&hist[q], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      int r = 0;
      for (; r + 8 <= n_tile; r += 8) {   // eight LDS reads in flight, then the eight additions in frame order
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = cb[r + u];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = acc + v[u];
      }
      for (; r < n_tile; ++r) acc = acc + cb[r];
    }
    __syncthreads();
  }
  if (bad && flags) atomicOr(flags, bad);
  if (tid == 0) {
    unsigned int max_count = 0u;
    int best = 0;
    for (int q = 0; q < 32; ++q)
      if (hist[q] > max_count) { max_count = hist[q]; best = q; }
    if (avg) *avg = __ddiv_rn(acc, (double)F);
    if (most) *most = best;
  }
}

__global__ __launch_bounds__(256) void chord_mirror_kernel(const double* half, int64_t total, int W, double* full) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int64_t f = e / W;
  const int k = (int)(e - f * W);
  const int K = W / 2 + 1;
  full[e] = half[f * K + (k < K ? k : W - k)];
}

int launch_chord_rows(const ChordArgs& a, hipStream_t s) {
  if (a.F < 1) return 0;
  if ((a.dim != 12 && a.dim != 24 && a.dim != 36) || a.max_cand < 0) return -1;
  if (a.record ? !a.rec : (a.kconf && !a.kidx)) return -1;
  const int64_t blocks = (a.F + CHORD_ROWS - 1) / CHORD_ROWS;
  if (blocks > INT32_MAX) return -1;
  const size_t lds = (size_t)64 * kStride * 8;   // 68,096 bytes: two blocks a CU
  (void)hipFuncSetAttribute((const void*)chord_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(chord_rows_kernel, dim3((unsigned)blocks), dim3(64), lds, s, a);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

int launch_chord_chain(const int32_t* rec, int64_t F, int smoothing, int window, int keeps, int32_t* hstate,
                       int32_t* kidx, int32_t* flags, hipStream_t s) {
  if (F < 1) return 0;
  hipLaunchKernelGGL(chord_chain_kernel, dim3(1), dim3(1024), 0, s, rec, F, smoothing, window, keeps, hstate, kidx,
                     flags);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

int launch_chord_stability(const int32_t* kidx, const double* kconf, int64_t F, int window, double* stability,
                           hipStream_t s) {
  if (F < 1 || window <= 0) return 0;
  if (window > CHORD_MAX_WINDOW) return -1;
  const int64_t blocks = (F + 255) / 256;
  hipLaunchKernelGGL(chord_stability_kernel, dim3((unsigned)blocks), dim3(256), 0, s, kidx, kconf, F, window, stability);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

int launch_chord_progression(const int32_t* quality, const double* conf, int64_t F, double* avg, int32_t* most,
                             int32_t* flags, hipStream_t s) {
  if (F < 1) return 0;
  hipLaunchKernelGGL(chord_progression_kernel, dim3(1), dim3(1024), 0, s, quality, conf, F, avg, most, flags);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

int launch_chord_mirror(const double* half, int64_t F, int W, double* full, hipStream_t s) {
  if (F < 1 || W < 1) return 0;
  const int64_t total = F * W, blocks = (total + 255) / 256;
  if (blocks > INT32_MAX) return -1;
  hipLaunchKernelGGL(chord_mirror_kernel, dim3((unsigned)blocks), dim3(256), 0, s, half, total, W, full);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // namespace sonar
