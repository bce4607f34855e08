// pair_score_kernels.hip -- sonar_align_pairs' scorer on gfx950: one wave per pair reduces its
// warping path and energy correlation on the device (the DTW that made the path is dtw_kernels.hip).
#include <cstdint>

#include "kernels.h"
#include "wave.h"

#pragma clang fp contract(off)

namespace sonar {

// sonar_align_pairs' scorer reductions on the device (alignment.go:380-643, correlation.go:526-667):
// one wave per pair over its warping path and energy correlation -- host::path_sums and
// host::corr_sums, bit for bit -- so a batch copies back ~150 bytes per pair instead of its path
// (16 B per point) and correlation, and its host thread only combines scalars.  Counts, extrema
// and the peak index (the first index of the largest |corr|, as Go's strict > scan) are order-free;
// the float sums keep Go's sequential order: 64 terms are formed at once (a smoothed cost is Go's
// window sum, a deviation is squared before it is added, as Go does) and then added one by one in
// index order (seq_add below).
namespace {
// the largest a over the wave (ties: the smallest index); a = -1 for "none"
__device__ __forceinline__ void wave_argmax(double& a, int64_t& i) {
  for (int o = 32; o > 0; o >>= 1) {
    const double ao = __shfl_xor(a, o, 64);
    const int64_t io = __shfl_xor(i, o, 64);
    if (ao > a || (ao == a && io < i)) { a = ao; i = io; }
  }
}
}  // namespace

// Sequential sums of 64 terms at a time (acc += v[lane 0], += v[lane 1], ... in lane order, for
// NC independent sums at once).  Round 6: the terms go through LDS and every lane runs the add chain
// on broadcast reads, so a term costs one dependent v_add_f64 (the reads are independent and issue
// ahead) instead of two v_readlane + the SGPR hazard + the add (3.2 -> 2.0 ms per launch).
template <int NC>
__device__ __forceinline__ void seq_add(double (&acc)[NC], const double (&v)[NC], int cnt, double* buf) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int c = 0; c < NC; ++c) buf[64 * c + lane] = v[c];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  // 32 terms per sum into registers with every read issued up front, then the adds in order
  for (int k0 = 0; k0 < cnt; k0 += 32) {
    double r[NC][32];
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int q = 0; q < 32; q += 2) {
        const double2 v2 = *reinterpret_cast<const double2*>(&buf[64 * c + k0 + q]);
        r[c][q] = v2.x; r[c][q + 1] = v2.y;
      }
    if (k0 + 32 <= cnt) {
#pragma unroll
      for (int q = 0; q < 32; ++q)
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[c] += r[c][q];
    } else {
#pragma unroll
      for (int q = 0; q < 32; ++q)
        if (k0 + q < cnt) {
#pragma unroll
          for (int c = 0; c < NC; ++c) acc[c] += r[c][q];
        }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");     // the next block's stores after every read
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

constexpr int SU = 4;   // 64-term steps whose terms are formed before their adds (loads in flight)
__global__ __launch_bounds__(64) void pair_score_kernel(const ScoreJob* jobs) {
  const ScoreJob j = jobs[blockIdx.x];
  const int lane = threadIdx.x;
  __shared__ __attribute__((aligned(16))) double sbuf[2 * 64];
  // ---- warping path
  const int64_t P = *j.plen;
  host::PathSums ps;
  ps.P = P;
  if (P > 0) {
    int64_t off = 0, dg = 0, ch = 0;
    const int64_t w = max((int64_t)2, min((int64_t)5, P / 4)), h = w / 2;
    auto smooth = [&](int64_t i) {                  // calculateCostConsistency's window mean
      double t = 0.0;
      const int64_t lo = max((int64_t)0, i - h), hi = min(P - 1, i + h);
      for (int64_t q = lo; q <= hi; ++q) t += j.pc[q];
      return t / (double)(hi - lo + 1);
    };
    double sc = 0.0, ss = 0.0;                       // Go's sequential sums (wave-uniform)
    // SU steps of 64 terms are formed first (their path loads all in flight at once), then added
    for (int64_t b0 = 0; b0 < P; b0 += 64 * SU) {
      double cu[SU], mu[SU];
#pragma unroll
      for (int u = 0; u < SU; ++u) {
        const int64_t i = b0 + 64 * u + lane;
        double c = 0.0, m = 0.0;
        if (i < P) {
          off += j.pr[i] - j.pq[i];
          c = j.pc[i];
          if (P > 1) m = smooth(i);
          if (i >= 1) {
            const int d0 = j.pq[i] - j.pq[i - 1], d1 = j.pr[i] - j.pr[i - 1];
            if (d0 > 0 && d1 > 0) dg++;
            if (i >= 2 && (d0 != j.pq[i - 1] - j.pq[i - 2] || d1 != j.pr[i - 1] - j.pr[i - 2])) ch++;
          }
        }
        cu[u] = c; mu[u] = m;
      }
#pragma unroll
      for (int u = 0; u < SU; ++u) {
        const int64_t b = b0 + 64 * u;
        if (b < P) {
          const int cnt = (int)min((int64_t)64, P - b);
          double acc[2] = {sc, ss};
          const double v[2] = {cu[u], mu[u]};
          seq_add<2>(acc, v, cnt, sbuf);
          sc = acc[0]; ss = acc[1];
        }
      }
    }
    ps.offset_sum = wave_sum(off);
    ps.diag_steps = wave_sum(dg);
    ps.changes = wave_sum(ch);
    ps.sum_cost = sc;
    ps.p0q = j.pq[0]; ps.p0r = j.pr[0]; ps.p1q = j.pq[P - 1]; ps.p1r = j.pr[P - 1];
    if (P > 1) {
      ps.sum_smooth = ss;
      const double mean = ss / (double)P;
      double vv = 0.0;
      for (int64_t b0 = 0; b0 < P; b0 += 64 * SU) {
        double du[SU];
#pragma unroll
        for (int u = 0; u < SU; ++u) {
          const int64_t i = b0 + 64 * u + lane;
          double d2 = 0.0;
          if (i < P) { const double d = smooth(i) - mean; d2 = d * d; }
          du[u] = d2;
        }
#pragma unroll
        for (int u = 0; u < SU; ++u) {
          const int64_t b = b0 + 64 * u;
          if (b < P) {
            const int cnt = (int)min((int64_t)64, P - b);
            double acc[1] = {vv};
            const double v[1] = {du[u]};
            seq_add<1>(acc, v, cnt, sbuf);
            vv = acc[0];
          }
        }
      }
      ps.var_smooth = vv;
    }
  }
  if (lane == 0) *j.path = ps;
  // ---- energy correlation
  if (!j.corr) return;
  const int64_t nl = j.nl;
  host::CorrSums cs;
  cs.num_lags = nl;
  if (nl > 0) {
    // findPeak: Go keeps corr[0] unless a strictly larger |corr| follows (a NaN corr[0] is kept)
    double a = -1.0;
    int64_t pi = nl;
    for (int64_t i = lane; i < nl; i += 64) {
      const double v = fabs(j.corr[i]);
      if (v > a) { a = v; pi = i; }                  // NaN never wins
    }
    wave_argmax(a, pi);
    const double c0 = j.corr[0];
    if (isnan(c0) || !(a > fabs(c0))) pi = 0;        // nothing strictly larger than |corr[0]|
    cs.peak_index = pi;
    cs.peak = j.corr[pi];
    double ns = 0.0, sa = -1.0, ms = 0.0;
    int64_t nc = 0, si = nl;
    for (int64_t b0 = 0; b0 < nl; b0 += 64 * SU) {
      double qu[SU];
#pragma unroll
      for (int u = 0; u < SU; ++u) {
        const int64_t i = b0 + 64 * u + lane;
        double sq = 0.0;                             // terms outside the mask add an exact +0
        if (i < nl) {
          const double c = j.corr[i], v = fabs(c);
          const int64_t d = i > pi ? i - pi : pi - i;
          if (d > 5) { sq = c * c; nc++; }
          if (i != pi && v > sa) { sa = v; si = i; }
          if (d > 10 && v > ms) ms = v;
        }
        qu[u] = sq;
      }
#pragma unroll
      for (int u = 0; u < SU; ++u) {
        const int64_t b = b0 + 64 * u;
        if (b < nl) {
          const int cnt = (int)min((int64_t)64, nl - b);
          double acc[1] = {ns};
          const double v[1] = {qu[u]};
          seq_add<1>(acc, v, cnt, sbuf);
          ns = acc[0];
        }
      }
    }
    cs.noise_sum = ns;
    cs.noise_count = wave_sum(nc);
    wave_argmax(sa, si);
    cs.second_peak = (si < nl && sa > 0.0) ? j.corr[si] : 0.0;   // Go starts from 0 with a strict >
    int64_t mi = 0;
    wave_argmax(ms, mi);                             // a max of non-negative values
    cs.max_sidelobe = ms;
    if (nl >= 3 && pi > 0 && pi < nl - 1) cs.sharpness = -(j.corr[pi + 1] - 2 * j.corr[pi] + j.corr[pi - 1]);
  }
  if (lane == 0) *j.corr_out = cs;
}

int launch_pair_scores(const ScoreJob* djobs, int n, hipStream_t s) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(pair_score_kernel, dim3((unsigned)n), dim3(64), 0, s, djobs);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // namespace sonar
