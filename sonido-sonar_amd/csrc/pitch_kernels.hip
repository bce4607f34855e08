// pitch_kernels.hip -- PitchDetector.DetectPitch per frame for every method of the switch
// (algorithms/tonal/pitch_detection.go:225-727), up to postProcessResult: the raw pitch, confidence,
// candidates and curve of each frame of a float64 signal.  Every method starts from preprocessFrame
// (:282-345): a fresh pre-emphasis of 0.97 per frame, then the window.
//
//  pitch_lag_kernel<R, NL, NSDF>  detectPitchYin (:349-420) / detectPitchNSDF (:485-550): one wave per
//                             frame, lane l owns the lags R l .. R l + R - 1 (yin_kernel's layout at any W)
//  pitch_zc_kernel            detectPitchZeroCrossing (:694-727): one wave per frame
//  pitch_stats_kernel         normalize's mean and deviation (correlation.go:464-501): one frame per LANE
//  pitch_acf_fft_kernel       detectPitchACF (:423-482) over computeFFT (correlation.go:231-291), W > 1000
//  pitch_acf_time_kernel      the same over pearsonCorrelation per lag (correlation.go:314-370), W <= 512
//  pitch_spectrum_kernel      detectPitchHPS (:553-620) / detectPitchCepstrum (:623-684): one block per frame
//
// Sums that feed a comparison run in Go's index order with unfused multiplies and adds (__d*_rn), so
// YIN, NSDF, ACF and the crossing count are bit-identical to a sequential float64 evaluation; the ACF
// is xcorr_kernels.hip's transform (same butterfly, same table, same order) on one LDS tile.  HPS and
// the cepstrum go through go-dsp's FFT in the reference: parity at tolerance, any float64 transform.
#include <cstdint>

#include "pitch_kernels.h"
#include "wave.h"
#include "../../include/sonar_gpu.h"

#pragma clang fp contract(off)

namespace sonar {

namespace {

constexpr int kNone = 0x7fffffff;

// preprocessFrame's sample i of the frame at s: applyPreEmphasis (:300-314), then the window (:292-294)
__device__ __forceinline__ double pre_sample(const double* pcm, int64_t s, int i, int pre, const double* win) {
  const double x = pcm[s + i];
  const double y = (pre && i > 0) ? __dsub_rn(x, __dmul_rn(0.97, pcm[s + i - 1])) : x;
  return __dmul_rn(y, win[i]);
}

// The candidates of detectPitchACF / detectPitchNSDF (:436-460, 515-529) over a curve cv the wave can
// read: strict local maxima above the threshold at i in [lo, hi] whose frequency sr / (i - lag0) is in
// range, ordered by descending confidence.  Go's sort.Slice is not stable; equal confidences are
// ordered by ascending lag here.  One scan per reported candidate (at least two: the second confidence
// feeds calculateClarity), each picking the best candidate after the previous pick in that order.
__device__ void pick_peaks(const double* cv, int lo, int hi, int lag0, const PitchArgs& a, int64_t fi, int lane) {
  const int rounds = a.K > 2 ? a.K : 2;
  if (lane == 0)
    for (int q = 0; q < a.K; ++q) {
      if (a.cand_index) a.cand_index[fi * a.K + q] = -1;
      if (a.cand_conf) a.cand_conf[fi * a.K + q] = 0.0;
    }
  double pv = 0.0, best = 0.0, second = 0.0;
  int pi = -1, besti = -1, total = 0;
  for (int k = 0; k < rounds; ++k) {
    double bv = 0.0;
    int bi = kNone, cnt = 0;
    for (int i = lo + lane; i <= hi; i += 64) {
      const double c = cv[i];
      if (!(c > cv[i - 1] && c > cv[i + 1] && c > a.ac_thr)) continue;
      const double f = __ddiv_rn((double)a.sr, (double)(i - lag0));
      if (!(f >= a.min_freq && f <= a.max_freq)) continue;
      ++cnt;
      if (k > 0 && !(c < pv || (c == pv && i > pi))) continue;
      if (bi == kNone || c > bv) { bv = c; bi = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (oi != kNone && (bi == kNone || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
    }
    if (k == 0) total = wave_sum<int>(cnt);
    if (bi == kNone) break;                      // wave-uniform
    if (k == 0) { best = bv; besti = bi; }
    if (k == 1) second = bv;
    if (lane == 0 && k < a.K) {
      if (a.cand_index) a.cand_index[fi * a.K + k] = bi - lag0;
      if (a.cand_conf) a.cand_conf[fi * a.K + k] = bv;
    }
    pv = bv; pi = bi;
  }
  if (lane == 0) {
    a.pitch[fi] = besti >= 0 ? __ddiv_rn((double)a.sr, (double)(besti - lag0)) : 0.0;
    a.conf[fi] = besti >= 0 ? best : 0.0;
    if (a.index) a.index[fi] = besti >= 0 ? besti - lag0 : -1;
    if (a.ncand) a.ncand[fi] = total;
    if (a.second) a.second[fi] = second;
  }
}

// one candidate (YIN, HPS, cepstrum, zero crossing), by lane 0 of the frame's first wave
__device__ void put_single(const PitchArgs& a, int64_t fi, double pitch, double conf, int index, int ncand) {
  a.pitch[fi] = pitch; a.conf[fi] = conf;
  if (a.index) a.index[fi] = index;
  if (a.ncand) a.ncand[fi] = ncand;
  if (a.second) a.second[fi] = 0.0;
  for (int q = 0; q < a.K; ++q) {
    if (a.cand_index) a.cand_index[fi * a.K + q] = (q == 0 && ncand) ? index : -1;
    if (a.cand_conf) a.cand_conf[fi * a.K + q] = (q == 0 && ncand) ? conf : 0.0;
  }
}

}  // namespace

// ---------------------------------------------------------------- YIN, NSDF ----
// The lag sums over j < W / 2 of a lane's R consecutive lags are R independent chains in Go's j order.
// Their operands x[j + tau] slide by one per j, so they live in a window of 2 R registers refilled with
// R LDS reads per R values of j; x[j] is an LDS broadcast.  YIN: d = x_j - x_{j+tau}, acc += d d (3 ops a
// term).  NSDF: acf += x_j x_{j+tau} and m2 += x_{j+tau}^2, whose product is shared by the R terms that
// read the same window register (3 ops a term and R multiplies per R x R terms); m1 (:502) is the m2
// chain of lag 0.  At W = 64 the 32 lags take half a wave; the other lanes walk lag 0 and write nothing.
// NL lanes own lags (64, or 32 at W = 64), so W = 2 R NL is a compile-time constant, as in yin_kernel
// (Kernel 4i, has the timing with a runtime W).
template <int R, int NL, bool NSDF>
__global__ __launch_bounds__(256) void pitch_lag_kernel(const PitchArgs a) {
  constexpr int nl = NL, halfN = R * NL, W = 2 * halfN;
  __shared__ double lds[PITCH_FRAMES_PER_BLOCK * W];     // static: the compiler sees the occupancy it allows
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t fi = (int64_t)blockIdx.x * PITCH_FRAMES_PER_BLOCK + w;
  if (fi >= a.F) return;
  const int64_t s = fi * a.hop;
  double* xw = lds + (size_t)w * W;
  for (int i = lane; i < W; i += 64) xw[i] = pre_sample(a.pcm, s, i, a.pre, a.win);
  wave_lds_sync();
  const bool on = lane < nl;
  const int t0 = on ? R * lane : 0;
  double acc[R], m2[R], win[2 * R];
#pragma unroll
  for (int r = 0; r < R; ++r) { acc[r] = 0.0; m2[r] = 0.0; win[r] = xw[t0 + r]; }
  for (int jb = 0; jb < halfN; jb += R) {
#pragma unroll
    for (int r = 0; r < R; ++r) win[R + r] = xw[jb + t0 + R + r];   // <= W - 1
    if constexpr (NSDF) {
      double sq[2 * R - 1];
#pragma unroll
      for (int r = 0; r < 2 * R - 1; ++r) sq[r] = __dmul_rn(win[r], win[r]);
#pragma unroll
      for (int jj = 0; jj < R; ++jj) {
        const double xj = xw[jb + jj];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          acc[r] = __dadd_rn(acc[r], __dmul_rn(xj, win[jj + r]));
          m2[r] = __dadd_rn(m2[r], sq[jj + r]);
        }
      }
    } else {
#pragma unroll
      for (int jj = 0; jj < R; ++jj) {
        const double xj = xw[jb + jj];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const double d = __dsub_rn(xj, win[jj + r]);
          acc[r] = __dadd_rn(acc[r], __dmul_rn(d, d));
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) win[r] = win[R + r];
  }
  if constexpr (NSDF) {
    const double m1 = readlane_f64(m2[0], 0);
    wave_lds_sync();                                       // every lane is done with the frame
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const double den = __dadd_rn(m1, m2[r]);
      const double v = den > 0 ? __ddiv_rn(__dmul_rn(2.0, acc[r]), den) : 0.0;   // :507-509
      if (on) {
        xw[t0 + r] = v;
        if (a.curve) a.curve[fi * a.width + t0 + r] = v;
      }
    }
    wave_lds_sync();
    pick_peaks(xw, 1, halfN - 2, 0, a, fi, lane);
    return;
  }
  // CMNDF :364-372: runningSum over tau = 1 .. halfN - 1 in order (a wave-uniform chain)
  double run = 0.0, myrun[R];
#pragma unroll
  for (int r = 0; r < R; ++r) myrun[r] = 0.0;
  for (int L = 0; L < nl; ++L) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (L == 0 && r == 0) continue;                      // tau = 0 is not summed
      run = __dadd_rn(run, readlane_f64(acc[r], L));
      myrun[r] = (lane == L) ? run : myrun[r];
    }
  }
  double cm[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int tau = t0 + r;
    cm[r] = tau == 0 ? 1.0 : __ddiv_rn(acc[r], __ddiv_rn(myrun[r], (double)tau));
    if (on && a.curve) a.curve[fi * a.width + tau] = cm[r];
  }
  // first tau in 1 .. halfN - 2 below the threshold with cm[tau] < cm[tau + 1] (:375-384)
  const double nxt0 = __shfl_down(cm[0], 1, 64);
  int fr = R;
#pragma unroll
  for (int r = R - 1; r >= 0; --r) {
    const int tau = t0 + r;
    const double nx = r < R - 1 ? cm[r + 1] : nxt0;
    if (on && tau >= 1 && cm[r] < a.yin_thr && tau + 1 < halfN && cm[r] < nx) fr = r;
  }
  const unsigned long long bal = __ballot(fr < R);
  int mt = -1;
  if (bal) {
    const int L = __ffsll((long long)bal) - 1;
    mt = R * L + __builtin_amdgcn_readlane(fr, L);
  }
  double p = 0.0, c = 0.0;
  int found = 0;
  if (mt > 0) {                                            // wave-uniform from here
    auto cm_at = [&](int tau) {                           // cm of a uniform tau, without a dynamic index
      const int r = tau % R, L = tau / R;
      double v = 0.0;
#pragma unroll
      for (int q = 0; q < R; ++q) { const double t = readlane_f64(cm[q], L); v = (r == q) ? t : v; }
      return v;
    };
    const double y2 = cm_at(mt);
    double period = (double)mt;                            // parabolicInterpolation :743-764
    if (mt < halfN - 1) {
      const double y1 = cm_at(mt - 1), y3 = cm_at(mt + 1);
      const double pa = __ddiv_rn(__dadd_rn(__dsub_rn(y1, __dmul_rn(2.0, y2)), y3), 2.0);
      const double pb = __ddiv_rn(__dsub_rn(y3, y1), 2.0);
      if (pa != 0.0) period = __dadd_rn((double)mt, __ddiv_rn(-pb, __dmul_rn(2.0, pa)));
    }
    const double f = __ddiv_rn((double)a.sr, period);
    if (f >= a.min_freq && f <= a.max_freq) { p = f; c = __dsub_rn(1.0, y2); found = 1; }
  }
  if (lane == 0) put_single(a, fi, p, c, mt, found);
}

// ------------------------------------------------------------ zero crossing ----
__global__ __launch_bounds__(256) void pitch_zc_kernel(const PitchArgs a) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t fi = (int64_t)blockIdx.x * PITCH_FRAMES_PER_BLOCK + w;
  if (fi >= a.F) return;
  const int64_t s = fi * a.hop;
  int cnt = 0;
  for (int i = 1 + lane; i < a.W; i += 64) {
    const double cur = pre_sample(a.pcm, s, i, a.pre, a.win), prv = pre_sample(a.pcm, s, i - 1, a.pre, a.win);
    if ((cur > 0 && prv <= 0) || (cur <= 0 && prv > 0)) ++cnt;          // :698
  }
  cnt = wave_sum<int>(cnt);
  if (lane == 0) {
    const double f = __ddiv_rn(__dmul_rn((double)cnt, (double)a.sr), __dmul_rn(2.0, (double)a.W));   // :704
    put_single(a, fi, f, 0.3, cnt, 1);
  }
}

// --------------------------------------------------------------------- ACF ----
// normalize (correlation.go:464-501) of the preprocessed frame: its mean and its population deviation
// are W-link ordered chains.  One frame per lane: a wave runs 64 chains at once (a wave per frame would
// run one), and the window value of a step is the same for every lane.  The consumers apply
// (x - mean) / sd while they load the frame.
__global__ __launch_bounds__(256) void pitch_stats_kernel(const PitchArgs a) {
  const int64_t fi = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (fi >= a.F) return;
  const double* x = a.pcm + fi * a.hop;
  double mean = 0.0, prev = 0.0;
  for (int i = 0; i < a.W; ++i) {
    const double v = x[i];
    const double y = (a.pre && i > 0) ? __dsub_rn(v, __dmul_rn(0.97, prev)) : v;
    prev = v;
    mean = __dadd_rn(mean, __dmul_rn(y, a.win[i]));
  }
  mean = __ddiv_rn(mean, (double)a.W);
  double var = 0.0;
  prev = 0.0;
  for (int i = 0; i < a.W; ++i) {
    const double v = x[i];
    const double y = (a.pre && i > 0) ? __dsub_rn(v, __dmul_rn(0.97, prev)) : v;
    prev = v;
    const double d = __dsub_rn(__dmul_rn(y, a.win[i]), mean);
    var = __dadd_rn(var, __dmul_rn(d, d));
  }
  a.stats[2 * fi] = mean;
  a.stats[2 * fi + 1] = sqrt(__ddiv_rn(var, (double)a.W));
}

__device__ __forceinline__ double z_sample(const PitchArgs& a, int64_t fi, int i) {
  const double d = __dsub_rn(pre_sample(a.pcm, fi * a.hop, i, a.pre, a.win), a.stats[2 * fi]);
  const double sd = a.stats[2 * fi + 1];
  return sd < 1e-10 ? d : __ddiv_rn(d, sd);               // minStdDev :488-499
}

// xcorr_kernels.hip's butterfly and level loop (Go's recursive fft unrolled, correlation.go:726-754)
// over N <= 4096 points held in LDS by one block; tw is the N-point table
__device__ __forceinline__ void butterfly(double c, double s, double& er, double& ei, double& odr, double& odi) {
  const double tr = __dsub_rn(__dmul_rn(c, odr), __dmul_rn(s, odi));
  const double ti = __dadd_rn(__dmul_rn(c, odi), __dmul_rn(s, odr));
  const double ar = er, ai = ei;
  er = __dadd_rn(ar, tr); ei = __dadd_rn(ai, ti);
  odr = __dsub_rn(ar, tr); odi = __dsub_rn(ai, ti);
}

__device__ void lds_fft(double* sre, double* sim, int N, int logN, const double2* tw) {
  for (int s = 1; s <= logN; ++s) {
    __syncthreads();
    const int h = 1 << (s - 1);
    const int stride = N >> s;
    for (int k = threadIdx.x; k < N / 2; k += 256) {
      const int i = k & (h - 1);
      const int p = ((k >> (s - 1)) << s) + i, q = p + h;
      const double2 w = tw[i * stride];
      double er = sre[p], ei = sim[p], odr = sre[q], odi = sim[q];
      butterfly(w.x, w.y, er, ei, odr, odi);
      sre[p] = er; sim[p] = ei; sre[q] = odr; sim[q] = odi;
    }
  }
  __syncthreads();
}

__device__ __forceinline__ int log2i(int N) { return 31 - __clz(N); }
__device__ __forceinline__ int bitrev(int j, int logN) { return (int)(__brev((unsigned)j) >> (32 - logN)); }

// computeFFT on (z, z), N = 2 W (nextPowerOf2(2 W - 1)): the transform, the point-wise
// conj(A conj(A)) with ifft's leading conjugate folded in, the transform again, re / N at lag or N + lag.
__global__ __launch_bounds__(256) void pitch_acf_fft_kernel(const PitchArgs a) {
  extern __shared__ double lds[];
  const int W = a.W, N = 2 * W, logN = log2i(N);
  double* sre = lds;
  double* sim = lds + N;
  const int64_t fi = blockIdx.x;
  for (int j = threadIdx.x; j < N; j += 256) {
    const int src = bitrev(j, logN);
    sre[j] = src < W ? z_sample(a, fi, src) : 0.0;
    sim[j] = 0.0;
  }
  lds_fft(sre, sim, N, logN, a.tw);
  double pr[PITCH_MAX_FFT / 256], pi[PITCH_MAX_FFT / 256];
#pragma unroll
  for (int q = 0; q < PITCH_MAX_FFT / 256; ++q) {
    const int j = threadIdx.x + 256 * q;
    pr[q] = 0.0; pi[q] = 0.0;
    if (j < N) {
      const double ux = sre[j], uy = sim[j];
      const double c = ux, d = -uy;
      pr[q] = __dsub_rn(__dmul_rn(ux, c), __dmul_rn(uy, d));
      pi[q] = -__dadd_rn(__dmul_rn(ux, d), __dmul_rn(uy, c));
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < PITCH_MAX_FFT / 256; ++q) {
    const int j = threadIdx.x + 256 * q;
    if (j < N) { const int jr = bitrev(j, logN); sre[jr] = pr[q]; sim[jr] = pi[q]; }
  }
  lds_fft(sre, sim, N, logN, a.tw);
  const int L = W - 1, nlag = 2 * W - 1;                   // calculateActualMaxLag: min(2 W, W - 1)
  for (int k = threadIdx.x; k < nlag; k += 256) {
    const int lag = k - L;
    const double v = __ddiv_rn(sre[lag >= 0 ? lag : N + lag], (double)N);
    sim[k] = v;
    if (a.curve) a.curve[fi * a.width + k] = v;
  }
  __syncthreads();
  if (threadIdx.x < 64) pick_peaks(sim, L + 1, nlag - 2, L, a, fi, threadIdx.x);   // lags 1 .. W - 2 (:436-443)
}

// pearsonCorrelation per lag on (z, z) (xcorr_pearson_kernel's arithmetic).  With both signals the same
// frame, lag -l is lag l with the two windows exchanged: the means and the squared sums change places, the
// products d1 d2 and q1 q2 commute, and every sum keeps its order, so the value has the same bits.  Only the
// lags 0 .. W - 1 are walked and each is written twice.  A thread takes the lags t and W - 1 - t, whose
// overlaps W - t and t + 1 add up to W + 1 for every thread.
__global__ __launch_bounds__(256) void pitch_acf_time_kernel(const PitchArgs a) {
  __shared__ double zs[512], cv[1024];
  const int W = a.W, L = W - 1, nlag = 2 * W - 1;
  const int64_t fi = blockIdx.x;
  for (int i = threadIdx.x; i < W; i += 256) zs[i] = z_sample(a, fi, i);
  __syncthreads();
  const int t = threadIdx.x;                               // W / 2 <= 256: one pair of lags per thread
  for (int h = 0; h < 2 && t < W / 2; ++h) {
    const int lag = h ? W - 1 - t : t;
    const int s1 = 0, s2 = lag;                             // calculateOverlapRegion :421-449
    const int ov = W - lag;
    double c = 0.0;
    if (ov > 1) {
      double m1 = 0.0, m2 = 0.0, num = 0.0, q1 = 0.0, q2 = 0.0;
      for (int i = 0; i < ov; ++i) { m1 = __dadd_rn(m1, zs[s1 + i]); m2 = __dadd_rn(m2, zs[s2 + i]); }
      m1 = __ddiv_rn(m1, (double)ov);
      m2 = __ddiv_rn(m2, (double)ov);
      for (int i = 0; i < ov; ++i) {
        const double d1 = __dsub_rn(zs[s1 + i], m1), d2 = __dsub_rn(zs[s2 + i], m2);
        num = __dadd_rn(num, __dmul_rn(d1, d2));
        q1 = __dadd_rn(q1, __dmul_rn(d1, d1));
        q2 = __dadd_rn(q2, __dmul_rn(d2, d2));
      }
      const double dn = sqrt(__dmul_rn(q1, q2));
      if (!(dn < 1e-10)) {
        c = __ddiv_rn(num, dn);
        if (c > 1.0) c = 1.0;
        else if (c < -1.0) c = -1.0;
      }
    }
    cv[L + lag] = c; cv[L - lag] = c;
    if (a.curve) { a.curve[fi * a.width + L + lag] = c; a.curve[fi * a.width + L - lag] = c; }
  }
  __syncthreads();
  if (threadIdx.x < 64) pick_peaks(cv, L + 1, nlag - 2, L, a, fi, threadIdx.x);
}

// ----------------------------------------------------------- HPS, cepstrum ----
// The first index of the largest value of cv[lo, end) that beats cv[i0], else i0: Go's scan from
// (i0, cv[i0]) with a strict > (a NaN never wins, and nothing beats a NaN start).  Wave 0 of the block.
__device__ void scan_max(const double* cv, int i0, int lo, int end, int lane, int* idx, double* val) {
  double bv = -__builtin_huge_val();
  int bi = kNone;
  for (int i = lo + lane; i < end; i += 64) {
    const double v = cv[i];
    if (v > bv) { bv = v; bi = i; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  const double init = cv[i0];
  const bool beats = bi != kNone && bv > init;
  *idx = beats ? bi : i0;
  *val = beats ? bv : init;
}

template <bool CEPSTRUM>
__global__ __launch_bounds__(256) void pitch_spectrum_kernel(const PitchArgs a) {
  extern __shared__ double lds[];
  const int W = a.W, N = CEPSTRUM ? W : W * a.zp, logN = log2i(N);
  double* sre = lds;
  double* sim = lds + N;
  const int64_t fi = blockIdx.x;
  const int64_t s = fi * a.hop;
  for (int j = threadIdx.x; j < N; j += 256) {
    const int src = bitrev(j, logN);
    sre[j] = src < W ? pre_sample(a.pcm, s, src, a.pre, a.win) : 0.0;
    sim[j] = 0.0;
  }
  lds_fft(sre, sim, N, logN, a.tw);
  double t[PITCH_MAX_FFT / 256];
  if constexpr (CEPSTRUM) {
    // ln(|X| + 1e-10) of all W bins (:627-634), then the inverse transform's real part (:637-643): the
    // input is real, so that is re(fft(.)) / W
#pragma unroll
    for (int q = 0; q < PITCH_MAX_FFT / 256; ++q) {
      const int j = threadIdx.x + 256 * q;
      t[q] = j < N ? log(hypot(sre[j], sim[j]) + 1e-10) : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < PITCH_MAX_FFT / 256; ++q) {
      const int j = threadIdx.x + 256 * q;
      if (j < N) { const int jr = bitrev(j, logN); sre[jr] = t[q]; sim[jr] = 0.0; }
    }
    lds_fft(sre, sim, N, logN, a.tw);
    for (int j = threadIdx.x; j < N; j += 256) {
      const double v = sre[j] / (double)N;
      sim[j] = v;
      if (a.curve) a.curve[fi * a.width + j] = v;
    }
    __syncthreads();
    if (threadIdx.x < 64) {
      int idx; double val;
      scan_max(sim, a.lo, a.lo, a.hi < N ? a.hi : N, threadIdx.x, &idx, &val);      // :646-657
      if (threadIdx.x == 0) {
        const double q = val / 0.1;
        const double conf = q != q ? q : (q < 1.0 ? q : 1.0);                        // math.Min(q, 1)
        put_single(a, fi, (double)a.sr / (double)idx, conf, idx, 1);
      }
    }
  } else {
    const int len = N / 2;                                                           // :562-565
#pragma unroll
    for (int q = 0; q < PITCH_MAX_FFT / 256; ++q) {
      const int j = threadIdx.x + 256 * q;
      t[q] = j < len ? sqrt(sre[j] * sre[j] + sim[j] * sim[j]) : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < PITCH_MAX_FFT / 256; ++q) {
      const int j = threadIdx.x + 256 * q;
      if (j < len) sre[j] = t[q];
    }
    __syncthreads();
    for (int j = threadIdx.x; j < len; j += 256) {                                   // :568-576
      double v = sre[j];
      for (int h = 2; h <= 5; ++h)
        if (j < len / h) v = v * sre[j * h];
      sim[j] = v;
      if (a.curve) a.curve[fi * a.width + j] = v;
    }
    __syncthreads();
    if (threadIdx.x < 64) {
      int idx; double val;
      scan_max(sim, 0, a.lo, a.hi < len ? a.hi : len, threadIdx.x, &idx, &val);      // :579-590
      if (threadIdx.x == 0) {
        const double f = (double)idx * (double)a.sr / (double)N;                     // :593
        double conf = 0.0;
        if (val > 0) { const double q = val / 1000.0; conf = q < 1.0 ? q : 1.0; }    // :596-600
        put_single(a, fi, f, conf, idx, 1);
      }
    }
  }
}

int launch_pitch_frames(const PitchArgs& a, hipStream_t s) {
  const int W = a.W;
  if (W < PITCH_MIN_W || W > PITCH_MAX_W || (W & (W - 1)) || a.F < 1 || a.hop < 1 || a.K < 0 ||
      a.K > PITCH_MAX_CANDIDATES || !a.pcm || !a.win || !a.pitch || !a.conf)
    return -1;
  if ((a.F - 1) * a.hop + W > a.n) return -1;
  const unsigned per4 = (unsigned)((a.F + PITCH_FRAMES_PER_BLOCK - 1) / PITCH_FRAMES_PER_BLOCK);
#define SONAR_PITCH_LAG(R, NL)                                                                                    \
  do {                                                                                                           \
    if (a.method == SONAR_PITCH_NSDF) hipLaunchKernelGGL((pitch_lag_kernel<R, NL, true>), dim3(per4), dim3(256), 0, s, a);       \
    else hipLaunchKernelGGL((pitch_lag_kernel<R, NL, false>), dim3(per4), dim3(256), 0, s, a);                    \
  } while (0)
  switch (a.method) {
    case SONAR_PITCH_YIN:
    case SONAR_PITCH_NSDF:
      switch (W) {
        case 64: SONAR_PITCH_LAG(1, 32); break;
        case 128: SONAR_PITCH_LAG(1, 64); break;
        case 256: SONAR_PITCH_LAG(2, 64); break;
        case 512: SONAR_PITCH_LAG(4, 64); break;
        case 1024: SONAR_PITCH_LAG(8, 64); break;
        default: SONAR_PITCH_LAG(16, 64); break;
      }
      break;
    case SONAR_PITCH_ZERO_CROSSING:
      hipLaunchKernelGGL(pitch_zc_kernel, dim3(per4), dim3(256), 0, s, a);
      break;
    case SONAR_PITCH_ACF:
      if (!a.stats || a.width != 2 * W - 1) return -1;
      hipLaunchKernelGGL(pitch_stats_kernel, dim3((unsigned)((a.F + 255) / 256)), dim3(256), 0, s, a);
      if (W > 1000) {
        if (!a.tw) return -1;
        hipLaunchKernelGGL(pitch_acf_fft_kernel, dim3((unsigned)a.F), dim3(256), (size_t)4 * W * sizeof(double), s, a);
      } else {
        if (W > 512) return -1;
        hipLaunchKernelGGL(pitch_acf_time_kernel, dim3((unsigned)a.F), dim3(256), 0, s, a);
      }
      break;
    case SONAR_PITCH_HPS: {
      const int N = W * a.zp;
      if (!a.tw || (a.zp != 1 && a.zp != 2 && a.zp != 4) || N > PITCH_MAX_FFT || a.lo < 0) return -1;
      hipLaunchKernelGGL((pitch_spectrum_kernel<false>), dim3((unsigned)a.F), dim3(256), (size_t)2 * N * sizeof(double), s, a);
      break;
    }
    case SONAR_PITCH_CEPSTRUM:
      if (!a.tw || a.lo < 0 || a.lo >= W) return -1;
      hipLaunchKernelGGL((pitch_spectrum_kernel<true>), dim3((unsigned)a.F), dim3(256), (size_t)2 * W * sizeof(double), s, a);
      break;
    default:
      return -1;
  }
#undef SONAR_PITCH_LAG
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // namespace sonar
