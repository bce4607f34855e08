// harmonic_ratio_kernels.hip -- HarmonicRatioAnalyzer.AnalyzeFrame per frame (algorithms/tonal/harmonic_ratio.go:205-924),
// up to postProcessResult, float64 like the Go reference.
//
//  hratio_kernel<PCM>      analyzeHNR / analyzeComb (:297-382, 457-461), analyzeHPS (:413-454) and
//                          analyzeSpectral (:463-512) after computeSpectrum (:273-294): one block per frame.
//                          PCM: the Hann-windowed frame is transformed in LDS (pitch_spectrum_kernel's
//                          butterfly, table and level order), |X| of the first W / 2 bins; else the row is loaded.
//  hratio_window_kernel    preprocessFrame (:260-270) into rows of W, the input of the pitch kernels that
//                          run AutoCorrelation.Compute (ACF) and the temporary detector's YIN
//  hratio_acf_tail_kernel  analyzeACF's tail (:392-410): one wave per row of correlations
//  hratio_yin_tail_kernel  analyzeYin's tail (:532-541)
//
// The stage of hratio_kernel, in order, every K-entry array in LDS:
//  1. MovingAverage (common/math.go:140-166): one bin per thread, its own trailing sum in j order.
//  2. estimateNoiseFloor (:632-705): one bin per thread; the <= 20 values of its window go to registers and
//     the quantile is a rank selection by comparison counts (the value with fewer than c smaller and at
//     least c not larger, c the first count that reaches p n); then MovingAverage again.
//  3. DetectPeaks (spectral_peaks.go:36-100), hpcp_rows_kernel's routine: candidates compacted in bin order
//     by wave 0, the distance rule against the last kept peak by lane 0 (from 3 bins on), the rank of every
//     kept peak in (magnitude descending, bin ascending) by all threads; ranks below 100 are the list.
//  4. the f0 of the method; findHarmonicPeaks (:565-594) with one lane per harmonic, compacted in h order.
//  5. per bin: the range, mask and isHarmonic flags; then the ordered K-link sums (total, harmonic and
//     noise energy, the two periodicity sums, the SNR's noise sum; its signal sum is the total energy's
//     chain term for term) as six concurrent chains on six lanes of wave 0, the masked terms added as exact
//     zeros (every term is >= 0 and the sums start at +0).
//  6. roughness: the pair terms in chunks by all threads, added in (i, j) order by one; the scalars.
// Every comparison and every sum here decides an output bit: built without FMA contraction.
#include <cstdint>

#include "harmonic_ratio_kernels.h"
#include "lds_fft.h"
#include "wave.h"
#include "../../include/sonar_gpu.h"

#pragma clang fp contract(off)

namespace sonar {

namespace {

constexpr int kNone = 0x7fffffff;

// hpcp_kernels.hip's key: larger magnitude <-> larger key; -0.0 and +0.0 share one
__device__ __forceinline__ uint64_t order_key(double m) {
  const uint64_t u = (uint64_t)__double_as_longlong(m + 0.0);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// freqBins[i] (:195); at a power-of-two W the detector's float64(i) * (sr / W) is the same double
__device__ __forceinline__ double bin_freq(int i, int sr, int W) { return (double)i * (double)sr / (double)W; }

// isHarmonic (:913-924)
__device__ __forceinline__ bool is_harmonic(double freq, double f0, double tol) {
  if (!(f0 > 0)) return false;
  const double expected = f0 * round(freq / f0);
  return fabs(freq - expected) < tol * expected;
}

// MovingAverage (common/math.go:140-166) of in[0, K) into out, by the block; L <= 1 copies (the callers'
// "if len > 1", :286, :645), and so do L > K (:141)
__device__ void moving_average(const double* in, double* out, int K, int L) {
  const bool on = L > 1 && L <= K;
  for (int i = threadIdx.x; i < K; i += 256) {
    double v = in[i];
    if (on) {
      const int j0 = i < L ? 0 : i - L + 1;
      double sum = 0.0;
      for (int j = j0; j <= i; ++j) sum = sum + in[j];
      v = sum / (double)(i < L ? i + 1 : L);
    }
    out[i] = v;
  }
  __syncthreads();
}

// compute*NoiseFloor (:650-705) of bin i over m[0, K)
__device__ double noise_floor_bin(const double* m, int K, int i, int method, double pct, int pct_ok) {
  constexpr int H = HRATIO_NOISE_WINDOW / 2;
  const int s = i - H > 0 ? i - H : 0, e = i + H < K ? i + H : K;
  const int n = e - s;
  double wv[HRATIO_NOISE_WINDOW];
#pragma unroll
  for (int k = 0; k < HRATIO_NOISE_WINDOW; ++k) wv[k] = k < n ? m[s + k] : 0.0;
  if (method == SONAR_HRATIO_NOISE_MINIMUM) {
    double mn = wv[0];
#pragma unroll
    for (int k = 1; k < HRATIO_NOISE_WINDOW; ++k)
      if (k < n && wv[k] < mn) mn = wv[k];
    return mn;
  }
  const double p = method == SONAR_HRATIO_NOISE_MEDIAN ? 0.5 : pct;
  if (method != SONAR_HRATIO_NOISE_MEDIAN && !pct_ok) return 0.0;       // common.Percentile (math.go:39)
  // stat.Quantile(p, stat.Empirical, sorted, nil): the first sorted value whose count reaches p n
  const double fidx = p * (double)n;
  int c = 1;
  while (c < n && (double)c < fidx) ++c;
  double r = 0.0;
#pragma unroll
  for (int j = 0; j < HRATIO_NOISE_WINDOW; ++j) {
    int less = 0, leq = 0;
#pragma unroll
    for (int k = 0; k < HRATIO_NOISE_WINDOW; ++k) {
      less += (k < n && wv[k] < wv[j]) ? 1 : 0;
      leq += (k < n && wv[k] <= wv[j]) ? 1 : 0;
    }
    if (j < n && less < c && c <= leq) r = wv[j];
  }
  return r;
}

struct Harmonic { int bin; double freq, amp; };

// findNearestPeak (:596-630) of one expected frequency and findHarmonicPeaks' tolerance test (:585-589)
__device__ bool nearest_peak(const double* m, int K, int W, int sr, int width, double expected, double tol, Harmonic* out) {
  const int tb = (int)(expected * (double)W / (double)sr);
  if (tb >= K) return false;
  const int64_t lo64 = (int64_t)tb - width, hi64 = (int64_t)tb + width + 1;
  const int lo = lo64 > 0 ? (int)lo64 : 0, hi = hi64 < K ? (int)hi64 : K;
  double mx = 0.0;
  int mb = tb;
  for (int i = lo; i < hi; ++i)
    if (m[i] > mx) { mx = m[i]; mb = i; }
  if (!(mb > 0 && mb < K - 1)) return false;
  if (!(m[mb] > m[mb - 1] && m[mb] > m[mb + 1])) return false;
  const double f = bin_freq(mb, sr, W);
  if (!(fabs(f - expected) < tol * expected)) return false;
  out->bin = mb; out->freq = f; out->amp = m[mb];
  return true;
}

}  // namespace

// LDS, in doubles: PCM  re[W] | im[W] | C[K]   with A = re + K, B = im + K (the upper halves the magnitudes
//                  do not read); spectrum  A[K] | B[K] | C[K].  A: |X|, then the raw floor, then scratch;
//                  B: hra.magnitude; C: hra.noiseFloor.
// Then keys[K / 2] (u64) | hf[64] | ha[64] | term[128] | sc[8] | hb[64] (int) | misc[8] (int) |
// cbin[K / 2] (u16) | sbin[128] | vbin[128] | flags[K] (u8)
size_t hratio_lds_bytes(int K, bool pcm) {
  return 8 * ((size_t)(pcm ? 5 : 3) * K + K / 2 + 64 + 64 + HRATIO_PEAK_SLOTS + 8) + 4 * (64 + 8) +
         2 * ((size_t)K / 2 + 2 * HRATIO_PEAK_SLOTS) + (size_t)K;
}

template <bool PCM>
__global__ __launch_bounds__(256) void hratio_kernel(const HratioArgs a) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int K = a.K, W = a.W, sr = a.sr;
  const int64_t fi = blockIdx.x;
  double *sre = lds, *sim = lds + W;
  double* A = PCM ? sre + K : lds;
  double* B = PCM ? sim + K : lds + K;
  double* C = PCM ? lds + 2 * W : lds + 2 * K;
  uint64_t* keys = (uint64_t*)(C + K);
  double* hf = (double*)(keys + K / 2);
  double* ha = hf + 64;
  double* term = ha + 64;
  double* sc = term + HRATIO_PEAK_SLOTS;
  int* hb = (int*)(sc + 8);
  int* misc = hb + 64;
  uint16_t* cbin = (uint16_t*)(misc + 8);
  uint16_t* sbin = cbin + K / 2;
  uint16_t* vbin = sbin + HRATIO_PEAK_SLOTS;
  uint8_t* flags = (uint8_t*)(vbin + HRATIO_PEAK_SLOTS);
  const uint64_t below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  const HratioOut& o = a.o;
  const bool hnr = a.method == SONAR_HRATIO_HNR;

  // ---- computeSpectrum: |X| (:278-283)
  if constexpr (PCM) {
    const int logN = fft_log2i(W);
    const int64_t s = fi * a.hop;
    for (int j = tid; j < W; j += 256) {
      const int src = fft_bitrev(j, logN);
      sre[j] = a.pcm[s + src] * a.win[src];
      sim[j] = 0.0;
    }
    lds_fft_256(sre, sim, W, logN, a.tw);
    for (int i = tid; i < K; i += 256) A[i] = sqrt(sre[i] * sre[i] + sim[i] * sim[i]);
  } else {
    for (int i = tid; i < K; i += 256) A[i] = a.mag[fi * K + i];
  }
  __syncthreads();
  moving_average(A, B, K, a.smooth);                                    // 1. (:286-288)
  // 2. the noise floor: only analyzeHNR's result carries it (:374-375)
  const bool want_floor = hnr && (o.snr || o.noise_floor);
  if (want_floor) {
    for (int i = tid; i < K; i += 256) A[i] = noise_floor_bin(B, K, i, a.nf_method, a.pct, a.pct_ok);
    __syncthreads();
    moving_average(A, C, K, a.nf_smooth);
  }
  if (o.noise_floor)
    for (int i = tid; i < K; i += 256) o.noise_floor[fi * K + i] = want_floor ? C[i] : 0.0;

  // ---- 3. DetectPeaks(B, W) -> sbin[0, nsel), by (magnitude descending, bin ascending)
  int nsel = 0;
  if (a.method != SONAR_HRATIO_HPS) {
    if (tid < 64) {
      int Cn = 0;
      for (int b0 = 1; b0 < K - 1; b0 += 64) {
        const int i = b0 + lane;
        bool cand = false;
        double m = 0.0;
        if (i < K - 1) {
          m = B[i];
          cand = m > B[i - 1] && m > B[i + 1] && m >= a.min_height;
        }
        const uint64_t b = __ballot(cand);
        if (cand) {
          const int pos = Cn + __popcll(b & below);                     // < (K - 1) / 2: strict maxima are 2 bins apart
          keys[pos] = order_key(m);
          cbin[pos] = (uint16_t)i;
        }
        Cn += __popcll(b);
      }
      wave_lds_sync();
      if (a.min_dist >= 3 && Cn > 1 && lane == 0) {                      // :56-73 against the last kept peak
        int n = 1;
        uint64_t lk = keys[0];
        int lb = cbin[0];
        for (int j = 1; j < Cn; ++j) {
          const uint64_t k = keys[j];
          const int b = cbin[j];
          if (b - lb < a.min_dist) {
            if (k > lk) { keys[n - 1] = k; cbin[n - 1] = (uint16_t)b; lk = k; lb = b; }
          } else {
            keys[n] = k; cbin[n] = (uint16_t)b; ++n; lk = k; lb = b;
          }
        }
        Cn = n;
      }
      if (lane == 0) misc[0] = Cn;
    }
    __syncthreads();
    const int Cn = misc[0];
    for (int s = tid; s < Cn; s += 256) {
      const uint64_t k = keys[s];
      int rank = 0;
      for (int j = 0; j < Cn; ++j) {
        const uint64_t kj = keys[j];
        rank += (kj > k || (kj == k && j < s)) ? 1 : 0;
      }
      if (rank < HRATIO_MAX_PEAKS) sbin[rank] = cbin[s];                // :95-97
    }
    nsel = Cn < HRATIO_MAX_PEAKS ? Cn : HRATIO_MAX_PEAKS;
    __syncthreads();
  }

  // ---- 4. the method's f0 -> sc[0], its confidence -> sc[1], the method's own value -> sc[2]
  int nv = 0;                                                           // SPECTRAL: validPeaks in vbin
  if (hnr) {
    if (tid < 64) {                                                     // detectFundamentalFrequency :546-563
      int first = kNone;
      for (int r0 = 0; r0 < nsel && first == kNone; r0 += 64) {
        const int r = r0 + lane;
        const bool ok = r < nsel && bin_freq(sbin[r], sr, W) >= a.min_freq;
        const uint64_t b = __ballot(ok);
        if (b) first = r0 + __ffsll((long long)b) - 1;
      }
      if (lane == 0) {
        const int r = first != kNone ? first : 0;
        sc[0] = nsel ? bin_freq(sbin[r], sr, W) : 0.0;
        sc[1] = nsel ? B[sbin[r]] : 0.0;
      }
    }
  } else if (a.method == SONAR_HRATIO_HPS) {
    const int top = a.max_h < 5 ? a.max_h : 5;                          // :420
    for (int i = tid; i < K; i += 256) {
      double v = B[i];
      for (int h = 2; h <= top; ++h)
        if (i < K / h) v = v * B[i * h];
      A[i] = v;
    }
    __syncthreads();
    if (tid < 64) {                                                     // :427-438, a strict > from (0, hps[0])
      const int end = a.hps_hi < K ? a.hps_hi : K;
      double bv = -__builtin_huge_val();
      int bi = kNone;
      for (int i = a.hps_lo + lane; i < end; i += 64) {
        const double v = A[i];
        if (v > bv) { bv = v; bi = i; }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(bv, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
      }
      if (lane == 0) {
        const double init = A[0];
        const bool beats = bi != kNone && bv > init;
        sc[0] = bin_freq(beats ? bi : 0, sr, W);
        sc[1] = 0.0;
        sc[2] = beats ? bv : init;
      }
    }
  } else {
    if (tid < 64) {                                                     // analyzeSpectral :468-477
      for (int r0 = 0; r0 < nsel; r0 += 64) {
        const int r = r0 + lane;
        bool ok = false;
        if (r < nsel) {
          const double f = bin_freq(sbin[r], sr, W);
          ok = f >= a.min_freq && f <= a.max_freq;
        }
        const uint64_t b = __ballot(ok);
        if (ok) vbin[nv + __popcll(b & below)] = sbin[r];
        nv += __popcll(b);
      }
      wave_lds_sync();
      // estimateF0FromPeaks (:832-863): validPeaks is sorted already and the second sort keeps its order
      double best_f0 = 0.0, best = 0.0;
      const int ncand = nv < 5 ? nv : 5;
      for (int q = 0; q < ncand; ++q) {
        const double cf = bin_freq(vbin[q], sr, W);                     // > 0: a peak's bin is >= 1
        const int maxh = (int)(a.max_freq / cf);                        // evaluateF0Candidate :865-892
        const int h = lane + 1;
        double t = 0.0;
        if (h <= maxh && h <= a.max_h) {
          const double expected = cf * (double)h;
          int cb = vbin[0];                                             // findClosestPeak :894-911
          double md = fabs(bin_freq(cb, sr, W) - expected);
          for (int k = 1; k < nv; ++k) {
            const double d = fabs(bin_freq(vbin[k], sr, W) - expected);
            if (d < md) { md = d; cb = vbin[k]; }
          }
          const double tolr = a.tol * expected;
          if (md < tolr) t = (1.0 - md / tolr) * B[cb];
        }
        double score = 0.0;
        for (int L = 0; L < HRATIO_MAX_HARMONICS; ++L) score = score + readlane_f64(t, L);
        if (score > best) { best = score; best_f0 = cf; }
      }
      if (lane == 0) { sc[0] = best_f0; sc[1] = 0.0; misc[1] = nv; }
    }
  }
  __syncthreads();
  const double f0 = sc[0];
  if (a.method == SONAR_HRATIO_SPECTRAL) nv = misc[1];

  // ---- findHarmonicPeaks(f0) :565-594 -> hb / hf / ha[0, nh), and the h_* rows
  if (tid < 64) {
    Harmonic hm{0, 0.0, 0.0};
    bool found = false;
    if (f0 > 0) {
      const double q = a.max_freq / f0;
      const int maxh = (int)((double)a.max_h < q ? (double)a.max_h : q);
      const int h = lane + 1;
      const double expected = f0 * (double)h;
      if (h <= maxh && !(expected > a.max_freq)) found = nearest_peak(B, K, W, sr, a.width, expected, a.tol, &hm);
    }
    const uint64_t b = __ballot(found);
    const int slot = __popcll(b & below), nh = __popcll(b);
    if (found) { hb[slot] = hm.bin; hf[slot] = hm.freq; ha[slot] = hm.amp; }
    if (lane == 0) misc[2] = nh;
    wave_lds_sync();
    if (lane < a.max_h) {
      const int64_t oi = fi * a.max_h + lane;
      const bool on = lane < nh;
      const int bin = on ? hb[lane] : -1;
      if (o.h_bin) o.h_bin[oi] = bin;
      if (o.h_freq) o.h_freq[oi] = on ? hf[lane] : 0.0;
      if (o.h_amp) o.h_amp[oi] = on ? ha[lane] : 0.0;
      if (o.h_phase) {
        double ph = 0.0;                                                // hra.phase[maxBin] :282, :623
        if (on) {
          if constexpr (PCM) ph = atan2(sim[bin], sre[bin]);
          else ph = a.phase ? a.phase[fi * K + bin] : 0.0;
        }
        o.h_phase[oi] = ph;
      }
    }
  }
  __syncthreads();
  const int nh = misc[2];

  // the outputs a method leaves unset are 0
  double ratio = 0.0, harm_e = 0.0, noise_e = 0.0, total_e = 0.0, snr = 0.0, periodicity = 0.0, harmonicity = 0.0,
         voicing = 0.0, roughness = 0.0;
  if (a.method == SONAR_HRATIO_HPS) {
    ratio = 20.0 * log10(sc[2] + 1e-10);                                // :446
  } else if (a.method == SONAR_HRATIO_SPECTRAL) {
    for (int k = tid; k < nv; k += 256) {                               // :484-492
      const double m = B[vbin[k]];
      term[k] = m * m;
      flags[k] = is_harmonic(bin_freq(vbin[k], sr, W), f0, a.tol) ? 1 : 0;
    }
    __syncthreads();
    if (tid == 0) {
      for (int k = 0; k < nv; ++k) {
        total_e = total_e + term[k];
        if (flags[k]) harm_e = harm_e + term[k];
      }
      noise_e = total_e - harm_e;                                        // :494
      ratio = noise_e > 0 ? 10.0 * log10(harm_e / noise_e) : 60.0;
    }
  } else {
    // ---- 5. flags: 1 in [min_freq, max_freq], 2 harmonicMask (:312-320), 4 isHarmonic(freq, f0)
    for (int i = tid; i < K; i += 256) {
      const double f = bin_freq(i, sr, W);
      int fl = (f >= a.min_freq && f <= a.max_freq) ? 1 : 0;
      for (int p = 0; p < nh; ++p) {
        const int64_t b = (int64_t)(int)(hf[p] * (double)W / (double)sr);
        if (i >= b - a.width && i < b + a.width + 1) { fl |= 2; break; }
      }
      if (is_harmonic(f, f0, a.tol)) fl |= 4;
      flags[i] = (uint8_t)fl;
    }
    __syncthreads();
    if (tid < 64) {
      // lanes 0..5: total / harmonic / noise energy (:323-335), total / harmonic strength (:716-725),
      // the SNR's noise energy (:798-807)
      const int need = lane == 1 ? 3 : lane == 4 ? 5 : 1;
      const int forbid = lane == 2 ? 2 : 0;
      const int sel = lane < 3 ? 0 : lane < 5 ? 1 : 2;
      const bool with_floor = want_floor;
      double acc = 0.0;
#pragma unroll 8                                                      // K is a multiple of 32; no measurable effect (Kernel 4j)
      for (int i = 0; i < K; ++i) {
        const int fl = flags[i];
        const double m = B[i], nf = with_floor ? C[i] : 0.0;
        const double v = sel == 0 ? m * m : sel == 1 ? m : nf * nf;
        const bool take = (fl & need) == need && !(fl & forbid);
        acc = acc + (take ? v : 0.0);
      }
      total_e = readlane_f64(acc, 0);
      harm_e = readlane_f64(acc, 1);
      noise_e = readlane_f64(acc, 2);
      const double strength = readlane_f64(acc, 3), hstrength = readlane_f64(acc, 4);
      const double floor_e = readlane_f64(acc, 5);
      ratio = noise_e > 0 ? 10.0 * log10(harm_e / noise_e) : 60.0;      // :338-343
      snr = floor_e > 0 ? 10.0 * log10(total_e / floor_e) : 60.0;        // :809-813
      periodicity = (f0 > 0 && strength > 0) ? hstrength / strength : 0.0;   // :707-732
      voicing = 1.0 / (1.0 + exp(-0.1 * (ratio - 10.0)));                // :759-763
      if (nh > 0 && f0 > 0) {                                            // calculateHarmonicity :734-757
        double dev = 0.0;
        for (int p = 0; p < nh; ++p) {
          const double expected = f0 * round(hf[p] / f0);
          dev = dev + fabs(hf[p] - expected) / expected;
        }
        harmonicity = exp(-(dev / (double)nh) * 10.0);
      }
    }
    // ---- 6. calculateRoughness (:765-791): the pair terms, K at a time into A, added in (i, j) order
    const int npairs = nh * (nh - 1) / 2;
    for (int c0 = 0; c0 < npairs; c0 += K) {
      __syncthreads();
      for (int t = tid; t < K && c0 + t < npairs; t += 256) {
        int p = c0 + t, i = 0;
        while (p >= nh - 1 - i) { p -= nh - 1 - i; ++i; }
        const int j = i + 1 + p;
        const double d = fabs(hf[i] - hf[j]);
        A[t] = d > 0 ? (ha[i] * ha[j]) / (d + 1.0) : 0.0;
      }
      __syncthreads();
      if (tid == 0)
        for (int t = 0; t < K && c0 + t < npairs; ++t) roughness = roughness + A[t];
    }
  }
  if (tid == 0) {
    if (o.ratio) o.ratio[fi] = ratio;
    if (o.harm_e) o.harm_e[fi] = harm_e;
    if (o.noise_e) o.noise_e[fi] = noise_e;
    if (o.total_e) o.total_e[fi] = total_e;
    if (o.f0) o.f0[fi] = f0;
    if (o.f0_conf) o.f0_conf[fi] = hnr ? sc[1] : 0.0;
    if (o.snr) o.snr[fi] = snr;
    if (o.periodicity) o.periodicity[fi] = periodicity;
    if (o.harmonicity) o.harmonicity[fi] = harmonicity;
    if (o.voicing) o.voicing[fi] = voicing;
    if (o.roughness) o.roughness[fi] = roughness;
    if (o.num) o.num[fi] = nh;
  }
}

__global__ __launch_bounds__(256) void hratio_window_kernel(const double* pcm, int64_t hop, int W, const double* win,
                                                            int64_t f0, double* out) {
  const int64_t f = blockIdx.x;
  const double* x = pcm + (f0 + f) * hop;
  for (int i = threadIdx.x; i < W; i += 256) out[f * W + i] = x[i] * win[i];
}

// max |corr| over the row (:396-401) and over its entries from 1 on (calculatePeriodicityFromACF :816-830);
// a NaN never wins either scan
__global__ __launch_bounds__(64) void hratio_acf_tail_kernel(const double* corr, int width, int64_t f0, const HratioOut o) {
  const int lane = threadIdx.x;
  const int64_t f = blockIdx.x, fo = f0 + f;
  const double* row = corr + f * (int64_t)width;
  double mx = 0.0, mx1 = 0.0;
  for (int i = lane; i < width; i += 64) {
    const double v = fabs(row[i]);
    if (v > mx) mx = v;
    if (i >= 1 && v > mx1) mx1 = v;
  }
  mx = wave_max<double>(mx);
  mx1 = wave_max<double>(mx1);
  if (lane == 0) {
    if (o.ratio) o.ratio[fo] = 20.0 * log10(mx / (1.0 - mx + 1e-10));   // :404
    if (o.periodicity) o.periodicity[fo] = mx1;
    if (o.voicing) o.voicing[fo] = mx;
  }
}

__global__ __launch_bounds__(256) void hratio_yin_tail_kernel(const double* pitch, const double* conf, int64_t f0, int64_t nf,
                                                              const HratioOut o) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= nf) return;
  const int64_t fo = f0 + f;
  // postProcessResult of the temporary detector (pitch_detection.go:767-790): Periodicity is the raw
  // confidence; the min_confidence gate at 0 zeroes pitch, confidence and voicing of a negative confidence
  const double raw = conf[f];
  const bool gated = raw < 0.0;
  const double c = gated ? 0.0 : raw;
  if (o.ratio) o.ratio[fo] = 20.0 * log10(c + 1e-10);                   // :533
  if (o.f0) o.f0[fo] = gated ? 0.0 : pitch[f];
  if (o.f0_conf) o.f0_conf[fo] = c;
  if (o.periodicity) o.periodicity[fo] = raw;
  if (o.voicing) o.voicing[fo] = c;
}

int launch_hratio(const HratioArgs& a, hipStream_t s) {
  if (a.F < 1) return 0;
  const int W = a.W, K = a.K;
  if (W < 64 || W > 2048 || (W & (W - 1)) || K != W / 2 || a.F > 2147483647 || a.sr < 1 || a.max_h > HRATIO_MAX_HARMONICS ||
      a.min_dist < 1)
    return -1;
  if (a.method != SONAR_HRATIO_HNR && a.method != SONAR_HRATIO_HPS && a.method != SONAR_HRATIO_SPECTRAL) return -1;
  if (a.method == SONAR_HRATIO_HPS && a.hps_lo < 0 && a.hps_hi > a.hps_lo) return -1;
  HratioArgs b = a;
  if (b.max_h < 0) b.max_h = 0;                                          // no harmonic, no row slot
  if (a.pcm) {
    if (!a.win || !a.tw || a.hop < 1 || (a.F - 1) * a.hop + W > a.n) return -1;
    hipLaunchKernelGGL((hratio_kernel<true>), dim3((unsigned)a.F), dim3(256), hratio_lds_bytes(K, true), s, b);
  } else {
    if (!a.mag) return -1;
    hipLaunchKernelGGL((hratio_kernel<false>), dim3((unsigned)a.F), dim3(256), hratio_lds_bytes(K, false), s, b);
  }
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

int launch_hratio_window(const double* pcm, int64_t hop, int W, const double* win, int64_t f0, int64_t nf, double* out,
                         hipStream_t s) {
  if (nf < 1) return 0;
  if (!pcm || !win || !out || hop < 1 || W < 1 || nf > 2147483647) return -1;
  hipLaunchKernelGGL(hratio_window_kernel, dim3((unsigned)nf), dim3(256), 0, s, pcm, hop, W, win, f0, out);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

int launch_hratio_acf_tail(const double* corr, int width, int64_t f0, int64_t nf, const HratioOut& o, hipStream_t s) {
  if (nf < 1) return 0;
  if (!corr || width < 1 || nf > 2147483647) return -1;
  hipLaunchKernelGGL(hratio_acf_tail_kernel, dim3((unsigned)nf), dim3(64), 0, s, corr, width, f0, o);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

int launch_hratio_yin_tail(const double* pitch, const double* conf, int64_t f0, int64_t nf, const HratioOut& o,
                           hipStream_t s) {
  if (nf < 1) return 0;
  if (!pitch || !conf) return -1;
  hipLaunchKernelGGL(hratio_yin_tail_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, s, pitch, conf, f0, nf, o);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // namespace sonar
