// fp_kernel.hip -- fused per-frame DSP for gfx950 (CDNA4, wave64).
//
// Replaces, for one batch of frames:
//   SpectralAnalyzer.ComputeSTFTWithWindow   fingerprint/analyzers/spectral.go:385-545
//     (frame t = x[tH : tH+W] * normalised symmetric window, go-dsp FFTReal, |X_k|, k <= W/2)
//   MFCC.Compute / ComputeFrames             algorithms/spectral/mfcc.go:113-191
//     (|X|^2 -> dense filterbank -> ln (floor 1e-10) -> DCT-II -> lifter)
//   per-frame spectral descriptors            fingerprint/extractors/speech.go:320-367, :438-458
//
// Layout / schedule (see DESIGN.md "Kernel 1"):
//  * block = 256 threads = 4 independent waves; the twiddle tables are built once
//    per block in LDS; afterwards no block barrier is used.  Every wave owns a
//    contiguous run of frames (halo re-reads of the overlapping PCM hit L1/L2)
//    and processes it in batches of NB frames; the next unit's PCM loads are
//    issued before the current FFT so they stay in flight.
//  * a wave computes FR frames at a time (FR = 8/R for R < 8): the W-point real
//    FFT is a M = W/2 = 64*R point complex FFT of z[n] = x[2n] + i x[2n+1]:
//      step 1: lane b holds z[64a+b] (a < R) -> R-point DFT in registers, twiddle w_M^{bc}
//      step 2: 64-point DFT across lanes for every column c, done as 8 x 8:
//              LDS exchange A, DFT8, twiddle w_64^{fg}, LDS exchange B, DFT8
//      step 3: real split X_k = E_k + w_W^k O_k (partner bin M-k by ds_bpermute)
//    Exchanges use XOR-swizzled addresses chosen so every ds_write_b32 / ds_read_b32
//    is bank-conflict-free (searched offline: tools/lds_banks.py).  The scratch
//    is the frame's own LDS spectrum row.
//  * batch epilogue with lane = (frame f, group g), NB frames x (64/NB) groups:
//    group g owns a set of filterbank rows balanced by nonzero count (sparse
//    triangle sums in Go's ascending-bin order), then DCT row g; descriptors are
//    per-group partial sums over a bin chunk reduced with xor-shuffles; results
//    are staged in LDS and written with coalesced stores.
#include "kernels.h"
#include "twiddles.h"
#include "wave.h"

namespace sonar {

namespace {

constexpr int ilog2(int n) { return n <= 1 ? 0 : 1 + ilog2(n >> 1); }
constexpr int bitrev(int x, int bits) {
  int r = 0;
  for (int i = 0; i < bits; i++) r = (r << 1) | ((x >> i) & 1);
  return r;
}

// In-register forward DFT of size N (N | 64), radix-2 DIT, compile-time twiddles.
template <typename T, int N>
__device__ __forceinline__ void dft_reg(T (&re)[N], T (&im)[N]) {
  constexpr int LB = ilog2(N);
#pragma unroll
  for (int i = 0; i < N; i++) {
    const int j = bitrev(i, LB);
    if (i < j) {
      T t = re[i]; re[i] = re[j]; re[j] = t;
      t = im[i]; im[i] = im[j]; im[j] = t;
    }
  }
#pragma unroll
  for (int len = 2; len <= N; len <<= 1) {
    const int half = len >> 1;
#pragma unroll
    for (int k = 0; k < half; k++) {
      const int ti = k * (64 / len);
#pragma unroll
      for (int i = k; i < N; i += len) {
        const int j = i + half;
        T xr, xi;
        if (ti == 0) {
          xr = re[j]; xi = im[j];
        } else if (ti == 16) {  // * (-i)
          xr = im[j]; xi = -re[j];
        } else {
          const T wr = (T)TW64R[ti], wi = (T)TW64I[ti];
          xr = re[j] * wr - im[j] * wi;
          xi = re[j] * wi + im[j] * wr;
        }
        re[j] = re[i] - xr; im[j] = im[i] - xi;
        re[i] = re[i] + xr; im[i] = im[i] + xi;
      }
    }
  }
}

// wave_lds_sync (wave.h) orders the LDS traffic of one wave's cross-lane exchanges through LDS.

template <typename T>
__device__ __forceinline__ T load_pcm(const void* pcm, int pcm_f64, int64_t i) {
  if (pcm_f64) return (T)((const double*)pcm)[i];
  return (T)((const float*)pcm)[i];
}

template <typename T>
__device__ __forceinline__ void store_out(void* out, int out_f64, int64_t i, T v) {
  if (out_f64) ((double*)out)[i] = (double)v;
  else ((float*)out)[i] = (float)v;
}

__device__ __forceinline__ float dev_log(float x) { return logf(x); }
__device__ __forceinline__ double dev_log(double x) { return log(x); }

template <typename T>
__device__ __forceinline__ void sincos_turns(double turns, T& c, T& s) {
  // e^{2 pi i turns}; evaluated in double then rounded to T
  double sd, cd;
  sincospi(2.0 * turns, &sd, &cd);
  c = (T)cd; s = (T)sd;
}

}  // namespace

template <typename P> struct Vec2;
template <> struct Vec2<float> { using type = float2; };
template <> struct Vec2<double> { using type = double2; };

#ifndef FP64_MIN_WAVES
#define FP64_MIN_WAVES 2
#endif
// FP64_MIN_WAVES: waves per SIMD the float64 MFCC / magnitude instance at W = 1024 is compiled for.
// 2 against 1 and 3 on the final code, same box, two alternating rounds (profiles/r06n_fp64_minwaves_ab.log):
// float64 PCM, MFCC only 3.17-3.19 / 3.30-3.31 / 3.73 ms per hour; float64 PCM, MFCC + descriptors
// (the GenerateFingerprint transform) 6.62-6.63 / 6.79-6.81 / 7.47-7.50 ms; float32 PCM equal at 1
// and 2.  (An earlier A/B, profiles/r06f_fp64_ab.log, had 3 ahead on the float32-PCM instance.)
// Dropping the PCM prefetch or re-reading the window instead of holding it: no faster (r06f).
template <typename T, typename P, int R, bool SPEC, bool CPLX = false>
__global__ __launch_bounds__(256, (sizeof(T) == 8 && !SPEC && !CPLX && R == 8) ? FP64_MIN_WAVES : 1)
void fp_wave_kernel(FpParams p) {
  constexpr int FR = (R >= 8) ? 1 : 8 / R;   // frames per FFT unit
  constexpr int V = R * FR;                   // values per lane
  constexpr int G = V / 8;                    // 8-column groups
  constexpr int M = 64 * R;                   // complex FFT size
  constexpr int K = M + 1;                    // bins per frame (LDS row stride)
  // frames per epilogue batch: float64 MFCC / magnitude launches take one FFT unit per batch (the
  // whole wave on its filterbank, ln and DCT), so a wave's LDS is one unit's rows and three 4-wave
  // blocks fit per CU; float32 and the fused SPEC epilogue batch at least four frames
  constexpr int NB = (sizeof(T) == 8 && !SPEC) ? FR : (FR > 4 ? FR : 4);
  constexpr int NG = 64 / NB;                 // epilogue lanes per frame
  constexpr int UPB = NB / FR;                // units per batch
  constexpr int PRE = SPEC ? FR : 0;          // rows before the batch (flux predecessor unit)

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  T* t1 = reinterpret_cast<T*>(smem + p.lds_tab_t1);   // [R][64] complex: w_M^{lane c}
  T* t2 = reinterpret_cast<T*>(smem + p.lds_tab_t2);   // [64] complex: w_64^j
  T* t3 = reinterpret_cast<T*>(smem + p.lds_tab_t3);   // [G*8][64] complex: w_W^k per lane slot
  unsigned char* wbase = smem + p.lds_wave0 + wave * p.lds_wave_stride;
  T* rows = reinterpret_cast<T*>(wbase);
  T* logmel = reinterpret_cast<T*>(wbase + p.lds_logmel);
  T* stage = reinterpret_cast<T*>(wbase + p.lds_stage);

  const int f2 = lane & 7, cl2 = lane >> 3;   // step-2 role: column cl2, f
  const int g3 = lane >> 3, cl3 = lane & 7;   // step-3 role: lane = 8 g + cl

  // ---- twiddle tables (double-evaluated, rounded to T), once per block ----
  for (int i = threadIdx.x; i < R * 64; i += blockDim.x) {
    const int c = i / 64, l = i % 64;
    T cr, ci; sincos_turns<T>(-(double)((l * c) % M) / (double)M, cr, ci);
    t1[2 * i] = cr; t1[2 * i + 1] = ci;
  }
  for (int i = threadIdx.x; i < 64; i += blockDim.x) {
    T cr, ci; sincos_turns<T>(-(double)i / 64.0, cr, ci);
    t2[2 * i] = cr; t2[2 * i + 1] = ci;
  }
  for (int i = threadIdx.x; i < G * 8 * 64; i += blockDim.x) {
    const int slot = i / 64, l = i % 64;          // slot = gm*8 + h
    const int gm = slot / 8, h = slot % 8;
    const int col = 8 * gm + (l & 7), c = col % R;
    const int k = c + R * (l >> 3) + 8 * R * h;
    T cr, ci; sincos_turns<T>(-(double)k / (double)(2 * M), cr, ci);
    t3[2 * i] = cr; t3[2 * i + 1] = ci;
  }
  // filterbank / DCT tables -> LDS (read by every epilogue lane, group-varying addresses)
  int* e_lo = reinterpret_cast<int*>(smem + p.lds_tab_mel);
  int* e_hi = e_lo + p.n_mels;
  int* e_woff = e_hi + p.n_mels;
  int* e_goff = e_woff + p.n_mels;
  int* e_gmel = e_goff + (p.n_groups + 1);
  T* e_w = reinterpret_cast<T*>(smem + p.lds_tab_w);
  T* e_dct = reinterpret_cast<T*>(smem + p.lds_tab_dct);
  T* e_lift = e_dct + p.n_mfcc * p.n_mels;
  if (p.out_mfcc) {
    for (int i = threadIdx.x; i < p.n_mels; i += blockDim.x) { e_lo[i] = p.mel_lo[i]; e_hi[i] = p.mel_hi[i]; e_woff[i] = p.mel_woff[i]; }
    for (int i = threadIdx.x; i <= p.n_groups; i += blockDim.x) e_goff[i] = p.grp_off[i];
    for (int i = threadIdx.x; i < p.n_mels; i += blockDim.x) e_gmel[i] = p.grp_mels[i];
    for (int i = threadIdx.x; i < p.nnz; i += blockDim.x) e_w[i] = reinterpret_cast<const T*>(p.mel_w)[i];
    for (int i = threadIdx.x; i < p.n_mfcc * p.n_mels; i += blockDim.x) e_dct[i] = reinterpret_cast<const T*>(p.dct)[i];
    for (int i = threadIdx.x; i < p.n_mfcc; i += blockDim.x) e_lift[i] = reinterpret_cast<const T*>(p.lift)[i];
  }
  __syncthreads();

  const T* win = reinterpret_cast<const T*>(p.window);
  T we[R], wo[R];                        // window at the lane's even/odd samples
#pragma unroll
  for (int a = 0; a < R; a++) {
    const int n0 = 2 * (64 * a + lane);
    we[a] = win[n0];
    wo[a] = win[n0 + 1];
  }

  // ---- this wave's frame range and unit sequence ---------------------------
  const int64_t gw = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
  const int64_t f_begin = p.f_first + gw * p.frames_per_wave;       // this launch: frames [f_first, f_last)
  if (f_begin >= p.f_last) return;
  const int64_t f_end = min(p.f_last, f_begin + p.frames_per_wave);
  const int64_t nbatch = (f_end - f_begin + NB - 1) / NB;
  const int pre = (SPEC && f_begin > 0) ? 1 : 0;
  const int64_t nunits = pre + nbatch * UPB;
  const bool fft_only = (p.flags >> 31) & 1u;

  // unit i -> first frame, first row
  auto unit_frame = [&](int64_t i) -> int64_t {
    if (pre) { if (i == 0) return f_begin - FR; i -= 1; }
    return f_begin + (i / UPB) * NB + (i % UPB) * FR;
  };
  auto unit_row = [&](int64_t i) -> int {
    if (pre) { if (i == 0) return 0; i -= 1; }
    return PRE + (int)(i % UPB) * FR;
  };
  // raw PCM of one unit (FR frames); validity is wave-uniform (depends on the frame only)
  auto load_unit = [&](int64_t uf, T (&er)[FR][R], T (&od)[FR][R]) {
#pragma unroll
    for (int fr = 0; fr < FR; fr++) {
      const int64_t t = uf + fr;
      // Go skips frames whose end passes the signal (spectral.go:524-534): row stays all-zero
      const bool valid = (t >= 0) && (t < p.F) && (t * p.H + p.W <= p.n);
      const int64_t s0 = t * p.H;
      if (valid) {
        const P* base = reinterpret_cast<const P*>(p.pcm) + s0 + 2 * lane;
        if ((s0 & 1) == 0) {       // 8 / 16-byte aligned pairs
          using V2 = typename Vec2<P>::type;
#pragma unroll
          for (int a = 0; a < R; a++) {
            const V2 v = *reinterpret_cast<const V2*>(base + 128 * a);
            er[fr][a] = (T)v.x; od[fr][a] = (T)v.y;
          }
        } else {
#pragma unroll
          for (int a = 0; a < R; a++) { er[fr][a] = (T)base[128 * a]; od[fr][a] = (T)base[128 * a + 1]; }
        }
      } else {
#pragma unroll
        for (int a = 0; a < R; a++) { er[fr][a] = 0; od[fr][a] = 0; }
      }
    }
  };

  // the next unit's PCM in registers during the current FFT
  T cur_e[FR][R], cur_o[FR][R];
  load_unit(unit_frame(0), cur_e, cur_o);

  for (int64_t ui = 0; ui < nunits; ++ui) {
    T nxt_e[FR][R], nxt_o[FR][R];
    if (ui + 1 < nunits) load_unit(unit_frame(ui + 1), nxt_e, nxt_o);
    const int rb = unit_row(ui);
    T* S = rows + (int64_t)rb * K;              // scratch = the unit's own rows

    // ======================= FFT of FR frames ===============================
    {
      T xr[FR][R], xi[FR][R];
#pragma unroll
      for (int fr = 0; fr < FR; fr++)
#pragma unroll
        for (int a = 0; a < R; a++) {
          xr[fr][a] = cur_e[fr][a] * we[a]; xi[fr][a] = cur_o[fr][a] * wo[a];
        }
      // step 1: R-point DFT over a, twiddle w_M^{lane c}
#pragma unroll
      for (int fr = 0; fr < FR; fr++) {
        dft_reg<T, R>(xr[fr], xi[fr]);
#pragma unroll
        for (int c = 1; c < R; c++) {
          const T wr = t1[2 * (c * 64 + lane)], wi = t1[2 * (c * 64 + lane) + 1];
          const T a_ = xr[fr][c], b_ = xi[fr][c];
          xr[fr][c] = a_ * wr - b_ * wi;
          xi[fr][c] = a_ * wi + b_ * wr;
        }
      }
      // exchange A: write S[gm*512 + 64*cl + (lane ^ 8cl)], read S[gm*512 + 64*cl2 + ((8e+f2) ^ 8cl2)]
      T yr[G][8], yi[G][8];
#pragma unroll
      for (int plane = 0; plane < 2; plane++) {
#pragma unroll
        for (int col = 0; col < V; col++) {
          const int gm = col >> 3, cl = col & 7;
          const T v = plane ? xi[col / R][col % R] : xr[col / R][col % R];
          S[gm * 512 + 64 * cl + (lane ^ (8 * cl))] = v;
        }
        wave_lds_sync();
#pragma unroll
        for (int gm = 0; gm < G; gm++)
#pragma unroll
          for (int e = 0; e < 8; e++) {
            const T v = S[gm * 512 + 64 * cl2 + ((8 * e + f2) ^ (8 * cl2))];
            if (plane) yi[gm][e] = v; else yr[gm][e] = v;
          }
        wave_lds_sync();
      }
      // step 2: DFT8 over e, twiddle w_64^{f g}
#pragma unroll
      for (int gm = 0; gm < G; gm++) {
        dft_reg<T, 8>(yr[gm], yi[gm]);
#pragma unroll
        for (int g = 1; g < 8; g++) {
          const int j = (f2 * g) & 63;
          const T wr = t2[2 * j], wi = t2[2 * j + 1];
          const T a_ = yr[gm][g], b_ = yi[gm][g];
          yr[gm][g] = a_ * wr - b_ * wi;
          yi[gm][g] = a_ * wi + b_ * wr;
        }
      }
      // exchange B: write S[gm*512 + 64*cl2 + ((8g+f2) ^ (9cl2 & 63))], read with lane = 8g3 + cl3
      T zr[G][8], zi[G][8];
#pragma unroll
      for (int plane = 0; plane < 2; plane++) {
#pragma unroll
        for (int gm = 0; gm < G; gm++)
#pragma unroll
          for (int g = 0; g < 8; g++)
            S[gm * 512 + 64 * cl2 + ((8 * g + f2) ^ ((9 * cl2) & 63))] = plane ? yi[gm][g] : yr[gm][g];
        wave_lds_sync();
#pragma unroll
        for (int gm = 0; gm < G; gm++)
#pragma unroll
          for (int f = 0; f < 8; f++) {
            const T v = S[gm * 512 + 64 * cl3 + ((8 * g3 + f) ^ ((9 * cl3) & 63))];
            if (plane) zi[gm][f] = v; else zr[gm][f] = v;
          }
        wave_lds_sync();
      }
      // step 3: DFT8 over f -> h;  lane holds Z_fr[c + R*g3 + 8R*h] for its columns
#pragma unroll
      for (int gm = 0; gm < G; gm++) dft_reg<T, 8>(zr[gm], zi[gm]);

      // real split needs the partner bin Z_fr[(M-k) mod M]
      T pr_[G][8], pi_[G][8];
      if constexpr (G == 1) {
        // partner is a fixed lane permutation: lane' = 8(7-g3) + fr R + (R-c) for c > 0,
        // 8(8-g3) + fr R for c == 0 < g3, itself (register (8-h) & 7) for c == g3 == 0;
        // source register 7-h.  ds_bpermute: no LDS allocation, no fences.
        const int fr = cl3 / R, c = cl3 % R;
        const bool self = (c == 0) && (g3 == 0);
        const int src = (c > 0) ? (8 * (7 - g3) + fr * R + (R - c)) : (8 * ((8 - g3) & 7) + fr * R);
#pragma unroll
        for (int h = 0; h < 8; h++) {
          const T sr = __shfl(zr[0][7 - h], src, 64);
          const T si = __shfl(zi[0][7 - h], src, 64);
          pr_[0][h] = self ? zr[0][(8 - h) & 7] : sr;
          pi_[0][h] = self ? zi[0][(8 - h) & 7] : si;
        }
      } else {
#pragma unroll
        for (int plane = 0; plane < 2; plane++) {
#pragma unroll
          for (int gm = 0; gm < G; gm++) {
            const int col = 8 * gm + cl3, fr = col / R, c = col % R;
#pragma unroll
            for (int h = 0; h < 8; h++) {
              const int k = c + R * g3 + 8 * R * h;
              S[fr * M + k] = plane ? zi[gm][h] : zr[gm][h];
            }
          }
          wave_lds_sync();
#pragma unroll
          for (int gm = 0; gm < G; gm++) {
            const int col = 8 * gm + cl3, fr = col / R, c = col % R;
#pragma unroll
            for (int h = 0; h < 8; h++) {
              const int k = c + R * g3 + 8 * R * h;
              const T v = S[fr * M + ((M - k) & (M - 1))];
              if (plane) pi_[gm][h] = v; else pr_[gm][h] = v;
            }
          }
          wave_lds_sync();
        }
      }
      // X_k = E + w O,  E = (A + B)/2, O = -i (A - B)/2, A = Z[k], B = conj(Z[M-k])
      const bool mag = SPEC || p.out_mag;
      const int64_t uf = CPLX ? unit_frame(ui) : 0;
#pragma unroll
      for (int gm = 0; gm < G; gm++) {
        const int col = 8 * gm + cl3, fr = col / R, c = col % R;
        T* row = rows + (int64_t)(rb + fr) * K;
#pragma unroll
        for (int h = 0; h < 8; h++) {
          const int k = c + R * g3 + 8 * R * h;
          const int ti = 2 * ((gm * 8 + h) * 64 + lane);
          const T wr = t3[ti], wi = t3[ti + 1];
          const T ar = zr[gm][h], ai = zi[gm][h];
          const T br = pr_[gm][h], bi = -pi_[gm][h];
          const T er = (T)0.5 * (ar + br), ei = (T)0.5 * (ai + bi);
          const T or_ = (T)0.5 * (ai - bi), oi = (T)-0.5 * (ar - br);
          const T xr_ = er + (wr * or_ - wi * oi);
          const T xi_ = ei + (wr * oi + wi * or_);
          const T pw = xr_ * xr_ + xi_ * xi_;
          row[k] = mag ? sqrt(pw) : pw;
          const int64_t tg = uf + fr;   // this frame's global index
          const bool own = CPLX && !(pre && ui == 0) && tg < f_end;
          if (own) {                    // SpectrogramResult.Complex / .Phase (spectral.go:491-493)
            if (p.out_cplx) {
              store_out<T>(p.out_cplx, p.out_f64, 2 * (tg * K + k), xr_);
              store_out<T>(p.out_cplx, p.out_f64, 2 * (tg * K + k) + 1, xi_);
            }
            if (p.out_phase) store_out<T>(p.out_phase, p.out_f64, tg * K + k, atan2(xi_, xr_));
          }
          if (k == 0) {                 // Nyquist bin M = E_0 - O_0 (both real)
            const T xn = er - or_;
            row[M] = mag ? fabs(xn) : xn * xn;
            if (own) {
              if (p.out_cplx) {
                store_out<T>(p.out_cplx, p.out_f64, 2 * (tg * K + M), xn);
                store_out<T>(p.out_cplx, p.out_f64, 2 * (tg * K + M) + 1, (T)0);
              }
              if (p.out_phase) store_out<T>(p.out_phase, p.out_f64, tg * K + M, atan2((T)0, xn));
            }
          }
        }
      }
      wave_lds_sync();
    }
#pragma unroll
    for (int fr = 0; fr < FR; fr++)
#pragma unroll
      for (int a = 0; a < R; a++) { cur_e[fr][a] = nxt_e[fr][a]; cur_o[fr][a] = nxt_o[fr][a]; }

    // ======================= batch epilogue (lane = frame x group) ==========
    const int64_t bi_ = pre ? ui - 1 : ui;
    if (bi_ < 0 || (bi_ % UPB) != UPB - 1 || fft_only) continue;
    const int64_t t0 = f_begin + (bi_ / UPB) * NB;        // first frame of the batch
    const int nv = (int)min((int64_t)NB, f_end - t0);       // frames of the batch that exist
    const int f = lane / NG, g = lane % NG;
    const bool act = f < nv;
    const T* row = rows + (int64_t)(PRE + f) * K;
    const bool mag = SPEC || p.out_mag;

    if (p.out_mag) {   // SpectrogramResult.Magnitude rows: contiguous in LDS and in HBM
      const int64_t cnt = (int64_t)nv * K;
      for (int64_t i = lane; i < cnt; i += 64)
        store_out<T>(p.out_mag, p.mag_f64, t0 * K + i, rows[(int64_t)PRE * K + i]);
    }
    if (p.out_mfcc) {
      if (act) {
        for (int q = e_goff[g]; q < e_goff[g + 1]; ++q) {
          const int m = e_gmel[q];
          const int lo = e_lo[m], hi = e_hi[m];
          const T* w = e_w + e_woff[m] - lo;
          T s = 0;
          // 8 independent LDS loads per step; lanes past `hi` add an exact 0 (Go adds
          // zero-weight bins too), so the ascending-bin summation order is unchanged
          for (int k = lo; k < hi; k += 8) {
            T pv[8], wv[8];
#pragma unroll
            for (int j = 0; j < 8; j++) { pv[j] = row[k + j]; wv[j] = w[k + j]; }
#pragma unroll
            for (int j = 0; j < 8; j++) {
              T v = pv[j];
              if (mag) v = v * v;                 // |X|^2
              if (p.input_power) v = v * v;       // F5: Compute() squares |X|^2 again
              v = (k + j < hi) ? v : (T)0;
              s += v * ((k + j < hi) ? wv[j] : (T)0);
            }
          }
          logmel[f * (p.n_mels + 1) + m] = (s > (T)0) ? dev_log(s) : dev_log((T)1e-10);
        }
      }
      wave_lds_sync();
      if (act) {
        const T* lm = logmel + f * (p.n_mels + 1);
        for (int kk = g; kk < p.n_mfcc; kk += NG) {
          const T* d = e_dct + kk * p.n_mels;
          T s = 0;
          for (int n = 0; n < p.n_mels; n += 8) {
            T a[8], b[8];
#pragma unroll
            for (int j = 0; j < 8; j++) { a[j] = lm[n + j]; b[j] = d[n + j]; }
#pragma unroll
            for (int j = 0; j < 8; j++) s += (n + j < p.n_mels) ? a[j] * b[j] : (T)0;
          }
          stage[f * p.n_mfcc + kk] = s * e_lift[kk];
        }
      }
      wave_lds_sync();
      const int cnt = nv * p.n_mfcc;
      for (int i = lane; i < cnt; i += 64) store_out<T>(p.out_mfcc, p.out_f64, t0 * p.n_mfcc + i, stage[i]);
    }
    if constexpr (SPEC) {
      // per-frame descriptors (speech.go:320-367, :438-458) from |X| in LDS.
      // Each of the NG lanes of a frame reduces a chunk of bins; xor-shuffles combine.
      const T* prev = row - K;                      // frame t-1 (row PRE-1+f), for flux
      const int64_t t = t0 + f;
      const bool has_prev = act && (t > 0);
      constexpr int CH = (K + NG - 1) / NG;
      const int k0 = g * CH, k1 = min(K, k0 + CH);
      const T fscale = (T)((double)p.sample_rate / (double)((K - 1) * 2));   // freqBins[i] = i sr / (2(K-1))
      const T inv_ln10 = (T)0.43429448190325182765;
      T s_m = 0, s_fm = 0, s_m2 = 0, mx = 0, s_ln = 0, s_lo = 0, s_hi = 0, s_fx = 0;
      double sx = 0, sy = 0, sxy = 0, sxx = 0;    // regression sums: f32 would cancel catastrophically
      int n_ln = 0, n_sl = 0;
      if (act) {
#pragma unroll 4
        for (int j = 0; j < CH; ++j) {
          const int k = k0 + j;
          if (k >= k1) break;
          const T m = row[k];
          const T fk = (T)k * fscale;
          s_m += m; s_fm += fk * m; s_m2 += m * m;
          if (m > mx) mx = m;
          if (k < K / 4) s_lo += m * m; else s_hi += m * m;       // speech.go:438-458: two sums
          if (m > (T)1e-10) {
            const T lm = dev_log(m);
            s_ln += lm; n_ln++;
            if (fk > (T)0) {
              const double x = (double)(dev_log(fk) * inv_ln10), y = (double)(lm * inv_ln10);
              sx += x; sy += y; sxy += x * y; sxx += x * x; n_sl++;
            }
          }
          if (has_prev) { const T d = m - prev[k]; if (d > (T)0) s_fx += d * d; }
        }
      }
      auto red = [](auto v) { return wave_sum<decltype(v), NG>(v); };        // over the frame's NG lanes
      const T S_m = red(s_m), S_fm = red(s_fm), S_m2 = red(s_m2), MX = wave_max<T, NG>(mx), S_ln = red(s_ln);
      const T S_lo = red(s_lo), S_hi = red(s_hi), S_fx = red(s_fx);
      const double SX = red(sx), SY = red(sy), SXY = red(sxy), SXX = red(sxx);
      const int N_ln = red(n_ln), N_sl = red(n_sl);
      const T cen = (S_m == (T)0) ? (T)0 : S_fm / S_m;                       // spectral_centroid.go:18-41
      T s_bw = 0;                                                            // spectral_bandwidth.go:22-47
      if (act) {
#pragma unroll 4
        for (int j = 0; j < CH; ++j) { const int k = k0 + j; if (k >= k1) break; const T d = (T)k * fscale - cen; s_bw += d * d * row[k]; }
      }
      const T S_bw = red(s_bw);
      // rolloff (spectral_rolloff.go:29-49): the first k whose cumulative m^2 reaches 0.85 of the
      // total, both sums sequential in Go.  Fast path: per-lane double partials + a lane scan
      // locate the bin and its two margins; the parallel sums differ from Go's sequential ones by
      // at most K u total each, so a bin whose margins both exceed 8 K u total is Go's bin.  Any
      // other frame re-runs Go's two chains (unfused, ascending k) on its g == 0 lane.  m^2 is
      // formed in double: exact for f32 magnitudes, Go's rounding for f64 ones.
      int ridx = 1 << 30;
      bool roll_zero = true;
      {
#pragma clang fp contract(off)
        double d_m2 = 0;
        if (act)
          for (int k = k0; k < k1; ++k) { const double m = (double)row[k]; d_m2 += m * m; }
        double incl = d_m2;                                                  // inclusive scan over the frame's lanes
        for (int o = 1; o < NG; o <<= 1) { const double u = __shfl_up(incl, o, NG); if (g >= o) incl += u; }
        const double tot = __shfl(incl, (lane / NG) * NG + NG - 1, 64);
        const double target = 0.85 * tot;
        const double delta = 8.0 * (double)K * 1.1102230246251565e-16 * tot;
        double cum = incl - d_m2, margin = 0;
        if (act && tot != 0.0)
          for (int k = k0; k < k1; ++k) {
            const double m = (double)row[k], prev_cum = cum;
            cum += m * m;
            if (cum >= target) { ridx = k; margin = fmin(cum - target, target - prev_cum); break; }
          }
        bool owner = ridx < (1 << 30);
        for (int o = NG / 2; o > 0; o >>= 1) { const int u = __shfl_xor(ridx, o, 64); ridx = u < ridx ? u : ridx; }
        owner = owner && ridx >= k0 && ridx < k1;
        int unsure = (owner && !(margin > delta)) ? 1 : 0;
        for (int o = NG / 2; o > 0; o >>= 1) unsure |= __shfl_xor(unsure, o, 64);
        if (act && tot != 0.0 && ridx >= K) unsure = 1;                     // rounding kept cum below target
        roll_zero = (tot == 0.0);
        if (act && g == 0 && unsure) {                                       // Go's chains, verbatim order
          double gt = 0;
          for (int k = 0; k < K; ++k) { const double m = (double)row[k]; gt += m * m; }
          roll_zero = (gt == 0.0);
          const double gtarget = 0.85 * gt;
          double gc = 0;
          ridx = K;
          for (int k = 0; k < K; ++k) { const double m = (double)row[k]; gc += m * m; if (gc >= gtarget) { ridx = k; break; } }
        }
      }
      if (act && g == 0) {
        const T fl_geo = N_ln > 0 ? exp(S_ln / (T)N_ln) : (T)0;              // spectral_flatness.go:31-73
        const T am = S_m / (T)K;
        T flat = 0;
        if (N_ln > 0 && am > (T)1e-10) { flat = fl_geo / am; if (flat > (T)1) flat = 1; }
        const T rms = sqrt(S_m2 / (T)K);                                     // spectral_crest.go:18-38
        T slope = 0;                                                         // spectral_slope.go:23-63
        if (N_sl >= 2) { const double dn = (double)N_sl * SXX - SX * SX; if (dn != 0.0) slope = (T)(((double)N_sl * SXY - SX * SY) / dn); }
        T roll = 0;
        if (!roll_zero) roll = (T)((double)(ridx < K ? ridx : K - 1) * (double)p.sample_rate / (double)((K - 1) * 2));
        const T vals[9] = {cen, roll, (S_m == (T)0) ? (T)0 : sqrt(S_bw / S_m), flat, rms == (T)0 ? (T)0 : MX / rms,
                           slope, sqrt(S_fx), S_m2 > (T)0 ? S_lo / S_m2 : (T)0, S_m2 > (T)0 ? S_hi / S_m2 : (T)0};
#pragma unroll
        for (int d = 0; d < 9; d++) {
          if (!p.out_spec[d]) continue;
          if (d == 6) { if (t > 0) store_out<T>(p.out_spec[6], p.out_f64, t - 1, vals[6]); }
          else store_out<T>(p.out_spec[d], p.out_f64, t, vals[d]);
        }
      }
      // the batch's last frame is the next batch's flux predecessor
      wave_lds_sync();
      for (int i = lane; i < K; i += 64) rows[(int64_t)(PRE - 1) * K + i] = rows[(int64_t)(PRE + NB - 1) * K + i];
      wave_lds_sync();
    }
  }
}

// ======================= spectral descriptors from |X| rows in HBM =========================
// SpeechFeatureExtractor.extractSpectralFeatures (extractors/speech.go:320-367) and the energy-band
// ratios (:438-458) over float64 |X| rows the transform already wrote to HBM: the fused kernel's
// magnitude output (fp_wave_kernel without SPEC) or the DFT path's scratch.  Round 6 (VERDICT r05
// item 3): the SPEC epilogue inside fp_wave_kernel ran at one wave per SIMD (256 VGPRs, 107 KB of
// LDS per 4-wave block) and cost 23 ms per hour against the 3 ms of the transform; here a wave takes
// one frame at a time over a contiguous frame run, every lane a contiguous chunk of CH = ceil(K/64)
// bins held in registers (with the previous frame's chunk, for the flux), at 20 KB of LDS per
// 4-wave block.  The arithmetic is the fused epilogue's: per-lane partial sums in ascending bin
// order, wave reductions, the rolloff bin by a lane scan with Go's sequential chains re-run on
// frames whose margins are within the scan's rounding (exact bin), spectral_centroid.go:18-41,
// spectral_rolloff.go:29-49, spectral_bandwidth.go:22-47, spectral_flatness.go:31-73,
// spectral_crest.go:18-38, spectral_slope.go:23-63, spectral_flux.go:299-318.
namespace {
// body(j) over the lane's chunk j < nk, fully unrolled when CHM > 0; body returns true to stop
template <int CHM, typename B>
__device__ __forceinline__ void chunk_for(int nk, B body) {
  if constexpr (CHM > 0) {
#pragma unroll
    for (int j = 0; j < CHM; ++j) {
      if (j >= nk) break;
      if (body(j)) break;
    }
  } else {
    for (int j = 0; j < nk; ++j)
      if (body(j)) break;
  }
}
}  // namespace

// CHM > 0: bin chunks of at most CHM bins (K <= 64 CHM), current and previous chunk in registers and
// one LDS row tile per wave (the coalesced-load transpose); CHM == 0: any K, both rows in LDS tiles
template <int CHM>
__global__ __launch_bounds__(256) void spec_rows_kernel(SpecParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int K = p.K;
  constexpr int NT = CHM > 0 ? 1 : 2;                       // LDS row tiles per wave
  double* xk = reinterpret_cast<double*>(smem);              // [K] log10 of each bin's frequency
  double* tbase = xk + K + (K & 1) + (size_t)wave * NT * K;
  const double fscale = (double)p.sample_rate / (double)((K - 1) * 2);   // freqBins[i] = i sr / (2(K-1))
  const double inv_ln10 = 0.43429448190325182765;
  const bool slope_on = fscale > 0.0;                        // sr <= 0: every bin frequency is <= 0 (F3)
  if (slope_on)
    for (int k = threadIdx.x; k < K; k += blockDim.x) xk[k] = k > 0 ? log((double)k * fscale) * inv_ln10 : 0.0;
  __syncthreads();
  const int64_t gw = (int64_t)blockIdx.x * nw + wave;
  const int64_t fb = p.f_first + gw * p.frames_per_wave;            // this launch: frames [f_first, f_last)
  if (fb >= p.f_last) return;
  const int64_t fe = min(p.f_last, fb + p.frames_per_wave);
  const int CH = (K + 63) >> 6;
  const int k0 = min(K, lane * CH), k1 = min(K, k0 + CH), nk = k1 - k0;
  const double* src = p.mag;

  double m[CHM > 0 ? CHM : 1], pv[CHM > 0 ? CHM : 1];
  int cur_tile = 0;
  auto tile = [&](int i) { return tbase + (size_t)(NT == 1 ? 0 : i) * K; };
  // the previous frame's chunk for the flux (frame fb - 1 when the run does not start at 0)
  if (fb > 0) {
    double* t = tile(1);
    const double* r = src + (fb - 1) * (int64_t)K;
    for (int k = lane; k < K; k += 64) t[k] = r[k];
    wave_lds_sync();
    if constexpr (CHM > 0) {
#pragma unroll
      for (int j = 0; j < CHM; ++j) pv[j] = j < nk ? t[k0 + j] : 0.0;
      wave_lds_sync();
    }
  }
  for (int64_t t = fb; t < fe; ++t) {
    double* cur = tile(cur_tile);
    double* prv = tile(cur_tile ^ 1);
    {
      const double* r = src + t * (int64_t)K;
      for (int k = lane; k < K; k += 64) cur[k] = r[k];       // coalesced row load -> LDS
    }
    wave_lds_sync();
    if constexpr (CHM > 0) {
#pragma unroll
      for (int j = 0; j < CHM; ++j) m[j] = j < nk ? cur[k0 + j] : 0.0;
    }
    auto M = [&](int j) -> double { if constexpr (CHM > 0) return m[j]; else return cur[k0 + j]; };
    auto PV = [&](int j) -> double { if constexpr (CHM > 0) return pv[j]; else return prv[k0 + j]; };
    const bool has_prev = t > 0;
    double s_m = 0, s_fm = 0, s_m2 = 0, mx = 0, s_ln = 0, s_lo = 0, s_hi = 0, s_fx = 0;
    double sx = 0, sy = 0, sxy = 0, sxx = 0;
    int n_ln = 0, n_sl = 0;
    chunk_for<CHM>(nk, [&](int j) {
      const int k = k0 + j;
      const double mv = M(j);
      const double fk = (double)k * fscale;
      s_m += mv; s_fm += fk * mv; s_m2 += mv * mv;
      if (mv > mx) mx = mv;
      if (k < K / 4) s_lo += mv * mv; else s_hi += mv * mv;
      if (mv > 1e-10) {
        const double lm = log(mv);
        s_ln += lm; n_ln++;
        if (fk > 0.0) {
          const double x = xk[k], y = lm * inv_ln10;
          sx += x; sy += y; sxy += x * y; sxx += x * x; n_sl++;
        }
      }
      if (has_prev) { const double d = mv - PV(j); if (d > 0.0) s_fx += d * d; }
      return false;
    });
    const double S_m = wave_sum(s_m), S_fm = wave_sum(s_fm), S_m2 = wave_sum(s_m2), MX = wave_max(mx);
    const double S_ln = wave_sum(s_ln), S_lo = wave_sum(s_lo), S_hi = wave_sum(s_hi);
    const double S_fx = has_prev ? wave_sum(s_fx) : 0.0;
    const int N_ln = wave_sum(n_ln);
    double SX = 0, SY = 0, SXY = 0, SXX = 0;
    int N_sl = 0;
    if (slope_on) { SX = wave_sum(sx); SY = wave_sum(sy); SXY = wave_sum(sxy); SXX = wave_sum(sxx); N_sl = wave_sum(n_sl); }
    const double cen = (S_m == 0.0) ? 0.0 : S_fm / S_m;
    double s_bw = 0;
    chunk_for<CHM>(nk, [&](int j) {
      const double d = (double)(k0 + j) * fscale - cen;
      s_bw += d * d * M(j);
      return false;
    });
    const double S_bw = wave_sum(s_bw);
    // rolloff: as the fused epilogue (lane scan + margins, Go's two chains on unsure frames)
    int ridx = 1 << 30;
    bool roll_zero = true;
    {
#pragma clang fp contract(off)
      double d_m2 = 0;
      chunk_for<CHM>(nk, [&](int j) {
        const double mv = M(j);
        d_m2 += mv * mv;
        return false;
      });
      double incl = d_m2;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) { const double u = __shfl_up(incl, o, 64); if (lane >= o) incl += u; }
      const double tot = __shfl(incl, 63, 64);
      const double target = 0.85 * tot;
      const double delta = 8.0 * (double)K * 1.1102230246251565e-16 * tot;
      double cum = incl - d_m2, margin = 0;
      if (tot != 0.0) {
        chunk_for<CHM>(nk, [&](int j) {
          const double mv = M(j), prev_cum = cum;
          cum += mv * mv;
          if (cum >= target) { ridx = k0 + j; margin = fmin(cum - target, target - prev_cum); return true; }
          return false;
        });
      }
      bool owner = ridx < (1 << 30);
      ridx = wave_min(ridx);
      owner = owner && ridx >= k0 && ridx < k1;
      int unsure = (owner && !(margin > delta)) ? 1 : 0;
      unsure = wave_sum(unsure);
      if (tot != 0.0 && ridx >= K) unsure = 1;                  // rounding kept every cum below target
      roll_zero = (tot == 0.0);
      if (unsure) {                                             // wave-uniform: Go's chains on lane 0
        if (lane == 0) {
          double gt = 0;
          for (int k = 0; k < K; ++k) { const double mv = cur[k]; gt += mv * mv; }
          roll_zero = (gt == 0.0);
          const double gtarget = 0.85 * gt;
          double gc = 0;
          ridx = K;
          for (int k = 0; k < K; ++k) { const double mv = cur[k]; gc += mv * mv; if (gc >= gtarget) { ridx = k; break; } }
        }
      }
    }
    if (lane == 0) {
      const double fl_geo = N_ln > 0 ? exp(S_ln / (double)N_ln) : 0.0;
      const double am = S_m / (double)K;
      double flat = 0;
      if (N_ln > 0 && am > 1e-10) { flat = fl_geo / am; if (flat > 1.0) flat = 1.0; }
      const double rms = sqrt(S_m2 / (double)K);
      double slope = 0;
      if (N_sl >= 2) { const double dn = (double)N_sl * SXX - SX * SX; if (dn != 0.0) slope = ((double)N_sl * SXY - SX * SY) / dn; }
      double roll = 0;
      if (!roll_zero) roll = (double)(ridx < K ? ridx : K - 1) * (double)p.sample_rate / (double)((K - 1) * 2);
      const double vals[9] = {cen, roll, (S_m == 0.0) ? 0.0 : sqrt(S_bw / S_m), flat, rms == 0.0 ? 0.0 : MX / rms,
                              slope, sqrt(S_fx), S_m2 > 0.0 ? S_lo / S_m2 : 0.0, S_m2 > 0.0 ? S_hi / S_m2 : 0.0};
#pragma unroll
      for (int d = 0; d < 9; d++) {
        if (!p.out_spec[d]) continue;
        if (d == 6) { if (t > 0) store_out<double>(p.out_spec[6], p.out_f64, t - 1, vals[6]); }
        else store_out<double>(p.out_spec[d], p.out_f64, t, vals[d]);
      }
    }
    if constexpr (CHM > 0) {
#pragma unroll
      for (int j = 0; j < CHM; ++j) pv[j] = m[j];
    } else {
      cur_tile ^= 1;
    }
    wave_lds_sync();                                            // the tile is rewritten by the next frame
  }
}

int launch_spec_rows(const SpecParams& p, hipStream_t s) {
  if (p.F <= 0 || p.f_last <= p.f_first) return 0;
  if (p.K < 2 || p.frames_per_wave <= 0) return -4;
  const int CH = (p.K + 63) / 64;
  const int waves_per_block = 4;
  const int nt = CH <= 9 ? 1 : 2;
  const size_t lds = (size_t)(p.K + (p.K & 1)) * 8 + (size_t)waves_per_block * nt * p.K * 8;
  if (lds > 160 * 1024) return -4;
  const int64_t waves = (p.f_last - p.f_first + p.frames_per_wave - 1) / p.frames_per_wave;
  const int64_t grid = (waves + waves_per_block - 1) / waves_per_block;
  const dim3 g((unsigned)grid), b(64 * waves_per_block);
#define SPEC_ROWS(C)                                                                             \
  do {                                                                                           \
    if (lds > 64 * 1024)                                                                         \
      hipFuncSetAttribute((const void*)spec_rows_kernel<C>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    hipLaunchKernelGGL(spec_rows_kernel<C>, g, b, lds, s, p);                                     \
  } while (0)
  if (CH <= 2) SPEC_ROWS(2);
  else if (CH <= 3) SPEC_ROWS(3);
  else if (CH <= 5) SPEC_ROWS(5);
  else if (CH <= 9) SPEC_ROWS(9);
  else SPEC_ROWS(0);
#undef SPEC_ROWS
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

bool fingerprint_supported(int W) {
  return W == 128 || W == 256 || W == 512 || W == 1024 || W == 2048;
}

template <typename T, typename P, int R, bool SPEC, bool CPLX>
static int launch_t(const FpParams& p, hipStream_t s) {
  auto kern = fp_wave_kernel<T, P, R, SPEC, CPLX>;
  if (p.lds_bytes > 64 * 1024)
    hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, p.lds_bytes);
  if (p.f_last <= p.f_first) return 0;
  const int64_t waves = (p.f_last - p.f_first + p.frames_per_wave - 1) / p.frames_per_wave;
  const int64_t grid = (waves + p.waves_per_block - 1) / p.waves_per_block;
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(64 * p.waves_per_block), p.lds_bytes, s, p);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

template <typename T, typename P, bool SPEC, bool CPLX>
static int launch_r(const FpParams& p, hipStream_t s) {
  switch (p.W / 128) {
    case 1: return launch_t<T, P, 1, SPEC, CPLX>(p, s);
    case 2: return launch_t<T, P, 2, SPEC, CPLX>(p, s);
    case 4: return launch_t<T, P, 4, SPEC, CPLX>(p, s);
    case 8: return launch_t<T, P, 8, SPEC, CPLX>(p, s);
    case 16: return launch_t<T, P, 16, SPEC, CPLX>(p, s);
  }
  return -4;
}

// SONAR_FP_SPECTRAL selects SPEC; Complex / Phase outputs select CPLX (its own instantiation: the
// extra stores and atan2 cost registers the other variants keep)
template <typename T, typename P>
static int launch_s(const FpParams& p, hipStream_t s) {
  const bool cplx = p.out_cplx || p.out_phase;
  if (p.flags & 4u) return cplx ? launch_r<T, P, true, true>(p, s) : launch_r<T, P, true, false>(p, s);
  return cplx ? launch_r<T, P, false, true>(p, s) : launch_r<T, P, false, false>(p, s);
}

int launch_fingerprint(const FpParams& p, int f64, hipStream_t s) {
  if (f64) return p.pcm_f64 ? launch_s<double, double>(p, s) : launch_s<double, float>(p, s);
  return p.pcm_f64 ? launch_s<float, double>(p, s) : launch_s<float, float>(p, s);
}

// batch geometry shared with the host (LDS carve)
int fp_batch_frames(int W, int f64, int spec) {
  const int R = W / 128;
  const int FR = R >= 8 ? 1 : 8 / R;
  return (f64 && !spec) ? FR : (FR > 4 ? FR : 4);
}
int fp_pre_rows(int W, int spec) {
  const int R = W / 128;
  const int FR = R >= 8 ? 1 : 8 / R;
  return spec ? FR : 0;
}

}  // namespace sonar
