// fp_tables.cpp -- host images of the fingerprint paths' device tables (fp_tables.h).  Pure C++17.
#include "fp_tables.h"

#include <algorithm>
#include <cmath>

#include "host_dsp.h"
#include "mfcc_pair_layout.h"

namespace sonar {
namespace host {
namespace {
constexpr double kPi = 3.14159265358979323846;

bool mfcc_tables(const sonar_fp_cfg* cfg, int W, MfccTables& mt) {
  return make_mfcc_tables(cfg->sample_rate, cfg->n_mfcc, cfg->n_filters, cfg->filterbank, cfg->low_freq,
                          cfg->high_freq, cfg->use_lifter != 0, cfg->lifter, W, mt);
}

// the six MFCC sections every per-frame path reads, in precision T = double or float
void put_mfcc(Image& im, const MfccTables& mt, bool f64, FpTableDesc& d) {
  d.mel_lo = put_section(im, mt.lo); d.mel_hi = put_section(im, mt.hi); d.mel_woff = put_section(im, mt.woff);
  d.mel_w = put_real(im, mt.w, f64); d.dct = put_real(im, mt.dct, f64); d.lift = put_real(im, mt.lift, f64);
  d.n_mels = mt.n_mels; d.n_mfcc = mt.n_mfcc; d.nnz = (int)mt.w.size();
  d.has_mfcc = true;
}
}  // namespace

size_t put_real(Image& im, const std::vector<double>& v, bool f64) {
  if (f64) return put_section(im, v);
  return put_section(im, std::vector<float>(v.begin(), v.end()));
}

std::vector<double> trig_table(int n) {
  std::vector<double> trig(2 * (size_t)n);
  for (int m = 0; m < n; ++m) {
    trig[2 * m] = std::cos(2.0 * kPi * (double)m / (double)n);
    trig[2 * m + 1] = -std::sin(2.0 * kPi * (double)m / (double)n);
  }
  return trig;
}

int build_dft_tables(const sonar_fp_cfg* cfg, bool raw_window, bool want_mfcc, Image& im, FpTableDesc& d) {
  const int W = cfg->window_size;
  std::vector<double> win;
  if (!make_window(cfg->window_type, W, true, !raw_window, kStftBeta, kStftAlpha, win)) return TABLES_BAD_WINDOW;
  d.window = put_section(im, win);
  d.trig = put_section(im, trig_table(W));
  if (want_mfcc) {
    MfccTables mt;
    if (!mfcc_tables(cfg, W, mt)) return TABLES_BAD_BANK;
    put_mfcc(im, mt, true, d);
  }
  return TABLES_OK;
}

int build_wave_tables(const sonar_fp_cfg* cfg, bool raw_window, bool f64, int groups, Image& im, FpTableDesc& d) {
  const int W = cfg->window_size;
  std::vector<double> win;
  if (!make_window(cfg->window_type, W, true, !raw_window, kStftBeta, kStftAlpha, win)) return TABLES_BAD_WINDOW;
  d.window = put_real(im, win, f64);
  MfccTables mt;
  if (!mfcc_tables(cfg, W, mt)) return TABLES_BAD_BANK;
  std::vector<int> off, mels;
  balance_groups(mt, groups, off, mels);
  d.grp_off = put_section(im, off); d.grp_mels = put_section(im, mels);
  put_mfcc(im, mt, f64, d);
  return TABLES_OK;
}

// Tables of the headline kernel (mfcc_pair.hip).  The filterbank is cut into
// per-lane chunks: a run of consecutive bins whose nonzero filters are the same
// pair (a, b) (a triangle bank has exactly the rising edge of filter j and the
// falling edge of filter j-1 over [p_j, p_{j+1}), mel_scale.go:65-83), split
// into pieces of at most J bins; every filter then sums the partials of its
// chunks in ascending-bin order.  Returns false when the bank does not fit
// (more than 2 filters on one bin, > 64 chunks at J = 16, > 8 chunks per filter).
namespace {
struct Seg { int k0, k1, a, b; };
struct Chunk { int k0, seg; };

// runs of bins whose nonzero filters fit in one pair {a, b}: a run may grow from one filter
// to two (the zero-weight rising start k = l of a triangle opens the run of [l, c)), never
// shrink (a one-filter tail after a two-filter run starts a run of its own)
bool pair_runs(const MfccTables& mt, int K, std::vector<Seg>& segs) {
  for (int k = 0; k < K; k++) {
    int act[3], na = 0;
    for (int m = 0; m < mt.n_mels; m++)
      if (k >= mt.lo[m] && k < mt.hi[m]) { if (na == 2) return false; act[na++] = m; }
    if (na == 0) continue;
    if (!segs.empty() && segs.back().k1 == k) {
      Seg& g = segs.back();
      int u[2] = {g.a, g.b}, nu = g.b >= 0 ? 2 : 1;
      bool fits = true;
      if (na < nu) fits = false;
      for (int i = 0; i < na && fits; i++) {
        bool in = false;
        for (int j = 0; j < nu; j++) in |= (u[j] == act[i]);
        if (!in) { if (nu == 2) { fits = false; break; } u[nu++] = act[i]; }
      }
      if (fits) {
        g.k1 = k + 1;
        if (nu == 2) { g.a = std::min(u[0], u[1]); g.b = std::max(u[0], u[1]); }
        continue;
      }
    }
    segs.push_back({k, k + 1, act[0], na > 1 ? act[1] : -1});
  }
  return true;
}

// Lane order of the chunks, per instance.  The filterbank's power-row reads ld2(prow(ks + i)) are
// ds_read_b64 in the float32 kernel (two 32-lane groups) and ds_read_b128 in the float64 kernel
// (four 16-lane groups), bank (byte / 4) mod 64: chunks whose rows fall on the same banks in one
// group serialise (tools/pair_lds_model.py: 59 extra LDS cycles per pair in ascending order at the
// headline bank in float32, the bulk of its SQ_LDS_BANK_CONFLICT).  A swap search between groups
// lowers that; the filters still sum their chunks in ascending-bin order (the source lists
// follow the chunk order, not the lanes), so the order changes no result bit.
const int kB128Group[64] = {0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0,
                            0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 3, 3, 3, 3,
                            2, 2, 2, 2, 3, 3, 3, 3, 2, 2, 2, 2, 2, 2, 2, 2, 3, 3, 3, 3};
std::vector<int> pair_lane_order(const std::vector<Chunk>& chunks, int J, int e) {
  const int pad = mfcc_pair_pad_rows(e), ew = e ? 4 : 2;   // dwords per lane access
  auto group_of = [&](int l) { return e ? kB128Group[l] : l >> 5; };
  auto fb_conflicts = [&](const std::vector<int>& o) {
    int extra = 0;
    for (int i = 0; i < J; i++) {
      int used[4][64][32], nu[4][64] = {};
      for (int l = 0; l < 64; l++) {
        const int k = chunks[o[l]].k0, g = group_of(l);
        const int dw = ew * (k + pad * (k >> 4)) + ew * i + ((i >= 16 - (k & 15)) ? ew * pad : 0);
        for (int d = 0; d < ew; d++) {
          const int b = (dw + d) & 63;
          bool seen = false;
          for (int u = 0; u < nu[g][b]; u++) seen |= used[g][b][u] == dw + d;
          if (!seen && nu[g][b] < 32) used[g][b][nu[g][b]++] = dw + d;
        }
      }
      for (int g = 0; g < (e ? 4 : 2); g++) {
        int mx = 1;
        for (int b = 0; b < 64; b++) mx = std::max(mx, nu[g][b]);
        extra += mx - 1;
      }
    }
    return extra;
  };
  std::vector<int> order(64);
  for (int l = 0; l < 64; l++) order[l] = l;
  for (int best = fb_conflicts(order), improved = 1; improved;) {
    improved = 0;
    for (int a = 0; a < 64; a++)
      for (int b = a + 1; b < 64; b++) {
        if (group_of(a) == group_of(b)) continue;
        std::swap(order[a], order[b]);
        const int c = fb_conflicts(order);
        if (c < best) { best = c; improved = 1; }
        else std::swap(order[a], order[b]);
      }
  }
  return order;
}
}  // namespace

bool build_pair_tables(const sonar_fp_cfg* cfg, Image& im, PairTableDesc& t) {
  const int W = 1024, K = W / 2 + 1;
  t.ok = false;
  std::vector<double> win;
  if (!make_window(cfg->window_type, W, true, true, kStftBeta, kStftAlpha, win)) return false;
  MfccTables mt;
  if (!mfcc_tables(cfg, W, mt)) return false;
  if (mt.n_mfcc > 16 || mt.n_mels > 64) return false;
  auto weight = [&](int m, int k) -> double {
    return (k >= mt.lo[m] && k < mt.hi[m]) ? mt.w[mt.woff[m] + (k - mt.lo[m])] : 0.0;
  };
  std::vector<Seg> segs;
  if (!pair_runs(mt, K, segs)) return false;
  int J = 1;
  for (;; J++) {
    if (J > 16) return false;
    size_t n = 0;
    for (auto& g : segs) n += (g.k1 - g.k0 + J - 1) / J;
    if (n <= 64) break;
  }
  const double scale = cfg->mfcc_input_power ? 1.0 / 16.0 : 0.25;   // |2X|^2 or |2X|^4 from the pair split
  std::vector<Chunk> chunks;
  for (size_t gi = 0; gi < segs.size(); gi++)
    for (int k0 = segs[gi].k0; k0 < segs[gi].k1; k0 += J) chunks.push_back({k0, (int)gi});
  chunks.resize(64, Chunk{0, -1});                 // idle lanes read bin 0 with zero weights
  for (int e = 0; e < 2; e++) {
    const int JS = mfcc_pair_w_stride(J, e);       // weight row stride (zero-filled past J)
    t.JS[e] = JS;
    const std::vector<int> order = pair_lane_order(chunks, J, e);
    std::vector<int> lane_of(64);
    for (int l = 0; l < 64; l++) lane_of[order[l]] = l;
    std::vector<int> ks(64, 0);
    std::vector<double> cw(64 * 2 * JS, 0.0);
    std::vector<std::vector<int>> src(64);
    for (size_t ci = 0; ci < chunks.size(); ci++) {   // chunk order = ascending bins
      const Chunk& ch = chunks[ci];
      if (ch.seg < 0) continue;
      const Seg& g = segs[ch.seg];
      const int lane = lane_of[ci], k0 = ch.k0;
      ks[lane] = k0;
      for (int i = 0; i < J && k0 + i < g.k1; i++) {
        cw[(lane * JS + i) * 2] = weight(g.a, k0 + i) * scale;
        cw[(lane * JS + i) * 2 + 1] = g.b >= 0 ? weight(g.b, k0 + i) * scale : 0.0;
      }
      src[g.a].push_back(2 * lane);
      if (g.b >= 0) src[g.b].push_back(2 * lane + 1);
    }
    std::vector<uint16_t> msrc(64 * 16, 0x8000);
    int max_src = 1;
    for (int m = 0; m < mt.n_mels; m++) {
      if (src[m].size() > 16) return false;
      max_src = std::max(max_src, (int)src[m].size());
      for (size_t i = 0; i < src[m].size(); i++) msrc[i * 64 + m] = (uint16_t)src[m][i];
    }
    t.max_src = max_src;
    t.chunk_w[e] = put_real(im, cw, e != 0);
    t.chunk_ks[e] = put_section(im, ks); t.mel_src[e] = put_section(im, msrc);
  }
  const int NMP = (mt.n_mels + 7) / 8 * 8;
  auto dct_rows = [&](int e) {             // [16][NMP + pad]
    const int st = NMP + mfcc_pair_dct_pad(e);
    std::vector<double> dct(16 * st, 0.0);
    for (int q = 0; q < mt.n_mfcc; q++)
      for (int m = 0; m < mt.n_mels; m++) dct[q * st + m] = mt.dct[(size_t)q * mt.n_mels + m] * mt.lift[q];
    return dct;
  };
  std::vector<double> tw1(64 * 16 * 2), tw2(64 * 2);
  for (int b = 0; b < 64; b++)
    for (int k = 0; k < 16; k++) {
      const double a = -2.0 * kPi * (double)((b * k) % 1024) / 1024.0;
      tw1[(b * 16 + k) * 2] = std::cos(a); tw1[(b * 16 + k) * 2 + 1] = std::sin(a);
    }
  for (int b = 0; b < 8; b++)
    for (int c = 0; c < 8; c++) {
      const double a = -2.0 * kPi * (double)(b * c) / 64.0;
      tw2[(b * 8 + c) * 2] = std::cos(a); tw2[(b * 8 + c) * 2 + 1] = std::sin(a);
    }
  // float32 tables = the float64 values rounded once; float64 tables as computed
  for (int e = 0; e < 2; e++) {
    t.window[e] = put_real(im, win, e != 0); t.tw1[e] = put_real(im, tw1, e != 0); t.tw2[e] = put_real(im, tw2, e != 0);
    t.dct[e] = put_real(im, dct_rows(e), e != 0);
  }
  t.zeros = put_section(im, std::vector<double>(1024, 0.0));
  t.J = J; t.NMP = NMP; t.n_mels = mt.n_mels; t.n_mfcc = mt.n_mfcc;
  t.ok = true;
  return true;
}

}  // namespace host
}  // namespace sonar
