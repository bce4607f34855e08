// fp_tables_check -- csrc/fp_tables.cpp under a plain host compiler: builds the table image of one
// fingerprint path for a bank given on the command line and prints what a test compares:
//   fp_tables_check pair SAMPLE_RATE N_FILTERS [INPUT_POWER]   per precision J, JS, NMP, max_src, the 64
//                                                              chunk_ks and every filter's source list
//   fp_tables_check dft  W SAMPLE_RATE N_FILTERS RAW MFCC
//   fp_tables_check wave W SAMPLE_RATE N_FILTERS F64 GROUPS RAW
// and, for each, an FNV-1a checksum of every section of the image (a section runs to the next one's start)
// and of the whole image.  The other fields of the configuration are sonar_fp_cfg_default's.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../sonido-sonar_amd/csrc/fp_tables.h"

namespace host = sonar::host;

static unsigned long long fnv(const unsigned char* p, size_t n) {
  unsigned long long h = 1469598103934665603ull;
  for (size_t i = 0; i < n; i++) { h ^= p[i]; h *= 1099511628211ull; }
  return h;
}

static int sections(const host::Image& im, std::vector<std::pair<size_t, std::string>> s) {
  std::sort(s.begin(), s.end());
  int bad = 0;
  for (size_t i = 0; i < s.size(); i++) {
    const size_t end = i + 1 < s.size() ? s[i + 1].first : im.size();
    if (s[i].first % host::kSectionAlign != 0 || end <= s[i].first || end > im.size()) {
      std::printf("FAIL section %s at %zu\n", s[i].second.c_str(), s[i].first);
      bad = 1;
      continue;
    }
    std::printf("section %s offset %zu bytes %zu fnv %016llx\n", s[i].second.c_str(), s[i].first, end - s[i].first,
                fnv(im.data() + s[i].first, end - s[i].first));
  }
  std::printf("image bytes %zu fnv %016llx\n", im.size(), fnv(im.data(), im.size()));
  return bad;
}

static sonar_fp_cfg config(int W, int sr, int nf) {
  sonar_fp_cfg c;
  std::memset(&c, 0, sizeof(c));
  c.window_size = W; c.hop_size = W / 4; c.window_type = SONAR_WIN_HANN; c.sample_rate = sr;
  c.n_mfcc = 13; c.n_filters = nf; c.filterbank = SONAR_FB_MEL; c.use_lifter = 1; c.lifter = 22.0;
  return c;
}

static int fp(const host::Image& im, const host::FpTableDesc& d, bool trig, bool groups) {
  std::printf("n_mels %d n_mfcc %d nnz %d has_mfcc %d\n", d.n_mels, d.n_mfcc, d.nnz, (int)d.has_mfcc);
  std::vector<std::pair<size_t, std::string>> s = {{d.window, "window"}};
  if (trig) s.push_back({d.trig, "trig"});
  if (d.has_mfcc) {
    s.insert(s.end(), {{d.mel_lo, "mel_lo"}, {d.mel_hi, "mel_hi"}, {d.mel_woff, "mel_woff"}, {d.mel_w, "mel_w"},
                       {d.dct, "dct"}, {d.lift, "lift"}});
    if (groups) s.insert(s.end(), {{d.grp_off, "grp_off"}, {d.grp_mels, "grp_mels"}});
  }
  return sections(im, s);
}

static int pair(int sr, int nf, int power) {
  sonar_fp_cfg c = config(1024, sr, nf);
  c.mfcc_input_power = power;
  host::Image im;
  host::PairTableDesc d;
  if (!host::build_pair_tables(&c, im, d) || !d.ok) { std::printf("refused\n"); return 0; }
  std::vector<std::pair<size_t, std::string>> s = {{d.zeros, "zeros"}};
  for (int e = 0; e < 2; e++) {
    const char* pr = e ? "f64" : "f32";
    std::printf("%s J %d JS %d NMP %d max_src %d n_mels %d n_mfcc %d\n", pr, d.J, d.JS[e], d.NMP, d.max_src, d.n_mels,
                d.n_mfcc);
    const int* ks = reinterpret_cast<const int*>(im.data() + d.chunk_ks[e]);
    std::printf("%s ks", pr);
    for (int l = 0; l < 64; l++) std::printf(" %d", ks[l]);
    std::printf("\n");
    const uint16_t* src = reinterpret_cast<const uint16_t*>(im.data() + d.mel_src[e]);   // [16][64], bit 15 = unused
    for (int m = 0; m < d.n_mels; m++) {
      std::printf("%s src %d:", pr, m);
      for (int i = 0; i < 16 && !(src[i * 64 + m] & 0x8000); i++) std::printf(" %d", (int)src[i * 64 + m]);
      std::printf("\n");
    }
    const std::string p = std::string(pr) + ".";
    s.insert(s.end(), {{d.window[e], p + "window"}, {d.tw1[e], p + "tw1"}, {d.tw2[e], p + "tw2"},
                       {d.chunk_w[e], p + "chunk_w"}, {d.dct[e], p + "dct"}, {d.chunk_ks[e], p + "chunk_ks"},
                       {d.mel_src[e], p + "mel_src"}});
  }
  return sections(im, s);
}

int main(int argc, char** argv) {
  auto arg = [&](int i) { return i < argc ? std::atoi(argv[i]) : 0; };
  const std::string kind = argc > 1 ? argv[1] : "";
  host::Image im;
  host::FpTableDesc d;
  if (kind == "pair" && argc >= 4) return pair(arg(2), arg(3), arg(4));
  if (kind == "dft" && argc >= 7) {
    const sonar_fp_cfg c = config(arg(2), arg(3), arg(4));
    const int rc = host::build_dft_tables(&c, arg(5) != 0, arg(6) != 0, im, d);
    if (rc != host::TABLES_OK) { std::printf("refused %d\n", rc); return 0; }
    return fp(im, d, true, false);
  }
  if (kind == "wave" && argc >= 8) {
    const sonar_fp_cfg c = config(arg(2), arg(3), arg(4));
    const int rc = host::build_wave_tables(&c, arg(7) != 0, arg(5) != 0, arg(6), im, d);
    if (rc != host::TABLES_OK) { std::printf("refused %d\n", rc); return 0; }
    return fp(im, d, false, true);
  }
  std::fprintf(stderr, "usage: fp_tables_check pair SR NF [POWER] | dft W SR NF RAW MFCC | wave W SR NF F64 GROUPS RAW\n");
  return 2;
}
