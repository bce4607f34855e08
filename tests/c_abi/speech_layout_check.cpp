// speech_layout_check -- csrc/speech_layout.h under a plain host compiler: the sections of the speech
// extractor's result block start on multiples of 8 doubles, are disjoint and in the stated order, the
// total is their sum, and the offsets are those of the hand-written sequence the header replaced
// (restated here, and one case as literals).  Prints one line per failure; exit status 1 if there is any.
#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "../../sonido-sonar_amd/csrc/speech_layout.h"

using sonar::SpeechPlan;

static int failures = 0;
static void eq(const char* what, const char* name, long long got, long long want) {
  if (got == want) return;
  std::printf("FAIL %s (%s): got %lld, want %lld\n", what, name, got, want);
  failures++;
}

struct Case { const char* name; int64_t n; int W, H, rate, win, hop, nm; bool mfcc, speech; };

static void one(const Case& k) {
  const int64_t F = (k.n - k.W) / k.H + 1;
  const SpeechPlan p(k.n, F, k.rate, k.win, k.hop, k.nm, k.mfcc, k.speech);
  // the frame counts, from the formulas of the Go code
  const int64_t Fe = k.n < k.win ? 0 : (k.n - k.win) / k.hop + 1, Fp = std::max<int64_t>((k.n - 1024) / 512 + 1, 0);
  const int64_t Fenv = k.n < 512 ? 0 : (k.n - 512) / 256 + 1;
  const int lw = (int)(0.4 * (double)k.rate), lh = std::max(1, lw / 4);
  const int64_t Fl = k.rate > 0 && k.n >= lw ? (k.n - lw) / lh + 1 : 0;
  const int nm = k.nm > 0 ? k.nm : 13;
  eq("F", k.name, p.F, F); eq("Fe", k.name, p.Fe, Fe); eq("Fp", k.name, p.Fp, Fp); eq("Fenv", k.name, p.Fenv, Fenv);
  eq("Fl", k.name, p.Fl, Fl); eq("lw", k.name, p.lw, lw); eq("lh", k.name, p.lh, lh); eq("nm", k.name, p.nm, nm);
  // what each section must hold
  const size_t need[SpeechPlan::NSEC] = {k.mfcc ? (size_t)F * nm : 0, (size_t)F * 9, (size_t)F, (size_t)Fe, (size_t)Fe,
                                         (size_t)Fp, (size_t)Fp, 1024, (size_t)Fenv, (size_t)Fl, k.speech ? (size_t)Fp : 0,
                                         (size_t)std::min<int64_t>(k.n, 1024), 6 * (size_t)Fp, Fe > F ? 2 * (size_t)Fe : 0};
  size_t at = 0;
  for (int i = 0; i < SpeechPlan::NSEC; i++) {
    eq("aligned", k.name, p.sec[i].off % 8, 0);
    eq("offset", k.name, p.sec[i].off, at);                      // in order, disjoint, no gap beyond the padding
    eq("count", k.name, p.sec[i].cnt, need[i]);
    at += (need[i] + 7) / 8 * 8;
  }
  eq("total", k.name, p.total, at);
  eq("lohi", k.name, p.lohi_copy(), Fe > F);
  // the hand-written sequence: take() after take(), each rounded up to 8 doubles
  size_t off = 0;
  auto take = [&](size_t cnt) { const size_t o = off; off += (cnt + 7) & ~size_t(7); return o; };
  const size_t Fz = (size_t)F, Fe_z = (size_t)Fe, Fp_z = (size_t)Fp;
  const size_t o_mfcc = take(k.mfcc ? Fz * nm : 0), o_spec = take(Fz * 9), o_zcr = take(Fz);
  const size_t o_en = take(Fe_z), o_ent = take(Fe_z), o_praw = take(Fp_z), o_craw = take(Fp_z);
  const size_t o_part = take(256 * 4), o_env = take((size_t)Fenv), o_loud = take((size_t)Fl);
  const size_t o_tilt = take(k.speech ? Fp_z : 0), o_head = take((size_t)std::min<int64_t>(k.n, 1024));
  const size_t o_trk = take(6 * Fp_z), o_lohi = take(Fe > F ? 2 * Fe_z : 0);
  const size_t old[SpeechPlan::NSEC] = {o_mfcc, o_spec, o_zcr, o_en, o_ent, o_praw, o_craw, o_part, o_env, o_loud, o_tilt,
                                        o_head, o_trk, o_lohi};
  for (int i = 0; i < SpeechPlan::NSEC; i++) eq("offset (old)", k.name, p.sec[i].off, old[i]);
  eq("total (old)", k.name, p.total, off);
  double base[1];
  eq("accessor", k.name, p.at(base, SpeechPlan::ZCR) - base, p.sec[SpeechPlan::ZCR].off);
}

int main() {
  const Case cases[] = {
      {"talk 2 s 16 kHz", 32000, 512, 128, 16000, 512, 128, 13, true, true},
      {"mfcc off", 32000, 512, 128, 16000, 512, 128, 13, false, true},
      {"speech off", 32000, 512, 128, 16000, 512, 128, 13, true, false},
      {"both off, 0 coefficients", 32000, 512, 128, 16000, 512, 128, 0, false, false},
      {"Fe > F", 32000, 1024, 256, 16000, 256, 64, 13, true, true},
      {"Fe < F", 32000, 512, 128, 16000, 2048, 512, 13, true, true},
      {"no energy frame", 3000, 512, 128, 16000, 4096, 128, 13, true, true},
      {"n < 1024", 1000, 256, 64, 16000, 256, 64, 13, true, true},
      {"n < 512", 300, 128, 32, 16000, 128, 32, 20, true, false},
      {"rate 0 (music, 10 s)", 441000, 1024, 256, 0, 1024, 256, 13, true, false},
      {"odd sizes", 100003, 1000, 333, 22050, 777, 111, 7, true, true},
  };
  for (const Case& k : cases) one(k);
  {  // worked out by hand: n = 32000, W = 512 / H = 128 both ways, rate 16000, 13 coefficients, all on.
     // F = Fe = 247, Fp = 61, Fenv = 124, lw = 6400, lh = 1600, Fl = 17
    const SpeechPlan p(32000, 247, 16000, 512, 128, 13, true, true);
    const long long want[SpeechPlan::NSEC] = {0, 3216, 5440, 5688, 5936, 6184, 6248, 6312, 7336, 7464, 7488, 7552, 8576, 8944};
    for (int i = 0; i < SpeechPlan::NSEC; i++) eq("offset (literal)", "talk 2 s 16 kHz", p.sec[i].off, want[i]);
    eq("total (literal)", "talk 2 s 16 kHz", p.total, 8944);
    eq("Fl (literal)", "talk 2 s 16 kHz", p.Fl, 17);
  }
  if (failures) return 1;
  std::printf("speech_layout ok\n");
  return 0;
}
