// pair_layout_check -- csrc/pair_batch_layout.h under a plain host compiler: the sections of a pair
// batch's buffer are 256-byte aligned, disjoint and in the stated order, the head is a prefix, the
// upload is one contiguous run starting at the DTW arguments, the total is the sum, and the offsets
// are those of the formulas the layout replaced (restated here, and a handful as literals).  Prints one
// line per failure; exit status 1 if there is any.
#include <cstdint>
#include <cstdio>

#include "../../sonido-sonar_amd/csrc/pair_batch_layout.h"

using sonar::PairBatchLayout;

static int failures = 0;
static void check(bool ok, const char* what, long long n, long long bands, size_t got, size_t want) {
  if (ok) return;
  std::printf("FAIL %s (n=%lld bands=%lld): got %zu, want %zu\n", what, n, bands, got, want);
  failures++;
}
static void eq(const char* what, long long n, long long bands, size_t got, size_t want) {
  check(got == want, what, n, bands, got, want);
}

// element sizes as the library has them on x86-64: DtwArgs, ScoreJob, PathSums, CorrSums
static const size_t ARGS = 192, JOB = 64, PSUM = 72, CSUM = 64;
static size_t up256(size_t x) { return (x + 255) / 256 * 256; }

static void one(int64_t n, int64_t bands, size_t corr_b, size_t path_b) {
  const PairBatchLayout L(n, bands, corr_b, path_b, ARGS, JOB, PSUM, CSUM);
  const size_t off[11] = {L.status, L.diag, L.path_sums, L.corr_sums, L.args, L.starts, L.map, L.jobs, L.corr, L.path,
                          L.total};
  // what each section must hold; corr and path totals are sums of 256-byte aligned regions already
  const size_t need[10] = {(size_t)n * 32 + 16, (size_t)n * 128, (size_t)n * PSUM, (size_t)n * CSUM, (size_t)n * ARGS,
                           (size_t)(n + 1) * 8, (size_t)bands * 8, (size_t)n * JOB, corr_b, path_b};
  size_t at = 0, sum = 0;
  eq("first section", n, bands, off[0], 0);
  for (int i = 0; i < 10; ++i) {
    eq("aligned", n, bands, off[i] % 256, 0);
    eq("offset", n, bands, off[i], at);                      // in order, disjoint, no gap beyond the padding
    check(off[i + 1] - off[i] >= need[i], "room", n, bands, off[i + 1] - off[i], need[i]);
    at += up256(need[i]);
    sum += up256(need[i]);
  }
  eq("total", n, bands, L.total, sum);
  eq("ticket", n, bands, L.ticket, (size_t)n * 32);
  check(L.ticket + 16 <= L.diag, "ticket inside status", n, bands, L.ticket + 16, L.diag);
  eq("head is a prefix ending at the arguments", n, bands, L.head_bytes(), L.args);
  eq("clear covers status and diag", n, bands, L.clear_bytes(), L.path_sums);
  eq("upload starts at the arguments", n, bands, L.upload_offset(), L.args);
  eq("upload ends at the correlations", n, bands, L.upload_offset() + L.upload_bytes(), L.corr);
  // the formulas of the hand-written layout this header replaced
  const size_t stat_b = up256((size_t)n * 32 + 16), diag_b = up256((size_t)n * 8 * 16), ps_b = up256((size_t)n * PSUM),
               cs_b = up256((size_t)n * CSUM), args_b = up256((size_t)n * ARGS), start_b = up256((size_t)(n + 1) * 8),
               map_b = up256((size_t)bands * 8), sj_b = up256((size_t)n * JOB);
  const size_t head_b = stat_b + diag_b + ps_b + cs_b, up_b = args_b + start_b + map_b + sj_b;
  eq("diag (old)", n, bands, L.diag, stat_b);
  eq("path_sums (old)", n, bands, L.path_sums, stat_b + diag_b);
  eq("corr_sums (old)", n, bands, L.corr_sums, stat_b + diag_b + ps_b);
  eq("head (old)", n, bands, L.head_bytes(), head_b);
  eq("starts (old)", n, bands, L.starts, head_b + args_b);
  eq("map (old)", n, bands, L.map, head_b + args_b + start_b);
  eq("jobs (old)", n, bands, L.jobs, head_b + args_b + start_b + map_b);
  eq("upload (old)", n, bands, L.upload_bytes(), up_b);
  eq("corr (old)", n, bands, L.corr, head_b + up_b);
  eq("path (old)", n, bands, L.path, head_b + up_b + corr_b);
  eq("total (old)", n, bands, L.total, head_b + up_b + corr_b + path_b);
  // the typed accessor is base + offset for either base
  char buf[1];
  eq("accessor", n, bands, (size_t)((char*)PairBatchLayout::at<int64_t>(buf, L.starts) - buf), L.starts);
}

int main() {
  const int64_t ns[4] = {1, 2, 8, 128};
  for (int64_t n : ns) {
    const int64_t bands[3] = {1, 2, n * 162};
    for (int64_t b : bands)
      for (int z = 0; z < 2; ++z) one(n, b, z ? (size_t)n * 55296 : 0, z ? (size_t)n * 331008 : 0);
  }
  // literals worked out by hand from the old formulas
  {
    const PairBatchLayout L(1, 1, 0, 0, ARGS, JOB, PSUM, CSUM);
    eq("n=1 head", 1, 1, L.head_bytes(), 1024);
    eq("n=1 corr", 1, 1, L.corr, 2048);
    eq("n=1 total", 1, 1, L.total, 2048);
  }
  {
    const PairBatchLayout L(2, 2, 0, 0, ARGS, JOB, PSUM, CSUM);
    eq("n=2 args", 2, 2, L.args, 1024);
    eq("n=2 starts", 2, 2, L.starts, 1536);
    eq("n=2 corr", 2, 2, L.corr, 2304);
  }
  {
    const PairBatchLayout L(8, 1296, 4096, 8192, ARGS, JOB, PSUM, CSUM);
    eq("n=8 diag", 8, 1296, L.diag, 512);
    eq("n=8 path_sums", 8, 1296, L.path_sums, 1536);
    eq("n=8 corr_sums", 8, 1296, L.corr_sums, 2304);
    eq("n=8 args", 8, 1296, L.args, 2816);
    eq("n=8 starts", 8, 1296, L.starts, 4352);
    eq("n=8 map", 8, 1296, L.map, 4608);
    eq("n=8 jobs", 8, 1296, L.jobs, 15104);
    eq("n=8 corr", 8, 1296, L.corr, 15616);
    eq("n=8 path", 8, 1296, L.path, 19712);
    eq("n=8 total", 8, 1296, L.total, 27904);
  }
  {
    const PairBatchLayout L(128, 20736, 0, 0, ARGS, JOB, PSUM, CSUM);
    eq("n=128 head", 128, 20736, L.head_bytes(), 38144);
    eq("n=128 upload", 128, 20736, L.upload_bytes(), 199936);
    eq("n=128 corr", 128, 20736, L.corr, 238080);
  }
  if (failures) return 1;
  std::printf("pair_layout ok\n");
  return 0;
}
