// pair_batch_layout.h -- the one description of a pair batch's "pb.small" (device) and "pb.host"
// (pinned) buffers of sonar_align_pairs (pairs_api.cpp).  Both hold the same sections at the same
// byte offsets, every section 256-byte aligned, in this order:
//   status      one PairStatus per pair, then the batch's ticket word
//   diag        the band kernel's diagnostic record of each pair
//   path_sums   the device scorer's PathSums of each pair
//   corr_sums   ... and its CorrSums               (status .. corr_sums: the head, what comes back)
//   args        one DtwArgs per pair
//   starts      n + 1 ticket starts
//   map         one (pair, band) ticket per band, band-major
//   jobs        one ScoreJob per pair               (args .. jobs: the upload, one copy)
//   corr, path  the pairs' energy correlations, then their path blocks (back with host scoring only)
// No HIP types here: the element sizes come in as numbers, so the plain host compiler can check the
// arithmetic (tests/c_abi/pair_layout_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

namespace sonar {

inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

// one pair's status words: DtwArgs::plen, cnm and sync point at them
struct PairStatus {
  int64_t plen;      // points of the warping path
  double cnm;        // C[nq][nr]
  int32_t sync[4];   // [0] band ticket, [1] error flag, [2] non-finite input flag
};
static_assert(sizeof(PairStatus) == 32, "the kernels write a pair's status as eight 32-bit words");
constexpr size_t PAIR_DIAG_BYTES = 128;   // per pair: DTW_DIAG_WORDS 64-bit words

struct PairBatchLayout {
  // section offsets in bytes, the ticket word's, and the buffer's size
  size_t status = 0, diag = 0, path_sums = 0, corr_sums = 0, args = 0, starts = 0, map = 0, jobs = 0, corr = 0,
         path = 0, ticket = 0, total = 0;

  PairBatchLayout() = default;
  PairBatchLayout(int64_t n, int64_t total_bands, size_t corr_bytes, size_t path_bytes, size_t args_size,
                  size_t job_size, size_t path_sums_size, size_t corr_sums_size) {
    auto take = [this](size_t bytes) { const size_t off = total; total += al256(bytes); return off; };
    ticket = (size_t)n * sizeof(PairStatus);
    status = take(ticket + 16);
    diag = take((size_t)n * PAIR_DIAG_BYTES);
    path_sums = take((size_t)n * path_sums_size);
    corr_sums = take((size_t)n * corr_sums_size);
    args = take((size_t)n * args_size);
    starts = take((size_t)(n + 1) * 8);
    map = take((size_t)total_bands * 8);
    jobs = take((size_t)n * job_size);
    corr = take(corr_bytes);
    path = take(path_bytes);
  }
  size_t head_bytes() const { return args; }         // [0, head): the copy back without host scoring
  size_t clear_bytes() const { return path_sums; }   // [0, clear): status and diag, zeroed per batch
  size_t upload_offset() const { return args; }
  size_t upload_bytes() const { return corr - args; }
  // section `off` of the buffer at `base` (the device or the pinned one) as an array of T
  template <class T>
  static T* at(void* base, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(base) + off); }
};

}  // namespace sonar
