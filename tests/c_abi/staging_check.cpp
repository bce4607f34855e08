// csrc/staging.h under the plain host compiler, against a stub of the few runtime calls Staging makes
// itself.  The stub is asynchronous as a stream is: a copy or a memset is only recorded, and carried
// out at the next hipStreamSynchronize; it can fail its k-th call.  Checked: the exact call list of an
// entry that uses every method, in host and in device pointer mode, and that the values arrive; and,
// with each call of that list failed in turn, that the entry returns SONAR_ERR_DEVICE naming the call
// and that nothing is left queued once its Staging is gone (what is left is carried out then, as a
// stream would: the sanitizer build sees that write into freed memory); and that a Staging which owns no
// host memory adds no synchronisation when it goes.
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "../../sonido-sonar_amd/csrc/staging.h"

namespace {

struct Op { std::function<void()> run; };
std::vector<Op> g_pending;            // queued on the one stream, in order
std::vector<std::string> g_calls;     // the runtime calls made, by name (+ the copy kind)
int g_fail_at = 0;                    // fail the call with this 1-based index; 0: none
std::map<std::string, void*> g_dev;   // the context's named scratch: "device" memory, alive to the end
int g_bad = 0;

bool refuse(const std::string& name) {
  g_calls.push_back(name);
  return (int)g_calls.size() == g_fail_at;
}
void run_stream() {
  for (Op& op : g_pending) op.run();
  g_pending.clear();
}
// stands for a kernel launch: not a runtime call Staging makes, so it is neither counted nor failed
void launch(std::function<void()> fn) { g_pending.push_back({std::move(fn)}); }

void expect(bool ok, const char* what, const std::string& where) {
  if (ok) return;
  std::printf("FAIL %s: %s\n", where.c_str(), what);
  ++g_bad;
}

}  // namespace

extern "C" {
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t) {
  const char* k = kind == hipMemcpyHostToDevice ? "H2D" : kind == hipMemcpyDeviceToHost ? "D2H" : "D2D";
  if (refuse(std::string("hipMemcpyAsync ") + k)) return hipErrorUnknown;
  g_pending.push_back({[=] { std::memcpy(dst, src, bytes); }});
  return hipSuccess;
}
hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t) {
  if (refuse("hipMemsetAsync")) return hipErrorUnknown;
  g_pending.push_back({[=] { std::memset(dst, value, bytes); }});
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) {
  if (refuse("hipStreamSynchronize")) return hipErrorUnknown;
  run_stream();
  return hipSuccess;
}
const char* hipGetErrorString(hipError_t) { return "stub failure"; }
}

namespace sonar {
namespace detail {
int fail(sonar_ctx* c, int code, const std::string& msg) {
  c->err = msg;
  return code;
}
void* dbuf(sonar_ctx*, const std::string& name, size_t bytes) {
  void*& p = g_dev[name];
  if (!p) p = std::calloc(1, bytes < 64 ? 64 : bytes);   // every request of one name is the same size here
  return p;
}
}  // namespace detail
}  // namespace sonar

namespace {

constexpr size_t N = 5;

// what the caller of the entry holds: "device" arrays in device mode, host arrays otherwise
struct Caller {
  double *in, *out, *rows;
  int32_t* code;
  int64_t count = -1;         // host memory in both modes
  int32_t flags = -1;         // what the entry saw in flags()
  double seen[2] = {-1, -1};  // what it read back mid-call
  Caller() : in(new double[N]), out(new double[N]()), rows(new double[N]()), code(new int32_t(0)) {
    for (size_t i = 0; i < N; ++i) in[i] = 1.0 + (double)i;
  }
  ~Caller() { delete[] in; delete[] out; delete[] rows; delete code; }
};

// An entry as the host layer writes them: allocations, ready, launches, a mid-call fetch, more
// launches, give and put, finish (and a second finish, which has nothing left to queue).
int entry(sonar_ctx* c, bool dev, Caller& u) {
  using sonar::detail::Staging;
  Staging o{c, "t.", dev};
  const double* din = o.in("in", u.in, N);
  double* dout = o.out("out", u.out, N);
  double* dtmp = o.tmp<double>("tmp", N);
  int64_t* dcount = o.tmp<int64_t>("count", 1);
  const uint8_t mask[3] = {1, 0, 1};
  const uint8_t* dmask = o.in_host("mask", mask, 3);
  int32_t* dflag = o.flag();
  o.host_out(&u.count, dcount, 1);
  int rc = o.ready("device allocation failed");
  if (rc != SONAR_OK) return rc;
  launch([=] {
    for (size_t i = 0; i < N; ++i) dtmp[i] = 2.0 * din[i];
    *dflag = 4 + dmask[0] + dmask[1] + dmask[2];
  });
  const double* seen = o.back(dtmp + 1, 2);
  rc = o.fetch();
  if (rc != SONAR_OK) return rc;
  u.flags = o.flags();
  u.seen[0] = seen[0];
  u.seen[1] = seen[1];
  launch([=] {
    for (size_t i = 0; i < N; ++i) dout[i] = dtmp[i] + 1.0;
    *dcount = 7;
  });
  rc = o.give(u.rows, dtmp, N * 8);
  if (rc != SONAR_OK) return rc;
  {
    const int32_t value = 42;   // gone before the stream runs
    rc = o.put(u.code, &value, 4);
  }
  if (rc != SONAR_OK) return rc;
  rc = o.finish();
  if (rc != SONAR_OK) return rc;
  return o.finish();
}

const std::vector<std::string> kHostCalls = {
    "hipMemcpyAsync H2D", "hipMemcpyAsync H2D", "hipMemsetAsync",                // ready: in, mask, flag
    "hipMemcpyAsync D2H", "hipMemcpyAsync D2H", "hipStreamSynchronize",          // fetch: flag, back
    "hipMemcpyAsync D2H",                                                        // give
    "hipMemcpyAsync D2H", "hipMemcpyAsync D2H", "hipStreamSynchronize",          // finish: out, count
    "hipStreamSynchronize"};                                                     // second finish
const std::vector<std::string> kDevCalls = {
    "hipMemcpyAsync H2D", "hipMemsetAsync",                                      // ready: mask, flag
    "hipMemcpyAsync D2H", "hipMemcpyAsync D2H", "hipStreamSynchronize",          // fetch: flag, back
    "hipMemcpyAsync D2D", "hipMemcpyAsync H2D",                                  // give, put
    "hipMemcpyAsync D2H", "hipStreamSynchronize",                                // finish: count
    "hipStreamSynchronize"};                                                     // second finish

// one call of the entry; returns its code; what was still queued when its Staging had gone is counted
// and then carried out
int call(bool dev, int fail_at, Caller& u, sonar_ctx& c, size_t* left) {
  g_calls.clear();
  g_fail_at = fail_at;
  const int rc = entry(&c, dev, u);
  g_fail_at = 0;
  *left = g_pending.size();
  if (*left) std::printf("FAIL: %zu operations still queued when the entry had returned\n", *left);
  std::fflush(stdout);
  run_stream();
  return rc;
}

void check_mode(bool dev) {
  const std::string mode = dev ? "device mode" : "host mode";
  const std::vector<std::string>& want = dev ? kDevCalls : kHostCalls;
  sonar_ctx c;
  size_t left = 0;
  {
    Caller u;
    const int rc = call(dev, 0, u, c, &left);
    expect(rc == SONAR_OK, "the entry succeeds", mode);
    expect(g_calls == want, "the call list is the expected one", mode);
    expect(left == 0, "nothing is queued after the entry", mode);
    expect(u.flags == 6, "flags() holds the device's word", mode);
    expect(u.seen[0] == 4.0 && u.seen[1] == 6.0, "the read-back holds the device's values", mode);
    expect(u.count == 7, "host_out arrives", mode);
    expect(*u.code == 42, "put arrives", mode);
    for (size_t i = 0; i < N; ++i)
      expect(u.out[i] == 2.0 * u.in[i] + 1.0 && u.rows[i] == 2.0 * u.in[i], "out and give arrive", mode);
  }
  for (int k = 1; k <= (int)want.size(); ++k) {
    Caller u;
    const std::string where = mode + ", call " + std::to_string(k) + " (" + want[(size_t)k - 1] + ") failed";
    const int rc = call(dev, k, u, c, &left);
    const std::string name = want[(size_t)k - 1].substr(0, want[(size_t)k - 1].find(' '));
    expect(rc == SONAR_ERR_DEVICE, "the entry returns SONAR_ERR_DEVICE", where);
    expect(c.err.compare(0, name.size() + 1, name + "(") == 0 && c.err.find(": stub failure") != std::string::npos,
           "the text names the failing call", where);
    expect(left == 0, "nothing is queued once the Staging is gone", where);
  }
}

// A helper that only stages scratch for a caller that waits itself owns no host memory: its Staging
// going out of scope adds no synchronisation.
void check_helper() {
  sonar_ctx c;
  const double pcm[2] = {1.0, 2.0};
  g_calls.clear();
  {
    sonar::detail::Staging st{&c, "h.", false};
    const double* d = st.in("pcm", pcm, 2);
    expect(st.ready("device allocation failed") == SONAR_OK && d != nullptr, "the helper stages its input", "helper");
  }
  expect(g_calls == std::vector<std::string>{"hipMemcpyAsync H2D"}, "no synchronisation when nothing is owned", "helper");
  run_stream();
}

}  // namespace

int main() {
  check_mode(false);
  check_mode(true);
  check_helper();
  for (auto& d : g_dev) std::free(d.second);
  if (g_bad) return 1;
  std::printf("staging ok\n");
  return 0;
}
