// staging.h -- where the arrays of one entry live during a call that takes host or device pointers
// (device_ptrs): the caller's own device arrays, or named scratch of the context that is filled from
// the caller's host arrays before the launches and copied back to them at the end; and the host memory
// of the call's other copies (device words read back, host values uploaded), kept until the stream is idle.
#pragma once
#include <cstring>
#include <deque>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

#include "ctx.h"

namespace sonar {
namespace detail {

// zeros a caller's output: device memory on the context's stream, host memory at once
inline int zero_out(sonar_ctx* c, void* p, size_t bytes, bool dev) {
  if (!p || bytes == 0) return SONAR_OK;
  if (dev) HIP_TRY(c, hipMemsetAsync(p, 0, bytes, c->stream));
  else std::memset(p, 0, bytes);
  return SONAR_OK;
}

struct Staging {
  sonar_ctx* c;
  const char* prefix;   // scratch buffers are named prefix + name
  bool dev;             // the caller's pointers are device pointers
  bool nomem = false;   // a scratch allocation failed: ready() reports it, once
  bool queued = false;  // something may be queued on c->stream since the last synchronisation issued here
  struct Copy { void* dst; const void* src; size_t bytes; };
  std::vector<Copy> h2d, d2h, backs;   // for ready() | finish() | fetch() and finish()
  std::deque<std::vector<unsigned char>> owned;   // host ends of backs and uploads; a deque keeps their addresses
  int32_t* dflag = nullptr; const int32_t* hflag = nullptr;   // the call's status word (flag) and its read-back

  Staging(sonar_ctx* ctx, const char* name_prefix, bool device_ptrs) : c(ctx), prefix(name_prefix), dev(device_ptrs) {}
  Staging(const Staging&) = delete;
  Staging& operator=(const Staging&) = delete;
  // an early exit: the stream is waited for (result ignored) before the owned host memory goes.  One that owns
  // none (scratch for a helper whose caller waits, fp_api.cpp, music_api.cpp, ...) has nothing to outlive.
  ~Staging() { if (queued && !owned.empty()) (void)hipStreamSynchronize(c->stream); }

  // scratch of the call
  template <typename T>
  T* tmp(const char* name, size_t count) {
    T* d = (T*)dbuf(c, std::string(prefix) + name, count * sizeof(T));
    if (!d) nomem = true;
    return d;
  }
  // an input: the caller's device array, or scratch that ready() fills from the caller's host array
  template <typename T>
  const T* in(const char* name, const T* user, size_t count) {
    if (dev || !user || count == 0) return user;
    T* d = tmp<T>(name, count);
    if (d) h2d.push_back({d, user, count * sizeof(T)});
    return d;
  }
  // host values of the entry's own as a device input, in either mode: ready() fills scratch from a copy kept here
  template <typename T>
  const T* in_host(const char* name, const T* host, size_t count) {
    T* d = tmp<T>(name, count);
    if (d) h2d.push_back({d, std::memcpy(own(count * sizeof(T)), host, count * sizeof(T)), count * sizeof(T)});
    return d;
  }
  // an output: the caller's device array, or scratch that finish() copies to the caller's host array;
  // an output the caller does not want (null) stays null
  template <typename T>
  T* out(const char* name, T* user, size_t count) {
    if (!user || dev) return user;
    T* d = tmp<T>(name, count);
    if (d) d2h.push_back({user, d, count * sizeof(T)});
    return d;
  }
  // an output that is host memory in both pointer modes: finish() copies dev_src to it
  template <typename T>
  void host_out(T* host, const T* dev_src, size_t count) {
    if (host && dev_src && count) d2h.push_back({host, dev_src, count * sizeof(T)});
  }
  // device values the host reads: at the returned address after the next fetch() or finish(), zeros before
  template <typename T>
  const T* back(const T* dev_src, size_t count) {
    T* h = (T*)own(count * sizeof(T));
    if (dev_src && count) backs.push_back({h, dev_src, count * sizeof(T)});
    return h;
  }
  // the call's one status word: ready() zeroes it, finish() or fetch() reads it back for flags()
  int32_t* flag() {
    dflag = tmp<int32_t>("flag", 1);
    hflag = back(dflag, 1);
    return dflag;
  }
  int32_t flags() const { return hflag ? *hflag : 0; }
  // after the allocations, before the launches: the one SONAR_ERR_NOMEM, else the input copies and
  // the zeroed status word queued
  int ready(const char* nomem_text) {
    if (nomem) return fail(c, SONAR_ERR_NOMEM, nomem_text);
    queued = queued || !h2d.empty() || dflag;
    for (const Copy& k : h2d) HIP_TRY(c, hipMemcpyAsync(k.dst, k.src, k.bytes, hipMemcpyHostToDevice, c->stream));
    h2d.clear();
    if (dflag) HIP_TRY(c, hipMemsetAsync(dflag, 0, 4, c->stream));
    return SONAR_OK;
  }
  // bytes of device scratch into an array of the caller's, whichever kind it is (queued)
  int give(void* user, const void* src, size_t bytes) {
    if (!user || bytes == 0) return SONAR_OK;
    queued = true;
    HIP_TRY(c, hipMemcpyAsync(user, src, bytes, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
    return SONAR_OK;
  }
  // a host value into an output of the caller's of either kind: written at once, or queued from a copy kept here
  int put(void* user, const void* host, size_t bytes) {
    if (!user || bytes == 0) return SONAR_OK;
    if (!dev) { std::memcpy(user, host, bytes); return SONAR_OK; }
    const void* kept = std::memcpy(own(bytes), host, bytes);
    queued = true;
    HIP_TRY(c, hipMemcpyAsync(user, kept, bytes, hipMemcpyHostToDevice, c->stream));
    return SONAR_OK;
  }
  // a result that is all zeros: fills the outputs where they are; device memory is waited for
  int zero(std::initializer_list<std::pair<void*, size_t>> outs) {
    queued = queued || dev;
    for (const auto& z : outs) {
      const int rc = zero_out(c, z.first, z.second, dev);
      if (rc != SONAR_OK) return rc;
    }
    return dev ? wait({}) : SONAR_OK;
  }
  // mid-call: queues the read-backs and waits for the stream
  int fetch() { return wait({&backs}); }
  // queues the read-backs and the copy-backs and waits for the stream
  int finish() { return wait({&backs, &d2h}); }
  // waits for the stream if a put() is still queued (an entry that ends on one)
  int settle() { return queued ? wait({}) : SONAR_OK; }

 private:
  void* own(size_t bytes) { return owned.emplace_back(bytes ? bytes : 1).data(); }
  int wait(std::initializer_list<std::vector<Copy>*> lists) {
    queued = true;   // the copies below, and the launches of the entry before them
    for (std::vector<Copy>* list : lists) {
      for (const Copy& k : *list)
        if (k.bytes) HIP_TRY(c, hipMemcpyAsync(k.dst, k.src, k.bytes, hipMemcpyDeviceToHost, c->stream));
      list->clear();
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    queued = false;
    return SONAR_OK;
  }
};

}  // namespace detail
}  // namespace sonar
