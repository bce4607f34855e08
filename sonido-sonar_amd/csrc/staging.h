// staging.h -- where the arrays of one entry live during a call that takes host or device pointers
// (device_ptrs): the caller's own device arrays, or named scratch of the context that is filled from
// the caller's host arrays before the launches and copied back to them at the end.
#pragma once
#include <cstring>
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
  struct Copy { void* dst; const void* src; size_t bytes; };
  std::vector<Copy> h2d, d2h;

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
  // an output: the caller's device array, or scratch that finish() copies to the caller's host array;
  // an output the caller does not want (null) stays null
  template <typename T>
  T* out(const char* name, T* user, size_t count) {
    if (!user || dev) return user;
    T* d = tmp<T>(name, count);
    if (d) d2h.push_back({user, d, count * sizeof(T)});
    return d;
  }
  // after the allocations, before the launches: the one SONAR_ERR_NOMEM, else the input copies queued
  int ready(const char* nomem_text) {
    if (nomem) return fail(c, SONAR_ERR_NOMEM, nomem_text);
    for (const Copy& k : h2d) HIP_TRY(c, hipMemcpyAsync(k.dst, k.src, k.bytes, hipMemcpyHostToDevice, c->stream));
    h2d.clear();
    return SONAR_OK;
  }
  // bytes of device scratch into an array of the caller's, whichever kind it is (queued)
  int give(void* user, const void* src, size_t bytes) {
    if (!user || bytes == 0) return SONAR_OK;
    HIP_TRY(c, hipMemcpyAsync(user, src, bytes, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
    return SONAR_OK;
  }
  // a result that is all zeros: fills the outputs where they are; device memory is waited for
  int zero(std::initializer_list<std::pair<void*, size_t>> outs) {
    for (const auto& z : outs) {
      const int rc = zero_out(c, z.first, z.second, dev);
      if (rc != SONAR_OK) return rc;
    }
    if (dev) HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SONAR_OK;
  }
  // queues the copy-backs and waits for the stream
  int finish() {
    for (const Copy& k : d2h)
      if (k.bytes) HIP_TRY(c, hipMemcpyAsync(k.dst, k.src, k.bytes, hipMemcpyDeviceToHost, c->stream));
    d2h.clear();
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SONAR_OK;
  }
};

}  // namespace detail
}  // namespace sonar
