// orbx_hostutil.h — host plumbing shared by the C ABI files: a thread-local
// last-error string per API family and device / pinned-host buffers that free
// themselves.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <string>

#include "../../include/orbx_c.h"

namespace orbx {

// One family's last error (orbx_, orbm_, orbv_, orbdb_): fail() formats into
// the calling thread's string and returns the code.
struct ErrorSlot {
  std::string msg;
  __attribute__((format(printf, 3, 4))) int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    msg = buf;
    return code;
  }
};
// the extractor family's slot, used by every orbx_* file (defined in orbx_runtime.hip)
extern thread_local ErrorSlot g_err;

// HIP_OK(slot, expr): return ORBX_EDEVICE with "<expr>: <HIP's text>" in `slot` unless expr succeeds
#define HIP_OK(slot, expr)                                                                           \
  do {                                                                                               \
    hipError_t e_ = (expr);                                                                          \
    if (e_ != hipSuccess) return (slot).fail(ORBX_EDEVICE, "%s: %s", #expr, hipGetErrorString(e_));  \
  } while (0)

// Device (hipMalloc) or pinned host (hipHostMalloc) memory owned by its
// holder. The owner orders the free after the work that uses the memory: the
// buffer knows nothing of streams, events or graphs.
template <bool kPinned>
struct OwnedBuf {
  void* p = nullptr;
  size_t n = 0;
  OwnedBuf() = default;
  OwnedBuf(const OwnedBuf&) = delete;
  OwnedBuf& operator=(const OwnedBuf&) = delete;
  ~OwnedBuf() { release(); }
  void release() {
    if (p) (void)(kPinned ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    n = 0;
  }
  // exactly `bytes` of fresh memory (0: none); empty after a failure
  hipError_t alloc(size_t bytes) {
    release();
    if (!bytes) return hipSuccess;
    const hipError_t e = kPinned ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes);
    if (e != hipSuccess) p = nullptr;
    else n = bytes;
    return e;
  }
  // grow-only: at least `bytes`; *grew tells whether the memory was replaced
  // (the old contents are gone then). No HIP call when it already holds them.
  hipError_t reserve(size_t bytes, bool* grew = nullptr) {
    if (grew) *grew = n < bytes;
    return n >= bytes ? hipSuccess : alloc(bytes);
  }
  template <class T>
  T* as() const { return (T*)p; }
};
using DeviceBuf = OwnedBuf<false>;
using PinnedBuf = OwnedBuf<true>;

// the extractor family's allocations, with its ORBX_ENOMEM messages
inline int device_alloc(DeviceBuf& b, size_t bytes) {
  return b.alloc(bytes) == hipSuccess ? ORBX_OK : g_err.fail(ORBX_ENOMEM, "hipMalloc(%zu) failed", bytes);
}
inline int pinned_reserve(PinnedBuf& b, size_t bytes) {
  return b.reserve(bytes) == hipSuccess ? ORBX_OK : g_err.fail(ORBX_ENOMEM, "hipHostMalloc(%zu)", bytes);
}

}  // namespace orbx
