// orbx_runtime.hip — what the rest of the library and its callers need from the
// HIP runtime, none of it tied to a handle: the extractor family's last-error
// string, the copy kernel, the per-kernel LDS limits and the thin orbx_*
// wrappers of memory, stream and event calls (include/orbx_c.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <utility>
#include <vector>

#include "orbx_hostutil.h"
#include "orbx_internal.h"
#include "orbx_sincosf.h"

thread_local orbx::ErrorSlot orbx::g_err;

namespace orbx {

// Rectangle copy by the compute units (orbx_copy2d_kernel_async): a thread per
// 16-byte destination chunk, grid-strided; the source may be pinned host
// memory read over the link. A row's last chunk is clipped to its width.
__global__ __launch_bounds__(256) void copy2d_kernel(uint8_t* __restrict__ d, size_t dp, const uint8_t* __restrict__ s,
                                                     size_t sp, size_t w, size_t rows) {
  const size_t cpr = (w + 15) / 16, total = cpr * rows;
  for (size_t i = blockIdx.x * 256ull + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t r = i / cpr, c = (i - r * cpr) * 16;
    const uint8_t* src = s + r * sp + c;
    uint8_t* dst = d + r * dp + c;
    if (c + 16 <= w) {
      *(uint4*)dst = *(const uint4*)src;  // unaligned source rows: the memory path takes unaligned dwordx4
    } else {
      for (size_t k = 0; k < 16 && c + k < w; ++k) dst[k] = src[k];
    }
  }
}

}  // namespace orbx

using namespace orbx;

// Dynamic-LDS limits are per kernel and device, shared by every handle of the
// process: only ever raise them (a handle with a smaller plan must not lower
// the limit a larger one launches with).
int orbx::raise_lds_limit(const void* fn, size_t bytes) {
  static std::mutex mu;
  static std::vector<std::pair<std::pair<const void*, int>, size_t>> set;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return ORBX_EDEVICE;
  std::lock_guard<std::mutex> lk(mu);
  for (auto& e : set)
    if (e.first.first == fn && e.first.second == dev) {
      if (bytes <= e.second) return ORBX_OK;
      if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
        return ORBX_EDEVICE;
      e.second = bytes;
      return ORBX_OK;
    }
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
    return ORBX_EDEVICE;
  set.push_back({{fn, dev}, bytes});
  return ORBX_OK;
}

int orbx::copy_to_host_async(void* host_dst, const void* dev_src, size_t bytes, hipStream_t stream) {
  void* d = nullptr;
  if (hipHostGetDevicePointer(&d, host_dst, 0) != hipSuccess) return g_err.fail(ORBX_EDEVICE, "hipHostGetDevicePointer failed");
  const int blocks = (int)std::min<size_t>(64, (bytes + 4095) / 4096);
  hipLaunchKernelGGL(orbx::copy2d_kernel, dim3(std::max(blocks, 1)), dim3(256), 0, stream, (uint8_t*)d, bytes,
                     (const uint8_t*)dev_src, bytes, bytes, (size_t)1);
  return hipGetLastError() == hipSuccess ? ORBX_OK : g_err.fail(ORBX_EDEVICE, "copy kernel launch failed");
}

extern "C" {

const char* orbx_last_error(void) { return g_err.msg.c_str(); }
#ifdef ORBX_DIAG
const char* orbx_version(void) { return "orbx 0.3 (gfx950, diag)"; }
#else
const char* orbx_version(void) { return "orbx 0.3 (gfx950)"; }
#endif
// ---------------------------------------------------------- plumbing
int orbx_device_count(int* n) {
  if (!n) return g_err.fail(ORBX_EINVAL, "null");
  HIP_OK(g_err, hipGetDeviceCount(n));
  return ORBX_OK;
}
int orbx_set_device(int d) { HIP_OK(g_err, hipSetDevice(d)); return ORBX_OK; }
int orbx_malloc(void** p, size_t b) { HIP_OK(g_err, hipMalloc(p, b)); return ORBX_OK; }
int orbx_free(void* p) { HIP_OK(g_err, hipFree(p)); return ORBX_OK; }
int orbx_memcpy_htod(void* d, const void* s, size_t b) { HIP_OK(g_err, hipMemcpy(d, s, b, hipMemcpyHostToDevice)); return ORBX_OK; }
int orbx_memcpy_dtoh(void* d, const void* s, size_t b) { HIP_OK(g_err, hipMemcpy(d, s, b, hipMemcpyDeviceToHost)); return ORBX_OK; }
int orbx_memset(void* d, int v, size_t b) { HIP_OK(g_err, hipMemset(d, v, b)); return ORBX_OK; }
int orbx_host_alloc(void** p, size_t b) { HIP_OK(g_err, hipHostMalloc(p, b, hipHostMallocDefault)); return ORBX_OK; }
int orbx_host_free(void* p) { HIP_OK(g_err, hipHostFree(p)); return ORBX_OK; }
int orbx_memcpy_htod_async(void* d, const void* s, size_t b, void* st) {
  HIP_OK(g_err, hipMemcpyAsync(d, s, b, hipMemcpyHostToDevice, (hipStream_t)st));
  return ORBX_OK;
}
int orbx_memcpy_dtoh_async(void* d, const void* s, size_t b, void* st) {
  HIP_OK(g_err, hipMemcpyAsync(d, s, b, hipMemcpyDeviceToHost, (hipStream_t)st));
  return ORBX_OK;
}
int orbx_memcpy2d_htod_async(void* d, size_t dp, const void* s, size_t sp, size_t w, size_t rows, void* st) {
  if (!d || !s || w > dp || w > sp) return g_err.fail(ORBX_EINVAL, "bad 2D copy");
  if (!w || !rows) return ORBX_OK;
  HIP_OK(g_err, hipMemcpy2DAsync(d, dp, s, sp, w, rows, hipMemcpyHostToDevice, (hipStream_t)st));
  return ORBX_OK;
}
int orbx_copy2d_kernel_async(void* d, size_t dp, const void* s, size_t sp, size_t w, size_t rows, int blocks,
                             void* st) {
  if (!d || !s || w > dp || w > sp || blocks < 1 || (dp & 15)) return g_err.fail(ORBX_EINVAL, "bad 2D copy");
  if (!w || !rows) return ORBX_OK;
  hipLaunchKernelGGL(orbx::copy2d_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)st, (uint8_t*)d, dp,
                     (const uint8_t*)s, sp, w, rows);
  return hipGetLastError() == hipSuccess ? ORBX_OK : g_err.fail(ORBX_EDEVICE, "copy kernel launch failed");
}
int orbx_memcpy_dtod_async(void* d, const void* s, size_t b, void* st) {
  HIP_OK(g_err, hipMemcpyAsync(d, s, b, hipMemcpyDeviceToDevice, (hipStream_t)st));
  return ORBX_OK;
}
int orbx_stream_create(void** s) { HIP_OK(g_err, hipStreamCreateWithFlags((hipStream_t*)s, hipStreamNonBlocking)); return ORBX_OK; }
int orbx_stream_create_priority(void** s, int high) {
  int least = 0, greatest = 0;
  HIP_OK(g_err, hipDeviceGetStreamPriorityRange(&least, &greatest));
  HIP_OK(g_err, hipStreamCreateWithPriority((hipStream_t*)s, hipStreamNonBlocking, high ? greatest : least));
  return ORBX_OK;
}
int orbx_stream_create_cumask(void** s, const uint32_t* mask, int nwords) {
  if (!s || !mask || nwords < 1) return g_err.fail(ORBX_EINVAL, "bad argument");
  HIP_OK(g_err, hipExtStreamCreateWithCUMask((hipStream_t*)s, (uint32_t)nwords, mask));
  return ORBX_OK;
}
int orbx_stream_destroy(void* s) { HIP_OK(g_err, hipStreamDestroy((hipStream_t)s)); return ORBX_OK; }
int orbx_stream_synchronize(void* s) { HIP_OK(g_err, hipStreamSynchronize((hipStream_t)s)); return ORBX_OK; }
int orbx_event_create(void** e) { HIP_OK(g_err, hipEventCreate((hipEvent_t*)e)); return ORBX_OK; }
int orbx_event_destroy(void* e) { HIP_OK(g_err, hipEventDestroy((hipEvent_t)e)); return ORBX_OK; }
int orbx_event_record(void* e, void* s) { HIP_OK(g_err, hipEventRecord((hipEvent_t)e, (hipStream_t)s)); return ORBX_OK; }
int orbx_sincosf_glibc(const float* x, int n, float* s, float* c) {
  if (n < 0 || (n && (!x || !s || !c))) return g_err.fail(ORBX_EINVAL, "bad argument");
  for (int i = 0; i < n; ++i) glibc_sincosf(x[i], s + i, c + i);
  return ORBX_OK;
}
int orbx_stream_wait_event(void* s, void* e) {
  HIP_OK(g_err, hipStreamWaitEvent((hipStream_t)s, (hipEvent_t)e, 0));
  return ORBX_OK;
}
int orbx_event_elapsed_ms(void* a, void* b, float* ms) {
  HIP_OK(g_err, hipEventElapsedTime(ms, (hipEvent_t)a, (hipEvent_t)b));
  return ORBX_OK;
}

}  // extern "C"
