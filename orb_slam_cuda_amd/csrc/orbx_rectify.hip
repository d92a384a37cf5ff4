// orbx_rectify.hip — stereo rectification ahead of the extraction: the two
// cv::remap(im, imRect, M1, M2, cv::INTER_LINEAR) calls the stereo examples
// make per frame (Examples/Stereo/stereo_euroc.cc:136-137, Examples/ROS/ROS_WS/
// src/stereo/src/ros_stereo.cc:161-162) and the cv::initUndistortRectifyMap
// that builds their maps once (stereo_euroc.cc:97-98, ros_stereo.cc:106-107).
//
//   remap_prepare_kernel  once per rectifier: the two float maps to one record
//                         per output pixel (orbx_remap.cuh: tap position offset
//                         by one, the two 5-bit fractions, a sentinel for "all
//                         taps outside"), 4 bytes where both source sides are
//                         at most 2046, else 8. Rows are padded to four records
//                         with sentinels.
//   remap_kernel          per batch of frames: a lane takes four adjacent
//                         output pixels: one 16-byte (32-byte) record load, the
//                         16 taps through L2 (a wave's 256 outputs touch a few
//                         short source row runs): three 8-byte loads where the
//                         four pixels' taps fall inside 8 columns x 3 rows of
//                         the source, as a rectification map has them almost
//                         everywhere; else eight 2-byte loads, a row's two taps
//                         together (one-column sources: byte loads). The kernel
//                         is bound by its count of sub-dword loads: 77.8, 53.9
//                         and 40.0 us per 64 EuRoC frames with 16, 8 and 3 of
//                         them per lane. One dword store
//                         of the four packed results. The float maps are never read
//                         here: at 8 bytes per pixel they would be four fifths
//                         of the traffic. No LDS, no barrier, no atomic; no byte
//                         outside [0, src_w) of a source row or [0, dst_w) of a
//                         destination row is touched.
//
// The per-pixel arithmetic is orbx_remap.cuh, shared with remap_host.
#include <algorithm>
#include <cmath>

#include "orbx_device.cuh"
#include "orbx_hostutil.h"
#include "orbx_remap.cuh"

namespace orbx {

constexpr int kRemapThreads = 256;

template <bool REC8>
__global__ __launch_bounds__(kRemapThreads) void remap_prepare_kernel(const float* __restrict__ map1,
                                                                      const float* __restrict__ map2, int dst_w,
                                                                      int dst_h, int src_w, int src_h, int mpitch,
                                                                      void* __restrict__ recs) {
  const int i = blockIdx.x * kRemapThreads + threadIdx.x;  // column of the padded row
  const int row = blockIdx.y;
  if (i >= mpitch || row >= dst_h) return;
  bool out = true;
  RemapPos p{};
  if (i < dst_w) {
    const size_t at = (size_t)row * dst_w + i;
    p = remap_pos(map1[at], map2[at]);
    out = remap_all_outside(p.x, p.y, src_w, src_h);
  }
  const size_t o = (size_t)row * mpitch + i;
  if (REC8) ((uint2*)recs)[o] = out ? make_uint2(kRemapOutside, kRemapOutside) : remap_rec8(p);
  else ((uint32_t*)recs)[o] = out ? kRemapOutside : remap_rec4(p);
}

struct RemapArgs {
  const void* recs;
  int mpitch;  // records per padded row, a multiple of 4
  int dst_w, dst_h, src_w, src_h;
  const uint8_t* src;
  size_t src_stride, src_fpitch;
  uint8_t* dst;
  size_t dst_stride, dst_fpitch;
};

// remap_pixel for a source at least two wide, with a row's two taps from one
// 2-byte load at column xb = clamp(x, 0, w - 2): tap x is its byte 0 (byte 1
// when x = w - 1), tap x + 1 its byte 1 (byte 0 when x = -1). Half the load
// instructions of remap_pixel; the same bytes of the source are read.
__device__ __forceinline__ int remap_pixel_pairs(const uint8_t* __restrict__ src, size_t stride, int w, int h,
                                                 const RemapPos& p) {
  const bool x0in = p.x >= 0, x1in = p.x + 1 < w, y0in = p.y >= 0, y1in = p.y + 1 < h;
  const int xb = min(max(p.x, 0), w - 2);
  uint16_t a, b;
  __builtin_memcpy(&a, src + (size_t)(y0in ? p.y : 0) * stride + xb, 2);
  __builtin_memcpy(&b, src + (size_t)(y1in ? p.y + 1 : h - 1) * stride + xb, 2);
  const int slo = x1in ? 0 : 8, shi = x0in ? 8 : 0;
  const int t00 = (x0in && y0in) ? (a >> slo) & 255 : 0, t01 = (x1in && y0in) ? (a >> shi) & 255 : 0;
  const int t10 = (x0in && y1in) ? (b >> slo) & 255 : 0, t11 = (x1in && y1in) ? (b >> shi) & 255 : 0;
  return remap_blend(t00, t01, t10, t11, p.fx, p.fy);
}

// DWORD: every destination row starts 4-byte aligned, so full groups of four
// go out as one dword; otherwise (and for a row's last 1..3 pixels) bytes.
template <bool REC8, bool DWORD, bool PAIRS>
__global__ __launch_bounds__(kRemapThreads) void remap_kernel(RemapArgs A) {
  const int qpr = A.mpitch >> 2;  // groups of four per row
  const int g = blockIdx.x * kRemapThreads + threadIdx.x;
  if (g >= qpr * A.dst_h) return;
  const int row = g / qpr, q = g - row * qpr;
  const int f = blockIdx.y;
  const uint8_t* __restrict__ src = A.src + (size_t)f * A.src_fpitch;
  RemapPos p[4];
  bool in[4];
  const size_t rat = (size_t)row * A.mpitch + (size_t)q * 4;
  if (REC8) {
    const uint4* r = (const uint4*)((const uint2*)A.recs + rat);
    const uint4 a = r[0], b = r[1];
    const uint2 u[4] = {make_uint2(a.x, a.y), make_uint2(a.z, a.w), make_uint2(b.x, b.y), make_uint2(b.z, b.w)};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      in[k] = u[k].x != kRemapOutside;
      p[k] = remap_unrec8(u[k]);
    }
  } else {
    const uint4 a = *(const uint4*)((const uint32_t*)A.recs + rat);
    const uint32_t u[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      in[k] = u[k] != kRemapOutside;
      p[k] = remap_unrec4(u[k]);
    }
  }
  int v[4];
  // Window path (what a rectification map gives almost everywhere): the four
  // pixels' taps lie inside 8 columns x 3 rows of the source, all of it inside
  // the image. Three 8-byte loads then serve the 16 taps.
  const int xmin = min(min(p[0].x, p[1].x), min(p[2].x, p[3].x)), xmax = max(max(p[0].x, p[1].x), max(p[2].x, p[3].x));
  const int ymin = min(min(p[0].y, p[1].y), min(p[2].y, p[3].y)), ymax = max(max(p[0].y, p[1].y), max(p[2].y, p[3].y));
  const bool window = PAIRS && in[0] && in[1] && in[2] && in[3] && xmin >= 0 && xmax - xmin <= 6 &&
                      xmin + 7 < A.src_w && ymin >= 0 && ymax - ymin <= 1 && ymin + 2 < A.src_h;
  if (window) {
    const uint8_t* r = src + (size_t)ymin * A.src_stride + xmin;
    uint64_t rows[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) __builtin_memcpy(&rows[j], r + (size_t)j * A.src_stride, 8);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int sh = (p[k].x - xmin) * 8;  // 0 .. 48: the pair's two bytes stay inside the 8
      const bool lower = p[k].y != ymin;
      const uint32_t a = (uint32_t)((lower ? rows[1] : rows[0]) >> sh), b = (uint32_t)((lower ? rows[2] : rows[1]) >> sh);
      v[k] = remap_blend(a & 255, (a >> 8) & 255, b & 255, (b >> 8) & 255, p[k].fx, p[k].fy);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      v[k] = !in[k] ? 0
             : PAIRS ? remap_pixel_pairs(src, A.src_stride, A.src_w, A.src_h, p[k])
                     : remap_pixel(src, A.src_stride, A.src_w, A.src_h, p[k].x, p[k].y, p[k].fx, p[k].fy);
  }
  uint8_t* __restrict__ d = A.dst + (size_t)f * A.dst_fpitch + (size_t)row * A.dst_stride + (size_t)q * 4;
  const int left = A.dst_w - q * 4;  // pixels of this group inside the row (the padding's records are sentinels)
  if (DWORD && left >= 4) {
    *(uint32_t*)d = pack4_u8(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < left) d[k] = (uint8_t)v[k];
  }
}

int rectifier_create(int device, const float* map1, const float* map2, int dst_w, int dst_h, int src_w, int src_h,
                     orbx_rectifier** out) {
  if (hipSetDevice(device) != hipSuccess) return ORBX_EDEVICE;
  orbx_rectifier* r = new orbx_rectifier{};
  r->device = device;
  r->dst_w = dst_w;
  r->dst_h = dst_h;
  r->src_w = src_w;
  r->src_h = src_h;
  r->rec_bytes = (src_w <= kRemapSmallSide && src_h <= kRemapSmallSide) ? 4 : 8;
  r->mpitch = (dst_w + 3) & ~3;
  const size_t n = (size_t)dst_w * dst_h, map_bytes = n * sizeof(float);
  const size_t rec_bytes = (size_t)r->mpitch * dst_h * r->rec_bytes;
  float* d_maps = nullptr;
  int rc = ORBX_OK;
  if (hipMalloc(&r->recs, rec_bytes) != hipSuccess || hipMalloc((void**)&d_maps, 2 * map_bytes) != hipSuccess) {
    rc = ORBX_ENOMEM;
  } else if (hipMemcpy(d_maps, map1, map_bytes, hipMemcpyHostToDevice) != hipSuccess ||
             hipMemcpy(d_maps + n, map2, map_bytes, hipMemcpyHostToDevice) != hipSuccess) {
    rc = ORBX_EDEVICE;
  } else {
    // the null stream: the blocking copies above and the wait below order it
    const dim3 grid((r->mpitch + kRemapThreads - 1) / kRemapThreads, dst_h);
    if (r->rec_bytes == 8)
      hipLaunchKernelGGL(remap_prepare_kernel<true>, grid, dim3(kRemapThreads), 0, nullptr, d_maps, d_maps + n, dst_w,
                         dst_h, src_w, src_h, r->mpitch, r->recs);
    else
      hipLaunchKernelGGL(remap_prepare_kernel<false>, grid, dim3(kRemapThreads), 0, nullptr, d_maps, d_maps + n, dst_w,
                         dst_h, src_w, src_h, r->mpitch, r->recs);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess) rc = ORBX_EDEVICE;
  }
  if (d_maps) (void)hipFree(d_maps);
  if (rc) {
    if (r->recs) (void)hipFree(r->recs);
    delete r;
    return rc;
  }
  *out = r;
  return ORBX_OK;
}

void rectifier_destroy(orbx_rectifier* r) {
  if (!r) return;
  if (r->recs) (void)hipFree(r->recs);
  delete r;
}

int launch_rectify(const orbx_rectifier& r, const uint8_t* src, size_t src_stride, size_t src_fpitch, uint8_t* dst,
                   size_t dst_stride, size_t dst_fpitch, int batch, hipStream_t stream) {
  if (batch <= 0) return ORBX_OK;
  const bool dword = ((uintptr_t)dst | dst_stride | dst_fpitch) % 4 == 0;
  const int groups = (r.mpitch >> 2) * r.dst_h;
  constexpr int kMaxGridY = 65535;
  for (int f0 = 0; f0 < batch; f0 += kMaxGridY) {
    const int nb = std::min(batch - f0, kMaxGridY);
    RemapArgs A{r.recs,     r.mpitch,   r.dst_w,
                r.dst_h,    r.src_w,    r.src_h,
                src + (size_t)f0 * src_fpitch, src_stride, src_fpitch,
                dst + (size_t)f0 * dst_fpitch, dst_stride, dst_fpitch};
    const dim3 grid((groups + kRemapThreads - 1) / kRemapThreads, nb);
    const bool pairs = r.src_w >= 2;  // a one-column source has no pair to load
    auto k = pairs ? (r.rec_bytes == 8 ? (dword ? remap_kernel<true, true, true> : remap_kernel<true, false, true>)
                                       : (dword ? remap_kernel<false, true, true> : remap_kernel<false, false, true>))
                   : (r.rec_bytes == 8 ? (dword ? remap_kernel<true, true, false> : remap_kernel<true, false, false>)
                                       : (dword ? remap_kernel<false, true, false> : remap_kernel<false, false, false>));
    hipLaunchKernelGGL(k, grid, dim3(kRemapThreads), 0, stream, A);
    if (hipGetLastError() != hipSuccess) return ORBX_EDEVICE;
  }
  return ORBX_OK;
}

void remap_host(const uint8_t* src, int src_w, int src_h, size_t src_stride, const float* map1, const float* map2,
                int dst_w, int dst_h, uint8_t* dst, size_t dst_stride) {
  for (int y = 0; y < dst_h; ++y)
    for (int x = 0; x < dst_w; ++x) {
      const size_t at = (size_t)y * dst_w + x;
      const RemapPos p = remap_pos(map1[at], map2[at]);
      dst[(size_t)y * dst_stride + x] =
          remap_all_outside(p.x, p.y, src_w, src_h)
              ? 0
              : (uint8_t)remap_pixel(src, src_stride, src_w, src_h, p.x, p.y, p.fx, p.fy);
    }
}

// cv::initUndistortRectifyMap(K, D, R, P(0..2, 0..2), size, CV_32F, M1, M2) of
// OpenCV 3.x, in double: iR = (P' R)^-1 by the closed-form 3x3 inverse, the
// row loop's running sums (started per row, one addition per column), the
// rational / tangential model with k1 k2 p1 p2 k3 (k4..k6 zero, so its
// denominator is 1), the results cast to float.
void rectify_maps_host(const double* K, const double* D, const double* R, const double* P, int w, int h, float* map1,
                       float* map2) {
  double A[9], ir[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      A[3 * i + j] = P[4 * i] * R[j] + P[4 * i + 1] * R[3 + j] + P[4 * i + 2] * R[6 + j];
  const double det = A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) +
                     A[2] * (A[3] * A[7] - A[4] * A[6]);
  const double d = 1. / det;
  ir[0] = (A[4] * A[8] - A[5] * A[7]) * d;
  ir[1] = (A[2] * A[7] - A[1] * A[8]) * d;
  ir[2] = (A[1] * A[5] - A[2] * A[4]) * d;
  ir[3] = (A[5] * A[6] - A[3] * A[8]) * d;
  ir[4] = (A[0] * A[8] - A[2] * A[6]) * d;
  ir[5] = (A[2] * A[3] - A[0] * A[5]) * d;
  ir[6] = (A[3] * A[7] - A[4] * A[6]) * d;
  ir[7] = (A[1] * A[6] - A[0] * A[7]) * d;
  ir[8] = (A[0] * A[4] - A[1] * A[3]) * d;
  const double fx = K[0], fy = K[4], u0 = K[2], v0 = K[5];
  const double k1 = D[0], k2 = D[1], p1 = D[2], p2 = D[3], k3 = D[4];
  for (int i = 0; i < h; ++i) {
    double _x = i * ir[1] + ir[2], _y = i * ir[4] + ir[5], _w = i * ir[7] + ir[8];
    for (int j = 0; j < w; ++j, _x += ir[0], _y += ir[3], _w += ir[6]) {
      const double iw = 1. / _w, x = _x * iw, y = _y * iw;
      const double x2 = x * x, y2 = y * y;
      const double r2 = x2 + y2, _2xy = 2 * x * y;
      const double kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2;
      const double u = fx * (x * kr + p1 * _2xy + p2 * (r2 + 2 * x2)) + u0;
      const double v = fy * (y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy) + v0;
      map1[(size_t)i * w + j] = (float)u;
      map2[(size_t)i * w + j] = (float)v;
    }
  }
}

}  // namespace orbx

// ------------------------------------------- C ABI (the rectifier's own entry points)
using namespace orbx;

static bool remap_side_ok(int v) { return v >= 1 && v <= 32766; }

extern "C" {

int orbx_rectify_maps(const double K[9], const double D[5], const double R[9], const double P[12], int w, int hh,
                      float* map1, float* map2) {
  if (!K || !D || !R || !P || !map1 || !map2) return g_err.fail(ORBX_EINVAL, "orbx_rectify_maps: null argument");
  if (!remap_side_ok(w) || !remap_side_ok(hh))
    return g_err.fail(ORBX_EINVAL, "orbx_rectify_maps: size %d x %d outside 1 .. 32766", w, hh);
  rectify_maps_host(K, D, R, P, w, hh, map1, map2);
  return ORBX_OK;
}

int orbx_remap_host(const uint8_t* src, int src_w, int src_h, size_t src_stride, const float* map1,
                    const float* map2, int dst_w, int dst_h, uint8_t* dst, size_t dst_stride) {
  if (!src || !map1 || !map2 || !dst) return g_err.fail(ORBX_EINVAL, "orbx_remap_host: null argument");
  if (!remap_side_ok(src_w) || !remap_side_ok(src_h) || !remap_side_ok(dst_w) || !remap_side_ok(dst_h))
    return g_err.fail(ORBX_EINVAL, "orbx_remap_host: %d x %d to %d x %d: a side outside 1 .. 32766", src_w, src_h, dst_w,
                dst_h);
  if (src_stride < (size_t)src_w || dst_stride < (size_t)dst_w)
    return g_err.fail(ORBX_EINVAL, "orbx_remap_host: a row stride below its width");
  remap_host(src, src_w, src_h, src_stride, map1, map2, dst_w, dst_h, dst, dst_stride);
  return ORBX_OK;
}

int orbx_rectify_create(int device, const float* map1, const float* map2, int dst_w, int dst_h, int src_w,
                        int src_h, orbx_rectify_handle* out) {
  if (!map1 || !map2 || !out) return g_err.fail(ORBX_EINVAL, "orbx_rectify_create: null argument");
  if (!remap_side_ok(src_w) || !remap_side_ok(src_h) || !remap_side_ok(dst_w) || !remap_side_ok(dst_h))
    return g_err.fail(ORBX_EINVAL, "orbx_rectify_create: %d x %d to %d x %d: a side outside 1 .. 32766", src_w, src_h, dst_w,
                dst_h);
  const int rc = rectifier_create(device, map1, map2, dst_w, dst_h, src_w, src_h, out);
  if (rc) return g_err.fail(rc, "orbx_rectify_create: %s", hipGetErrorString(hipGetLastError()));
  return ORBX_OK;
}

int orbx_rectify_destroy(orbx_rectify_handle r) {
  if (!r) return ORBX_OK;
  (void)hipSetDevice(r->device);
  rectifier_destroy(r);
  return ORBX_OK;
}

int orbx_rectify_batch(orbx_rectify_handle r, const uint8_t* d_src, size_t src_stride, size_t src_frame_pitch,
                       uint8_t* d_dst, size_t dst_stride, size_t dst_frame_pitch, int batch, void* stream) {
  if (!r) return g_err.fail(ORBX_EINVAL, "orbx_rectify_batch: null rectifier");
  if (batch < 0) return g_err.fail(ORBX_EINVAL, "orbx_rectify_batch: negative batch");
  if (batch == 0) return ORBX_OK;
  if (!d_src || !d_dst) return g_err.fail(ORBX_EINVAL, "orbx_rectify_batch: null image");
  if (src_stride < (size_t)r->src_w || dst_stride < (size_t)r->dst_w)
    return g_err.fail(ORBX_EINVAL, "orbx_rectify_batch: row strides %zu / %zu below the widths %d / %d", src_stride,
                dst_stride, r->src_w, r->dst_w);
  // the last row of a frame needs its width only
  if (batch > 1 && (src_frame_pitch < src_stride * (size_t)(r->src_h - 1) + r->src_w ||
                    dst_frame_pitch < dst_stride * (size_t)(r->dst_h - 1) + r->dst_w))
    return g_err.fail(ORBX_EINVAL, "orbx_rectify_batch: a frame pitch below one frame");
  HIP_OK(g_err, hipSetDevice(r->device));
  if (launch_rectify(*r, d_src, src_stride, src_frame_pitch, d_dst, dst_stride, dst_frame_pitch, batch,
                     (hipStream_t)stream))
    return g_err.fail(ORBX_EDEVICE, "remap launch failed: %s", hipGetErrorString(hipGetLastError()));
  return ORBX_OK;
}

}  // extern "C"
