// orbx_frametail.hip — what every reference Frame constructor does straight
// after ExtractORB, on the keypoints where the extraction left them:
// Frame::UndistortKeyPoints (src/Frame.cc:403-433) and, for an RGB-D frame,
// Frame::ComputeStereoFromRGBD (:642-663) on the raw depth image, the
// convertTo of Tracking::GrabImageRGBD (src/Tracking.cc:276-277) applied to
// the sampled pixels only.
//
//   frame_tail_kernel   frames x chunks of keypoints, one keypoint per lane:
//                       the 28-byte orbx_kp in, its copy with the undistorted
//                       pt out (a plain copy when k1 == 0, :405-409), and
//                       mvuRight / mvDepth from the depth pixel under the
//                       distorted keypoint. No LDS, no barrier, no atomic.
//
// The host half (the four corners of Frame::ComputeImageBounds, :435-463, and
// orbx_undistort_points) is the same undistort_point, orbx_undistort.cuh.
#include <algorithm>
#include <cmath>

#include "orbx_hostutil.h"
#include "orbx_undistort.cuh"

namespace orbx {

constexpr int kTailThreads = 256;

static_assert(sizeof(orbx_kp) == 28, "orbx_kp layout");

__global__ __launch_bounds__(kTailThreads) void frame_tail_kernel(FrameTailParams P, const orbx_kp* __restrict__ kps,
                                                                  const int* __restrict__ counts,
                                                                  const uint8_t* __restrict__ depth_img,
                                                                  orbx_kp* __restrict__ kps_un,
                                                                  float* __restrict__ uright,
                                                                  float* __restrict__ depth) {
  const int f = blockIdx.y;
  const int n = min(counts[f], P.kp_pitch);
  const int i = blockIdx.x * kTailThreads + threadIdx.x;
  if (i >= n) return;
  const size_t at = (size_t)f * P.kp_pitch + i;
  union {
    uint32_t q[7];
    orbx_kp r;
  } a;
  const uint32_t* src = (const uint32_t*)(kps + at);  // 28-byte records: 4-byte aligned
#pragma unroll
  for (int k = 0; k < 7; ++k) a.q[k] = src[k];
  const float u = a.r.x, v = a.r.y;
  if (P.calib.k1 != 0.0f) undistort_point(P.calib, u, v, &a.r.x, &a.r.y);
  uint32_t* dst = (uint32_t*)(kps_un + at);
#pragma unroll
  for (int k = 0; k < 7; ++k) dst[k] = a.q[k];
  if (!depth_img) return;
  // imDepth.at<float>(v, u): both truncated to int from the distorted keypoint
  const int iu = (int)u, iv = (int)v;
  float d = -1.f;  // outside the image (undefined in the reference): no depth
  if (iu >= 0 && iu < P.w && iv >= 0 && iv < P.h) {
    const uint8_t* row = depth_img + (size_t)f * P.depth_frame_pitch + (size_t)iv * P.depth_row_stride;
    d = P.depth_type == ORBX_DEPTH_U16 ? (float)((const uint16_t*)row)[iu] : ((const float*)row)[iu];
    if (P.convert) d = __fmul_rn(d, P.factor);  // one float multiply, never fused
  }
  float ur, dp;
  depth_to_stereo(d, a.r.x, P.mbf, &ur, &dp);
  uright[at] = ur;
  depth[at] = dp;
}

int launch_frame_tail(const FrameTailParams& P, const orbx_kp* kps, const int* counts, int batch,
                      const void* depth_img, orbx_kp* kps_un, float* uright, float* depth, void* stream) {
  if (batch <= 0 || P.kp_pitch <= 0) return ORBX_OK;
  const dim3 grid((P.kp_pitch + kTailThreads - 1) / kTailThreads, batch);
  hipLaunchKernelGGL(frame_tail_kernel, grid, dim3(kTailThreads), 0, (hipStream_t)stream, P, kps, counts,
                     (const uint8_t*)depth_img, kps_un, uright, depth);
  return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
}

void undistort_points_host(const orbx_calib& c, const float* xy, int n, float* xy_out) {
  for (int i = 0; i < n; ++i) undistort_point(c, xy[2 * i], xy[2 * i + 1], &xy_out[2 * i], &xy_out[2 * i + 1]);
}

void image_bounds_host(const orbx_calib& c, int w, int h, orbm_grid_bounds* out) {
  if (c.k1 != 0.0f) {
    const float in[8] = {0.f, 0.f, (float)w, 0.f, 0.f, (float)h, (float)w, (float)h};
    float o[8];
    undistort_points_host(c, in, 4, o);
    out->min_x = std::min(o[0], o[4]);
    out->max_x = std::max(o[2], o[6]);
    out->min_y = std::min(o[1], o[3]);
    out->max_y = std::max(o[5], o[7]);
  } else {
    out->min_x = 0.0f;
    out->max_x = (float)w;
    out->min_y = 0.0f;
    out->max_y = (float)h;
  }
}

size_t depth_elem_size(int depth_type) {
  return depth_type == ORBX_DEPTH_U16 ? 2 : depth_type == ORBX_DEPTH_F32 ? 4 : 0;
}

FrameTailParams tail_params(const orbx_calib& c, int kp_pitch, int depth_type, size_t frame_pitch, size_t row_stride,
                            int w, int hh, float factor, float mbf) {
  FrameTailParams P{};
  P.calib = c;
  P.kp_pitch = kp_pitch;
  P.depth_type = depth_type;
  P.convert = fabsf(factor - 1.0f) > 1e-5f || depth_type != ORBX_DEPTH_F32;  // src/Tracking.cc:276
  P.w = w;
  P.h = hh;
  P.factor = factor;
  P.mbf = mbf;
  P.depth_frame_pitch = frame_pitch;
  P.depth_row_stride = row_stride;
  return P;
}

}  // namespace orbx

// ------------------------------------------- C ABI (the handle-free entry points)
using namespace orbx;

extern "C" {

int orbx_undistort_points(const orbx_calib* calib, const float* xy, int n, float* xy_out) {
  if (!calib || n < 0 || (n && (!xy || !xy_out))) return g_err.fail(ORBX_EINVAL, "orbx_undistort_points: bad argument");
  undistort_points_host(*calib, xy, n, xy_out);
  return ORBX_OK;
}

int orbx_image_bounds(const orbx_calib* calib, int w, int hh, orbm_grid_bounds* out) {
  if (!calib || !out || w < 0 || hh < 0) return g_err.fail(ORBX_EINVAL, "orbx_image_bounds: bad argument");
  image_bounds_host(*calib, w, hh, out);
  return ORBX_OK;
}

int orbx_frame_tail_batch(const orbx_calib* calib, const orbx_kp* d_kps, const int* d_counts, int kp_pitch,
                          int batch, const void* d_depth_img, int depth_type, size_t depth_frame_pitch,
                          size_t depth_row_stride, int w, int hh, float depth_factor, float mbf,
                          orbx_kp* d_kps_un, float* d_uRight, float* d_depth, void* stream) {
  if (!calib) return g_err.fail(ORBX_EINVAL, "orbx_frame_tail_batch: null calib");
  if (batch < 0 || kp_pitch < 0) return g_err.fail(ORBX_EINVAL, "orbx_frame_tail_batch: negative batch or kp_pitch");
  if (batch == 0 || kp_pitch == 0) return ORBX_OK;
  if (!d_kps || !d_counts || !d_kps_un) return g_err.fail(ORBX_EINVAL, "orbx_frame_tail_batch: null keypoint buffer");
  if (d_depth_img) {
    const size_t es = depth_elem_size(depth_type);
    if (!es) return g_err.fail(ORBX_EINVAL, "orbx_frame_tail_batch: unknown depth_type %d", depth_type);
    if (w < 0 || hh < 0 || depth_row_stride < (size_t)w * es)
      return g_err.fail(ORBX_EINVAL, "orbx_frame_tail_batch: depth_row_stride %zu below %d elements of %zu bytes",
                  depth_row_stride, w, es);
    if (depth_row_stride % es || depth_frame_pitch % es || (uintptr_t)d_depth_img % es)
      return g_err.fail(ORBX_EINVAL, "orbx_frame_tail_batch: depth image not aligned to its %zu-byte elements", es);
    if (batch > 1 && depth_frame_pitch < depth_row_stride * (size_t)hh)
      return g_err.fail(ORBX_EINVAL, "orbx_frame_tail_batch: depth_frame_pitch %zu below one frame", depth_frame_pitch);
    if (!d_uRight || !d_depth) return g_err.fail(ORBX_EINVAL, "orbx_frame_tail_batch: null uRight / depth output");
  }
  const FrameTailParams P = tail_params(*calib, kp_pitch, depth_type, depth_frame_pitch, depth_row_stride, w, hh,
                                        depth_factor, mbf);
  if (launch_frame_tail(P, d_kps, d_counts, batch, d_depth_img, d_kps_un, d_uRight, d_depth, stream))
    return g_err.fail(ORBX_EDEVICE, "frame tail launch failed: %s", hipGetErrorString(hipGetLastError()));
  return ORBX_OK;
}

int orbx_undistort_keypoints(const orbx_calib* calib, const orbx_kp* kps, int n, orbx_kp* kps_un) {
  if (!calib || n < 0 || (n && (!kps || !kps_un))) return g_err.fail(ORBX_EINVAL, "orbx_undistort_keypoints: bad argument");
  if (n == 0) return ORBX_OK;
  const size_t kb = (size_t)n * sizeof(orbx_kp);
  DeviceBuf in, out;  // in: the count (16 bytes) + the keypoints
  int rc;
  if ((rc = device_alloc(in, 16 + kb)) || (rc = device_alloc(out, kb))) return rc;
  HIP_OK(g_err, hipMemcpy(in.p, &n, sizeof n, hipMemcpyHostToDevice));
  HIP_OK(g_err, hipMemcpy(in.as<uint8_t>() + 16, kps, kb, hipMemcpyHostToDevice));
  if ((rc = orbx_frame_tail_batch(calib, (const orbx_kp*)(in.as<uint8_t>() + 16), in.as<int>(), n, 1, nullptr, 0, 0, 0,
                                  0, 0, 1.f, 0.f, out.as<orbx_kp>(), nullptr, nullptr, nullptr)))
    return rc;
  HIP_OK(g_err, hipMemcpy(kps_un, out.p, kb, hipMemcpyDeviceToHost));  // the null stream: after the kernel
  return ORBX_OK;
}

}  // extern "C"
