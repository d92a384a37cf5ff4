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

}  // namespace orbx
