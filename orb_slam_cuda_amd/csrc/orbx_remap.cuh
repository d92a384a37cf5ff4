// orbx_remap.cuh — the per-pixel arithmetic of cv::remap(src, dst, map1, map2,
// INTER_LINEAR) with BORDER_CONSTANT 0 for 8-bit single-channel images and
// CV_32FC1 maps, as the stereo examples call it on every frame
// (Examples/Stereo/stereo_euroc.cc:136-137, Examples/ROS/ROS_WS/src/stereo/src/
// ros_stereo.cc:161-162), shared by the kernels of orbx_rectify.hip and the
// host entry orbx_remap_host. OpenCV 3.x takes its fixed-point path here:
// coordinates rounded to 1/32 px, four weights that sum to 2^15, one rounding
// shift.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

namespace orbx {

constexpr int kRemapMaxSide = 32766;  // x, x + 1 stay inside a short for every source and destination side

// cvRound(m * 32): a float product, rounded half to even. NaN, infinities and
// products outside int convert to INT_MIN, as cvtss2si does on x86.
__host__ __device__ inline int remap_fix(float m) {
  const float p = m * 32.0f;
  if (!(p >= -2147483648.0f && p < 2147483648.0f)) return INT_MIN;
  return (int)rintf(p);
}

__host__ __device__ inline int remap_sat_short(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// One output pixel's source position: the top-left tap (x, y) = the integer
// parts sx >> 5, sy >> 5 saturated to short, the fractions fx, fy = the low
// five bits.
struct RemapPos {
  int x, y, fx, fy;
};
__host__ __device__ inline RemapPos remap_pos(float m1, float m2) {
  const int sx = remap_fix(m1), sy = remap_fix(m2);
  return RemapPos{remap_sat_short(sx >> 5), remap_sat_short(sy >> 5), sx & 31, sy & 31};
}

// all four taps (x, y), (x + 1, y), (x, y + 1), (x + 1, y + 1) outside a w x h source
__host__ __device__ inline bool remap_all_outside(int x, int y, int w, int h) {
  return x >= w || x + 1 < 0 || y >= h || y + 1 < 0;
}

// The weighted sum of the four taps (t00 at (x, y), t01 at (x + 1, y), t10 at
// (x, y + 1), t11 at (x + 1, y + 1); a tap outside the source is passed as 0):
// weights (32-fx)(32-fy)*32, fx(32-fy)*32, (32-fx)fy*32, fx*fy*32, then
// (sum + 2^14) >> 15. At most 255 * 2^15: no saturation is needed.
__host__ __device__ inline int remap_blend(int t00, int t01, int t10, int t11, int fx, int fy) {
  const int w00 = (32 - fx) * (32 - fy) * 32, w01 = fx * (32 - fy) * 32;
  const int w10 = (32 - fx) * fy * 32, w11 = fx * fy * 32;
  return (t00 * w00 + t01 * w01 + t10 * w10 + t11 * w11 + (1 << 14)) >> 15;
}

// One output pixel from a w x h source with rows `stride` bytes apart. Taps
// are read at clamped coordinates (always inside the source) and dropped by
// their inside test, so no byte outside [0, w) x [0, h) is touched. (The
// kernel fetches a row's two taps with one 2-byte load where the source has
// two columns, remap_pixel_pairs in orbx_rectify.hip, and blends them with
// the same remap_blend.)
__host__ __device__ inline int remap_pixel(const uint8_t* __restrict__ src, size_t stride, int w, int h, int x, int y,
                                           int fx, int fy) {
  const bool x0in = x >= 0, x1in = x + 1 < w, y0in = y >= 0, y1in = y + 1 < h;
  const int xa = x0in ? x : 0, xb = x1in ? x + 1 : w - 1;
  const uint8_t* ra = src + (size_t)(y0in ? y : 0) * stride;
  const uint8_t* rb = src + (size_t)(y1in ? y + 1 : h - 1) * stride;
  const int t00 = (x0in && y0in) ? ra[xa] : 0, t01 = (x1in && y0in) ? ra[xb] : 0;
  const int t10 = (x0in && y1in) ? rb[xa] : 0, t11 = (x1in && y1in) ? rb[xb] : 0;
  return remap_blend(t00, t01, t10, t11, fx, fy);
}

// The prepared map's records (orbx_rectify.hip): what the per-frame kernel
// reads instead of the two float maps. x + 1 in [0, w] and y + 1 in [0, h] of
// a pixel with at least one tap inside, and the fractions; all ones = every
// tap outside. Four bytes when both source sides fit 11 bits less the
// sentinel, eight otherwise.
constexpr int kRemapSmallSide = 2046;
constexpr uint32_t kRemapOutside = 0xFFFFFFFFu;
__host__ __device__ inline uint32_t remap_rec4(const RemapPos& p) {
  return (uint32_t)p.fx | ((uint32_t)p.fy << 5) | ((uint32_t)(p.x + 1) << 10) | ((uint32_t)(p.y + 1) << 21);
}
__host__ __device__ inline RemapPos remap_unrec4(uint32_t r) {
  return RemapPos{(int)((r >> 10) & 2047u) - 1, (int)(r >> 21) - 1, (int)(r & 31u), (int)((r >> 5) & 31u)};
}
__host__ __device__ inline uint2 remap_rec8(const RemapPos& p) {
  return make_uint2((uint32_t)(p.x + 1) | ((uint32_t)(p.y + 1) << 16), (uint32_t)p.fx | ((uint32_t)p.fy << 5));
}
__host__ __device__ inline RemapPos remap_unrec8(uint2 r) {
  return RemapPos{(int)(r.x & 0xFFFFu) - 1, (int)(r.x >> 16) - 1, (int)(r.y & 31u), (int)((r.y >> 5) & 31u)};
}

}  // namespace orbx
