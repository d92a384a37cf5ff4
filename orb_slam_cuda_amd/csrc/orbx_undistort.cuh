// orbx_undistort.cuh — the arithmetic of the Frame constructors' tail
// (Frame::UndistortKeyPoints src/Frame.cc:403-433, Frame::ComputeImageBounds
// :435-463, Frame::ComputeStereoFromRGBD :642-663 after the depth image's
// convertTo of Tracking::GrabImageRGBD, src/Tracking.cc:276-277), shared by
// frame_tail_kernel (orbx_frametail.hip) and the host entry points
// (orbx_undistort_points, orbx_image_bounds): one rounding per reference
// operation, spelled through the pm_* operators of orbx_posemath.cuh.
#pragma once
#include "orbx_posemath.cuh"

namespace orbx {

static_assert(sizeof(orbx_calib) == 36, "orbx_calib layout");

// cv::undistortPoints(src, dst, K, dist, Mat(), K) of OpenCV 3.x for one
// point, in double: the normalised point is refined by five fixed-point
// iterations of the distortion model (k1, k2, p1, p2, k3) and projected with
// the same K. No early exit and no icdist < 0 guard: both came with later
// OpenCV versions. fx, fy, cx, cy and the coefficients are the floats of
// mK / mDistCoef widened to double.
__host__ __device__ inline void undistort_point(const orbx_calib& c, float u, float v, float* uo, float* vo) {
  const double fx = c.fx, fy = c.fy, cx = c.cx, cy = c.cy;
  const double k0 = c.k1, k1 = c.k2, k2 = c.p1, k3 = c.p2, k4 = c.k3;
  const double ifx = pm_ddiv(1., fx), ify = pm_ddiv(1., fy);
  const double x0 = pm_dmul(pm_dadd((double)u, -cx), ifx), y0 = pm_dmul(pm_dadd((double)v, -cy), ify);
  double x = x0, y = y0;
  for (int it = 0; it < 5; ++it) {
    const double xx = pm_dmul(x, x), yy = pm_dmul(y, y);
    const double r2 = pm_dadd(xx, yy);
    // 1./(1 + ((k[4]*r2 + k[1])*r2 + k[0])*r2)
    const double poly = pm_dmul(pm_dadd(pm_dmul(pm_dadd(pm_dmul(k4, r2), k1), r2), k0), r2);
    const double icdist = pm_ddiv(1., pm_dadd(1., poly));
    // 2*k[2]*x*y + k[3]*(r2 + 2*x*x)
    const double dX = pm_dadd(pm_dmul(pm_dmul(pm_dmul(2., k2), x), y), pm_dmul(k3, pm_dadd(r2, pm_dmul(pm_dmul(2., x), x))));
    // k[2]*(r2 + 2*y*y) + 2*k[3]*x*y
    const double dY = pm_dadd(pm_dmul(k2, pm_dadd(r2, pm_dmul(pm_dmul(2., y), y))), pm_dmul(pm_dmul(pm_dmul(2., k3), x), y));
    x = pm_dmul(pm_dadd(x0, -dX), icdist);
    y = pm_dmul(pm_dadd(y0, -dY), icdist);
  }
  *uo = pm_d2f(pm_dadd(pm_dmul(fx, x), cx));
  *vo = pm_d2f(pm_dadd(pm_dmul(fy, y), cy));
}

// Mat::convertTo(CV_32F, factor) for the one pixel ComputeStereoFromRGBD
// samples: Tracking converts the image iff |factor - 1| > 1e-5 or its type is
// not CV_32F, as (float)raw * factor in float.
__host__ __device__ inline bool depth_converts(int depth_type, float factor) {
  return fabsf(pm_fsub(factor, 1.0f)) > 1e-5f || depth_type != ORBX_DEPTH_F32;
}

// ComputeStereoFromRGBD for one keypoint with its (converted) depth d and its
// undistorted x: mvDepth / mvuRight, -1 for both where d > 0 fails (NaN too)
__host__ __device__ inline void depth_to_stereo(float d, float xu, float mbf, float* uright, float* depth) {
  if (d > 0) {
    *depth = d;
    *uright = pm_fsub(xu, pm_fdiv(mbf, d));
  } else {
    *depth = -1.f;
    *uright = -1.f;
  }
}

}  // namespace orbx
