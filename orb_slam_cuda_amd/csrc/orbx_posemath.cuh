// orbx_posemath.cuh — the projection arithmetic the pose-projection kernels
// (orbx_project_pose.hip) and Frame::isInFrustum (orbx_frustum.hip, and
// orbm_is_in_frustum on the host) share, one rounding per reference
// operation: the device spells each as an explicitly rounded intrinsic, the
// host as a plain operator (the library is built with -ffp-contract=off, and
// the x86-64 baseline has no FMA to contract into).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "orbx_internal.h"

namespace orbx {

#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ float pm_fmul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float pm_fadd(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float pm_fsub(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ float pm_fdiv(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ double pm_dmul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double pm_dadd(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double pm_ddiv(double a, double b) { return __ddiv_rn(a, b); }
__device__ __forceinline__ double pm_dsqrt(double a) { return __dsqrt_rn(a); }
__device__ __forceinline__ float pm_d2f(double a) { return __double2float_rn(a); }
#else
inline float pm_fmul(float a, float b) { return a * b; }
inline float pm_fadd(float a, float b) { return a + b; }
inline float pm_fsub(float a, float b) { return a - b; }
inline float pm_fdiv(float a, float b) { return a / b; }
inline double pm_dmul(double a, double b) { return a * b; }
inline double pm_dadd(double a, double b) { return a + b; }
inline double pm_ddiv(double a, double b) { return a / b; }
inline double pm_dsqrt(double a) { return std::sqrt(a); }
inline float pm_d2f(double a) { return (float)a; }
#endif

// R*x + t, row r of the 3x4 T: gemm's small-matrix path (float dot products,
// then (float)(t*1.0 + c*1.0) in double)
__host__ __device__ inline float pose_row(const float* T, int r, float x, float y, float z) {
  const float t = pm_fadd(pm_fadd(pm_fmul(T[4 * r], x), pm_fmul(T[4 * r + 1], y)), pm_fmul(T[4 * r + 2], z));
  return pm_d2f(pm_dadd((double)t, (double)T[4 * r + 3]));
}

// Ow = -Rcw.t()*tcw of a 3x4 T via the general gemm path (double accumulation,
// alpha = -1): orbm_prepare_pose on the host, the pose solve's orbm_pose on the
// device
__host__ __device__ inline void neg_rt_t(const float* T, float* d) {
  for (int r = 0; r < 3; ++r) {
    double s = 0;
    for (int k = 0; k < 3; ++k) s = pm_dadd(s, pm_dmul((double)T[4 * k + r], (double)T[4 * k + 3]));
    d[r] = pm_d2f(pm_dmul(s, -1.0));
  }
}

// The orbm_pose of a camera whose 3x4 transform is Rt, as orbm_prepare_pose
// fills it for every mode before the last-frame overload's level_mode: the
// pose solve writes the same record on the device for its new Tcw.
__host__ __device__ inline void pose_from_rt(const orbm_camera& cam, const float* Rt, orbm_pose* p) {
  for (int k = 0; k < 12; ++k) p->Rt[k] = Rt[k];
  neg_rt_t(p->Rt, p->Ow);
  p->fx = cam.fx;
  p->fy = cam.fy;
  p->cx = cam.cx;
  p->cy = cam.cy;
  p->mbf = cam.mbf;
  p->level_mode = 0;
  for (int k = 0; k < 12; ++k) p->Rt2[k] = 0.0f;
}

// The 3x4 transform of the Sim3 overloads from Scw (src/ORBmatcher.cc:298-303,
// 986-991): scw = sqrt(sRcw.row(0).dot(sRcw.row(0))), Rcw = sRcw/scw, tcw =
// t/scw; Mat::dot in double, Mat / s = convertTo(1/s). orbm_prepare_pose on the
// host, the Sim3 refinement's orbm_pose on the device. Returns scw.
__host__ __device__ inline float rt_from_scw(const float* S, float* Rt) {
  const double d = pm_dadd(pm_dadd(pm_dmul((double)S[0], (double)S[0]), pm_dmul((double)S[1], (double)S[1])),
                           pm_dmul((double)S[2], (double)S[2]));
  const float scw = pm_d2f(pm_dsqrt(d));
  const float a = pm_d2f(pm_ddiv(1.0, (double)scw));
  for (int k = 0; k < 12; ++k) Rt[k] = pm_fadd(pm_fmul(S[k], a), 0.0f);
  return scw;
}

// cv::norm (NORM_L2) of 3 floats: sqrt of the double sum of squares
__host__ __device__ inline float norm3(float a, float b, float c) {
  const double s = pm_dadd(pm_dadd(pm_dmul((double)a, (double)a), pm_dmul((double)b, (double)b)),
                           pm_dmul((double)c, (double)c));
  return pm_d2f(pm_dsqrt(s));
}

// MapPoint::PredictScale (src/MapPoint.cc:390-422) from the host's thresholds
// (orbm_predict_scale_thresholds), L = mnScaleLevels
__host__ __device__ inline int predict_level(const float* thr, int L, float maxd, float dist) {
  const float ratio = pm_fdiv(maxd, dist);
  if (__builtin_isinf(ratio)) return 0;  // ceil(log(inf)) -> int: INT_MIN on x86, clamped to 0
  int l = 0;
#pragma unroll
  for (int k = 0; k < kMaxLevels - 1; ++k) l += (k < L - 1 && ratio >= thr[k]) ? 1 : 0;
  return l;
}
__device__ inline int predict_level(const PoseParams& P, float maxd, float dist) {
  return predict_level(P.pred_thr, P.L, maxd, dist);
}

// Frame::isInFrustum (src/Frame.cc:268-324) for one point, operation by
// operation. The pose is an ORBM_PROJ_KEYFRAME orbm_pose of the frame (Rt =
// mTcw, Ow = mOw). Returns mbTrackInView; *o gets the mTrack* fields, or zeros
// (obs_positive apart) when the point is not tested or not in view. The
// comparisons keep the reference's form, so a NaN falls through them as there.
__host__ __device__ inline bool frustum_point(const FrustumParams& P, const orbm_pose& C,
                                              const orbm_map_point_world& mp, orbm_map_point_proj* o) {
  o->proj_x = o->proj_y = o->proj_xr = o->view_cos = 0.0f;
  o->predicted_level = 0;
  o->track_in_view = 0;
  o->obs_positive = mp.obs_positive;
  o->pad[0] = o->pad[1] = 0;
  if (!mp.valid) return false;  // isBad() or mnLastFrameSeen == mCurrentFrame.mnId (src/Tracking.cc:1256-1259)
  const float X = mp.pos[0], Y = mp.pos[1], Z = mp.pos[2];
  // Pc = mRcw*P + mtcw (:276)
  const float xc = pose_row(C.Rt, 0, X, Y, Z), yc = pose_row(C.Rt, 1, X, Y, Z), zc = pose_row(C.Rt, 2, X, Y, Z);
  if (zc < 0.0f) return false;  // :282
  const float invz = pm_fdiv(1.0f, zc);  // :286, float
  const float u = pm_fadd(pm_fmul(pm_fmul(C.fx, xc), invz), C.cx);  // :287-288
  const float v = pm_fadd(pm_fmul(pm_fmul(C.fy, yc), invz), C.cy);
  if (u < P.minX || u > P.maxX) return false;  // :290-293
  if (v < P.minY || v > P.maxY) return false;
  const float maxDistance = pm_fmul(1.2f, mp.max_distance);  // GetMaxDistanceInvariance (src/MapPoint.cc:384-388)
  const float minDistance = pm_fmul(0.8f, mp.min_distance);  // GetMinDistanceInvariance (:378-382)
  const float PO0 = pm_fsub(X, C.Ow[0]), PO1 = pm_fsub(Y, C.Ow[1]), PO2 = pm_fsub(Z, C.Ow[2]);  // :298
  const float dist = norm3(PO0, PO1, PO2);  // :299
  if (dist < minDistance || dist > maxDistance) return false;  // :301
  // viewCos = PO.dot(Pn)/dist (:307): Mat::dot in double, a double divide, one rounding to float
  const double dot = pm_dadd(pm_dadd(pm_dmul((double)PO0, (double)mp.normal[0]),
                                     pm_dmul((double)PO1, (double)mp.normal[1])),
                             pm_dmul((double)PO2, (double)mp.normal[2]));
  const float viewCos = pm_d2f(pm_ddiv(dot, (double)dist));
  if (viewCos < P.cos_limit) return false;  // :309
  o->predicted_level = predict_level(P.pred_thr, P.L, mp.max_distance, dist);  // :313
  o->proj_x = u;  // :316-321
  o->proj_y = v;
  o->proj_xr = pm_fsub(u, pm_fmul(C.mbf, invz));
  o->view_cos = viewCos;
  o->track_in_view = 1;
  return true;
}

}  // namespace orbx
