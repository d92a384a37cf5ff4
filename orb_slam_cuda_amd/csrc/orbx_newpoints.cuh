// orbx_newpoints.cuh — the body of LocalMapping::CreateNewMapPoints
// (src/LocalMapping.cc:321-464) for one match (idx1, idx2) of one keyframe
// pair, restated operation by operation for the kernel (orbx_newpoints.hip)
// and the host form alike: the parallax test, the linear triangulation
// (cv::SVD::compute of a 4x4 CV_32F matrix), the two UnprojectStereo
// fallbacks (src/KeyFrame.cc:624-640) and the depth, reprojection and
// scale-consistency gates. Every float and double operation is one explicitly
// rounded pm_* call (orbx_posemath.cuh), so host and device differ only where
// libm and the device's math library do (atan2 in double). The OpenCV
// conventions are those of DESIGN.md section 3, "CreateNewMapPoints",
// UNPINNED.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "orbx_posemath.cuh"
#include "orbx_sim3.cuh"  // pm_dsub
#include "orbx_sincosf.h"

namespace orbx {

constexpr int kStatusNewPtBad = 1024;       // matcher status bit: idx2 / octave out of range, stereo depth <= 0
constexpr int kStatusNewPtOverflow = 2048;  // matcher status bit: more new points than `capacity`

// reason codes (include/orbx_c.h, ORBM_NEWPT_*)
enum : uint8_t {
  kNpNone = 0,
  kNpTriangulated = 1,
  kNpUnproject1 = 2,
  kNpUnproject2 = 3,
  kNpLowParallax = 4,
  kNpWZero = 5,
  kNpStereoDepth = 6,
  kNpBehind1 = 7,
  kNpBehind2 = 8,
  kNpReproj1 = 9,
  kNpReproj2 = 10,
  kNpDistZero = 11,
  kNpRatioLow = 12,
  kNpRatioHigh = 13,
  kNpDuplicate = 14,
  kNpBad = 15,
};
__host__ __device__ inline bool newpt_accepted(uint8_t r) { return r >= kNpTriangulated && r <= kNpUnproject2; }

// lapack.cpp's hypot<double>
__host__ __device__ inline double np_hypot(double a, double b) {
  a = fabs(a);
  b = fabs(b);
  if (a > b) {
    b = pm_ddiv(b, a);
    return pm_dmul(a, pm_dsqrt(pm_dadd(1.0, pm_dmul(b, b))));
  }
  if (b > 0) {
    a = pm_ddiv(a, b);
    return pm_dmul(b, pm_dsqrt(pm_dadd(1.0, pm_dmul(a, a))));
  }
  return 0.0;
}

// The work arrays of JacobiSVDImpl_<float> for a 4x4 matrix: At = the rows of
// the transposed input, Vt, and the squared row norms W in double. Every index
// into them below is a compile-time constant, so on the device the 36 values
// are registers.
struct NpSvd {
  float A[4][4], V[4][4];
  double W[4];
};

// one step (i, j) of a sweep: returns whether the rows were rotated
template <int I, int J>
__host__ __device__ __forceinline__ bool np_svd_pair(NpSvd& S) {
  const double eps = 2.384185791015625e-07;  // (float)(FLT_EPSILON*2) as the _Tp eps argument
  double a = S.W[I], p = 0, b = S.W[J];
#pragma unroll
  for (int k = 0; k < 4; ++k) p = pm_dadd(p, pm_dmul((double)S.A[I][k], (double)S.A[J][k]));
  if (fabs(p) <= pm_dmul(eps, pm_dsqrt(pm_dmul(a, b)))) return false;
  p = pm_dmul(p, 2.0);
  const double beta = pm_dsub(a, b), gamma = np_hypot(p, beta);
  float c, s;
  if (beta < 0) {
    const double delta = pm_dmul(pm_dsub(gamma, beta), 0.5);
    s = pm_d2f(pm_dsqrt(pm_ddiv(delta, gamma)));
    c = pm_d2f(pm_ddiv(p, pm_dmul(pm_dmul(gamma, (double)s), 2.0)));
  } else {
    c = pm_d2f(pm_dsqrt(pm_ddiv(pm_dadd(gamma, beta), pm_dmul(gamma, 2.0))));
    s = pm_d2f(pm_ddiv(p, pm_dmul(pm_dmul(gamma, (double)c), 2.0)));
  }
  a = b = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float t0 = pm_fadd(pm_fmul(c, S.A[I][k]), pm_fmul(s, S.A[J][k]));
    const float t1 = pm_fadd(pm_fmul(-s, S.A[I][k]), pm_fmul(c, S.A[J][k]));
    S.A[I][k] = t0;
    S.A[J][k] = t1;
    a = pm_dadd(a, pm_dmul((double)t0, (double)t0));
    b = pm_dadd(b, pm_dmul((double)t1, (double)t1));
  }
  S.W[I] = a;
  S.W[J] = b;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float t0 = pm_fadd(pm_fmul(c, S.V[I][k]), pm_fmul(s, S.V[J][k]));
    const float t1 = pm_fadd(pm_fmul(-s, S.V[I][k]), pm_fmul(c, S.V[J][k]));
    S.V[I][k] = t0;
    S.V[J][k] = t1;
  }
  return true;
}

// the final selection sort's step for position I: the first largest W of I..3
// comes to I, with its row of Vt (the rows of At are not needed after it)
template <int I>
__host__ __device__ __forceinline__ void np_svd_sort_step(NpSvd& S) {
  int j = I;
  double wj = S.W[I];
#pragma unroll
  for (int k = I + 1; k < 4; ++k)
    if (wj < S.W[k]) {
      j = k;
      wj = S.W[k];
    }
#pragma unroll
  for (int k = I + 1; k < 4; ++k)
    if (j == k) {
      const double w = S.W[I];
      S.W[I] = S.W[k];
      S.W[k] = w;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float v = S.V[I][q];
        S.V[I][q] = S.V[k][q];
        S.V[k][q] = v;
      }
    }
}

// cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV) of a 4x4 CV_32F matrix as
// far as vt.row(3): OpenCV 3.x JacobiSVDImpl_<float> (modules/core/src/
// lapack.cpp) on the transposed matrix. M is A row-major; x gets vt.row(3).
__host__ __device__ inline void np_svd4_last_row(const float (&M)[4][4], float* x) {
  NpSvd S;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double sd = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float t = M[k][i];  // At = A.t()
      S.A[i][k] = t;
      sd = pm_dadd(sd, pm_dmul((double)t, (double)t));
      S.V[i][k] = i == k ? 1.0f : 0.0f;
    }
    S.W[i] = sd;
  }
  for (int iter = 0; iter < 30; ++iter) {  // max(m, 30)
    bool changed = false;
    changed |= np_svd_pair<0, 1>(S);
    changed |= np_svd_pair<0, 2>(S);
    changed |= np_svd_pair<0, 3>(S);
    changed |= np_svd_pair<1, 2>(S);
    changed |= np_svd_pair<1, 3>(S);
    changed |= np_svd_pair<2, 3>(S);
    if (!changed) break;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double sd = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) sd = pm_dadd(sd, pm_dmul((double)S.A[i][k], (double)S.A[i][k]));
    S.W[i] = pm_dsqrt(sd);
  }
  np_svd_sort_step<0>(S);
  np_svd_sort_step<1>(S);
  np_svd_sort_step<2>(S);
#pragma unroll
  for (int k = 0; k < 4; ++k) x[k] = S.V[3][k];
}

// Rcw.row(r).dot(x3Dt) + tcw.at<float>(r): Mat::dot's double sum, the float
// term added in double, one rounding to the float it is assigned to
__host__ __device__ inline float np_row_dot(const float* T, int r, const float* x) {
  const double d = pm_dadd(pm_dadd(pm_dmul((double)T[4 * r], (double)x[0]), pm_dmul((double)T[4 * r + 1], (double)x[1])),
                           pm_dmul((double)T[4 * r + 2], (double)x[2]));
  return pm_d2f(pm_dadd(d, (double)T[4 * r + 3]));
}

// cos(2*atan2(mb/2, depth)) (:345, :347). TemplatedVocabulary.h and
// block_solver.hpp put `using namespace std` in front of LocalMapping.cc, so
// with float arguments these are std::atan2(float, float) and std::cos(float):
// atan2f, a float product, cosf. cosf is glibc's (orbx_sincosf.h). atan2f is
// taken as the correctly rounded one (glibc 2.41's; older ones are within an
// ulp of it), computed as the float of the double atan2.
__host__ __device__ inline float np_cos_parallax_stereo(float mb, float depth) {
  const float ang = pm_d2f(atan2((double)pm_fdiv(mb, 2.0f), (double)depth));
  if (ang != ang) return ang;  // cosf(NaN); the restated cosf converts its argument to an integer
  float sn, cs;
  glibc_sincosf(pm_fmul(2.0f, ang), &sn, &cs);
  return cs;
}

// KeyFrame::UnprojectStereo (src/KeyFrame.cc:624-640) with z > 0: u, v are
// mvKeys[i].pt, the distorted keypoint
__host__ __device__ inline void np_unproject(float u, float v, float z, float cx, float cy, float invfx, float invfy,
                                             const float* Twc, float* x3D) {
  const float x = pm_fmul(pm_fmul(pm_fsub(u, cx), z), invfx);
  const float y = pm_fmul(pm_fmul(pm_fsub(v, cy), z), invfy);
  for (int r = 0; r < 3; ++r) x3D[r] = pose_row(Twc, r, x, y, z);
}

// one keyframe's side of a match
struct NpSide {
  float x, y;    // mvKeysUn[idx].pt
  float rx, ry;  // mvKeys[idx].pt
  float uright, depth;
  float sigma2, scale;  // mvLevelSigma2 / mvScaleFactors [mvKeysUn[idx].octave]
};

// the reprojection gate of one keyframe (:396-420, :423-446); mbf is the
// current keyframe's for both (:413, :439)
__host__ __device__ inline bool np_reproj_fails(const float* Tcw, const float* x3D, float z, float fx, float fy, float cx,
                                                float cy, float mbf, bool stereo, const NpSide& k) {
  const float x = np_row_dot(Tcw, 0, x3D), y = np_row_dot(Tcw, 1, x3D);
  const float invz = pm_d2f(pm_ddiv(1.0, (double)z));
  const float u = pm_fadd(pm_fmul(pm_fmul(fx, x), invz), cx);
  const float v = pm_fadd(pm_fmul(pm_fmul(fy, y), invz), cy);
  const float ex = pm_fsub(u, k.x), ey = pm_fsub(v, k.y);
  const float e2 = pm_fadd(pm_fmul(ex, ex), pm_fmul(ey, ey));
  if (!stereo) return (double)e2 > pm_dmul(5.991, (double)k.sigma2);
  const float ur = pm_fsub(u, pm_fmul(mbf, invz));
  const float er = pm_fsub(ur, k.uright);
  return (double)pm_fadd(e2, pm_fmul(er, er)) > pm_dmul(7.8, (double)k.sigma2);
}

// The loop body for one match. Returns the reason code; pos gets x3D when the
// point is accepted (codes 1..3), zeros otherwise.
__host__ __device__ inline uint8_t newpt_match(const orbm_newpt_pair& P, const NpSide& k1, const NpSide& k2, float* pos) {
  pos[0] = pos[1] = pos[2] = 0.0f;
  const bool bStereo1 = k1.uright >= 0, bStereo2 = k2.uright >= 0;
  // :333-338
  const float xn1[3] = {pm_fmul(pm_fsub(k1.x, P.cx1), P.invfx1), pm_fmul(pm_fsub(k1.y, P.cy1), P.invfy1), 1.0f};
  const float xn2[3] = {pm_fmul(pm_fsub(k2.x, P.cx2), P.invfx2), pm_fmul(pm_fsub(k2.y, P.cy2), P.invfy2), 1.0f};
  float ray1[3], ray2[3];
  for (int r = 0; r < 3; ++r) {  // Rwc*xn: gemm's small-matrix path, float dot products
    ray1[r] = pm_fadd(pm_fadd(pm_fmul(P.Rwc1[3 * r], xn1[0]), pm_fmul(P.Rwc1[3 * r + 1], xn1[1])),
                      pm_fmul(P.Rwc1[3 * r + 2], xn1[2]));
    ray2[r] = pm_fadd(pm_fadd(pm_fmul(P.Rwc2[3 * r], xn2[0]), pm_fmul(P.Rwc2[3 * r + 1], xn2[1])),
                      pm_fmul(P.Rwc2[3 * r + 2], xn2[2]));
  }
  const double dot = pm_dadd(pm_dadd(pm_dmul((double)ray1[0], (double)ray2[0]), pm_dmul((double)ray1[1], (double)ray2[1])),
                             pm_dmul((double)ray1[2], (double)ray2[2]));
  const double n1 = pm_dsqrt(pm_dadd(pm_dadd(pm_dmul((double)ray1[0], (double)ray1[0]), pm_dmul((double)ray1[1], (double)ray1[1])),
                                     pm_dmul((double)ray1[2], (double)ray1[2])));
  const double n2 = pm_dsqrt(pm_dadd(pm_dadd(pm_dmul((double)ray2[0], (double)ray2[0]), pm_dmul((double)ray2[1], (double)ray2[1])),
                                     pm_dmul((double)ray2[2], (double)ray2[2])));
  const float cosParallaxRays = pm_d2f(pm_ddiv(dot, pm_dmul(n1, n2)));
  // :340-349
  float cosParallaxStereo = pm_fadd(cosParallaxRays, 1.0f);
  float cosParallaxStereo1 = cosParallaxStereo, cosParallaxStereo2 = cosParallaxStereo;
  if (bStereo1)
    cosParallaxStereo1 = np_cos_parallax_stereo(P.mb1, k1.depth);
  else if (bStereo2)
    cosParallaxStereo2 = np_cos_parallax_stereo(P.mb2, k2.depth);
  cosParallaxStereo = cosParallaxStereo2 < cosParallaxStereo1 ? cosParallaxStereo2 : cosParallaxStereo1;  // std::min

  float x3D[3];
  uint8_t kind;
  if (cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 &&
      (bStereo1 || bStereo2 || (double)cosParallaxRays < 0.9998)) {
    // :355-370. s*Tcw.row(2) - Tcw.row(k) is one addWeighted: (s*a + (-1)*b) + 0 in float
    float A[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      A[0][c] = pm_fadd(pm_fadd(pm_fmul(P.Tcw1[8 + c], xn1[0]), pm_fmul(P.Tcw1[c], -1.0f)), 0.0f);
      A[1][c] = pm_fadd(pm_fadd(pm_fmul(P.Tcw1[8 + c], xn1[1]), pm_fmul(P.Tcw1[4 + c], -1.0f)), 0.0f);
      A[2][c] = pm_fadd(pm_fadd(pm_fmul(P.Tcw2[8 + c], xn2[0]), pm_fmul(P.Tcw2[c], -1.0f)), 0.0f);
      A[3][c] = pm_fadd(pm_fadd(pm_fmul(P.Tcw2[8 + c], xn2[1]), pm_fmul(P.Tcw2[4 + c], -1.0f)), 0.0f);
    }
    float h[4];
    np_svd4_last_row(A, h);
    if (h[3] == 0) return kNpWZero;
    const float a = pm_d2f(pm_ddiv(1.0, (double)h[3]));  // Mat / float: convertTo with the scale 1/s
    for (int r = 0; r < 3; ++r) x3D[r] = pm_fadd(pm_fmul(h[r], a), 0.0f);
    kind = kNpTriangulated;
  } else if (bStereo1 && cosParallaxStereo1 < cosParallaxStereo2) {
    if (!(k1.depth > 0)) return kNpStereoDepth;  // the reference dereferences an empty Mat here
    np_unproject(k1.rx, k1.ry, k1.depth, P.cx1, P.cy1, P.invfx1, P.invfy1, P.Twc1, x3D);
    kind = kNpUnproject1;
  } else if (bStereo2 && cosParallaxStereo2 < cosParallaxStereo1) {
    if (!(k2.depth > 0)) return kNpStereoDepth;
    np_unproject(k2.rx, k2.ry, k2.depth, P.cx2, P.cy2, P.invfx2, P.invfy2, P.Twc2, x3D);
    kind = kNpUnproject2;
  } else {
    return kNpLowParallax;
  }
  // :387-393
  const float z1 = np_row_dot(P.Tcw1, 2, x3D);
  if (z1 <= 0) return kNpBehind1;
  const float z2 = np_row_dot(P.Tcw2, 2, x3D);
  if (z2 <= 0) return kNpBehind2;
  // :396-446
  if (np_reproj_fails(P.Tcw1, x3D, z1, P.fx1, P.fy1, P.cx1, P.cy1, P.mbf1, bStereo1, k1)) return kNpReproj1;
  if (np_reproj_fails(P.Tcw2, x3D, z2, P.fx2, P.fy2, P.cx2, P.cy2, P.mbf1, bStereo2, k2)) return kNpReproj2;
  // :449-464
  const float dist1 = norm3(pm_fsub(x3D[0], P.Ow1[0]), pm_fsub(x3D[1], P.Ow1[1]), pm_fsub(x3D[2], P.Ow1[2]));
  const float dist2 = norm3(pm_fsub(x3D[0], P.Ow2[0]), pm_fsub(x3D[1], P.Ow2[1]), pm_fsub(x3D[2], P.Ow2[2]));
  if (dist1 == 0 || dist2 == 0) return kNpDistZero;
  const float ratioDist = pm_fdiv(dist2, dist1);
  const float ratioOctave = pm_fdiv(k1.scale, k2.scale);
  if (pm_fmul(ratioDist, P.ratio_factor) < ratioOctave) return kNpRatioLow;
  if (ratioDist > pm_fmul(ratioOctave, P.ratio_factor)) return kNpRatioHigh;
  pos[0] = x3D[0];
  pos[1] = x3D[1];
  pos[2] = x3D[2];
  return kind;
}

// One entry of matches12 with its range checks: idx2 < 0 is no match; idx2 >=
// n2 or an octave outside [0, nlevels) is kNpBad. kr1 / kr2: mvKeys, or null
// for "the same as mvKeysUn". *bad is set for kNpBad and kNpStereoDepth.
__host__ __device__ inline uint8_t newpt_entry(const orbm_newpt_pair& P, const orbx_kp* kp1, const orbx_kp* kr1,
                                               const float* ur1, const float* dp1, int idx1, const orbx_kp* kp2,
                                               const orbx_kp* kr2, const float* ur2, const float* dp2, int n2, int idx2,
                                               const float* sigma2, const float* scale, int nlevels, float* pos,
                                               bool* bad) {
  pos[0] = pos[1] = pos[2] = 0.0f;
  *bad = false;
  if (idx2 < 0) return kNpNone;
  if (idx2 >= n2) {
    *bad = true;
    return kNpBad;
  }
  const orbx_kp a = kp1[idx1], b = kp2[idx2];
  if (a.octave < 0 || a.octave >= nlevels || b.octave < 0 || b.octave >= nlevels) {
    *bad = true;
    return kNpBad;
  }
  NpSide k1, k2;
  k1.x = a.x;
  k1.y = a.y;
  k1.rx = kr1 ? kr1[idx1].x : a.x;
  k1.ry = kr1 ? kr1[idx1].y : a.y;
  k1.uright = ur1[idx1];
  k1.depth = dp1[idx1];
  k1.sigma2 = sigma2[a.octave];
  k1.scale = scale[a.octave];
  k2.x = b.x;
  k2.y = b.y;
  k2.rx = kr2 ? kr2[idx2].x : b.x;
  k2.ry = kr2 ? kr2[idx2].y : b.y;
  k2.uright = ur2[idx2];
  k2.depth = dp2[idx2];
  k2.sigma2 = sigma2[b.octave];
  k2.scale = scale[b.octave];
  const uint8_t r = newpt_match(P, k1, k2, pos);
  if (r == kNpStereoDepth) *bad = true;
  return r;
}

// orbm_prepare_new_points: KeyFrame::SetPose's Rwc, Ow, Twc (src/KeyFrame.cc:79-95)
// and the Frame constructor's invfx / invfy for both cameras
__host__ __device__ inline void newpt_prepare(const orbm_camera& c1, const orbm_camera& c2, float scale_factor,
                                              uint32_t kf1, uint32_t kf2, uint32_t desc_base1, uint32_t desc_base2,
                                              int kf2_first, orbm_newpt_pair* o) {
  o->fx1 = c1.fx; o->fy1 = c1.fy; o->cx1 = c1.cx; o->cy1 = c1.cy;
  o->invfx1 = pm_fdiv(1.0f, c1.fx);
  o->invfy1 = pm_fdiv(1.0f, c1.fy);
  o->mb1 = c1.mb;
  o->mbf1 = c1.mbf;
  o->fx2 = c2.fx; o->fy2 = c2.fy; o->cx2 = c2.cx; o->cy2 = c2.cy;
  o->invfx2 = pm_fdiv(1.0f, c2.fx);
  o->invfy2 = pm_fdiv(1.0f, c2.fy);
  o->mb2 = c2.mb;
  o->ratio_factor = pm_fmul(1.5f, scale_factor);
  for (int k = 0; k < 12; ++k) {
    o->Tcw1[k] = c1.Tcw[k];
    o->Tcw2[k] = c2.Tcw[k];
  }
  neg_rt_t(c1.Tcw, o->Ow1);
  neg_rt_t(c2.Tcw, o->Ow2);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) {
      o->Rwc1[3 * r + c] = o->Twc1[4 * r + c] = c1.Tcw[4 * c + r];
      o->Rwc2[3 * r + c] = o->Twc2[4 * r + c] = c2.Tcw[4 * c + r];
    }
    o->Twc1[4 * r + 3] = o->Ow1[r];
    o->Twc2[4 * r + 3] = o->Ow2[r];
  }
  o->kf1 = kf1;
  o->kf2 = kf2;
  o->desc_base1 = desc_base1;
  o->desc_base2 = desc_base2;
  o->kf2_first = kf2_first ? 1 : 0;
  o->pad = 0;
}

}  // namespace orbx
