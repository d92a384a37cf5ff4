// orbx_mappoint.cuh — the arithmetic MapPoint::ComputeDistinctiveDescriptors
// (src/MapPoint.cc:247-312) and MapPoint::UpdateNormalAndDepth (:335-376)
// share between the refresh kernels (orbx_mappoint.hip) and the host-only
// entries orbm_distinctive_descriptor / orbm_update_normal_and_depth: one
// rounding per reference operation, through the pm_* helpers.
#pragma once
#include "orbx_posemath.cuh"

namespace orbx {

// ORBmatcher::DescriptorDistance of two descriptors held as 8 words
__host__ __device__ inline int mp_hamming(const uint32_t* a, const uint32_t* b) {
  int d = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) d += __builtin_popcount(a[k] ^ b[k]);
  return d;
}

// normali / cv::norm(normali), normali = mWorldPos - Owi (:359-360): the
// difference in float, the norm in double (not rounded to float), Mat / double
// as a scale by (float)(1.0 / s). s == 0 gives inf * 0 = NaN, as there.
__host__ __device__ inline void mp_normal_term(const float* pos, const float* Ow, float* t) {
  const float v0 = pm_fsub(pos[0], Ow[0]), v1 = pm_fsub(pos[1], Ow[1]), v2 = pm_fsub(pos[2], Ow[2]);
  const double s = pm_dsqrt(pm_dadd(pm_dadd(pm_dmul((double)v0, (double)v0), pm_dmul((double)v1, (double)v1)),
                                    pm_dmul((double)v2, (double)v2)));
  const float a = pm_d2f(pm_ddiv(1.0, s));
  t[0] = pm_fmul(v0, a);
  t[1] = pm_fmul(v1, a);
  t[2] = pm_fmul(v2, a);
}

// normal = normal + term (:360), one observation of the ordered sum
__host__ __device__ inline void mp_normal_add(float* normal, const float* t) {
  normal[0] = pm_fadd(normal[0], t[0]);
  normal[1] = pm_fadd(normal[1], t[1]);
  normal[2] = pm_fadd(normal[2], t[2]);
}

// the tail (:364-374): mNormalVector = normal / n, dist = norm(Pos - Ow_ref),
// mfMaxDistance = dist * mvScaleFactors[level], mfMinDistance = mfMaxDistance /
// mvScaleFactors[nLevels - 1]. out: normal[3], min_distance, max_distance (the
// order of orbm_map_point_world).
__host__ __device__ inline void mp_finish(const float* sum, unsigned n, const float* pos, const float* Ow_ref,
                                          float ref_scale, float last_scale, float* out) {
  const float a = pm_d2f(pm_ddiv(1.0, (double)n));
  out[0] = pm_fmul(sum[0], a);
  out[1] = pm_fmul(sum[1], a);
  out[2] = pm_fmul(sum[2], a);
  const float dist = norm3(pm_fsub(pos[0], Ow_ref[0]), pm_fsub(pos[1], Ow_ref[1]), pm_fsub(pos[2], Ow_ref[2]));
  const float maxd = pm_fmul(dist, ref_scale);
  out[4] = maxd;
  out[3] = pm_fdiv(maxd, last_scale);
}

}  // namespace orbx
