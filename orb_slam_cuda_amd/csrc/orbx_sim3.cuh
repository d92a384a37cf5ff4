// orbx_sim3.cuh — Sim3Solver (src/Sim3Solver.cc) restated operation by
// operation for the kernels (orbx_sim3.hip) and the host form alike: the
// gather's per-correspondence record, RandomInt and the draw without
// replacement, ComputeSim3 (Horn's closed form with cv::eigen's float Jacobi
// and cv::Rodrigues), CheckInliers and the selection rule. Every float and
// double operation is one explicitly rounded pm_* call (orbx_posemath.cuh), so
// host and device differ only where libm and the device's math library do
// (atan2, sin, cos in double). The OpenCV conventions are those of DESIGN.md
// section 3, "Sim3Solver", UNPINNED.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "orbx_posemath.cuh"

namespace orbx {

constexpr int kStatusSim3Skipped = 512;  // matcher status bit: a match, keypoint index or octave out of range
constexpr int kSim3MaxIts = 1024;        // cap of orbm_sim3_params.max_iterations
constexpr int kSim3Chunk = 32;           // hypotheses per workgroup of the solve-and-count kernel
constexpr int kSim3LdsCorr = 1024;       // pair pitches up to this keep the gathered list in LDS
constexpr int kSim3Fields = 13;          // floats per gathered correspondence
constexpr uint32_t kSim3RandMax = 2147483647u;  // RAND_MAX of the reference's platform (glibc)

#if defined(__HIP_DEVICE_COMPILE__)
// IEEE square root: hipcc rounds sqrtf correctly by default (__fsqrt_rn is the approximate instruction alone)
__device__ __forceinline__ float pm_fsqrt(float a) { return __builtin_sqrtf(a); }
__device__ __forceinline__ double pm_dsub(double a, double b) { return __dsub_rn(a, b); }
#else
inline float pm_fsqrt(float a) { return std::sqrt(a); }
inline double pm_dsub(double a, double b) { return a - b; }
#endif
__host__ __device__ inline int s3_f2i(float f) { return __builtin_bit_cast(int, f); }
__host__ __device__ inline float s3_i2f(int i) { return __builtin_bit_cast(float, i); }

// The gathered correspondences, structure of arrays: field f of entry k at
// f*stride + k. Fields: 0..2 X3Dc1, 3..5 X3Dc2, 6..7 mvP1im1, 8..9 mvP2im2,
// 10 / 11 mvnMaxError1 / 2 as the float they are compared as, 12 the bits of i1.
struct Sim3Recs {
  float* f;
  int stride;
  __host__ __device__ float& at(int field, int k) const { return f[(size_t)field * stride + k]; }
};

// mvnMaxError = 9.210*sigma2 pushed into a vector<size_t> (:87-88,
// include/Sim3Solver.h:78-79): the double product truncated to an integer, and
// `err < maxErr` compares with that integer converted to float. A negative or
// NaN product (undefined in the reference) gives 0.
__host__ __device__ inline float sim3_max_error(float sigma2) {
  const double v = pm_dmul(9.210, (double)sigma2);
  if (!(v >= 0.0)) return 0.0f;
  if (v >= 18446744073709549568.0) return 18446744073709551616.0f;
  return (float)(unsigned long long)v;
}

// FromCameraToImage (:405-423)
__host__ __device__ inline void sim3_to_image(const orbm_camera& K, float X, float Y, float Z, float* u, float* v) {
  const float invz = pm_fdiv(1.0f, Z);
  *u = pm_fadd(pm_fmul(K.fx, pm_fmul(X, invz)), K.cx);
  *v = pm_fadd(pm_fmul(K.fy, pm_fmul(Y, invz)), K.cy);
}

// one entry of the constructor's loop body (:81-101) and of FromCameraToImage
__host__ __device__ inline void sim3_make_record(const orbm_camera& c1, const orbm_camera& c2, const float* Xw1,
                                                 const float* Xw2, float max_err1, float max_err2, int i1,
                                                 const Sim3Recs& R, int k) {
  float X1[3], X2[3], u, v;
  for (int r = 0; r < 3; ++r) {
    X1[r] = pose_row(c1.Tcw, r, Xw1[0], Xw1[1], Xw1[2]);
    X2[r] = pose_row(c2.Tcw, r, Xw2[0], Xw2[1], Xw2[2]);
    R.at(r, k) = X1[r];
    R.at(3 + r, k) = X2[r];
  }
  sim3_to_image(c1, X1[0], X1[1], X1[2], &u, &v);
  R.at(6, k) = u;
  R.at(7, k) = v;
  sim3_to_image(c2, X2[0], X2[1], X2[2], &u, &v);
  R.at(8, k) = u;
  R.at(9, k) = v;
  R.at(10, k) = max_err1;
  R.at(11, k) = max_err2;
  R.at(12, k) = s3_i2f(i1);
}

// DUtils::Random::RandomInt(0, d - 1) of the raw rand() value r
// (Thirdparty/DBoW2/DUtils/Random.cpp:47-50): int(((double)r / ((double)RAND_MAX
// + 1.0)) * d). With RAND_MAX + 1 = 2^31 and d < 2^22 both double operations
// are exact, so this is floor(r*d / 2^31) in integers. A value above RAND_MAX
// (no rand() result) is clamped into range. d >= 1.
__host__ __device__ inline int sim3_random_int(uint32_t r, int d) {
  const int v = (int)(((uint64_t)r * (uint64_t)d) >> 31);
  return v < d ? v : d - 1;
}

// The three draws without replacement on vAvailableIndices (:163-177): take
// [randi], move back() into the hole, pop. The list starts as the identity of
// length N >= 3; after two draws at most two slots differ from it.
__host__ __device__ inline void sim3_draw(const uint32_t* r3, int N, int* idx) {
  const int j0 = sim3_random_int(r3[0], N);
  idx[0] = j0;  // slot j0 now holds N - 1; N - 1 slots are left
  const int j1 = sim3_random_int(r3[1], N - 1);
  idx[1] = j1 == j0 ? N - 1 : j1;
  const int back1 = (N - 2 == j0) ? N - 1 : N - 2;  // slot j1 now holds this; N - 2 slots are left
  const int j2 = sim3_random_int(r3[2], N - 2);
  idx[2] = j2 == j1 ? back1 : (j2 == j0 ? N - 1 : j2);
}

// cv::eigen's work arrays for one 4x4 CV_32F matrix; the caller owns the
// storage (LDS on the device: k and l of a rotation are run-time indices)
struct Sim3Jacobi {
  float A[16], V[16], W[4];
  int indR[4], indC[4];
  int pad;
};

// lapack.cpp's hypot<float>
__host__ __device__ inline float sim3_hypot(float a, float b) {
  a = fabsf(a);
  b = fabsf(b);
  if (a > b) {
    b = pm_fdiv(b, a);
    return pm_fmul(a, pm_fsqrt(pm_fadd(1.0f, pm_fmul(b, b))));
  }
  if (b > 0) {
    a = pm_fdiv(a, b);
    return pm_fmul(b, pm_fsqrt(pm_fadd(1.0f, pm_fmul(a, a))));
  }
  return 0.0f;
}

// JacobiImpl_<float> (OpenCV 3.x modules/core/src/lapack.cpp) for n = 4: the
// largest off-diagonal element is the pivot (row maxima indR, column maxima
// indC kept up to date), at most n*n*30 = 480 rotations, eigenvalues sorted
// descending with their rows of V. J->A holds the symmetric matrix on entry.
__host__ __device__ inline void sim3_jacobi4(Sim3Jacobi* J) {
  constexpr int n = 4;
  const float eps = 1.1920928955078125e-07f;  // FLT_EPSILON
  float* A = J->A;
  float* V = J->V;
  float* W = J->W;
  int* indR = J->indR;
  int* indC = J->indC;
  for (int i = 0; i < n; i++) {
    for (int j = 0; j < n; j++) V[i * n + j] = 0.0f;
    V[i * n + i] = 1.0f;
  }
  for (int k = 0; k < n; k++) {
    W[k] = A[(n + 1) * k];
    if (k < n - 1) {
      int m = k + 1;
      float mv = fabsf(A[n * k + m]);
      for (int i = k + 2; i < n; i++) {
        const float val = fabsf(A[n * k + i]);
        if (mv < val) mv = val, m = i;
      }
      indR[k] = m;
    }
    if (k > 0) {
      int m = 0;
      float mv = fabsf(A[k]);
      for (int i = 1; i < k; i++) {
        const float val = fabsf(A[n * i + k]);
        if (mv < val) mv = val, m = i;
      }
      indC[k] = m;
    }
  }
  for (int iters = 0; iters < n * n * 30; iters++) {
    // the pivot (k, l)
    int k = 0;
    float mv = fabsf(A[indR[0]]);
    for (int i = 1; i < n - 1; i++) {
      const float val = fabsf(A[n * i + indR[i]]);
      if (mv < val) mv = val, k = i;
    }
    int l = indR[k];
    for (int i = 1; i < n; i++) {
      const float val = fabsf(A[n * indC[i] + i]);
      if (mv < val) mv = val, k = indC[i], l = i;
    }
    const float p = A[n * k + l];
    if (fabsf(p) <= eps) break;
    const float y = pm_d2f(pm_dmul((double)pm_fsub(W[l], W[k]), 0.5));
    float t = pm_fadd(fabsf(y), sim3_hypot(p, y));
    float s = sim3_hypot(p, t);
    const float c = pm_fdiv(t, s);
    s = pm_fdiv(p, s);
    t = pm_fmul(pm_fdiv(p, t), p);
    if (y < 0) s = -s, t = -t;
    A[n * k + l] = 0.0f;
    W[k] = pm_fsub(W[k], t);
    W[l] = pm_fadd(W[l], t);
#define ORBX_S3_ROTATE(v0, v1)                           \
  {                                                      \
    const float a0 = v0, b0 = v1;                        \
    v0 = pm_fsub(pm_fmul(a0, c), pm_fmul(b0, s));        \
    v1 = pm_fadd(pm_fmul(a0, s), pm_fmul(b0, c));        \
  }
    for (int i = 0; i < k; i++) ORBX_S3_ROTATE(A[n * i + k], A[n * i + l]);
    for (int i = k + 1; i < l; i++) ORBX_S3_ROTATE(A[n * k + i], A[n * i + l]);
    for (int i = l + 1; i < n; i++) ORBX_S3_ROTATE(A[n * k + i], A[n * l + i]);
    for (int i = 0; i < n; i++) ORBX_S3_ROTATE(V[n * k + i], V[n * l + i]);
#undef ORBX_S3_ROTATE
    for (int j = 0; j < 2; j++) {
      const int idx = j == 0 ? k : l;
      if (idx < n - 1) {
        int m = idx + 1;
        float mx = fabsf(A[n * idx + m]);
        for (int i = idx + 2; i < n; i++) {
          const float val = fabsf(A[n * idx + i]);
          if (mx < val) mx = val, m = i;
        }
        indR[idx] = m;
      }
      if (idx > 0) {
        int m = 0;
        float mx = fabsf(A[idx]);
        for (int i = 1; i < idx; i++) {
          const float val = fabsf(A[n * i + idx]);
          if (mx < val) mx = val, m = i;
        }
        indC[idx] = m;
      }
    }
  }
  for (int k = 0; k < n - 1; k++) {
    int m = k;
    for (int i = k + 1; i < n; i++)
      if (W[m] < W[i]) m = i;
    if (k != m) {
      const float w = W[m];
      W[m] = W[k];
      W[k] = w;
      for (int i = 0; i < n; i++) {
        const float v = V[n * m + i];
        V[n * m + i] = V[n * k + i];
        V[n * k + i] = v;
      }
    }
  }
}

// float dot of 3, left to right (gemm's small-matrix path)
__host__ __device__ inline float sim3_dot3(float a0, float b0, float a1, float b1, float a2, float b2) {
  return pm_fadd(pm_fadd(pm_fmul(a0, b0), pm_fmul(a1, b1)), pm_fmul(a2, b2));
}

// ComputeCentroid (:215-224): reduce(SUM) in float, C / 3 a convertTo scale
__host__ __device__ inline void sim3_centre(const float P[3][3], float Pr[3][3], float* O) {
  const float third = pm_d2f(pm_ddiv(1.0, 3.0));
  for (int r = 0; r < 3; ++r) {
    O[r] = pm_fadd(pm_fmul(pm_fadd(pm_fadd(P[0][r], P[1][r]), P[2][r]), third), 0.0f);
    for (int k = 0; k < 3; ++k) Pr[k][r] = pm_fsub(P[k][r], O[r]);
  }
}

// ComputeSim3 (:226-316) of the three point pairs P1[k] <-> P2[k] (camera
// frames 1 and 2): ms12i, mR12i (row-major), mt12i
__host__ __device__ inline void sim3_solve(const float P1[3][3], const float P2[3][3], bool fix_scale, Sim3Jacobi* J,
                                           float* s_out, float* R, float* t) {
  // Step 1
  float Pr1[3][3], Pr2[3][3], O1[3], O2[3];
  sim3_centre(P1, Pr1, O1);
  sim3_centre(P2, Pr2, O2);
  // Step 2: M = Pr2*Pr1.t()
  float M[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) M[i][j] = sim3_dot3(Pr2[0][i], Pr1[0][j], Pr2[1][i], Pr1[1][j], Pr2[2][i], Pr1[2][j]);
  // Step 3: the at<float> sums are float expressions (:251-260)
  const float N11 = pm_fadd(pm_fadd(M[0][0], M[1][1]), M[2][2]);
  const float N12 = pm_fsub(M[1][2], M[2][1]);
  const float N13 = pm_fsub(M[2][0], M[0][2]);
  const float N14 = pm_fsub(M[0][1], M[1][0]);
  const float N22 = pm_fsub(pm_fsub(M[0][0], M[1][1]), M[2][2]);
  const float N23 = pm_fadd(M[0][1], M[1][0]);
  const float N24 = pm_fadd(M[2][0], M[0][2]);
  const float N33 = pm_fsub(pm_fadd(-M[0][0], M[1][1]), M[2][2]);
  const float N34 = pm_fadd(M[1][2], M[2][1]);
  const float N44 = pm_fadd(pm_fsub(-M[0][0], M[1][1]), M[2][2]);
  float* A = J->A;
  A[0] = N11, A[1] = N12, A[2] = N13, A[3] = N14;
  A[4] = N12, A[5] = N22, A[6] = N23, A[7] = N24;
  A[8] = N13, A[9] = N23, A[10] = N33, A[11] = N34;
  A[12] = N14, A[13] = N24, A[14] = N34, A[15] = N44;
  // Step 4
  sim3_jacobi4(J);
  const float q0 = J->V[0];
  float vec[3] = {J->V[1], J->V[2], J->V[3]};
  const double nrm = pm_dsqrt(pm_dadd(pm_dadd(pm_dmul((double)vec[0], (double)vec[0]),
                                              pm_dmul((double)vec[1], (double)vec[1])),
                                      pm_dmul((double)vec[2], (double)vec[2])));
  const double ang = atan2(nrm, (double)q0);
  // vec = 2*ang*vec/norm(vec): one scale by (2*ang)*(1/norm)
  const float a = pm_d2f(pm_dmul(pm_dmul(2.0, ang), pm_ddiv(1.0, nrm)));
  for (int k = 0; k < 3; ++k) vec[k] = pm_fadd(pm_fmul(vec[k], a), 0.0f);
  // cv::Rodrigues in double, rounded to float
  {
    double rx = vec[0], ry = vec[1], rz = vec[2];
    const double theta = pm_dsqrt(pm_dadd(pm_dadd(pm_dmul(rx, rx), pm_dmul(ry, ry)), pm_dmul(rz, rz)));
    if (theta < 2.220446049250313e-16) {
      for (int k = 0; k < 9; ++k) R[k] = (k % 4 == 0) ? 1.0f : 0.0f;
    } else {
      const double c = cos(theta), s = sin(theta), c1 = pm_dsub(1.0, c);
      const double itheta = theta ? pm_ddiv(1.0, theta) : 0.0;
      rx = pm_dmul(rx, itheta);
      ry = pm_dmul(ry, itheta);
      rz = pm_dmul(rz, itheta);
      const double rrt[9] = {pm_dmul(rx, rx), pm_dmul(rx, ry), pm_dmul(rx, rz), pm_dmul(rx, ry), pm_dmul(ry, ry),
                             pm_dmul(ry, rz), pm_dmul(rx, rz), pm_dmul(ry, rz), pm_dmul(rz, rz)};
      const double r_x[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
      for (int k = 0; k < 9; ++k) {
        const double I = (k % 4 == 0) ? 1.0 : 0.0;
        R[k] = pm_d2f(pm_dadd(pm_dadd(pm_dmul(c, I), pm_dmul(c1, rrt[k])), pm_dmul(s, r_x[k])));
      }
    }
  }
  // Step 5: P3 = R*Pr2
  float P3[3][3];  // [point][component]
  for (int k = 0; k < 3; ++k)
    for (int i = 0; i < 3; ++i)
      P3[k][i] = sim3_dot3(R[3 * i], Pr2[k][0], R[3 * i + 1], Pr2[k][1], R[3 * i + 2], Pr2[k][2]);
  // Step 6: nom = Pr1.dot(P3) in double; den the double sum of the float squares; row-major order
  float s12 = 1.0f;
  if (!fix_scale) {
    double nom = 0.0, den = 0.0;
    for (int i = 0; i < 3; ++i)
      for (int k = 0; k < 3; ++k) {
        nom = pm_dadd(nom, pm_dmul((double)Pr1[k][i], (double)P3[k][i]));
        den = pm_dadd(den, (double)pm_fmul(P3[k][i], P3[k][i]));
      }
    s12 = pm_d2f(pm_ddiv(nom, den));
  }
  *s_out = s12;
  // Step 7: t = O1 - s*R*O2, one gemm (alpha = -s, C = O1)
  for (int r = 0; r < 3; ++r) {
    const float d = sim3_dot3(R[3 * r], O2[0], R[3 * r + 1], O2[1], R[3 * r + 2], O2[2]);
    t[r] = pm_d2f(pm_dadd(pm_dmul((double)d, -(double)s12), pm_dmul((double)O1[r], 1.0)));
  }
}

// Step 8 (:320-336) and src/ORBmatcher.cc:1118-1120 alike: S12 = [s*R | t],
// S21 = [(1.0/s)*R.t() | -sRinv*t] as 3x4: scalar * Mat a convertTo scale in
// float, -A*t gemm's small path with alpha -1
__host__ __device__ inline void sim3_transforms(float s12, const float* R12, const float* t12, float* S12,
                                                float* S21) {
  const float a12 = pm_d2f((double)s12), a21 = pm_d2f(pm_ddiv(1.0, (double)s12));
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      S12[4 * r + c] = pm_fadd(pm_fmul(R12[3 * r + c], a12), 0.0f);
      S21[4 * r + c] = pm_fadd(pm_fmul(R12[3 * c + r], a21), 0.0f);
    }
  for (int r = 0; r < 3; ++r) {
    S12[4 * r + 3] = t12[r];
    const float t = sim3_dot3(S21[4 * r], t12[0], S21[4 * r + 1], t12[1], S21[4 * r + 2], t12[2]);
    S21[4 * r + 3] = pm_d2f(pm_dadd(pm_dmul((double)t, -1.0), pm_dmul(0.0, 0.0)));
  }
}

// the two orbm_pose records of orbm_prepare_sim3_match
__host__ __device__ inline void sim3_match_poses(const orbm_camera& cam1, const float* T1w, const float* T2w,
                                                 float s12, const float* R12, const float* t12, orbm_pose* out) {
  float S12[12], S21[12];
  sim3_transforms(s12, R12, t12, S12, S21);
  for (int d = 0; d < 2; ++d) {
    orbm_pose* p = &out[d];
    const float* T = d == 0 ? T1w : T2w;
    const float* S = d == 0 ? S21 : S12;
    for (int k = 0; k < 12; ++k) p->Rt[k] = T[k];
    neg_rt_t(p->Rt, p->Ow);
    p->fx = cam1.fx;
    p->fy = cam1.fy;
    p->cx = cam1.cx;
    p->cy = cam1.cy;
    p->mbf = cam1.mbf;
    p->level_mode = 0;
    for (int k = 0; k < 12; ++k) p->Rt2[k] = S[k];
  }
}

// Project (:382-403) of one point, then dist.dot(dist) against the stored image point
__host__ __device__ inline float sim3_reproj_error(const float* S, const orbm_camera& K, float X, float Y, float Z,
                                                   float u0, float v0, bool stored_first) {
  const float x = pose_row(S, 0, X, Y, Z), y = pose_row(S, 1, X, Y, Z), z = pose_row(S, 2, X, Y, Z);
  float u, v;
  sim3_to_image(K, x, y, z, &u, &v);
  const float d0 = stored_first ? pm_fsub(u0, u) : pm_fsub(u, u0);
  const float d1 = stored_first ? pm_fsub(v0, v) : pm_fsub(v, v0);
  return pm_d2f(pm_dadd(pm_dmul((double)d0, (double)d0), pm_dmul((double)d1, (double)d1)));
}

// CheckInliers (:340-364) for entry k; a NaN error compares false
__host__ __device__ inline bool sim3_is_inlier(const float* S12, const float* S21, const orbm_camera& K1,
                                               const orbm_camera& K2, const Sim3Recs& R, int k) {
  const float err1 = sim3_reproj_error(S12, K1, R.at(3, k), R.at(4, k), R.at(5, k), R.at(6, k), R.at(7, k), true);
  const float err2 = sim3_reproj_error(S21, K2, R.at(0, k), R.at(1, k), R.at(2, k), R.at(8, k), R.at(9, k), false);
  return err1 < R.at(10, k) && err2 < R.at(11, k);
}

// iterate()'s bookkeeping (:181-200) over the counts of hypotheses [first,
// max_its): the running best (ties to the later one) and the first accepted
// index, -1 when there is none. count(h) gives mnInliersi of hypothesis h.
struct Sim3Selection {
  int accepted, best_inliers, best_iteration;
};
template <class CountAt>
__host__ __device__ inline Sim3Selection sim3_select(int first, int max_its, int min_inliers, int best0,
                                                     CountAt count) {
  Sim3Selection S{-1, best0, -1};
  for (int h = first; h < max_its; ++h) {
    const int c = count(h);
    if (c >= S.best_inliers) {
      S.best_inliers = c;
      S.best_iteration = h;
      if (c > min_inliers) {
        S.accepted = h;
        break;
      }
    }
  }
  return S;
}

// the result record of one pair; N = correspondences, max_its = 0 when N < min_inliers or N < 3
__host__ __device__ inline orbm_sim3_result sim3_result(const Sim3Selection& S, int accepted_count, int N,
                                                        int max_its, int first) {
  orbm_sim3_result r;
  r.ret = S.accepted >= 0 ? accepted_count : 0;
  r.iterations = S.accepted >= 0 ? S.accepted + 1 : (max_its > first ? max_its : first);
  r.no_more = S.accepted >= 0 ? 0 : 1;
  r.n_corr = N;
  r.max_its = max_its;
  r.best_inliers = S.best_inliers;
  r.best_iteration = S.best_iteration;
  r.reserved = 0;
  return r;
}

}  // namespace orbx
