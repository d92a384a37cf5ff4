// orbx_poseopt.cuh — the arithmetic of Optimizer::PoseOptimization
// (src/Optimizer.cc:334-543) as g2o carries it out, shared between the kernel
// (orbx_poseopt.hip) and the host-only entry orbm_pose_optimization_host. All
// of it is double, written with plain operators: the library is built with
// -ffp-contract=off for host and device, so no product and sum fuse.
//
// Sources restated here, from Thirdparty/g2o/g2o:
//   types/types_six_dof_expmap.{h,cpp}  the two OnlyPose edges: computeError,
//                                       cam_project, linearizeOplus; oplusImpl
//   types/se3quat.h                     SE3Quat: constructors, operator*, map,
//                                       exp, to_homogeneous_matrix, normalizeRotation
//   core/optimization_algorithm_levenberg.cpp  solve, computeLambdaInit, computeScale
//   core/sparse_optimizer.cpp           optimize, computeActiveErrors, activeRobustChi2
//   core/base_unary_edge.hpp            constructQuadraticForm
//   core/base_edge.h                    chi2, robustInformation
//   core/robust_kernel_impl.{h,cpp}     RobustKernelHuber (dsqr is a float)
//   solvers/linear_solver_dense.h       LDL^T of the dense 6x6 system
// and src/Converter.cc:37-53 (toSE3Quat, toCvMat). Eigen's own expressions
// (Quaterniond(R), quaternion product and rotation, toRotationMatrix,
// normalize) follow Eigen 3's formulas; where Eigen's evaluation order is not
// visible in the reference tree the order here is left to right.
//
// The solve itself (po_run, and the Levenberg-Marquardt loop lm_optimize under
// it that orbx_optsim3.cuh runs over 7 unknowns) is written once, over a
// context that supplies the three sums over the edges: the kernel reduces them
// lane -> wave -> workgroup, the host entry adds edge after edge in keypoint
// order.
#pragma once
#include <cfloat>

#include "orbx_posemath.cuh"

namespace orbx {

constexpr int kStatusPoseOptSkipped = 256;  // matcher status bit: a keypoint with an octave or map point row out of range

// SE3Quat: _r as (x, y, z, w), _t
struct PoPose {
  double q[4], t[3];
};
// the edges' fx, fy, cx, cy, bf (floats of the Frame, widened)
struct PoCam {
  double fx, fy, cx, cy, bf;
};
// One correspondence, 32 bytes: Xw, the observation (obs[2] = mvuRight, read
// by stereo edges only), mvInvLevelSigma2[octave], and tag = keypoint index |
// kPoStereo | kPoObs | kPoOutlier.
struct PoEdge {
  float X[3], obs[3], w;
  uint32_t tag;
};
constexpr uint32_t kPoIndexMask = 0xFFFFu;  // max_kps <= 65535
constexpr uint32_t kPoStereo = 1u << 16;    // mvuRight[i] >= 0
constexpr uint32_t kPoObs = 1u << 17;       // the point's Observations() > 0
constexpr uint32_t kPoOutlier = 1u << 18;   // mvbOutlier[i] (the edge is at level 1)

// accumulators of one linearisation: the upper triangle of H row by row, the
// negated b, the robust chi2
constexpr int kPoSums = 28, kPoB = 21, kPoChi = 27;

// Eigen::Quaterniond(Matrix3d) (Shoemake), R row-major. The branch for a
// largest diagonal element i is spelled per i: an index known only at run
// time would put q and R in scratch memory on the device.
template <int i>
__host__ __device__ inline void po_quat_diag(const double* R, double* q) {
  constexpr int j = (i + 1) % 3, k = (j + 1) % 3;
  double t = pm_dsqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0);
  q[i] = 0.5 * t;
  t = 0.5 / t;
  q[3] = (R[3 * k + j] - R[3 * j + k]) * t;
  q[j] = (R[3 * j + i] + R[3 * i + j]) * t;
  q[k] = (R[3 * k + i] + R[3 * i + k]) * t;
}
__host__ __device__ inline void po_quat_from_R(const double* R, double* q) {
  double t = R[0] + R[4] + R[8];
  if (t > 0.0) {
    t = pm_dsqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (R[7] - R[5]) * t;
    q[1] = (R[2] - R[6]) * t;
    q[2] = (R[3] - R[1]) * t;
  } else if (R[4] > R[0]) {  // i = 1 unless R22 is larger still
    if (R[8] > R[4])
      po_quat_diag<2>(R, q);
    else
      po_quat_diag<1>(R, q);
  } else {
    if (R[8] > R[0])
      po_quat_diag<2>(R, q);
    else
      po_quat_diag<0>(R, q);
  }
}

// SE3Quat::normalizeRotation: w >= 0, then unit norm
__host__ __device__ inline void po_normalize(double* q) {
  if (q[3] < 0) {
    q[0] *= -1;
    q[1] *= -1;
    q[2] *= -1;
    q[3] *= -1;
  }
  const double n = pm_dsqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  q[0] /= n;
  q[1] /= n;
  q[2] /= n;
  q[3] /= n;
}

// Quaterniond * Vector3d: uv = 2 (q.vec x v); v + w uv + q.vec x uv
__host__ __device__ inline void po_rotate(const double* q, const double* v, double* o) {
  double u0 = q[1] * v[2] - q[2] * v[1], u1 = q[2] * v[0] - q[0] * v[2], u2 = q[0] * v[1] - q[1] * v[0];
  u0 += u0;
  u1 += u1;
  u2 += u2;
  o[0] = v[0] + q[3] * u0 + (q[1] * u2 - q[2] * u1);
  o[1] = v[1] + q[3] * u1 + (q[2] * u0 - q[0] * u2);
  o[2] = v[2] + q[3] * u2 + (q[0] * u1 - q[1] * u0);
}

// Quaterniond product a * b
__host__ __device__ inline void po_qmul(const double* a, const double* b, double* o) {
  o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
  o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  o[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
  o[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
}

// Quaterniond::toRotationMatrix, row-major
__host__ __device__ inline void po_to_R(const double* q, double* R) {
  const double tx = 2.0 * q[0], ty = 2.0 * q[1], tz = 2.0 * q[2];
  const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
  const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
  const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
  R[0] = 1.0 - (tyy + tzz);
  R[1] = txy - twz;
  R[2] = txz + twy;
  R[3] = txy + twz;
  R[4] = 1.0 - (txx + tzz);
  R[5] = tyz - twx;
  R[6] = txz - twy;
  R[7] = tyz + twx;
  R[8] = 1.0 - (txx + tyy);
}

// Converter::toSE3Quat (src/Converter.cc:37-47): float -> double -> quaternion -> normalised
__host__ __device__ inline void po_from_Tcw(const float* T, PoPose* p) {
  double R[9];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) R[3 * r + c] = (double)T[4 * r + c];
    p->t[r] = (double)T[4 * r + 3];
  }
  po_quat_from_R(R, p->q);
  po_normalize(p->q);
}

// Converter::toCvMat(SE3Quat) (:49-53, :63-71): to_homogeneous_matrix rounded to float, rows 0..2
__host__ __device__ inline void po_to_Tcw(const PoPose& p, float* T) {
  double R[9];
  po_to_R(p.q, R);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T[4 * r + c] = pm_d2f(R[3 * r + c]);
    T[4 * r + 3] = pm_d2f(p.t[r]);
  }
}

// VertexSE3Expmap::oplusImpl: est = SE3Quat::exp(x) * est, x = [omega, upsilon]
__host__ __device__ inline void po_oplus(const double* x, PoPose* est) {
  const double o0 = x[0], o1 = x[1], o2 = x[2];
  const double theta = pm_dsqrt(o0 * o0 + o1 * o1 + o2 * o2);
  const double Om[9] = {0.0, -o2, o1, o2, 0.0, -o0, -o1, o0, 0.0};  // skew(omega)
  double Om2[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
      Om2[3 * r + c] = Om[3 * r] * Om[c] + Om[3 * r + 1] * Om[3 + c] + Om[3 * r + 2] * Om[6 + c];
  double R[9], V[9];
  if (theta < 0.00001) {
    for (int k = 0; k < 9; ++k) {
      R[k] = ((k % 4 == 0) ? 1.0 : 0.0) + Om[k] + Om2[k];
      V[k] = R[k];
    }
  } else {
    const double s = sin(theta), c = cos(theta);
    const double a = s / theta, b = (1 - c) / (theta * theta), d = (theta - s) / (theta * theta * theta);
    for (int k = 0; k < 9; ++k) {
      const double I = (k % 4 == 0) ? 1.0 : 0.0;
      R[k] = I + a * Om[k] + b * Om2[k];
      V[k] = I + b * Om[k] + d * Om2[k];
    }
  }
  PoPose e;  // SE3Quat(Quaterniond(R), V * upsilon)
  po_quat_from_R(R, e.q);
  for (int r = 0; r < 3; ++r) e.t[r] = V[3 * r] * x[3] + V[3 * r + 1] * x[4] + V[3 * r + 2] * x[5];
  po_normalize(e.q);
  // operator*: t = e.t + e.r * est.t; r = e.r * est.r; normalizeRotation
  double rt[3], q[4];
  po_rotate(e.q, est->t, rt);
  po_qmul(e.q, est->q, q);
  for (int r = 0; r < 3; ++r) est->t[r] = e.t[r] + rt[r];
  for (int r = 0; r < 4; ++r) est->q[r] = q[r];
  po_normalize(est->q);
}

// SE3Quat::map: _r * Xw + _t
__host__ __device__ inline void po_map(const PoPose& p, const PoEdge& e, double* P) {
  const double X[3] = {(double)e.X[0], (double)e.X[1], (double)e.X[2]};
  po_rotate(p.q, X, P);
  P[0] += p.t[0];
  P[1] += p.t[1];
  P[2] += p.t[2];
}

// computeError of the edge at `p` from the mapped point P: obs - cam_project.
// The monocular edge divides in double (project2d), the stereo edge takes
// invz = 1.0f / z as a float (types_six_dof_expmap.cpp:300). err[2] = 0 for a
// monocular edge.
__host__ __device__ inline void po_error(const PoCam& c, const PoEdge& e, const double* P, double* err) {
  if (e.tag & kPoStereo) {
    const double invz = (double)pm_d2f(1.0 / P[2]);
    const double u = P[0] * invz * c.fx + c.cx;
    err[0] = (double)e.obs[0] - u;
    err[1] = (double)e.obs[1] - (P[1] * invz * c.fy + c.cy);
    err[2] = (double)e.obs[2] - (u - c.bf * invz);
  } else {
    err[0] = (double)e.obs[0] - (P[0] / P[2] * c.fx + c.cx);
    err[1] = (double)e.obs[1] - (P[1] / P[2] * c.fy + c.cy);
    err[2] = 0.0;
  }
}

// BaseEdge::chi2: _error.dot(information() * _error), information = w * I
__host__ __device__ inline double po_chi2(const PoEdge& e, const double* err) {
  const double w = (double)e.w;
  double s = err[0] * (w * err[0]) + err[1] * (w * err[1]);
  if (e.tag & kPoStereo) s = s + err[2] * (w * err[2]);
  return s;
}

// the edge's chi2 at pose p
__host__ __device__ inline double po_edge_chi2(const PoCam& c, const PoPose& p, const PoEdge& e) {
  double P[3], err[3];
  po_map(p, e, P);
  po_error(c, e, P, err);
  return po_chi2(e, err);
}

// RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91): delta is
// (float)sqrt(5.991) or (float)sqrt(7.815) widened, dsqr the float of its
// square (robust_kernel_impl.h:84). rho[2] is not used (robustInformation).
__host__ __device__ inline void lm_huber(double delta, double dsqr, double e, double* rho0, double* rho1) {
  if (e <= dsqr) {
    *rho0 = e;
    *rho1 = 1.0;
  } else {
    const double sqrte = pm_dsqrt(e);
    *rho0 = 2 * sqrte * delta - dsqr;
    *rho1 = delta / sqrte;
  }
}
__host__ __device__ inline void po_huber(bool stereo, double e, double* rho0, double* rho1) {
  const double delta = (double)pm_d2f(pm_dsqrt(stereo ? 7.815 : 5.991));  // deltaStereo / deltaMono, :368-369
  lm_huber(delta, (double)pm_d2f(delta * delta), e, rho0, rho1);
}

// one edge's term of activeRobustChi2 at pose p
__host__ __device__ inline double po_edge_robust_chi2(const PoCam& c, const PoPose& p, const PoEdge& e, bool robust) {
  const double chi2 = po_edge_chi2(c, p, e);
  if (!robust) return chi2;
  double r0, r1;
  po_huber((e.tag & kPoStereo) != 0, chi2, &r0, &r1);
  return r0;
}

// computeError, linearizeOplus and constructQuadraticForm of one edge at pose
// p, added to acc: H += J^T (rho1 w) J, b -= rho1 J^T w e (acc holds -b), and
// the edge's robust chi2.
__host__ __device__ inline void po_edge_linearise(const PoCam& c, const PoPose& p, const PoEdge& e, bool robust,
                                                  double* acc) {
  double P[3], err[3];
  po_map(p, e, P);
  po_error(c, e, P, err);
  const bool stereo = (e.tag & kPoStereo) != 0;
  const double chi2 = po_chi2(e, err);
  double rho0 = chi2, rho1 = 1.0;
  if (robust) po_huber(stereo, chi2, &rho0, &rho1);
  acc[kPoChi] += rho0;
  const double x = P[0], y = P[1], invz = 1.0 / P[2], invz_2 = invz * invz;
  double J[18];
  J[0] = x * y * invz_2 * c.fx;
  J[1] = -(1 + (x * x * invz_2)) * c.fx;
  J[2] = y * invz * c.fx;
  J[3] = -invz * c.fx;
  J[4] = 0;
  J[5] = x * invz_2 * c.fx;
  J[6] = (1 + y * y * invz_2) * c.fy;
  J[7] = -x * y * invz_2 * c.fy;
  J[8] = -x * invz * c.fy;
  J[9] = 0;
  J[10] = -invz * c.fy;
  J[11] = y * invz_2 * c.fy;
  J[12] = J[0] - c.bf * y * invz_2;
  J[13] = J[1] + c.bf * x * invz_2;
  J[14] = J[2];
  J[15] = J[3];
  J[16] = 0;
  J[17] = J[5] - c.bf * invz_2;
  const double w = (double)e.w;
  const double rw = robust ? rho1 * w : w;  // robustInformation: rho[1] * information, nothing else
  int k = 0;
  for (int r = 0; r < 6; ++r) {
    const double a0 = J[r] * rw, a1 = J[6 + r] * rw, a2 = J[12 + r] * rw;
    for (int col = r; col < 6; ++col, ++k) {
      double h = a0 * J[col] + a1 * J[6 + col];
      if (stereo) h = h + a2 * J[12 + col];
      acc[k] += h;
    }
    double g = (J[r] * w) * err[0] + (J[6 + r] * w) * err[1];
    if (stereo) g = g + (J[12 + r] * w) * err[2];
    acc[kPoB + r] += robust ? rho1 * g : g;
  }
}

// the classification of :485-497 / :514-526: (float)chi2 against 5.991f / 7.815f
__host__ __device__ inline bool po_is_outlier(const PoEdge& e, double chi2) {
  const float c = pm_d2f(chi2);
  return (e.tag & kPoStereo) ? c > 7.815f : c > 5.991f;
}

// LinearSolverDense::solve on (H + lambda I) x = b for N unknowns: LDL^T
// without pivoting (Eigen's pivots; the signs of D are the same by inertia). A
// negative pivot is Eigen's !isPositive(): false, x untouched. H: upper
// triangle, row by row.
template <int N>
__host__ __device__ inline bool lm_ldlt_solve(const double* H, double lambda, const double* b, double* x) {
  double A[N][N], D[N], y[N];
  int k = 0;
#pragma unroll
  for (int r = 0; r < N; ++r)
#pragma unroll
    for (int c = r; c < N; ++c, ++k) A[c][r] = H[k] + ((r == c) ? lambda : 0.0);  // lower triangle
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double d = A[j][j];
#pragma unroll
    for (int m = 0; m < j; ++m) d = d - A[j][m] * A[j][m] * D[m];
    if (d < 0) return false;
    D[j] = d;
#pragma unroll
    for (int i = j + 1; i < N; ++i) {
      double s = A[i][j];
#pragma unroll
      for (int m = 0; m < j; ++m) s = s - A[i][m] * A[j][m] * D[m];
      A[i][j] = s / d;
    }
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double s = b[i];
#pragma unroll
    for (int m = 0; m < i; ++m) s = s - A[i][m] * y[m];
    y[i] = s;
  }
#pragma unroll
  for (int i = N - 1; i >= 0; --i) {
    double s = y[i] / D[i];
#pragma unroll
    for (int m = i + 1; m < N; ++m) s = s - A[m][i] * x[m];
    x[i] = s;
  }
  return true;
}

// the vertex's oplus as lm_optimize applies it; orbx_optsim3.cuh overloads it for its Sim3 vertex
template <class Ctx>
__host__ __device__ inline void lm_oplus(Ctx&, const double* x, PoPose* est) {
  po_oplus(x, est);
}

// SparseOptimizer::optimize(iterations) on one vertex of N unknowns, one
// OptimizationAlgorithmLevenberg::solve per iteration, continuing from *est.
// Ctx supplies over its active edges
//   void linearise(const Est&, bool robust, double acc[N(N+1)/2 + N + 1])
//     the upper triangle of H row by row, the negated b, the robust chi2
//     (computeActiveErrors, activeRobustChi2, buildSystem)
//   double robust_chi2(const Est&, bool robust)
// and lm_oplus(ctx, x, Est*) applies an update. *err_est follows the estimate
// the edges' _error was last computed at: a rejected trial restores the
// estimate, not the errors. Lambda, ni and the stall counter start afresh at
// iteration 0.
template <int N, class Est, class Ctx>
__host__ __device__ inline void lm_optimize(Ctx& ctx, int iterations, bool robust, Est* est_io, Est* err_est,
                                            int* trials, int* rejected) {
  constexpr int kB = N * (N + 1) / 2, kChi = kB + N;
  Est est = *est_io;
  double lambda = 0, ni = 2;
  int nStop = 0;
  double x[N];
#pragma unroll
  for (int k = 0; k < N; ++k) x[k] = 0;
  for (int i = 0; i < iterations; ++i) {
    double acc[kChi + 1];
    ctx.linearise(est, robust, acc);  // computeActiveErrors, activeRobustChi2, buildSystem
    *err_est = est;
    double currentChi = acc[kChi], tempChi = currentChi;
    const double iniChi = currentChi;
    double b[N];
#pragma unroll
    for (int k = 0; k < N; ++k) b[k] = -acc[kB + k];
    if (i == 0) {  // computeLambdaInit: tau * max |H_jj|
      double maxDiagonal = 0.;
      int k = 0;
#pragma unroll
      for (int r = 0; r < N; k += N - r, ++r) {
        const double a = fabs(acc[k]);
        maxDiagonal = (a < maxDiagonal) ? maxDiagonal : a;  // std::max(fabs(hessian(j,j)), maxDiagonal)
      }
      lambda = 1e-5 * maxDiagonal;
      ni = 2;
      nStop = 0;
    }
    double rho = 0;
    int qmax = 0;
    do {
      const Est backup = est;  // push
      const bool ok2 = lm_ldlt_solve<N>(acc, lambda, b, x);
      lm_oplus(ctx, x, &est);  // update(x): after a failed solve x is the previous one
      tempChi = ctx.robust_chi2(est, robust);
      *err_est = est;
      if (!ok2) tempChi = DBL_MAX;
      rho = (currentChi - tempChi);
      double scale = 0.;  // computeScale
#pragma unroll
      for (int k = 0; k < N; ++k) scale += x[k] * (lambda * x[k] + b[k]);
      scale += 1e-3;
      rho /= scale;
      ++*trials;
      if (rho > 0 && __builtin_isfinite(tempChi)) {  // last step was good
        const double c = 2 * rho - 1;
        double alpha = 1. - c * c * c;
        alpha = (2. / 3. < alpha) ? 2. / 3. : alpha;                 // std::min(alpha, _goodStepUpperScale)
        const double scaleFactor = (1. / 3. < alpha) ? alpha : 1. / 3.;  // std::max(_goodStepLowerScale, alpha)
        lambda *= scaleFactor;
        ni = 2;
        currentChi = tempChi;
      } else {
        lambda *= ni;
        ni *= 2;
        est = backup;  // pop: the estimate is restored, the edges' errors are not
        ++*rejected;
      }
      qmax++;
    } while (rho < 0 && qmax < 10);
    if (qmax == 10 || rho == 0) break;  // Terminate
    if ((iniChi - currentChi) * 1e3 < iniChi)  // the added stop rule
      nStop++;
    else
      nStop = 0;
    if (nStop >= 3) break;
  }
  *est_io = est;
}

// what po_run reports beside the pose
struct PoStats {
  int n_bad, rounds, trials, rejected;
};

// Optimizer::PoseOptimization from :459 on, for a frame with n_initial >= 3
// edges whose outlier marks are clear. Ctx supplies, over the edges that are
// not marked outlier:
//   void linearise(const PoPose&, bool robust, double acc[kPoSums])  the sums of po_edge_linearise
//   double robust_chi2(const PoPose&, bool robust)                   the sum of po_edge_robust_chi2
// and over all edges
//   int classify(const PoPose& est, const PoPose& err_pose)
// which marks each edge by its chi2 (at est for an edge marked outlier, which
// gets a fresh computeError at :480-483, at err_pose for the others, whose
// _error is what the last computeActiveErrors left) and returns nBad.
// On the device every thread of the workgroup runs this with the same values.
template <class Ctx>
__host__ __device__ inline void po_run(Ctx& ctx, const PoPose& T0, int n_initial, PoPose* out, PoStats* st) {
  int nBad = 0;
  st->rounds = st->trials = st->rejected = 0;
  PoPose est = T0;
  for (int it = 0; it < 4; ++it) {
    est = T0;  // vSE3->setEstimate(toSE3Quat(pFrame->mTcw)), :469
    PoPose err_pose = T0;
    const bool robust = it < 3;  // setRobustKernel(0) after the third classification
    if (n_initial - nBad > 0)  // else optimize() finds no vertex to optimise and returns
      lm_optimize<6>(ctx, 10, robust, &est, &err_pose, &st->trials, &st->rejected);  // SparseOptimizer::optimize(10)
    nBad = ctx.classify(est, err_pose);
    ++st->rounds;
    if (n_initial < 10) break;  // optimizer.edges().size() < 10, :532
  }
  st->n_bad = nBad;
  *out = est;
}

}  // namespace orbx
