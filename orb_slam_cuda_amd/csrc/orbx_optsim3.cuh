// orbx_optsim3.cuh — the arithmetic of Optimizer::OptimizeSim3
// (src/Optimizer.cc:1190-1385) as g2o carries it out, shared between the kernel
// (orbx_optsim3.hip) and the host-only entry orbm_optimize_sim3_host. All of it
// is double, written with plain operators: the library is built with
// -ffp-contract=off for host and device, so no product and sum fuse.
//
// Sources restated here, from Thirdparty/g2o/g2o:
//   types/types_seven_dof_expmap.{h,cpp}  VertexSim3Expmap::oplusImpl, cam_map1 / cam_map2,
//                                         EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ::computeError
//   types/sim3.h                          Sim3(Vector7d) with its four branches, map, inverse, operator*
//   types/se3_ops.hpp                     skew, project
//   core/base_binary_edge.hpp             linearizeOplus (the numeric Jacobian: the edges' own
//                                         linearizeOplus is commented out), constructQuadraticForm
//   core/robust_kernel_impl.{h,cpp}       RobustKernelHuber (lm_huber)
// and, through orbx_poseopt.cuh, the Levenberg-Marquardt loop and the dense
// LDL^T (lm_optimize<7>), Eigen's quaternion expressions (po_*). Neither
// Sim3::operator* nor Sim3(R, t, s) normalises or flips the quaternion.
//
// The solve (os3_run) is written once over a context that supplies the sums
// over the edge pairs: the kernel reduces them lane -> wave -> workgroup, the
// host entry adds pair after pair in i1 order, e12(i) before e21(i).
#pragma once
#include "orbx_poseopt.cuh"

namespace orbx {

constexpr int kStatusOptSim3Skipped = 8192;  // matcher status bit: a match, found index or octave out of range
constexpr int kOs3LdsCorr = 1024;            // pair pitches up to this keep the edge pairs in LDS

// g2o::Sim3: r as (x, y, z, w), t, s
struct Os3Est {
  double q[4], t[3], s;
};
// _focal_length1 / _principle_point1 and 2 (floats of mK, widened)
struct Os3Cam {
  double fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2;
};
// RobustKernelHuber::setDelta(deltaHuber), deltaHuber = sqrt(th2) a float: delta widened, _dsqr the float of
// its square (robust_kernel_impl.h:84); th2 widened for `chi2() > th2` (:1337, :1371)
struct Os3Huber {
  double delta, dsqr, th2;
};
__host__ inline Os3Huber os3_huber(float th2) {
  const float d = std::sqrt(th2);
  return Os3Huber{(double)d, (double)(float)((double)d * (double)d), (double)th2};
}

// One edge pair, 56 bytes: P3D1c, P3D2c (float cv::Mat products), the two
// observations, mvInvLevelSigma2 of their octaves, i1 and kOs3Removed /
// kOs3Rejected.
struct Os3Edge {
  float X1[3], X2[3], obs1[2], obs2[2], w1, w2;
  int32_t i1;
  uint32_t tag;
};
constexpr uint32_t kOs3Removed = 1;   // removeEdge after the first optimisation (:1337-1346)
constexpr uint32_t kOs3Rejected = 2;  // nulled by the second check (:1371-1375)

// accumulators of one linearisation: the upper triangle of H row by row, the negated b, the robust chi2
constexpr int kOs3Sums = 36, kOs3B = 28, kOs3Chi = 35;
constexpr int kOs3Disp = 28;  // 7 columns x (+delta, -delta) x (estimate, its inverse)

// R1w*P3D1w + t1w as the float cv::Mat product (:1262, :1270), the gather of Sim3Solver (sim3_make_record)
__host__ __device__ inline void os3_make_edge(const orbm_camera& c1, const orbm_camera& c2, const float* Xw1,
                                              const float* Xw2, const orbx_kp& k1, const orbx_kp& k2, float w1,
                                              float w2, int i1, Os3Edge* e) {
  for (int r = 0; r < 3; ++r) {
    e->X1[r] = pose_row(c1.Tcw, r, Xw1[0], Xw1[1], Xw1[2]);
    e->X2[r] = pose_row(c2.Tcw, r, Xw2[0], Xw2[1], Xw2[2]);
  }
  e->obs1[0] = k1.x;
  e->obs1[1] = k1.y;
  e->obs2[0] = k2.x;
  e->obs2[1] = k2.y;
  e->w1 = w1;
  e->w2 = w2;
  e->i1 = i1;
  e->tag = 0;
}

// vpMatches1[i1] as the caller's lists give it (orbx_c.h): the RANSAC inlier
// of match12, else the mutual agreement of found12 / found21 on a keypoint of
// KF2 that no kept match targets (taken(i2)). -1: none; *bad |= 1 for a value
// out of range.
__host__ __device__ inline bool os3_kept(const int* match12, const uint8_t* inlier, int i1) {
  return match12[i1] >= 0 && (!inlier || inlier[i1]);
}
template <class Taken>
__host__ __device__ inline int os3_merge(int i1, int n1, int n2, const int* match12, const uint8_t* inlier,
                                         const int* found12, const int* found21, Taken taken, int* bad) {
  if (os3_kept(match12, inlier, i1)) {
    if (match12[i1] >= n2) {
      *bad |= 1;
      return -1;
    }
    return match12[i1];
  }
  if (!found12) return -1;
  const int i2 = found12[i1];
  if (i2 < 0) return -1;
  if (i2 >= n2) {
    *bad |= 1;
    return -1;
  }
  if (taken(i2)) return -1;
  const int back = found21[i2];
  if (back >= n1) {
    *bad |= 1;
    return -1;
  }
  return back == i1 ? i2 : -1;
}

// g2o::Sim3(Matrix3d, Vector3d, double) of floats: LoopClosing.cc:364, :372
__host__ __device__ inline void os3_from_float(float s, const float* R, int stride, const float* t, int tstride,
                                               Os3Est* S) {
  double Rd[9];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) Rd[3 * r + c] = (double)R[stride * r + c];
    S->t[r] = (double)t[tstride * r];
  }
  po_quat_from_R(Rd, S->q);
  S->s = (double)s;
}

// Sim3(const Vector7d& update): update = [omega, upsilon, sigma]
__host__ __device__ inline void os3_exp(const double* u, Os3Est* S) {
  const double o0 = u[0], o1 = u[1], o2 = u[2], sigma = u[6];
  const double theta = pm_dsqrt(o0 * o0 + o1 * o1 + o2 * o2);
  const double Om[9] = {0.0, -o2, o1, o2, 0.0, -o0, -o1, o0, 0.0};  // skew(omega)
  double Om2[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
      Om2[3 * r + c] = Om[3 * r] * Om[c] + Om[3 * r + 1] * Om[3 + c] + Om[3 * r + 2] * Om[6 + c];
  const double s = exp(sigma);
  const double eps = 0.00001;
  double A, B, C, ra = 1.0, rb = 1.0;  // R = I + ra Omega + rb Omega2
  if (fabs(sigma) < eps) {
    C = 1;
    if (theta < eps) {
      A = 1. / 2.;
      B = 1. / 6.;
    } else {
      const double theta2 = theta * theta;
      A = (1 - cos(theta)) / (theta2);
      B = (theta - sin(theta)) / (theta2 * theta);
      ra = sin(theta) / theta;
      rb = (1 - cos(theta)) / (theta * theta);
    }
  } else {
    C = (s - 1) / sigma;
    if (theta < eps) {
      const double sigma2 = sigma * sigma;
      A = ((sigma - 1) * s + 1) / sigma2;
      B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
    } else {
      ra = sin(theta) / theta;
      rb = (1 - cos(theta)) / (theta * theta);
      const double a = s * sin(theta);
      const double b = s * cos(theta);
      const double theta2 = theta * theta;
      const double sigma2 = sigma * sigma;
      const double c = theta2 + sigma2;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
    }
  }
  double R[9], W[9];
  const bool small = theta < eps;  // R = I + Omega + Omega*Omega without the factors
  for (int k = 0; k < 9; ++k) {
    const double I = (k % 4 == 0) ? 1.0 : 0.0;
    R[k] = small ? I + Om[k] + Om2[k] : I + ra * Om[k] + rb * Om2[k];
    W[k] = A * Om[k] + B * Om2[k] + C * I;
  }
  po_quat_from_R(R, S->q);
  for (int r = 0; r < 3; ++r) S->t[r] = W[3 * r] * u[3] + W[3 * r + 1] * u[4] + W[3 * r + 2] * u[5];
  S->s = s;
}

// Sim3::operator*: r = a.r*b.r, t = a.s*(a.r*b.t) + a.t, s = a.s*b.s
__host__ __device__ inline void os3_mul(const Os3Est& a, const Os3Est& b, Os3Est* o) {
  double rt[3], q[4];
  po_rotate(a.q, b.t, rt);
  po_qmul(a.q, b.q, q);
  for (int r = 0; r < 3; ++r) o->t[r] = a.s * rt[r] + a.t[r];
  for (int r = 0; r < 4; ++r) o->q[r] = q[r];
  o->s = a.s * b.s;
}

// VertexSim3Expmap::oplusImpl: update[6] = 0 under _fix_scale, estimate = Sim3(update) * estimate
__host__ __device__ inline void os3_oplus(const double* x, bool fix_scale, Os3Est* est) {
  const double u[7] = {x[0], x[1], x[2], x[3], x[4], x[5], fix_scale ? 0.0 : x[6]};
  Os3Est e, o;
  os3_exp(u, &e);
  os3_mul(e, *est, &o);
  *est = o;
}
template <class Ctx>
__host__ __device__ inline void lm_oplus(Ctx& ctx, const double* x, Os3Est* est) {
  os3_oplus(x, ctx.fix_scale, est);
}

// Sim3::inverse: (r*, r* * ((-1/s) t), 1/s)
__host__ __device__ inline void os3_inverse(const Os3Est& S, Os3Est* I) {
  I->q[0] = -S.q[0];
  I->q[1] = -S.q[1];
  I->q[2] = -S.q[2];
  I->q[3] = S.q[3];
  const double a = -1. / S.s;
  const double v[3] = {a * S.t[0], a * S.t[1], a * S.t[2]};
  po_rotate(I->q, v, I->t);
  I->s = 1. / S.s;
}

// The estimates linearizeOplus visits for column k >> 1: oplus(+delta) for even
// k, oplus(-delta) for odd k, delta = 1e-9, each applied to a copy of `est`
// (push / pop); and the inverse EdgeInverseSim3ProjectXYZ::computeError takes.
__host__ __device__ inline void os3_displace(const Os3Est& est, bool fix_scale, int k, Os3Est* fwd, Os3Est* inv) {
  const double d = (k & 1) ? -1e-9 : 1e-9;
  const int col = k >> 1;
  double u[7];
  for (int j = 0; j < 7; ++j) u[j] = (j == col) ? d : 0.0;
  *fwd = est;
  os3_oplus(u, fix_scale, fwd);
  os3_inverse(*fwd, inv);
}

// obs - cam_map(project(S.map(X))): map = s*(r*x) + t, project divides in double
__host__ __device__ inline void os3_error(const Os3Est& S, const float* X, const float* obs, double fx, double fy,
                                          double cx, double cy, double* err) {
  const double Xd[3] = {(double)X[0], (double)X[1], (double)X[2]};
  double r[3];
  po_rotate(S.q, Xd, r);
  const double P0 = S.s * r[0] + S.t[0], P1 = S.s * r[1] + S.t[1], P2 = S.s * r[2] + S.t[2];
  err[0] = (double)obs[0] - (P0 / P2 * fx + cx);
  err[1] = (double)obs[1] - (P1 / P2 * fy + cy);
}
// EdgeSim3ProjectXYZ at S (x1 = S12*X2) and EdgeInverseSim3ProjectXYZ at S.inverse() (x2 = S21*X1)
__host__ __device__ inline void os3_error12(const Os3Cam& c, const Os3Est& S, const Os3Edge& e, double* err) {
  os3_error(S, e.X2, e.obs1, c.fx1, c.fy1, c.cx1, c.cy1, err);
}
__host__ __device__ inline void os3_error21(const Os3Cam& c, const Os3Est& Sinv, const Os3Edge& e, double* err) {
  os3_error(Sinv, e.X1, e.obs2, c.fx2, c.fy2, c.cx2, c.cy2, err);
}

// BaseEdge::chi2 with information = w * I
__host__ __device__ inline double os3_chi2(float wf, const double* err) {
  const double w = (double)wf;
  return err[0] * (w * err[0]) + err[1] * (w * err[1]);
}

// both chi2 of a pair at S (Sinv its inverse)
__host__ __device__ inline void os3_pair_chi2(const Os3Cam& c, const Os3Est& S, const Os3Est& Sinv, const Os3Edge& e,
                                              double* chi12, double* chi21) {
  double err[2];
  os3_error12(c, S, e, err);
  *chi12 = os3_chi2(e.w1, err);
  os3_error21(c, Sinv, e, err);
  *chi21 = os3_chi2(e.w2, err);
}

// the pair's two terms of activeRobustChi2, added to *sum in edge order
__host__ __device__ inline void os3_pair_robust_chi2(const Os3Cam& c, const Os3Huber& K, const Os3Est& S,
                                                     const Os3Est& Sinv, const Os3Edge& e, double* sum) {
  double c12, c21, r0, r1;
  os3_pair_chi2(c, S, Sinv, e, &c12, &c21);
  lm_huber(K.delta, K.dsqr, c12, &r0, &r1);
  *sum += r0;
  lm_huber(K.delta, K.dsqr, c21, &r0, &r1);
  *sum += r0;
}

// constructQuadraticForm of one 2 x 7 edge (the point vertex is fixed): with
// rho from the Huber kernel, H += J^T (rho1 w) J, omega_r = -(w e) rho1 and
// b += J^T omega_r (acc holds -b), and the edge's robust chi2. J[0..6] is row
// 0, J[7..13] row 1.
__host__ __device__ inline void os3_quadratic_form(const Os3Huber& K, float wf, const double* err, const double* J,
                                                   double* acc) {
  const double w = (double)wf;
  double rho0, rho1;
  lm_huber(K.delta, K.dsqr, os3_chi2(wf, err), &rho0, &rho1);
  acc[kOs3Chi] += rho0;
  const double rw = rho1 * w;
  const double r0 = (w * err[0]) * rho1, r1 = (w * err[1]) * rho1;
  int k = 0;
#pragma unroll
  for (int r = 0; r < 7; ++r) {
    const double a0 = J[r] * rw, a1 = J[7 + r] * rw;
#pragma unroll
    for (int col = r; col < 7; ++col, ++k) acc[k] += a0 * J[col] + a1 * J[7 + col];
    acc[kOs3B + r] += J[r] * r0 + J[7 + r] * r1;
  }
}

// Keeps the device compiler from loading a later column's displaced estimates
// (28 x 8 doubles in LDS) before the current column is done, or all of them
// ahead of the loop over the pairs: that hoisting cost 1.3 KB of scratch per lane.
#if defined(__HIP_DEVICE_COMPILE__)
#define ORBX_OS3_LOAD_FENCE() asm volatile("" ::: "memory")
#else
#define ORBX_OS3_LOAD_FENCE()
#endif

// computeError, linearizeOplus and constructQuadraticForm of the pair's two
// edges at S, e12 first. D[4*col + 2*sign + {0, 1}]: os3_displace's estimates
// and inverses. Each Jacobian column is scalar * (error(+delta) -
// error(-delta)), scalar = 1 / (2 delta) (base_binary_edge.hpp:147-196); the
// edge's own error is the one at S (errorBeforeNumeric).
__host__ __device__ inline void os3_pair_linearise(const Os3Cam& c, const Os3Huber& K, const Os3Est& S,
                                                   const Os3Est& Sinv, const Os3Est* D, const Os3Edge& e,
                                                   double* acc) {
  const double delta = 1e-9;
  const double scalar = 1.0 / (2 * delta);
  double err[2], J[14], ep[2], em[2];
  os3_error12(c, S, e, err);
#pragma unroll
  for (int d = 0; d < 7; ++d) {
    ORBX_OS3_LOAD_FENCE();
    os3_error12(c, D[4 * d], e, ep);
    os3_error12(c, D[4 * d + 2], e, em);
    J[d] = scalar * (ep[0] - em[0]);
    J[7 + d] = scalar * (ep[1] - em[1]);
  }
  os3_quadratic_form(K, e.w1, err, J, acc);
  os3_error21(c, Sinv, e, err);
#pragma unroll
  for (int d = 0; d < 7; ++d) {
    ORBX_OS3_LOAD_FENCE();
    os3_error21(c, D[4 * d + 1], e, ep);
    os3_error21(c, D[4 * d + 3], e, em);
    J[d] = scalar * (ep[0] - em[0]);
    J[7 + d] = scalar * (ep[1] - em[1]);
  }
  os3_quadratic_form(K, e.w2, err, J, acc);
}

// `e12->chi2() > th2 || e21->chi2() > th2`: double against the widened float, no cast
__host__ __device__ inline bool os3_is_outlier(const Os3Huber& K, double chi12, double chi21) {
  return chi12 > K.th2 || chi21 > K.th2;
}

struct Os3Stats {
  int ret, n_bad, rounds, more_iterations, trials, rejected;
};

// Optimizer::OptimizeSim3 from :1325 on, over n_corr edge pairs. Ctx supplies
//   bool fix_scale
//   void linearise(const Os3Est&, bool, double acc[kOs3Sums])  the sums of os3_pair_linearise
//   double robust_chi2(const Os3Est&, bool)                    the sum of os3_pair_robust_chi2
// over the pairs not marked kOs3Removed, and
//   int classify(const Os3Est& err_est, uint32_t mark)
// which marks each such pair whose chi2 at err_est (the _error the last
// computeActiveErrors left: no fresh computeError precedes chi2()) is above
// th2 and returns their number. *out is S0 when the function returns 0 at
// :1355, before g2oS12 is written. On the device every thread of the workgroup
// runs this with the same values.
// Both optimisations go through one call site, so the kernel holds the
// linearisation once; inlined, so the context stays in registers.
template <class Ctx>
__host__ __device__ __attribute__((always_inline)) inline void os3_run(Ctx& ctx, const Os3Est& S0, int n_corr,
                                                                        Os3Est* out, Os3Stats* st) {
  Os3Est est = S0, err_est = S0;
  st->trials = st->rejected = 0;
  st->ret = st->n_bad = st->rounds = 0;
  st->more_iterations = 5;
  *out = S0;
  for (int round = 0; round < 2; ++round) {
    if (n_corr > 0)  // else optimize() finds no active vertex and returns
      lm_optimize<7>(ctx, round == 0 ? 5 : st->more_iterations, true, &est, &err_est, &st->trials, &st->rejected);
    ++st->rounds;
    const int bad = ctx.classify(err_est, round == 0 ? kOs3Removed : kOs3Rejected);
    if (round == 0) {
      st->n_bad = bad;
      st->more_iterations = bad > 0 ? 10 : 5;
      if (n_corr - bad < 10) return;  // :1355
    } else {
      st->ret = n_corr - st->n_bad - bad;
      *out = est;
    }
  }
}

// mg2oScw = gScm * gSmw with gSmw = Sim3(R2w, t2w, 1.0), then rows 0..2 of
// Converter::toCvMat(Sim3): [s * toRotationMatrix | t] rounded to float
// (src/LoopClosing.cc:372-374, src/Converter.cc:55-61, :92-108)
__host__ __device__ inline void os3_scw(const Os3Est& S12, const float* T2w, float* Scw) {
  Os3Est M, P;
  os3_from_float(1.0f, T2w, 4, T2w + 3, 4, &M);
  os3_mul(S12, M, &P);
  double R[9];
  po_to_R(P.q, R);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) Scw[4 * r + c] = pm_d2f(P.s * R[3 * r + c]);
    Scw[4 * r + 3] = pm_d2f(P.t[r]);
  }
}

// orbm_prepare_pose(ORBM_PROJ_SIM3, cam1 with Tcw = Scw)
__host__ __device__ inline void os3_pose(const orbm_camera& cam1, const float* Scw, orbm_pose* p) {
  float Rt[12];
  rt_from_scw(Scw, Rt);
  pose_from_rt(cam1, Rt, p);
}

__host__ __device__ inline orbm_optsim3_result os3_result(const Os3Stats& st, int n_corr) {
  orbm_optsim3_result r;
  r.ret = st.ret;
  r.n_corr = n_corr;
  r.n_bad = st.n_bad;
  r.rounds = st.rounds;
  r.more_iterations = st.more_iterations;
  r.trials = st.trials;
  r.rejected = st.rejected;
  r.reserved = 0;
  return r;
}

// lin[36]: the upper triangle of H, b and the robust chi2 of a linearisation
__host__ __device__ inline void os3_store_lin(const double* acc, double* lin) {
  for (int k = 0; k < kOs3B; ++k) lin[k] = acc[k];
  for (int k = kOs3B; k < kOs3Chi; ++k) lin[k] = -acc[k];
  lin[kOs3Chi] = acc[kOs3Chi];
}

}  // namespace orbx
