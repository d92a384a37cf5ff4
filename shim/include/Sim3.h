// g2o::Sim3 as Optimizer::OptimizeSim3's signature needs it: a quaternion r
// (x, y, z, w), a translation t and a scale s in double, with the product,
// map and inverse of g2o's types/sim3.h. A build with g2o uses g2o's own class
// (over Eigen); this one stands alone, with plain arrays.
//
// Sim3(R, t, s) keeps the matrix it was built from beside the quaternion:
// LoopClosing builds gScm from the solver's float R (src/LoopClosing.cc:364),
// and liborbx takes the estimate as those floats, so the way back must be exact.
#ifndef ORBX_SHIM_SIM3_H
#define ORBX_SHIM_SIM3_H
#include <cmath>

namespace g2o {

struct Sim3 {
  double r[4] = {0, 0, 0, 1}, t[3] = {0, 0, 0}, s = 1.0;
  bool has_matrix = false;
  double R0[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};  // row-major, with has_matrix

  Sim3() {}
  Sim3(const double q[4], const double t_[3], double s_) : s(s_) {
    for (int k = 0; k < 4; ++k) r[k] = q[k];
    for (int k = 0; k < 3; ++k) t[k] = t_[k];
  }
  // g2o's Sim3(const Matrix3d& R, const Vector3d& t, double s), R row-major: r = Eigen::Quaterniond(R)
  // (Shoemake), not normalised. A named constructor: arrays of 4 and of 9 doubles are one parameter type.
  static Sim3 fromMatrix(const double R[9], const double t_[3], double s_) {
    Sim3 S;
    S.set_matrix(R, t_, s_);
    return S;
  }

 private:
  void set_matrix(const double R[9], const double t_[3], double s_) {
    s = s_;
    has_matrix = true;
    for (int k = 0; k < 9; ++k) R0[k] = R[k];
    for (int k = 0; k < 3; ++k) t[k] = t_[k];
    double tr = R[0] + R[4] + R[8];
    if (tr > 0.0) {
      tr = std::sqrt(tr + 1.0);
      r[3] = 0.5 * tr;
      tr = 0.5 / tr;
      r[0] = (R[7] - R[5]) * tr;
      r[1] = (R[2] - R[6]) * tr;
      r[2] = (R[3] - R[1]) * tr;
    } else {
      int i = 0;
      if (R[4] > R[0]) i = 1;
      if (R[8] > R[4 * i]) i = 2;
      const int j = (i + 1) % 3, k = (j + 1) % 3;
      tr = std::sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0);
      r[i] = 0.5 * tr;
      tr = 0.5 / tr;
      r[3] = (R[3 * k + j] - R[3 * j + k]) * tr;
      r[j] = (R[3 * j + i] + R[3 * i + j]) * tr;
      r[k] = (R[3 * k + i] + R[3 * i + k]) * tr;
    }
  }

 public:
  const double* rotation() const { return r; }
  const double* translation() const { return t; }
  double scale() const { return s; }

  // Quaterniond::toRotationMatrix, row-major
  void rotationMatrix(double R[9]) const {
    const double tx = 2.0 * r[0], ty = 2.0 * r[1], tz = 2.0 * r[2];
    const double twx = tx * r[3], twy = ty * r[3], twz = tz * r[3];
    const double txx = tx * r[0], txy = ty * r[0], txz = tz * r[0];
    const double tyy = ty * r[1], tyz = tz * r[1], tzz = tz * r[2];
    R[0] = 1.0 - (tyy + tzz), R[1] = txy - twz, R[2] = txz + twy;
    R[3] = txy + twz, R[4] = 1.0 - (txx + tzz), R[5] = tyz - twx;
    R[6] = txz - twy, R[7] = tyz + twx, R[8] = 1.0 - (txx + tyy);
  }

  // s*(r*xyz) + t
  void map(const double xyz[3], double out[3]) const {
    double v[3];
    rotate(r, xyz, v);
    for (int k = 0; k < 3; ++k) out[k] = s * v[k] + t[k];
  }

  // (r*, r* * ((-1/s) t), 1/s)
  Sim3 inverse() const {
    const double q[4] = {-r[0], -r[1], -r[2], r[3]};
    const double a = -1. / s, v[3] = {a * t[0], a * t[1], a * t[2]};
    double ti[3];
    rotate(q, v, ti);
    return Sim3(q, ti, 1. / s);
  }

  // neither normalised nor flipped, as g2o's
  Sim3 operator*(const Sim3& o) const {
    Sim3 ret;
    ret.r[3] = r[3] * o.r[3] - r[0] * o.r[0] - r[1] * o.r[1] - r[2] * o.r[2];
    ret.r[0] = r[3] * o.r[0] + r[0] * o.r[3] + r[1] * o.r[2] - r[2] * o.r[1];
    ret.r[1] = r[3] * o.r[1] + r[1] * o.r[3] + r[2] * o.r[0] - r[0] * o.r[2];
    ret.r[2] = r[3] * o.r[2] + r[2] * o.r[3] + r[0] * o.r[1] - r[1] * o.r[0];
    double v[3];
    rotate(r, o.t, v);
    for (int k = 0; k < 3; ++k) ret.t[k] = s * v[k] + t[k];
    ret.s = s * o.s;
    return ret;
  }

 private:
  // Quaterniond * Vector3d
  static void rotate(const double q[4], const double v[3], double o[3]) {
    double u0 = q[1] * v[2] - q[2] * v[1], u1 = q[2] * v[0] - q[0] * v[2], u2 = q[0] * v[1] - q[1] * v[0];
    u0 += u0, u1 += u1, u2 += u2;
    o[0] = v[0] + q[3] * u0 + (q[1] * u2 - q[2] * u1);
    o[1] = v[1] + q[3] * u1 + (q[2] * u0 - q[0] * u2);
    o[2] = v[2] + q[3] * u2 + (q[0] * u1 - q[1] * u0);
  }
};

}  // namespace g2o
#endif
