// orbx_initializer.cuh — Initializer (src/Initializer.cc) restated operation by
// operation for the kernels (orbx_initializer.hip) and the host form alike:
// RandomInt and the eight draws without replacement (:82-97), Normalize
// (:749-795), ComputeH21 / ComputeF21 (:226-303) with cv::SVDecomp's
// JacobiSVDImpl_<float> for a general m x n and its FULL_UV fill, the two
// score terms of CheckHomography / CheckFundamental (:305-468), the model
// choice (:112-118), DecomposeE (:909-929), ReconstructF / ReconstructH's
// candidates and acceptance rules (:470-732), Triangulate (:734-747) and
// CheckRT (:798-907). Every float and double operation is one explicitly
// rounded pm_* call (orbx_posemath.cuh), so host and device differ only where
// libm's acosf and the device's do. Work arrays whose indices are run-time
// values are addressed as base[word * stride]: stride 1 on the host, the lane
// count of an LDS image laid out [word][lane] on the device. The OpenCV
// conventions are those of DESIGN.md section 3, "Initializer", UNPINNED.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "orbx_newpoints.cuh"  // np_hypot, np_svd4_last_row; pm_* and pm_fsqrt / pm_dsub through it

namespace orbx {

constexpr int kStatusInitSkipped = 4096;  // matcher status bit: a matches12 value at or above n2 was left out
constexpr int kInitzMaxIts = 1024;        // cap of orbm_init_params.max_iterations
constexpr int kInitzChunk = 16;           // hypotheses per workgroup of the solve-and-score kernel
constexpr int kInitzSvdFloats = 225;      // float words of one hypothesis's SVD work area (9x16 At + 9x9 Vt)
constexpr int kInitzSvdDoubles = 9;       // its squared row norms

// reason codes (include/orbx_c.h, ORBM_INIT_*)
enum : int {
  kIzTooFewMatches = 1,
  kIzNoScore = 2,
  kIzDegenerate = 3,
  kIzNoClearWinner = 4,
  kIzTooFewPoints = 5,
  kIzLowParallax = 6,
  kIzAccepted = 7,
};
enum : int { kIzModelNone = 0, kIzModelH = 1, kIzModelF = 2 };

// DUtils::Random::RandomInt(0, d - 1) of the raw rand() value r
// (Thirdparty/DBoW2/DUtils/Random.cpp:47-50): int(((double)r / ((double)RAND_MAX
// + 1.0)) * d). The quotient is exact (RAND_MAX + 1 = 2^31). A value above
// RAND_MAX (no rand() result) is clamped; so is a product that rounds up to d
// (d >= 2^22 only). d >= 1.
__host__ __device__ inline int iz_random_int(uint32_t r, int d) {
  if (r > kSim3RandMax) r = kSim3RandMax;
  const int v = (int)pm_dmul(pm_ddiv((double)r, 2147483648.0), (double)d);
  return v < d ? v : d - 1;
}

// The eight draws without replacement on vAvailableIndices (:84-96): take
// [randi], move back() into the hole, pop. The list starts as the identity of
// length N >= 8; draw j leaves override j (slot randi now holds what back()
// held), and a slot's latest override is the one that counts.
__host__ __device__ inline void iz_draw(const uint32_t* r8, int N, int* idx) {
  int pos[8], val[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int size = N - j;
    const int randi = iz_random_int(r8[j], size);
    int v = randi, back = size - 1;
#pragma unroll
    for (int k = 0; k < j; ++k) {
      v = pos[k] == randi ? val[k] : v;
      back = pos[k] == size - 1 ? val[k] : back;
    }
    idx[j] = v;
    pos[j] = randi;
    val[j] = back;
  }
}

// one float addition of a running sum, for host loops and kernels alike
__host__ __device__ inline float iz_fadd(float a, float b) { return pm_fadd(a, b); }

// Normalize (:749-795): the float sums run in index order (the caller's
// loops); these are the steps between and after them.
struct IzNorm {
  float mx, my, sx, sy;
};
__host__ __device__ inline float iz_norm_mean(float sum, int n) { return pm_fdiv(sum, (float)n); }  // :763-764, :778-779
__host__ __device__ inline float iz_norm_dev(float v, float mean) { return fabsf(pm_fsub(v, mean)); }  // :771-775
__host__ __device__ inline float iz_norm_scale(float mean_dev) { return pm_d2f(pm_ddiv(1.0, (double)mean_dev)); }  // :781-782
__host__ __device__ inline void iz_norm_T(const IzNorm& n, float* T) {  // :790-794
  T[0] = n.sx, T[1] = 0.0f, T[2] = pm_fmul(-n.mx, n.sx);
  T[3] = 0.0f, T[4] = n.sy, T[5] = pm_fmul(-n.my, n.sy);
  T[6] = 0.0f, T[7] = 0.0f, T[8] = 1.0f;
}
__host__ __device__ inline float iz_norm_pt(float v, float mean, float s) { return pm_fmul(pm_fsub(v, mean), s); }  // :771-772, :786-787

// ---------------------------------------------------------------- small matrices
// d = (float)(t*alpha + c*beta) of gemm's small-matrix path without C: c is a
// zero buffer, beta 0 (a -0 sum comes out as +0)
__host__ __device__ inline float iz_gemm_out(float t, double alpha) {
  return pm_d2f(pm_dadd(pm_dmul((double)t, alpha), 0.0));
}
__host__ __device__ inline float iz_dot3f(float a0, float b0, float a1, float b1, float a2, float b2) {
  return pm_fadd(pm_fadd(pm_fmul(a0, b0), pm_fmul(a1, b1)), pm_fmul(a2, b2));
}
// D = alpha*A*B, 3x3 row-major, gemm's small-matrix path (flags == 0): float dot products left to right
__host__ __device__ inline void iz_mul33(const float* A, const float* B, double alpha, float* D) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      D[3 * i + j] = iz_gemm_out(iz_dot3f(A[3 * i], B[j], A[3 * i + 1], B[3 + j], A[3 * i + 2], B[6 + j]), alpha);
}
// d = A*b, 3x3 by 3x1, the same path
__host__ __device__ inline void iz_mul31(const float* A, const float* b, float* d) {
#pragma unroll
  for (int i = 0; i < 3; ++i) d[i] = iz_gemm_out(iz_dot3f(A[3 * i], b[0], A[3 * i + 1], b[1], A[3 * i + 2], b[2]), 1.0);
}
// D = A.t()*B (TA) or A*B.t() (!TA): a transposed operand takes gemm's general
// path, double accumulation from 0 in k order, one rounding of s*alpha
template <bool TA>
__host__ __device__ inline void iz_mul33_t(const float* A, const float* B, float* D) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k)
        s = pm_dadd(s, pm_dmul((double)(TA ? A[3 * k + i] : A[3 * i + k]), (double)(TA ? B[3 * k + j] : B[3 * j + k])));
      D[3 * i + j] = pm_d2f(pm_dmul(s, 1.0));
    }
}
// lapack.cpp's det3: double throughout
__host__ __device__ inline double iz_det3(const float* m) {
  const double a = pm_dmul((double)m[0], pm_dsub(pm_dmul((double)m[4], (double)m[8]), pm_dmul((double)m[5], (double)m[7])));
  const double b = pm_dmul((double)m[1], pm_dsub(pm_dmul((double)m[3], (double)m[8]), pm_dmul((double)m[5], (double)m[6])));
  const double c = pm_dmul((double)m[2], pm_dsub(pm_dmul((double)m[3], (double)m[7]), pm_dmul((double)m[4], (double)m[6])));
  return pm_dadd(pm_dsub(a, b), c);
}
// cv::invert of a 3x3 CV_32F (DECOMP_LU): the closed form for n = 3, the
// determinant and the cofactors in double, one rounding per element; a zero
// determinant gives the zero matrix
__host__ __device__ inline bool iz_invert3(const float* S, float* D) {
  double d = iz_det3(S);
  if (d == 0.0) {
#pragma unroll
    for (int k = 0; k < 9; ++k) D[k] = 0.0f;
    return false;
  }
  d = pm_ddiv(1.0, d);
#define ORBX_IZ_COF(a, b, c, e) pm_d2f(pm_dmul(pm_dsub(pm_dmul((double)S[a], (double)S[b]), pm_dmul((double)S[c], (double)S[e])), d))
  D[0] = ORBX_IZ_COF(4, 8, 5, 7);
  D[1] = ORBX_IZ_COF(2, 7, 1, 8);
  D[2] = ORBX_IZ_COF(1, 5, 2, 4);
  D[3] = ORBX_IZ_COF(5, 6, 3, 8);
  D[4] = ORBX_IZ_COF(0, 8, 2, 6);
  D[5] = ORBX_IZ_COF(2, 3, 0, 5);
  D[6] = ORBX_IZ_COF(3, 7, 4, 6);
  D[7] = ORBX_IZ_COF(1, 6, 0, 7);
  D[8] = ORBX_IZ_COF(0, 4, 1, 3);
#undef ORBX_IZ_COF
  return true;
}
// cv::norm (NORM_L2) of 3 floats as the double it returns
__host__ __device__ inline double iz_norm3d(float a, float b, float c) {
  return pm_dsqrt(pm_dadd(pm_dadd(pm_dmul((double)a, (double)a), pm_dmul((double)b, (double)b)), pm_dmul((double)c, (double)c)));
}
// t / cv::norm(t) (:637, :915): a convertTo with the float scale 1/norm
__host__ __device__ inline void iz_unit3(const float* t, float* o) {
  const float a = pm_d2f(pm_ddiv(1.0, iz_norm3d(t[0], t[1], t[2])));
#pragma unroll
  for (int k = 0; k < 3; ++k) o[k] = pm_fadd(pm_fmul(t[k], a), 0.0f);
}

// ---------------------------------------------------------------- JacobiSVDImpl_<float>
// OpenCV 3.x modules/core/src/lapack.cpp on At: N rows of length M (the
// transposed input, or the input itself when it has fewer rows than columns),
// Vt N x N when HAS_V, W the squared row norms in double. Element (i, k) of At
// is At[(i*M + k)*s]. On return the rows are sorted by descending singular
// value (W holds them) and At's rows and Vt's rows are swapped with them.
template <int M, int N, bool HAS_V>
__host__ __device__ inline void iz_jacobi_svd(float* At, float* Vt, double* W, int s) {
  const double eps = 2.384185791015625e-07;  // (float)(FLT_EPSILON*2) as the _Tp eps argument
#pragma unroll 1
  for (int i = 0; i < N; ++i) {
    double sd = 0;
    for (int k = 0; k < M; ++k) {
      const float t = At[(i * M + k) * s];
      sd = pm_dadd(sd, pm_dmul((double)t, (double)t));
    }
    W[i * s] = sd;
    if (HAS_V)
      for (int k = 0; k < N; ++k) Vt[(i * N + k) * s] = i == k ? 1.0f : 0.0f;
  }
#pragma unroll 1
  for (int iter = 0; iter < (M > 30 ? M : 30); ++iter) {
    bool changed = false;
#pragma unroll 1
    for (int i = 0; i < N - 1; ++i)
#pragma unroll 1
      for (int j = i + 1; j < N; ++j) {
        float* Ai = At + (size_t)i * M * s;
        float* Aj = At + (size_t)j * M * s;
        double a = W[i * s], p = 0, b = W[j * s];
        for (int k = 0; k < M; ++k) p = pm_dadd(p, pm_dmul((double)Ai[k * s], (double)Aj[k * s]));
        if (fabs(p) <= pm_dmul(eps, pm_dsqrt(pm_dmul(a, b)))) continue;
        p = pm_dmul(p, 2.0);
        const double beta = pm_dsub(a, b), gamma = np_hypot(p, beta);
        float c, sn;
        if (beta < 0) {
          const double delta = pm_dmul(pm_dsub(gamma, beta), 0.5);
          sn = pm_d2f(pm_dsqrt(pm_ddiv(delta, gamma)));
          c = pm_d2f(pm_ddiv(p, pm_dmul(pm_dmul(gamma, (double)sn), 2.0)));
        } else {
          c = pm_d2f(pm_dsqrt(pm_ddiv(pm_dadd(gamma, beta), pm_dmul(gamma, 2.0))));
          sn = pm_d2f(pm_ddiv(p, pm_dmul(pm_dmul(gamma, (double)c), 2.0)));
        }
        a = b = 0;
        for (int k = 0; k < M; ++k) {
          const float x = Ai[k * s], y = Aj[k * s];
          const float t0 = pm_fadd(pm_fmul(c, x), pm_fmul(sn, y));
          const float t1 = pm_fadd(pm_fmul(-sn, x), pm_fmul(c, y));
          Ai[k * s] = t0;
          Aj[k * s] = t1;
          a = pm_dadd(a, pm_dmul((double)t0, (double)t0));
          b = pm_dadd(b, pm_dmul((double)t1, (double)t1));
        }
        W[i * s] = a;
        W[j * s] = b;
        changed = true;
        if (HAS_V) {
          float* Vi = Vt + (size_t)i * N * s;
          float* Vj = Vt + (size_t)j * N * s;
          for (int k = 0; k < N; ++k) {
            const float x = Vi[k * s], y = Vj[k * s];
            Vi[k * s] = pm_fadd(pm_fmul(c, x), pm_fmul(sn, y));
            Vj[k * s] = pm_fadd(pm_fmul(-sn, x), pm_fmul(c, y));
          }
        }
      }
    if (!changed) break;
  }
#pragma unroll 1
  for (int i = 0; i < N; ++i) {
    double sd = 0;
    for (int k = 0; k < M; ++k) {
      const float t = At[(i * M + k) * s];
      sd = pm_dadd(sd, pm_dmul((double)t, (double)t));
    }
    W[i * s] = pm_dsqrt(sd);
  }
#pragma unroll 1
  for (int i = 0; i < N - 1; ++i) {
    int j = i;
    for (int k = i + 1; k < N; ++k)
      if (W[j * s] < W[k * s]) j = k;
    if (i != j) {
      const double w = W[i * s];
      W[i * s] = W[j * s];
      W[j * s] = w;
      for (int k = 0; k < M; ++k) {
        const float t = At[(i * M + k) * s];
        At[(i * M + k) * s] = At[(j * M + k) * s];
        At[(j * M + k) * s] = t;
      }
      if (HAS_V)
        for (int k = 0; k < N; ++k) {
          const float t = Vt[(i * N + k) * s];
          Vt[(i * N + k) * s] = Vt[(j * N + k) * s];
          Vt[(j * N + k) * s] = t;
        }
    }
  }
}

// The tail of JacobiSVDImpl_ over the n1 = N1 rows of the left factor (At has
// room for N1 rows): a row whose singular value is <= FLT_MIN, and every row
// from N on, is filled from RNG(0x12345678) with +-1/M, orthogonalised twice
// against the rows before it (L1 renormalisation after each) and divided by
// its 2-norm, in up to 100 attempts; every row is scaled by 1/W.
template <int M, int N, int N1>
__host__ __device__ inline void iz_svd_fill(float* At, const double* W, int s) {
  const double minval = 1.17549435082228750797e-38;  // FLT_MIN
  const float eps100 = pm_fmul(2.384185791015625e-07f, 100.0f);
  uint64_t state = 0x12345678u;
#pragma unroll 1
  for (int i = 0; i < N1; ++i) {
    float* Ai = At + (size_t)i * M * s;
    double sd = i < N ? W[i * s] : 0.0;
#pragma unroll 1
    for (int ii = 0; ii < 100 && sd <= minval; ++ii) {
      const float val0 = pm_d2f(pm_ddiv(1.0, (double)M));
      for (int k = 0; k < M; ++k) {
        state = (uint64_t)(uint32_t)state * 4164903690u + (uint32_t)(state >> 32);  // RNG::next
        Ai[k * s] = ((uint32_t)state & 256u) != 0 ? val0 : -val0;
      }
#pragma unroll 1
      for (int iter = 0; iter < 2; ++iter)
#pragma unroll 1
        for (int j = 0; j < i; ++j) {
          const float* Aj = At + (size_t)j * M * s;
          sd = 0;
          for (int k = 0; k < M; ++k) sd = pm_dadd(sd, (double)pm_fmul(Ai[k * s], Aj[k * s]));
          float asum = 0;
          for (int k = 0; k < M; ++k) {
            const float t = pm_d2f(pm_dsub((double)Ai[k * s], pm_dmul(sd, (double)Aj[k * s])));
            Ai[k * s] = t;
            asum = pm_fadd(asum, fabsf(t));
          }
          asum = asum > eps100 ? pm_fdiv(1.0f, asum) : 0.0f;
          for (int k = 0; k < M; ++k) Ai[k * s] = pm_fmul(Ai[k * s], asum);
        }
      sd = 0;
      for (int k = 0; k < M; ++k) {
        const float t = Ai[k * s];
        sd = pm_dadd(sd, pm_dmul((double)t, (double)t));
      }
      sd = pm_dsqrt(sd);
    }
    const float sc = pm_d2f(sd > minval ? pm_ddiv(1.0, sd) : 0.0);
    for (int k = 0; k < M; ++k) Ai[k * s] = pm_fmul(Ai[k * s], sc);
  }
}

// cv::SVDecomp / cv::SVD::compute of a 3x3 CV_32F matrix M (row-major) with
// u, w, vt: a square matrix runs on its transpose and FULL_UV adds no rows.
// Work: 18 floats at F and 3 doubles at W, strided by s.
__host__ __device__ inline void iz_svd3(const float* M, float* F, double* W, int s, float* w, float* u, float* vt) {
  float* At = F;
  float* Vt = F + 9 * s;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) At[(i * 3 + k) * s] = M[3 * k + i];
  iz_jacobi_svd<3, 3, true>(At, Vt, W, s);
#pragma unroll
  for (int i = 0; i < 3; ++i) w[i] = pm_d2f(W[i * s]);
  iz_svd_fill<3, 3, 3>(At, W, s);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      u[3 * k + i] = At[(i * 3 + k) * s];  // u = temp_u.t()
      vt[3 * i + k] = Vt[(i * 3 + k) * s];
    }
}

// ---------------------------------------------------------------- the two solves
// ComputeH21 (:226-266) of eight normalised pairs and :160-161: H21i =
// T2inv*Hn*T1, H12i = H21i.inv(). The 16x9 system runs as At = 9 rows of 16;
// vt is V, so vt.row(8) is the Jacobi output and the fill, which touches only
// u, is left out. Work: kInitzSvdFloats floats, kInitzSvdDoubles doubles.
__host__ __device__ inline void iz_solve_h(const float* x1, const float* y1, const float* x2, const float* y2,
                                           const float* T1, const float* T2inv, float* F, double* W, int s, float* H21,
                                           float* H12) {
  float* At = F;
  float* Vt = F + 144 * s;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float u1 = x1[i], v1 = y1[i], u2 = x2[i], v2 = y2[i];
    const float r0[9] = {0.0f, 0.0f, 0.0f, -u1, -v1, -1.0f, pm_fmul(v2, u1), pm_fmul(v2, v1), v2};
    const float r1[9] = {u1, v1, 1.0f, 0.0f, 0.0f, 0.0f, pm_fmul(-u2, u1), pm_fmul(-u2, v1), -u2};
#pragma unroll
    for (int c = 0; c < 9; ++c) {
      At[(c * 16 + 2 * i) * s] = r0[c];
      At[(c * 16 + 2 * i + 1) * s] = r1[c];
    }
  }
  iz_jacobi_svd<16, 9, true>(At, Vt, W, s);
  float Hn[9], tmp[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) Hn[k] = Vt[(72 + k) * s];
  iz_mul33(T2inv, Hn, 1.0, tmp);
  iz_mul33(tmp, T1, 1.0, H21);
  iz_invert3(H21, H12);
}

// ComputeF21 (:268-303) and :212: F21i = T2t*Fn*T1. The 8x9 system has fewer
// rows than columns, so it runs as it stands (8 rows of 9) and vt is the left
// factor: its rows 0..7 are the normalised Jacobi rows, row 8 the fill.
__host__ __device__ inline void iz_solve_f(const float* x1, const float* y1, const float* x2, const float* y2,
                                           const float* T1, const float* T2, float* F, double* W, int s, float* F21) {
  float* At = F;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float u1 = x1[i], v1 = y1[i], u2 = x2[i], v2 = y2[i];
    const float r[9] = {pm_fmul(u2, u1), pm_fmul(u2, v1), u2, pm_fmul(v2, u1), pm_fmul(v2, v1), v2, u1, v1, 1.0f};
#pragma unroll
    for (int c = 0; c < 9; ++c) At[(i * 9 + c) * s] = r[c];
  }
#pragma unroll
  for (int c = 0; c < 9; ++c) At[(72 + c) * s] = 0.0f;  // temp_u = Scalar::all(0)
  iz_jacobi_svd<9, 8, false>(At, nullptr, W, s);
  iz_svd_fill<9, 8, 9>(At, W, s);
  float Fpre[9], w[3], u[9], vt[9], D[9], uD[9], Fn[9], T2t[9], tmp[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) Fpre[k] = At[(72 + k) * s];
  iz_svd3(Fpre, F, W, s, w, u, vt);
  w[2] = 0.0f;
#pragma unroll
  for (int k = 0; k < 9; ++k) D[k] = 0.0f;
  D[0] = w[0], D[4] = w[1], D[8] = w[2];
  iz_mul33(u, D, 1.0, uD);
  iz_mul33(uD, vt, 1.0, Fn);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) T2t[3 * i + j] = T2[3 * j + i];
  iz_mul33(T2t, Fn, 1.0, tmp);
  iz_mul33(tmp, T1, 1.0, F21);
}

// ---------------------------------------------------------------- the scores
// invSigmaSquare = 1.0/(sigma*sigma) (:335, :411)
__host__ __device__ inline float iz_inv_sigma2(float sigma) { return pm_d2f(pm_ddiv(1.0, (double)pm_fmul(sigma, sigma))); }

// One match of CheckHomography (:337-385): the two amounts `score +=` adds, in
// order (0 where the term is over the threshold: adding +0 leaves a
// non-negative sum's bits alone), and bIn.
__host__ __device__ inline bool iz_check_h(const float* H21, const float* H12, float invs2, float u1, float v1, float u2,
                                           float v2, float* t1, float* t2) {
  const float th = 5.991f;
  bool bIn = true;
  const float w2in1inv = pm_d2f(pm_ddiv(1.0, (double)pm_fadd(pm_fadd(pm_fmul(H12[6], u2), pm_fmul(H12[7], v2)), H12[8])));
  const float u2in1 = pm_fmul(pm_fadd(pm_fadd(pm_fmul(H12[0], u2), pm_fmul(H12[1], v2)), H12[2]), w2in1inv);
  const float v2in1 = pm_fmul(pm_fadd(pm_fadd(pm_fmul(H12[3], u2), pm_fmul(H12[4], v2)), H12[5]), w2in1inv);
  const float du1 = pm_fsub(u1, u2in1), dv1 = pm_fsub(v1, v2in1);
  const float chi1 = pm_fmul(pm_fadd(pm_fmul(du1, du1), pm_fmul(dv1, dv1)), invs2);
  *t1 = 0.0f;
  if (chi1 > th)
    bIn = false;
  else
    *t1 = pm_fsub(th, chi1);
  const float w1in2inv = pm_d2f(pm_ddiv(1.0, (double)pm_fadd(pm_fadd(pm_fmul(H21[6], u1), pm_fmul(H21[7], v1)), H21[8])));
  const float u1in2 = pm_fmul(pm_fadd(pm_fadd(pm_fmul(H21[0], u1), pm_fmul(H21[1], v1)), H21[2]), w1in2inv);
  const float v1in2 = pm_fmul(pm_fadd(pm_fadd(pm_fmul(H21[3], u1), pm_fmul(H21[4], v1)), H21[5]), w1in2inv);
  const float du2 = pm_fsub(u2, u1in2), dv2 = pm_fsub(v2, v1in2);
  const float chi2 = pm_fmul(pm_fadd(pm_fmul(du2, du2), pm_fmul(dv2, dv2)), invs2);
  *t2 = 0.0f;
  if (chi2 > th)
    bIn = false;
  else
    *t2 = pm_fsub(th, chi2);
  return bIn;
}

// One match of CheckFundamental (:413-465)
__host__ __device__ inline bool iz_check_f(const float* F, float invs2, float u1, float v1, float u2, float v2, float* t1,
                                           float* t2) {
  const float th = 3.841f, thScore = 5.991f;
  bool bIn = true;
  const float a2 = pm_fadd(pm_fadd(pm_fmul(F[0], u1), pm_fmul(F[1], v1)), F[2]);
  const float b2 = pm_fadd(pm_fadd(pm_fmul(F[3], u1), pm_fmul(F[4], v1)), F[5]);
  const float c2 = pm_fadd(pm_fadd(pm_fmul(F[6], u1), pm_fmul(F[7], v1)), F[8]);
  const float num2 = pm_fadd(pm_fadd(pm_fmul(a2, u2), pm_fmul(b2, v2)), c2);
  const float chi1 = pm_fmul(pm_fdiv(pm_fmul(num2, num2), pm_fadd(pm_fmul(a2, a2), pm_fmul(b2, b2))), invs2);
  *t1 = 0.0f;
  if (chi1 > th)
    bIn = false;
  else
    *t1 = pm_fsub(thScore, chi1);
  const float a1 = pm_fadd(pm_fadd(pm_fmul(F[0], u2), pm_fmul(F[3], v2)), F[6]);
  const float b1 = pm_fadd(pm_fadd(pm_fmul(F[1], u2), pm_fmul(F[4], v2)), F[7]);
  const float c1 = pm_fadd(pm_fadd(pm_fmul(F[2], u2), pm_fmul(F[5], v2)), F[8]);
  const float num1 = pm_fadd(pm_fadd(pm_fmul(a1, u1), pm_fmul(b1, v1)), c1);
  const float chi2 = pm_fmul(pm_fdiv(pm_fmul(num1, num1), pm_fadd(pm_fmul(a1, a1), pm_fmul(b1, b1))), invs2);
  *t2 = 0.0f;
  if (chi2 > th)
    bIn = false;
  else
    *t2 = pm_fsub(thScore, chi2);
  return bIn;
}

// :112-118: RH = SH/(SH+SF) in float against the double 0.40. Both scores
// zero (or a NaN ratio with no F) would hand an empty Mat to ReconstructF.
__host__ __device__ inline int iz_choose_model(float SH, float SF, int best_h, int best_f, float* RH) {
  *RH = pm_fdiv(SH, pm_fadd(SH, SF));
  if ((double)*RH > 0.40) return best_h >= 0 ? kIzModelH : kIzModelNone;
  return best_f >= 0 ? kIzModelF : kIzModelNone;
}

// ---------------------------------------------------------------- the candidates
__host__ __device__ inline void iz_K(const orbm_camera& c, float* K) {
  K[0] = c.fx, K[1] = 0.0f, K[2] = c.cx;
  K[3] = 0.0f, K[4] = c.fy, K[5] = c.cy;
  K[6] = 0.0f, K[7] = 0.0f, K[8] = 1.0f;
}

// ReconstructF's candidates (:479-487) through DecomposeE (:909-929): rt[0..3]
// = (R1, t), (R2, t), (R1, -t), (R2, -t). Work as iz_svd3.
__host__ __device__ inline void iz_candidates_f(const float* F21, const orbm_camera& cam, float* Fw, double* W, int s,
                                                orbm_init_rt* rt) {
  float K[9], KtF[9], E[9], w[3], u[9], vt[9];
  iz_K(cam, K);
  iz_mul33_t<true>(K, F21, KtF);  // K.t()*F21
  iz_mul33(KtF, K, 1.0, E);
  iz_svd3(E, Fw, W, s, w, u, vt);
  const float ucol[3] = {u[2], u[5], u[8]};
  float t[3];
  iz_unit3(ucol, t);
  const float Wm[9] = {0.0f, -1.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f};
  float uW[9], R1[9], R2[9];
  iz_mul33(u, Wm, 1.0, uW);
  iz_mul33(uW, vt, 1.0, R1);
  if (iz_det3(R1) < 0)
#pragma unroll
    for (int k = 0; k < 9; ++k) R1[k] = -R1[k];
  iz_mul33_t<false>(u, Wm, uW);  // u*W.t()
  iz_mul33(uW, vt, 1.0, R2);
  if (iz_det3(R2) < 0)
#pragma unroll
    for (int k = 0; k < 9; ++k) R2[k] = -R2[k];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    rt[0].R[k] = rt[2].R[k] = R1[k];
    rt[1].R[k] = rt[3].R[k] = R2[k];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    rt[0].t[k] = rt[1].t[k] = t[k];
    rt[2].t[k] = rt[3].t[k] = -t[k];
  }
}

// ReconstructH's eight candidates after Faugeras (:584-686). False where
// d1/d2 or d2/d3 is below 1.00001 (:597). The plane normals vn are not used
// by the reference after they are built and are left out.
__host__ __device__ inline bool iz_candidates_h(const float* H21, const orbm_camera& cam, float* Fw, double* W, int s,
                                                orbm_init_rt* rt) {
  float K[9], invK[9], tmp[9], A[9], w[3], U[9], Vt[9];
  iz_K(cam, K);
  iz_invert3(K, invK);
  iz_mul33(invK, H21, 1.0, tmp);
  iz_mul33(tmp, K, 1.0, A);
  iz_svd3(A, Fw, W, s, w, U, Vt);
  const float sgn = pm_d2f(pm_dmul(iz_det3(U), iz_det3(Vt)));
  const float d1 = w[0], d2 = w[1], d3 = w[2];
  if ((double)pm_fdiv(d1, d2) < 1.00001 || (double)pm_fdiv(d2, d3) < 1.00001) return false;
  const float d11 = pm_fmul(d1, d1), d22 = pm_fmul(d2, d2), d33 = pm_fmul(d3, d3);
  const float aux1 = pm_fsqrt(pm_fdiv(pm_fsub(d11, d22), pm_fsub(d11, d33)));
  const float aux3 = pm_fsqrt(pm_fdiv(pm_fsub(d22, d33), pm_fsub(d11, d33)));
  const float x1[4] = {aux1, aux1, -aux1, -aux1};
  const float x3[4] = {aux3, -aux3, aux3, -aux3};
  const float root = pm_fsqrt(pm_fmul(pm_fsub(d11, d22), pm_fsub(d22, d33)));
  // case d' = d2
  const float aux_stheta = pm_fdiv(root, pm_fmul(pm_fadd(d1, d3), d2));
  const float ctheta = pm_fdiv(pm_fadd(d22, pm_fmul(d1, d3)), pm_fmul(pm_fadd(d1, d3), d2));
  const float stheta[4] = {aux_stheta, -aux_stheta, -aux_stheta, aux_stheta};
  // case d' = -d2
  const float aux_sphi = pm_fdiv(root, pm_fmul(pm_fsub(d1, d3), d2));
  const float cphi = pm_fdiv(pm_fsub(pm_fmul(d1, d3), d22), pm_fmul(pm_fsub(d1, d3), d2));
  const float sphi[4] = {aux_sphi, -aux_sphi, -aux_sphi, aux_sphi};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int q = i & 3;
    float Rp[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    float tp[3];
    float scale;
    if (i < 4) {
      Rp[0] = ctheta, Rp[2] = -stheta[q], Rp[6] = stheta[q], Rp[8] = ctheta;
      tp[0] = x1[q], tp[1] = 0.0f, tp[2] = -x3[q];
      scale = pm_fsub(d1, d3);
    } else {
      Rp[0] = cphi, Rp[2] = sphi[q], Rp[4] = -1.0f, Rp[6] = sphi[q], Rp[8] = -cphi;
      tp[0] = x1[q], tp[1] = 0.0f, tp[2] = x3[q];
      scale = pm_fadd(d1, d3);
    }
    float sURp[9], R[9], t[3], tn[3];
    iz_mul33(U, Rp, (double)sgn, sURp);  // s*U*Rp: one gemm with alpha = s
    iz_mul33(sURp, Vt, 1.0, R);
    // tp *= d: a convertTo with the float scale
#pragma unroll
    for (int k = 0; k < 3; ++k) tp[k] = pm_fadd(pm_fmul(tp[k], scale), 0.0f);
    iz_mul31(U, tp, t);
    iz_unit3(t, tn);
#pragma unroll
    for (int k = 0; k < 9; ++k) rt[i].R[k] = R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) rt[i].t[k] = tn[k];
  }
  return true;
}

// ---------------------------------------------------------------- CheckRT
// What CheckRT (:798-907) prepares per candidate: P2 = K*[R|t] (:821-824),
// [R|t] and O2 = -R.t()*t (:826)
struct IzRt {
  float P2[12], Rt[12], O2[3];
};
__host__ __device__ inline void iz_prepare_rt(const orbm_camera& cam, const orbm_init_rt& c, IzRt* o) {
  float K[9];
  iz_K(cam, K);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int k = 0; k < 3; ++k) o->Rt[4 * r + k] = c.R[3 * r + k];
    o->Rt[4 * r + 3] = c.t[r];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      o->P2[4 * i + j] = iz_gemm_out(iz_dot3f(K[3 * i], o->Rt[j], K[3 * i + 1], o->Rt[4 + j], K[3 * i + 2], o->Rt[8 + j]), 1.0);
  neg_rt_t(o->Rt, o->O2);
}

// the threshold CheckRT gets: 4.0*mSigma2 passed as a float (:494, :703)
__host__ __device__ inline float iz_th2(float sigma) { return pm_d2f(pm_dmul(4.0, (double)pm_fmul(sigma, sigma))); }

// The loop body of CheckRT for one inlier match (:835-893). Returns whether
// the point is counted (nGood++, vP3D written, its cosine pushed); *good is
// vbGood's value (set only below the 0.99998 cosine; the `vbGood[first]=false;
// continue` of a non-finite point writes the value the entry already has).
__host__ __device__ inline bool iz_check_rt(const orbm_camera& cam, const IzRt& C, float th2, float u1, float v1,
                                            float u2, float v2, float* p, float* cosp, bool* good) {
  *good = false;
  *cosp = 0.0f;
  // Triangulate (:734-747): x*P.row(2) - P.row(k) is one addWeighted, (x*a + (-1)*b) + 0 in float; P1 = K[I|0]
  const float P1r0[4] = {cam.fx, 0.0f, cam.cx, 0.0f}, P1r1[4] = {0.0f, cam.fy, cam.cy, 0.0f};
  const float P1r2[4] = {0.0f, 0.0f, 1.0f, 0.0f};
  float A[4][4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    A[0][c] = pm_fadd(pm_fadd(pm_fmul(P1r2[c], u1), pm_fmul(P1r0[c], -1.0f)), 0.0f);
    A[1][c] = pm_fadd(pm_fadd(pm_fmul(P1r2[c], v1), pm_fmul(P1r1[c], -1.0f)), 0.0f);
    A[2][c] = pm_fadd(pm_fadd(pm_fmul(C.P2[8 + c], u2), pm_fmul(C.P2[c], -1.0f)), 0.0f);
    A[3][c] = pm_fadd(pm_fadd(pm_fmul(C.P2[8 + c], v2), pm_fmul(C.P2[4 + c], -1.0f)), 0.0f);
  }
  float h[4];
  np_svd4_last_row(A, h);
  const float a = pm_d2f(pm_ddiv(1.0, (double)h[3]));  // Mat / float: convertTo with the scale 1/s
#pragma unroll
  for (int r = 0; r < 3; ++r) p[r] = pm_fadd(pm_fmul(h[r], a), 0.0f);
  if (!__builtin_isfinite(p[0]) || !__builtin_isfinite(p[1]) || !__builtin_isfinite(p[2])) return false;  // :841-845
  // :848-854; normal1 = p3dC1 - O1 with O1 = 0
  const float dist1 = norm3(p[0], p[1], p[2]);
  const float n2x = pm_fsub(p[0], C.O2[0]), n2y = pm_fsub(p[1], C.O2[1]), n2z = pm_fsub(p[2], C.O2[2]);
  const float dist2 = norm3(n2x, n2y, n2z);
  const double dot = pm_dadd(pm_dadd(pm_dmul((double)p[0], (double)n2x), pm_dmul((double)p[1], (double)n2y)),
                             pm_dmul((double)p[2], (double)n2z));
  const float cosParallax = pm_d2f(pm_ddiv(dot, (double)pm_fmul(dist1, dist2)));
  *cosp = cosParallax;
  const bool low = (double)cosParallax < 0.99998;
  if (p[2] <= 0 && low) return false;  // :857
  const float x2 = pose_row(C.Rt, 0, p[0], p[1], p[2]), y2 = pose_row(C.Rt, 1, p[0], p[1], p[2]);
  const float z2 = pose_row(C.Rt, 2, p[0], p[1], p[2]);
  if (z2 <= 0 && low) return false;  // :863
  // :867-875
  const float invZ1 = pm_d2f(pm_ddiv(1.0, (double)p[2]));
  const float im1x = pm_fadd(pm_fmul(pm_fmul(cam.fx, p[0]), invZ1), cam.cx);
  const float im1y = pm_fadd(pm_fmul(pm_fmul(cam.fy, p[1]), invZ1), cam.cy);
  const float e1x = pm_fsub(im1x, u1), e1y = pm_fsub(im1y, v1);
  if (pm_fadd(pm_fmul(e1x, e1x), pm_fmul(e1y, e1y)) > th2) return false;
  // :878-886
  const float invZ2 = pm_d2f(pm_ddiv(1.0, (double)z2));
  const float im2x = pm_fadd(pm_fmul(pm_fmul(cam.fx, x2), invZ2), cam.cx);
  const float im2y = pm_fadd(pm_fmul(pm_fmul(cam.fy, y2), invZ2), cam.cy);
  const float e2x = pm_fsub(im2x, u2), e2y = pm_fsub(im2y, v2);
  if (pm_fadd(pm_fmul(e2x, e2x), pm_fmul(e2y, e2y)) > th2) return false;
  *good = low;  // :892
  return true;
}

// The order of std::sort on floats as unsigned keys (NaNs, which sort has no
// order for, go to the ends by their sign)
__host__ __device__ inline uint32_t iz_cos_key(float c) {
  const uint32_t u = __builtin_bit_cast(uint32_t, c);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float iz_key_cos(uint32_t k) {
  return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
// :896-904 from the selected cosine: acos of a float under `using namespace
// std` is acosf; *180 in float, /CV_PI in double
__host__ __device__ inline float iz_parallax(float cosv) {
  return pm_d2f(pm_ddiv((double)pm_fmul(acosf(cosv), 180.0f), 3.1415926535897932384626433832795));
}

// ---------------------------------------------------------------- acceptance
struct IzVerdict {
  int ok, code, best;
};
// ReconstructF (:499-569); n_inl = the inliers of F
__host__ __device__ inline IzVerdict iz_accept_f(const int* nGood, const float* parallax, int n_inl, float min_parallax,
                                                 int min_tri) {
  int maxGood = nGood[0];
#pragma unroll
  for (int k = 1; k < 4; ++k) maxGood = nGood[k] > maxGood ? nGood[k] : maxGood;
  const int n09 = (int)pm_dmul(0.9, (double)n_inl);
  const int nMinGood = n09 > min_tri ? n09 : min_tri;
  int nsimilar = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) nsimilar += (double)nGood[k] > pm_dmul(0.7, (double)maxGood) ? 1 : 0;
  int best = 3;
#pragma unroll
  for (int k = 2; k >= 0; --k) best = nGood[k] == maxGood ? k : best;  // the if / else-if chain (:523-567)
  if (maxGood < nMinGood) return IzVerdict{0, kIzTooFewPoints, best};
  if (nsimilar > 1) return IzVerdict{0, kIzNoClearWinner, best};
  float pb = parallax[3];
#pragma unroll
  for (int k = 2; k >= 0; --k) pb = best == k ? parallax[k] : pb;
  if (pb > min_parallax) return IzVerdict{1, kIzAccepted, best};
  return IzVerdict{0, kIzLowParallax, best};
}
// ReconstructH (:689-731); best = -1 when no candidate has a good point
__host__ __device__ inline IzVerdict iz_accept_h(const int* nGood, const float* parallax, int n_inl, float min_parallax,
                                                 int min_tri) {
  int bestGood = 0, secondBestGood = 0, best = -1;
  float bestParallax = -1.0f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (nGood[i] > bestGood) {
      secondBestGood = bestGood;
      bestGood = nGood[i];
      best = i;
      bestParallax = parallax[i];
    } else if (nGood[i] > secondBestGood) {
      secondBestGood = nGood[i];
    }
  }
  if (!((double)secondBestGood < pm_dmul(0.75, (double)bestGood))) return IzVerdict{0, kIzNoClearWinner, best};
  if (!(bestGood > min_tri && (double)bestGood > pm_dmul(0.9, (double)n_inl))) return IzVerdict{0, kIzTooFewPoints, best};
  if (!(bestParallax >= min_parallax)) return IzVerdict{0, kIzLowParallax, best};
  return IzVerdict{1, kIzAccepted, best};
}

}  // namespace orbx
