// orbm_initialize_host on built-in frame pairs, stand-alone, for a run under
// AddressSanitizer and UBSan on the CPU (no device is touched):
//   cd orb_slam_cuda_amd/csrc && make
//   S="-fsanitize=address,undefined"; F="--offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=off -I../../include"
//   hipcc $F -Xarch_host $S -c orbx_initializer.hip -o /tmp/initz_san.o
//   hipcc $F -Xarch_host $S -c orbx_matcher.hip -o /tmp/matcher_san.o
//   g++ -O1 -g -std=c++17 -I../../include $S -c ../../tools/initializer_host_check.cpp -o /tmp/check_main.o
//   hipcc --offload-arch=gfx950 $S /tmp/check_main.o /tmp/initz_san.o /tmp/matcher_san.o \
//     $(ls build/*.o | grep -v -e orbx_matcher -e orbx_initializer) -o /tmp/initializer_host_check && \
//     /tmp/initializer_host_check
// The host form and everything it inlines from orbx_initializer.cuh are then
// instrumented; the other objects only satisfy the link. Two embedded scenes, a
// general one (the fundamental matrix wins) and a planar one (the homography
// wins), at 0, 7, 8, 9, 120 and 3000 matches, with unmatched keypoints, a match
// beyond frame 2, raw draws at both ends of rand()'s range and above it, every
// keypoint on one spot (NaN throughout), 1 and 1024 iterations, every output
// NULL, and tight output buffers on the heap. Prints each pair's result; exit
// status 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "orbx_c.h"

static uint64_t g_s = 88172645463325252ull;
static double rnd() {  // xorshift, uniform in [0, 1)
  g_s ^= g_s << 13;
  g_s ^= g_s >> 7;
  g_s ^= g_s << 17;
  return (double)(g_s >> 11) / 9007199254740992.0;
}
static double gauss() { return std::sqrt(-2.0 * std::log(rnd() + 1e-300)) * std::cos(6.283185307179586 * rnd()); }

// kind 0: a general scene; 1: a tilted plane; 2: every keypoint on one spot; 3: a match beyond frame 2
static int run(int N, int kind, int its, bool null_outputs) {
  const int n1 = N + N / 2 + 3, n2 = N + 5;
  const float fx = 520.f, fy = 518.f, cx = 321.5f, cy = 239.25f;
  std::vector<orbx_kp> k1(n1), k2(n2);
  std::vector<int> m12(n1, -1);
  for (int i = 0; i < n1; ++i) k1[i] = orbx_kp{(float)(10 + rnd() * 620), (float)(10 + rnd() * 460), 31.f, 0.f, 0.f, 0, -1};
  for (int i = 0; i < n2; ++i) k2[i] = orbx_kp{(float)(10 + rnd() * 620), (float)(10 + rnd() * 460), 31.f, 0.f, 0.f, 0, -1};
  // X2 = R(y, th)*X1 + t
  const double th = -0.06, t[3] = {kind == 1 ? 0.62 : 0.6, kind == 1 ? -1.5 : 0.05, kind == 1 ? 0.01 : 0.12};
  for (int k = 0; k < N; ++k) {
    const int i1 = k + k / 2, i2 = N - 1 - k;
    double u, v, z, X[3], Y[3], u2, v2;
    do {
      u = 20 + rnd() * 600, v = 20 + rnd() * 440;
      const double x = (u - cx) / fx, y = (v - cy) / fy;
      z = kind == 1 ? 3.06 / (1 - 1.19 * x - 1.12 * y) : 4 + rnd() * 5;
      X[0] = x * z, X[1] = y * z, X[2] = z;
      Y[0] = std::cos(th) * X[0] + std::sin(th) * X[2] + t[0];
      Y[1] = X[1] + t[1];
      Y[2] = -std::sin(th) * X[0] + std::cos(th) * X[2] + t[2];
      u2 = fx * Y[0] / Y[2] + cx, v2 = fy * Y[1] / Y[2] + cy;
    } while (!(z > 1 && z < 50 && Y[2] > 0.5 && u2 > 5 && u2 < 635 && v2 > 5 && v2 < 475));
    k1[i1].x = (float)(u + 0.1 * gauss()), k1[i1].y = (float)(v + 0.1 * gauss());
    k2[i2].x = (float)(u2 + 0.1 * gauss()), k2[i2].y = (float)(v2 + 0.1 * gauss());
    if (rnd() < 0.05) k2[i2].x = (float)(10 + rnd() * 620), k2[i2].y = (float)(10 + rnd() * 460);
    m12[i1] = i2;
  }
  if (kind == 2) {
    for (auto& k : k1) k.x = 100.f, k.y = 50.f;
    for (auto& k : k2) k.x = 100.f, k.y = 50.f;
  }
  if (kind == 3 && N > 30) m12[1] = n2, m12[4] = n2 + 7;  // i1 = 1 and 4 hold no match of the scene
  orbm_camera cam{fx, fy, cx, cy, 0.f, 0.f, {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}};
  std::vector<uint32_t> rand8(8 * (size_t)its);
  for (size_t k = 0; k < rand8.size(); ++k) rand8[k] = (uint32_t)(rnd() * 2147483648.0);
  if (its >= 4)
    for (int c = 0; c < 8; ++c) rand8[c] = 0u, rand8[8 + c] = 2147483647u, rand8[16 + c] = 0xFFFFFFFFu, rand8[24 + c] = 12345678u;
  orbm_init_params P{1.0f, its, 1.0f, 50};
  orbm_init_result r{};
  std::vector<float> R21(9), t21(3), Tcw(12), p3d(3 * (size_t)n1), T1(9), T2(9), H21(9), F21(9);
  std::vector<uint8_t> tri(n1), inl_h(n1), inl_f(n1);
  std::vector<int> m12o(n1);
  std::vector<orbm_init_hyp> hyp(2 * (size_t)its);
  std::vector<orbm_init_rt> rt(8);
  int status = -1, rc;
  if (null_outputs)
    rc = orbm_initialize_host(k1.data(), n1, k2.data(), n2, m12.data(), &cam, &P, rand8.data(), &r, nullptr, nullptr,
                              nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                              nullptr, nullptr, &status);
  else
    rc = orbm_initialize_host(k1.data(), n1, k2.data(), n2, m12.data(), &cam, &P, rand8.data(), &r, R21.data(), t21.data(),
                              Tcw.data(), p3d.data(), tri.data(), m12o.data(), inl_h.data(), inl_f.data(), T1.data(),
                              T2.data(), H21.data(), F21.data(), hyp.data(), rt.data(), &status);
  int ntri = 0;
  for (uint8_t b : tri) ntri += b;
  printf("N %d kind %d its %d null %d: rc %d status %d n %d ok %d code %d model %d SH %.2f SF %.2f RH %.4f best %d/%d rt %d "
         "nGood %d %d %d %d parallax %.3f inliers %d triangulated %d\n",
         N, kind, its, (int)null_outputs, rc, status, r.n, r.ok, r.code, r.model, r.SH, r.SF, r.RH, r.best_h, r.best_f,
         r.best_rt, r.n_good[0], r.n_good[1], r.n_good[2], r.n_good[3], r.best_rt >= 0 ? r.parallax[r.best_rt] : 0.f,
         r.n_inliers, ntri);
  return rc;
}

int main() {
  int rc = 0;
  const int sizes[] = {0, 7, 8, 9, 120, 3000};
  for (int n : sizes)
    for (int kind = 0; kind < 4; ++kind) rc |= run(n, kind, n == 3000 ? 24 : 200, false);
  rc |= run(120, 0, 1, false);
  rc |= run(120, 1, 1024, false);
  rc |= run(120, 0, 40, true);
  uint32_t r[16];
  rc |= orbm_initializer_rand_fill(r, 2);
  int a, b, c;
  rc |= orbm_initializer_limits(&a, &b, &c);
  printf("limits: %d %d %d\n", a, b, c);
  return rc ? 1 : 0;
}
