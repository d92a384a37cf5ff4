// orbm_optimize_sim3_host on built-in keyframe pairs, stand-alone, for a run under
// AddressSanitizer and UBSan on the CPU (no device is touched):
//   cd orb_slam_cuda_amd/csrc && make
//   S="-fsanitize=address,undefined"; F="--offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=off -I../../include"
//   hipcc $F -Xarch_host $S -c orbx_matcher.hip -o /tmp/matcher_san.o
//   hipcc $F -Xarch_host $S -c orbx_optsim3.hip -o /tmp/optsim3_san.o
//   g++ -O1 -g -std=c++17 -I../../include $S -c ../../tools/optsim3_host_check.cpp -o /tmp/check_main.o
//   hipcc --offload-arch=gfx950 $S /tmp/check_main.o /tmp/matcher_san.o /tmp/optsim3_san.o \
//     $(ls build/*.o | grep -v -e orbx_matcher -e orbx_optsim3) -o /tmp/optsim3_host_check && /tmp/optsim3_host_check
// The entry point, the host function and everything it inlines from
// orbx_optsim3.cuh and orbx_poseopt.cuh are then instrumented; the other
// objects only satisfy the link. Pairs of 0, 9, 12, 100 and 3000 matches, both
// scale modes, with and without the inlier and found lists, with bad indices and
// octaves, every output array tight on the heap. Prints each pair's result;
// exit status 0.
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

static int run(int n, bool fix_scale, bool lists, bool bad_entries) {
  const float fx = 718.856f, fy = 718.856f, cx = 607.1928f, cy = 185.2157f, bf = 386.1448f;
  const int n1 = n + n / 4 + 3, n2 = n + n / 5 + 2;
  const double s = fix_scale ? 1.0 : 1.17, t[3] = {0.3, -0.1, 0.2}, yaw = 0.05;
  std::vector<orbx_kp> k1(n1), k2(n2);
  std::vector<orbm_map_point_world> m1(n1), m2(n2);
  std::vector<int> match12(n1, -1), found12(n1, -1), found21(n2, -1), out(n1, -5);
  std::vector<uint8_t> inlier(n1, 1);
  std::vector<float> sig(8);
  for (int l = 0; l < 8; ++l) sig[l] = (float)(1.0 / std::pow(1.2, 2 * l));
  for (int i = 0; i < n1; ++i) k1[i] = orbx_kp{(float)(rnd() * 1241), (float)(rnd() * 376), 31.f, 0.f, 0.f, (int)(rnd() * 8), -1};
  for (int i = 0; i < n2; ++i) k2[i] = orbx_kp{(float)(rnd() * 1241), (float)(rnd() * 376), 31.f, 0.f, 0.f, (int)(rnd() * 8), -1};
  for (auto* m : {&m1, &m2})
    for (auto& p : *m) {
      p = orbm_map_point_world{};
      p.pos[2] = 10;
      p.valid = 1;
    }
  // both cameras at the world's origin: camera coordinates are world coordinates
  for (int k = 0; k < n; ++k) {
    const int i1 = k + k / 4, i2 = n2 - 1 - k;
    const double u = 20 + rnd() * 1200, v = 20 + rnd() * 330, z = 4 + rnd() * 36;
    const double x2[3] = {(u - cx) * z / fx, (v - cy) * z / fy, z};
    const double x1[3] = {s * (std::cos(yaw) * x2[0] + std::sin(yaw) * x2[2]) + t[0], s * x2[1] + t[1],
                          s * (-std::sin(yaw) * x2[0] + std::cos(yaw) * x2[2]) + t[2]};
    const double g = rnd() < 0.15 ? 60 : 0;
    k1[i1].x = (float)(x1[0] / x1[2] * fx + cx + gauss() * std::pow(1.2, k1[i1].octave) + g);
    k1[i1].y = (float)(x1[1] / x1[2] * fy + cy + gauss() * std::pow(1.2, k1[i1].octave));
    k2[i2].x = (float)(u + gauss() * std::pow(1.2, k2[i2].octave));
    k2[i2].y = (float)(v + gauss() * std::pow(1.2, k2[i2].octave));
    for (int r = 0; r < 3; ++r) {
      m1[i1].pos[r] = (float)x1[r];
      m2[i2].pos[r] = (float)x2[r];
    }
    if (lists && k % 3 == 0) {
      found12[i1] = i2;
      found21[i2] = i1;
    } else {
      match12[i1] = i2;
      if (lists && k % 7 == 0) inlier[i1] = 0;
    }
  }
  if (bad_entries && n > 20) {
    match12[0] = n2;
    k1[5].octave = 8;
    found12[n1 - 1] = n2 + 7;
    m1[10].valid = 0;
  }
  const orbm_camera cam1{fx, fy, cx, cy, bf / fx, bf, {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}};
  const orbm_camera cam2 = cam1;
  const float s12 = (float)(s * 1.03), t12[3] = {(float)(t[0] + 0.05), (float)(t[1] - 0.04), (float)(t[2] + 0.03)};
  const float c = (float)std::cos(yaw + 0.01), sn = (float)std::sin(yaw + 0.01);
  const float R12[9] = {c, 0, sn, 0, 1, 0, -sn, 0, c};
  std::vector<double> S12(8), lin(36);
  std::vector<float> Scw(12);
  orbm_pose pose;
  orbm_optsim3_result r;
  int status = -1;
  const int rc = orbm_optimize_sim3_host(k1.data(), n1, k2.data(), n2, m1.data(), m2.data(), &cam1, &cam2, match12.data(),
                                         lists ? inlier.data() : nullptr, lists ? found12.data() : nullptr,
                                         lists ? found21.data() : nullptr, sig.data(), 8, &s12, R12, t12, 10.0f,
                                         fix_scale ? 1 : 0, out.data(), S12.data(), Scw.data(), &pose, &r, lin.data(),
                                         &status);
  printf("n %d fix %d lists %d rc %d status %d ret %d of %d, bad %d, rounds %d (+%d), trials %d (%d rejected), s = %.6f t = %.4f %.4f %.4f\n",
         n, (int)fix_scale, (int)lists, rc, status, r.ret, r.n_corr, r.n_bad, r.rounds, r.more_iterations, r.trials,
         r.rejected, S12[7], S12[4], S12[5], S12[6]);
  return rc;
}

int main() {
  int rc = 0;
  const int sizes[] = {0, 9, 12, 100, 3000};
  for (int n : sizes)
    for (int mode = 0; mode < 4; ++mode) rc |= run(n, mode & 1, (mode & 2) != 0, mode == 3);
  return rc ? 1 : 0;
}
