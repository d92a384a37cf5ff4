// orbm_sim3_ransac_host on built-in keyframe pairs, stand-alone, for a run under
// AddressSanitizer and UBSan on the CPU (no device is touched):
//   cd orb_slam_cuda_amd/csrc && make
//   S="-fsanitize=address,undefined"; F="--offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=off -I../../include"
//   hipcc $F -Xarch_host $S -c orbx_sim3.hip -o /tmp/sim3_san.o
//   hipcc $F -Xarch_host $S -c orbx_matcher.hip -o /tmp/matcher_san.o
//   g++ -O1 -g -std=c++17 -I../../include $S -c ../../tools/sim3_host_check.cpp -o /tmp/check_main.o
//   hipcc --offload-arch=gfx950 $S /tmp/check_main.o /tmp/sim3_san.o /tmp/matcher_san.o \
//     $(ls build/*.o | grep -v -e orbx_matcher -e orbx_sim3) -o /tmp/sim3_host_check && /tmp/sim3_host_check
// The host form and everything it inlines from orbx_sim3.cuh are then
// instrumented; the other objects only satisfy the link. Pairs of 0, 2, 19, 20,
// 21, 100 and 3000 correspondences with and without a fixed scale, unmatched and
// bad entries, a keypoint index table, raw draws at both ends of rand()'s range
// and above it, triples of coincident points, identical point sets (the zero
// rotation: NaN throughout), a resumed call and tight output buffers on the
// heap. Prints each pair's result; exit status 0.
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

// kind 0: a scene with 35 % outliers; 1: every point of pKF2 the same (coincident triples);
// 2: identical sets and poses (the zero rotation); 3: bad entries and a keypoint index table
static int run(int ncorr, int kind, bool fix_scale, int its) {
  const int n1 = ncorr + ncorr / 2 + 3, n2 = ncorr + 5;
  const float fx = 458.654f, fy = 457.296f, cx = 367.215f, cy = 248.375f;
  std::vector<orbx_kp> k1(n1), k2(n2);
  std::vector<orbm_map_point_world> m1(n1), m2(n2);
  std::vector<int> match12(n1, -1), index1(n1);
  std::vector<float> sig(8);
  for (int l = 0; l < 8; ++l) sig[l] = (float)std::pow(1.2, 2 * l);
  for (int i = 0; i < n1; ++i) {
    k1[i] = orbx_kp{0.f, 0.f, 31.f, 0.f, 0.f, (int)(rnd() * 8), -1};
    m1[i] = orbm_map_point_world{};
    m1[i].valid = rnd() < 0.9;
    index1[i] = i;
  }
  for (int i = 0; i < n2; ++i) {
    k2[i] = orbx_kp{0.f, 0.f, 31.f, 0.f, 0.f, (int)(rnd() * 8), -1};
    m2[i] = orbm_map_point_world{};
    m2[i].valid = 1;
  }
  const double s = fix_scale ? 1.0 : 1.3, th = 0.2, t[3] = {0.3, -0.1, 0.2};
  for (int k = 0; k < ncorr; ++k) {
    const int i1 = k + k / 2, i2 = ncorr - 1 - k;
    const double z = 2 + rnd() * 10, X1[3] = {(40 + rnd() * 670 - cx) * z / fx, (40 + rnd() * 400 - cy) * z / fy, z};
    // X1 = s*R(y, th)*X2 + t
    const double d[3] = {(X1[0] - t[0]) / s, (X1[1] - t[1]) / s, (X1[2] - t[2]) / s};
    double X2[3] = {std::cos(th) * d[0] - std::sin(th) * d[2], d[1], std::sin(th) * d[0] + std::cos(th) * d[2]};
    if (kind == 0 && rnd() < 0.35) X2[0] += 1 + rnd(), X2[1] -= rnd();
    for (int c = 0; c < 3; ++c) {
      m1[i1].pos[c] = (float)X1[c];
      m2[i2].pos[c] = (float)(kind == 1 ? (c == 2 ? 5.0 : 0.1) : kind == 2 ? X1[c] : X2[c] + gauss() * 0.0004 * X2[2]);
    }
    m1[i1].valid = 1;
    match12[i1] = i2;
  }
  if (kind == 3 && ncorr > 30) {
    match12[0] = n2 + 7;  // a match beyond pKF2's keypoints
    k2[match12[3]].octave = 8;
    k1[6].octave = -1;
    index1[9] = n1;  // a keypoint index beyond pKF1's
    index1[12] = -1; // no keypoint: left out without a status bit
    index1[15] = 16;
  }
  orbm_camera cam1{fx, fy, cx, cy, 0.11f, 47.9f, {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}};
  orbm_camera cam2 = cam1;
  std::vector<uint32_t> rand3(3 * (size_t)its);
  for (size_t k = 0; k < rand3.size(); ++k) rand3[k] = (uint32_t)(rnd() * 2147483648.0);
  if (its >= 4) {
    for (int c = 0; c < 3; ++c) rand3[c] = 0u, rand3[3 + c] = 2147483647u, rand3[6 + c] = 0xFFFFFFFFu;
    rand3[9] = rand3[10] = rand3[11] = 12345678u;  // the same slot three times
  }
  orbm_sim3_params P{0.99, 20, its, fix_scale ? 1 : 0, 0, 0, 0};
  orbm_sim3_result r{};
  std::vector<float> srt(13, -1.f);
  std::vector<orbm_pose> pose(2);
  std::vector<uint8_t> inlier(n1);
  std::vector<orbm_sim3_hyp> hyp(its);
  int status = -1, rc, calls = 0, accepted = 0;
  do {  // to the end, resuming after every acceptance
    rc = orbm_sim3_ransac_host(k1.data(), n1, k2.data(), n2, m1.data(), m2.data(), &cam1, &cam2, match12.data(),
                               kind == 3 ? index1.data() : nullptr, sig.data(), 8, &P, rand3.data(), &r, srt.data(),
                               srt.data() + 1, srt.data() + 10, pose.data(), inlier.data(),
                               calls % 2 ? nullptr : hyp.data(), &status);
    ++calls;
    accepted += r.ret > 0;
    P.first_iteration = r.iterations;
    P.best_inliers = r.best_inliers;
  } while (rc == 0 && !r.no_more && calls < 50);
  printf("corr %d kind %d fix %d its %d: rc %d status %d N %d max_its %d, %d calls, %d accepted, best %d at %d, s %.4f\n",
         ncorr, kind, (int)fix_scale, its, rc, status, r.n_corr, r.max_its, calls, accepted, r.best_inliers,
         r.best_iteration, srt[0]);
  return rc;
}

int main() {
  int rc = 0;
  const int sizes[] = {0, 2, 19, 20, 21, 100, 3000};
  for (int n : sizes)
    for (int kind = 0; kind < 4; ++kind) rc |= run(n, kind, kind == 2 || n == 100, n == 3000 ? 40 : 300);
  rc |= run(100, 0, false, 1);
  rc |= run(100, 0, false, 1024);
  uint32_t r[6];
  rc |= orbm_sim3_rand_fill(r, 2);
  std::vector<int> tab(4001);
  rc |= orbm_sim3_iteration_table(0.99, 20, 300, 4000, tab.data());
  printf("table: %d %d %d %d %d\n", tab[19], tab[20], tab[21], tab[100], tab[4000]);
  return rc ? 1 : 0;
}
