// orbm_create_new_map_points_host, orbm_prepare_new_points and orbm_compute_f12 on
// built-in keyframe pairs, stand-alone, for a run under AddressSanitizer and UBSan
// on the CPU (no device is touched):
//   cd orb_slam_cuda_amd/csrc && make
//   S="-fsanitize=address,undefined"; F="--offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=off -I../../include"
//   hipcc $F -Xarch_host $S -c orbx_newpoints.hip -o /tmp/newpoints_san.o
//   hipcc $F -Xarch_host $S -c orbx_matcher.hip -o /tmp/matcher_san.o
//   g++ -O1 -g -std=c++17 -I../../include $S -c ../../tools/newpoints_host_check.cpp -o /tmp/check_main.o
//   hipcc --offload-arch=gfx950 $S /tmp/check_main.o /tmp/newpoints_san.o /tmp/matcher_san.o \
//     $(ls build/*.o | grep -v -e orbx_matcher -e orbx_newpoints) -o /tmp/newpoints_host_check && /tmp/newpoints_host_check
// The host form and everything it inlines from orbx_newpoints.cuh are then
// instrumented; the other objects only satisfy the link. Pairs of 0, 1, 63, 300
// and 5000 keypoints with monocular, stereo and mixed keypoints, with and without
// the distorted keypoint arrays, matches at both ends of the arrays, indices and
// octaves out of range, stereo keypoints without a depth, NaN and infinite
// inputs, coincident cameras (a singular A) and tight output buffers on the
// heap. Prints each pair's counts per reason; exit status 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
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

// kind 0: a scene; 1: the same with mvKeys arrays; 2: bad entries; 3: NaN / inf inputs; 4: coincident cameras
static int run(int n, int kind, double stereo) {
  const float fx = 718.856f, fy = 718.856f, cx = 607.1928f, cy = 185.2157f, bf = 386.1448f;
  const int n1 = n, n2 = n + n / 3 + (n ? 2 : 0);
  orbm_camera cam1{fx, fy, cx, cy, bf / fx, bf, {1, 0, 0, 0.2f, 0, 1, 0, -0.1f, 0, 0, 1, 0.3f}};
  const double th = 0.03, bx = kind == 4 ? 0.0 : 0.3 + 2.7 * rnd();
  orbm_camera cam2 = cam1;
  const float R2[9] = {(float)std::cos(th), 0, (float)std::sin(th), 0, 1, 0, (float)-std::sin(th), 0, (float)std::cos(th)};
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) cam2.Tcw[4 * r + c] = R2[3 * r + c];
    cam2.Tcw[4 * r + 3] = cam1.Tcw[4 * r + 3] - (float)(R2[3 * r] * bx);
  }
  if (kind == 4)
    for (int k = 0; k < 12; ++k) cam2.Tcw[k] = cam1.Tcw[k];
  orbm_newpt_pair P;
  int rc = orbm_prepare_new_points(&cam1, &cam2, 1.2f, 0, 1, 0, 4096, n & 1, &P);
  float F12[9];
  rc |= orbm_compute_f12(&cam1, &cam2, F12);
  std::vector<orbx_kp> k1(n1), k2(n2), r1(n1), r2(n2);
  std::vector<float> u1(n1, -1.f), d1(n1, -1.f), u2(n2, -1.f), d2(n2, -1.f), sig(8), sf(8);
  std::vector<int> m12(n1, -1);
  for (int l = 0; l < 8; ++l) sf[l] = (float)std::pow(1.2, l), sig[l] = sf[l] * sf[l];
  for (int i = 0; i < n2; ++i) k2[i] = r2[i] = orbx_kp{(float)(rnd() * 1241), (float)(rnd() * 376), 31.f, 0.f, 0.f, (int)(rnd() * 8), -1};
  for (int i = 0; i < n1; ++i) {
    const double z = 4 + 56 * rnd(), u = 20 + 1200 * rnd(), v = 20 + 336 * rnd();
    const int o = (int)(rnd() * 8);
    k1[i] = orbx_kp{(float)(u + 0.7 * gauss()), (float)(v + 0.7 * gauss()), 31.f, 0.f, 0.f, o, -1};
    r1[i] = k1[i];
    r1[i].x += 0.5f;
    if (rnd() < stereo) u1[i] = (float)(u - bf / z), d1[i] = (float)z;
    if (i == 0 || i == n1 - 1 || rnd() < 0.8) {
      const int j = (i * 7 + 3) % n2;
      // the point in camera 1, then in camera 2
      const double X[3] = {(u - cx) * z / fx - 0.2, (v - cy) * z / fy + 0.1, z - 0.3};
      double c2[3];
      for (int r = 0; r < 3; ++r) c2[r] = cam2.Tcw[4 * r] * X[0] + cam2.Tcw[4 * r + 1] * X[1] + cam2.Tcw[4 * r + 2] * X[2] + cam2.Tcw[4 * r + 3];
      k2[j].x = (float)(fx * c2[0] / c2[2] + cx + 0.7 * gauss());
      k2[j].y = (float)(fy * c2[1] / c2[2] + cy + 0.7 * gauss());
      k2[j].octave = o;
      r2[j] = k2[j];
      if (rnd() < stereo) u2[j] = (float)(k2[j].x - bf / c2[2]), d2[j] = (float)c2[2];
      m12[i] = j;
    }
  }
  if (kind == 2 && n1 > 20) {
    m12[1] = n2;           // beyond pKF2's keypoints
    m12[2] = 2147483647;
    k1[3].octave = 8;
    k1[4].octave = -1;
    if (m12[5] >= 0) k2[m12[5]].octave = 1000;
    u1[6] = 100.f, d1[6] = 0.f;   // stereo keypoints without a depth
    u1[7] = 100.f, d1[7] = -1.f;
    if (m12[8] >= 0) u1[8] = -1.f, u2[m12[8]] = 50.f, d2[m12[8]] = -2.f;
  }
  if (kind == 3 && n1 > 20) {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    k1[1].x = nan;
    k1[2].y = inf;
    u1[3] = nan;
    u1[4] = 10.f, d1[4] = nan;
    u1[5] = 10.f, d1[5] = inf;
    k1[6].x = 3e38f;
    if (m12[7] >= 0) k2[m12[7]].x = -inf;
    sig[7] = nan;
  }
  const bool raw = kind == 1;
  std::vector<float> pos(3 * (size_t)n1);
  std::vector<uint8_t> reason(n1);
  int nnew = -1, status = -1;
  rc |= orbm_create_new_map_points_host(&P, k1.data(), raw ? r1.data() : nullptr, u1.data(), d1.data(), n1, k2.data(),
                                        raw ? r2.data() : nullptr, u2.data(), d2.data(), n2, sig.data(), sf.data(), 8,
                                        m12.data(), pos.data(), reason.data(), &nnew, kind & 1 ? nullptr : &status);
  int hist[16] = {};
  for (int i = 0; i < n1; ++i) ++hist[reason[i] & 15];
  printf("n %d kind %d stereo %.1f: rc %d status %d nnew %d, reasons", n, kind, stereo, rc, status, nnew);
  for (int k = 0; k < 16; ++k) printf(" %d", hist[k]);
  printf("\n");
  return rc;
}

int main() {
  int rc = 0;
  const int sizes[] = {0, 1, 63, 300, 5000};
  for (int n : sizes)
    for (int kind = 0; kind < 5; ++kind) rc |= run(n, kind, kind == 0 ? 0.0 : (kind == 1 ? 1.0 : 0.4));
  return rc ? 1 : 0;
}
