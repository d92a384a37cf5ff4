// orbm_pose_optimization_host on a built-in scene, stand-alone, for a run under
// AddressSanitizer and UBSan on the CPU (no device is touched):
//   cd orb_slam_cuda_amd/csrc && make
//   S="-fsanitize=address,undefined"; F="--offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=off -I../../include"
//   hipcc $F -Xarch_host $S -c orbx_matcher.hip -o /tmp/matcher_san.o
//   g++ -O1 -g -std=c++17 -I../../include $S -c ../../tools/poseopt_host_check.cpp -o /tmp/check_main.o
//   hipcc --offload-arch=gfx950 $S /tmp/check_main.o /tmp/matcher_san.o $(ls build/*.o | grep -v orbx_matcher) \
//     -o /tmp/poseopt_host_check && /tmp/poseopt_host_check
// The host function and everything it inlines from orbx_poseopt.cuh are then
// instrumented (orbx_matcher.hip is compiled with the sanitizers); the other
// objects only satisfy the link. Frames of 0, 2, 9, 300 and 3000 keypoints,
// monocular, stereo and mixed, with a bad octave and a bad row, tight output
// buffers on the heap. Prints each frame's result; exit status 0.
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

static int run(int n, int kind, bool bad_entries) {
  const float fx = 718.856f, fy = 718.856f, cx = 607.1928f, cy = 185.2157f, bf = 386.1448f;
  std::vector<orbx_kp> kps(n);
  std::vector<float> ur(n, -1.0f);
  std::vector<int> assign(n, -1);
  std::vector<orbm_map_point_world> mps;
  std::vector<float> sig(8);
  for (int l = 0; l < 8; ++l) sig[l] = (float)(1.0 / std::pow(1.2, 2 * l));
  for (int i = 0; i < n; ++i) {
    const double u = 20 + rnd() * 1200, v = 20 + rnd() * 330, z = 4 + rnd() * 36;
    const int oct = (int)(rnd() * 8);
    const double s = std::pow(1.2, oct);
    const bool gross = rnd() < 0.15;
    kps[i] = orbx_kp{(float)(u + gauss() * s + (gross ? 50 : 0)), (float)(v + gauss() * s), 31.f, 0.f, 0.f, oct, -1};
    if (rnd() < 0.3) continue;
    orbm_map_point_world p{};
    p.pos[0] = (float)((u - cx) * z / fx);
    p.pos[1] = (float)((v - cy) * z / fy);
    p.pos[2] = (float)z;
    p.valid = 1;
    p.obs_positive = rnd() < 0.8;
    assign[i] = (int)mps.size();
    mps.push_back(p);
    if (kind == 1 || (kind == 2 && rnd() < 0.5)) ur[i] = (float)(u - bf / z + gauss() * s);
  }
  if (bad_entries && n > 20) {
    kps[3].octave = 8;
    assign[3] = 0;
    assign[5] = (int)mps.size();
  }
  orbm_camera cam{fx, fy, cx, cy, bf / fx, bf, {1, 0, 0, 0.05f, 0, 1, 0, -0.03f, 0, 0, 1, 0.08f}};
  std::vector<float> Tcw(12);
  std::vector<uint8_t> outlier(n);
  orbm_pose pose;
  orbm_poseopt_result r;
  int status = -1;
  const int rc = orbm_pose_optimization_host(kps.data(), n, kind == 0 ? nullptr : ur.data(), assign.data(), mps.data(),
                                             (int)mps.size(), sig.data(), 8, &cam, ORBM_POSEOPT_DISCARD_OUTLIERS,
                                             Tcw.data(), &pose, outlier.data(), &r, &status);
  printf("n %d kind %d rc %d status %d ret %d of %d, bad %d, rounds %d, trials %d (%d rejected), t = %.4f %.4f %.4f\n", n,
         kind, rc, status, r.ret, r.n_initial, r.n_bad, r.rounds, r.trials, r.rejected, Tcw[3], Tcw[7], Tcw[11]);
  return rc;
}

int main() {
  int rc = 0;
  const int sizes[] = {0, 2, 9, 300, 3000};
  for (int n : sizes)
    for (int kind = 0; kind < 3; ++kind) rc |= run(n, kind, kind == 2);
  return rc ? 1 : 0;
}
