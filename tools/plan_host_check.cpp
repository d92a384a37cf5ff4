// The extractor's host plan (csrc/orbx_plan.hip) stand-alone, for a run under
// AddressSanitizer and UBSan on the CPU (no device is touched):
//   cd orb_slam_cuda_amd/csrc && make
//   S="-fsanitize=address,undefined"; F="--offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=off -I../../include"
//   hipcc $F -Xarch_host $S -c orbx_plan.hip -o /tmp/plan_san.o
//   g++ -O1 -g -std=c++17 -I../../include $S -c ../../tools/plan_host_check.cpp -o /tmp/plan_main.o
//   hipcc --offload-arch=gfx950 $S /tmp/plan_main.o /tmp/plan_san.o $(ls build/*.o | grep -v orbx_plan) \
//     -o /tmp/plan_host_check && /tmp/plan_host_check
// The planner is then instrumented (orbx_plan.hip is compiled with the
// sanitizers); the other objects only satisfy the link (make removes objects
// of sources that no longer exist, so the glob holds the current ones only).
// Plans the configurations of tests/test_plan.py, each twice (the digests must
// repeat), their band-pyramid records, two sizes in turn in one process, and
// the configurations the planner refuses. Prints each digest; exit status 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "orbx_c.h"

extern "C" int orbx_plan_digest(const orbx_config* cfg, unsigned long long out[3]);
extern "C" int orbx_pyr_plan_check(const orbx_config* cfg, long long* records, int cap, int* nplans);

static orbx_config config(int W, int H, int nl, float sf, int B, int mode) {
  orbx_config c;
  memset(&c, 0, sizeof c);
  c.nfeatures = 2000;
  c.scale_factor = sf;
  c.nlevels = nl;
  c.ini_th_fast = 20;
  c.min_th_fast = 7;
  c.width = W;
  c.height = H;
  c.max_batch = B;
  c.scale_mode = mode;
  return c;
}

static int plan(const char* name, int W, int H, int nl, float sf, int B, int mode) {
  const orbx_config c = config(W, H, nl, sf, B, mode);
  unsigned long long a[3], b[3];
  if (orbx_plan_digest(&c, a) || orbx_plan_digest(&c, b)) {
    printf("%s %dx%d: %s\n", name, W, H, orbx_last_error());
    return 1;
  }
  if (memcmp(a, b, sizeof a)) {
    printf("%s %dx%d: two runs differ\n", name, W, H);
    return 1;
  }
  long long records[8];
  int nplans = 0;
  if (orbx_pyr_plan_check(&c, records, 8, &nplans)) {
    printf("%s %dx%d: %s\n", name, W, H, orbx_last_error());
    return 1;
  }
  for (int i = 0; i < nplans; ++i)
    if (records[i] < 0) {
      printf("%s %dx%d: plan %d fails its bounds\n", name, W, H, i);
      return 1;
    }
  printf("%-12s %4dx%-4d L%-2d sf%.1f B%-2d mode%d  %016llx %016llx %016llx  %d band plans\n", name, W, H, nl, sf, B, mode,
         a[0], a[1], a[2], nplans);
  return 0;
}

static int refused(const char* name, int W, int H, int nl, float sf, int B) {
  const orbx_config c = config(W, H, nl, sf, B, 0);
  unsigned long long a[3];
  const int rc = orbx_plan_digest(&c, a);
  printf("%-12s %4dx%-4d L%-2d: %d %s\n", name, W, H, nl, rc, rc ? orbx_last_error() : "planned (expected a refusal)");
  return rc == ORBX_EINVAL ? 0 : 1;
}

int main() {
  static const struct { const char* name; int W, H, nl; float sf; int B; } G[] = {
      {"kitti", 1241, 376, 8, 1.2f, 64}, {"euroc", 752, 480, 8, 1.2f, 64}, {"kitti14", 1226, 370, 10, 1.2f, 64},
      {"intcatch1080", 1920, 1080, 3, 1.2f, 16}, {"small", 208, 131, 4, 1.2f, 3}, {"small", 209, 131, 4, 1.2f, 3},
      {"small", 201, 131, 4, 1.2f, 3}, {"small", 203, 131, 4, 1.2f, 3}, {"small", 207, 131, 4, 1.2f, 3},
      {"small", 219, 140, 4, 1.2f, 3}, {"small", 640, 131, 4, 1.2f, 3}, {"small2", 203, 131, 2, 2.0f, 3},
      {"small2", 204, 132, 2, 2.0f, 3}, {"l8", 651, 459, 8, 1.2f, 3}, {"s2", 652, 520, 3, 2.0f, 3},
      {"s2", 651, 519, 3, 2.0f, 3}, {"tum", 640, 480, 8, 1.2f, 1}, {"hd", 1280, 720, 8, 1.2f, 8},
      {"kitti_b1", 1241, 376, 8, 1.2f, 1}, {"odd", 1023, 767, 6, 1.3f, 2}, {"deep", 2048, 1536, 12, 1.2f, 1}};
  int bad = 0;
  for (const auto& g : G) bad += plan(g.name, g.W, g.H, g.nl, g.sf, g.B, ORBX_SCALE_U);
  bad += plan("kitti_modeF", 1241, 376, 8, 1.2f, 64, ORBX_SCALE_F);
  setenv("ORBX_QT_GENERIC", "1", 1);
  bad += plan("kitti_generic", 1241, 376, 8, 1.2f, 64, ORBX_SCALE_U);
  unsetenv("ORBX_QT_GENERIC");
  setenv("ORBX_QT_SORTED", "0", 1);
  bad += plan("kitti_legacy", 1241, 376, 8, 1.2f, 64, ORBX_SCALE_U);
  unsetenv("ORBX_QT_SORTED");
  // a handle re-plans when the image size changes: two sizes in turn, twice
  for (int k = 0; k < 2; ++k) {
    bad += plan("replan", 752, 480, 8, 1.2f, 1, ORBX_SCALE_U);
    bad += plan("replan", 209, 131, 4, 1.2f, 1, ORBX_SCALE_U);
  }
  bad += refused("tiny_level", 208, 131, 8, 1.2f, 1);    // a level smaller than one FAST cell
  bad += refused("over_4096", 4200, 400, 2, 1.2f, 1);    // a level over 4096 px
  bad += refused("tall", 200, 900, 2, 1.2f, 1);          // nIni = 0
  printf(bad ? "FAILED: %d\n" : "ok\n", bad);
  return bad ? 1 : 0;
}
