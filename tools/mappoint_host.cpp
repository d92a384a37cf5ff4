// The host algorithm the shim's stand-in MapPoint uses for
// ComputeDistinctiveDescriptors (shim/host/KeyFrame.h): per point the full
// N x N distance matrix, then a copy and std::sort of every row. Stand-alone,
// one core, for tools/mappoint_time.py.
//
// Input file: int32 points, int32 rows, uint32 off[points + 1], uint8 desc[rows][32]
// (each point's kept descriptors gathered in list order). Prints the median of
// 3 passes over all points in milliseconds and a checksum of the winners.
#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <vector>

static int descriptor_distance(const uint8_t* a, const uint8_t* b) {
  int d = 0;
  for (int k = 0; k < 32; ++k) d += __builtin_popcount((unsigned)(a[k] ^ b[k]));
  return d;
}

static size_t distinctive(const uint8_t* desc, size_t N) {
  std::vector<const uint8_t*> v;
  for (size_t i = 0; i < N; ++i) v.push_back(desc + 32 * i);
  std::vector<std::vector<int>> D(N, std::vector<int>(N, 0));
  for (size_t i = 0; i < N; ++i)
    for (size_t j = i + 1; j < N; ++j) D[i][j] = D[j][i] = descriptor_distance(v[i], v[j]);
  int best = INT_MAX;
  size_t bestIdx = 0;
  for (size_t i = 0; i < N; ++i) {
    std::vector<int> d = D[i];
    std::sort(d.begin(), d.end());
    const int median = d[(size_t)(0.5 * (N - 1))];
    if (median < best) {
      best = median;
      bestIdx = i;
    }
  }
  return bestIdx;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hdr[2];
  if (fread(hdr, 4, 2, f) != 2 || hdr[0] < 0 || hdr[1] < 0) return 2;
  std::vector<uint32_t> off((size_t)hdr[0] + 1);
  std::vector<uint8_t> desc((size_t)hdr[1] * 32);
  if (fread(off.data(), 4, off.size(), f) != off.size()) return 2;
  if (!desc.empty() && fread(desc.data(), 32, (size_t)hdr[1], f) != (size_t)hdr[1]) return 2;
  fclose(f);
  for (int p = 0; p < hdr[0]; ++p)
    if (off[p + 1] < off[p] || off[p + 1] > (uint32_t)hdr[1]) return 2;
  double ms[3];
  unsigned long long sum = 0;
  for (int rep = 0; rep < 3; ++rep) {
    const auto t0 = std::chrono::steady_clock::now();
    sum = 0;
    for (int p = 0; p < hdr[0]; ++p)
      if (off[p + 1] > off[p]) sum += distinctive(desc.data() + 32 * (size_t)off[p], off[p + 1] - off[p]);
    ms[rep] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  std::sort(ms, ms + 3);
  printf("{\"ms\": %.4f, \"winner_sum\": %llu}\n", ms[1], sum);
  return 0;
}
