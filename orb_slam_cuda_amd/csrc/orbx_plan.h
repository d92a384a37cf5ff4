// orbx_plan.h — the host plan of the extractor (orbx_plan.hip): plain host
// data in, plain host data out, no HIP runtime call.
#pragma once
#include <vector>

#include "orbx_internal.h"

namespace orbx {

// ORBextractor's constructor tables for one orbx_config (compute_scales)
struct ScaleTables {
  std::vector<float> scale, inv_scale, sigma2, inv_sigma2;
  std::vector<int> nfeat;
  int umax[16];
};

// What the kernels need for one (config, frame size, batch): the parameter
// block and the two tables uploaded beside it (build_plan_host)
struct HostPlan {
  int W = 0, H = 0, B = 0;
  long long level_bytes = 0;  // the planes of every level of B frames (pyramid and blur buffers)
  ExtractParams P{};
  std::vector<CellGeom> cells;
  std::vector<int2> rtab;
};

void compute_scales(const orbx_config& c, ScaleTables& t);
// Geometry, tables and tilings of W x H frames in batches of up to B. A
// configuration the kernels cannot run is ORBX_EINVAL with the reason in
// orbx_last_error; pl.P and pl.W/H/B are then as before the call.
int build_plan_host(const orbx_config& c, const ScaleTables& t, int W, int H, int B, HostPlan& pl);

// m = ceil(2^32 / d) when mulhi(id, m) == id / d for every id < d * batch, else
// 0 (the kernel divides): exact while id * (m * d - 2^32) < 2^32
unsigned exact_div_magic(unsigned long long d, unsigned long long batch);

}  // namespace orbx
