// orbx_optsim3.hip — Optimizer::OptimizeSim3 (src/Optimizer.cc:1190-1385): the
// host form and the kernel of orbm_optimize_sim3_batch, one workgroup of 256
// threads per keyframe pair, the whole refinement in one launch. The
// arithmetic is orbx_optsim3.cuh's for both.
//
// The workgroup builds vpMatches1 from the caller's lists (the kept matches
// mark their KF2 keypoints in a bitmap first, then every i1 applies the merge
// rule), compacts the edge pairs in i1 order into 56-byte Os3Edge records in
// LDS and never goes back to HBM for them. Per linearisation, threads 0..13
// write the 14 displaced estimates of the numeric Jacobian and their inverses
// to LDS (they are the same for every edge); then one lane per pair evaluates
// both edges, their 14 displaced errors each and the two quadratic forms into
// 36 sums of its own. Thread t owns pairs t, t + 256, ...; the wave adds its
// lanes with a fixed DPP tree and every thread adds the four waves' partial
// sums from LDS in wave order (BlockSum, orbx_wave.cuh). So a sum's bits
// depend on the pairs' order alone, not on the batch, the slot, the pitch or
// the run, and no floating-point atomic is involved. The 7x7 LDL^T, exp and
// the lambda logic run in every thread on the same reduced values (os3_run).
//
// A pair pitch above kOs3LdsCorr keeps its records and the bitmap in a
// workspace in device memory instead (written and read by the same workgroup).
#include <hip/hip_runtime.h>

#include <vector>

#include "orbx_optsim3.cuh"
#include "orbx_wave.cuh"

namespace orbx {

namespace {

constexpr int kT = 256, kW = kT / 64;

struct Os3Args {
  const orbx_kp *kps1, *kps2;
  const int *n1, *n2;
  int kp_pitch, mp_pitch;
  const orbm_map_point_world *mps1, *mps2;
  const orbm_camera *cam1, *cam2;
  const int* match12;
  const uint8_t* inlier;
  const int *found12, *found21;
  float inv_sigma2[kMaxLevels];
  int nlevels;
  const float *s12, *R12, *t12;
  Os3Huber K;
  int fix_scale;
  int* match12_out;
  double* S12;
  float* Scw;
  orbm_pose* pose;
  orbm_optsim3_result* result;
  double* lin;
  int* err;
  Os3Edge* rec_ws;     // spill: [pairs][kp_pitch]
  uint32_t* taken_ws;  // spill: [pairs][(kp_pitch + 31) / 32]
};

__device__ __forceinline__ int clampn(int n, int hi) { return n < 0 ? 0 : (n > hi ? hi : n); }

struct DeviceCtx {
  Os3Edge* E;
  int ne;
  Os3Cam cam;
  Os3Huber K;
  bool fix_scale;
  BlockSum<kW, kOs3Sums> red;
  Os3Est* D;    // LDS: kOs3Disp displaced estimates and inverses
  double* lin;  // where the first linearisation goes, or null
  bool first = true;

  __device__ void linearise(const Os3Est& est, bool, double* acc) {
    // the previous readers of D have passed a reduction's barrier since
    if (threadIdx.x < kOs3Disp / 2) os3_displace(est, fix_scale, threadIdx.x, &D[2 * threadIdx.x], &D[2 * threadIdx.x + 1]);
    __syncthreads();
    Os3Est inv;
    os3_inverse(est, &inv);
#pragma unroll
    for (int k = 0; k < kOs3Sums; ++k) acc[k] = 0.0;
    for (int i = threadIdx.x; i < ne; i += kT) {
      const Os3Edge e = E[i];
      if (!(e.tag & kOs3Removed)) os3_pair_linearise(cam, K, est, inv, D, e, acc);
    }
    red.sum<kOs3Sums>(acc);
    if (first && lin && threadIdx.x == 0) os3_store_lin(acc, lin);
    first = false;
  }
  __device__ double robust_chi2(const Os3Est& est, bool) {
    Os3Est inv;
    os3_inverse(est, &inv);
    double s = 0.0;
    for (int i = threadIdx.x; i < ne; i += kT) {
      const Os3Edge e = E[i];
      if (!(e.tag & kOs3Removed)) os3_pair_robust_chi2(cam, K, est, inv, e, &s);
    }
    red.sum<1>(&s);
    return s;
  }
  __device__ int classify(const Os3Est& err_est, uint32_t mark) {
    Os3Est inv;
    os3_inverse(err_est, &inv);
    int bad = 0;
    for (int i = threadIdx.x; i < ne; i += kT) {
      const Os3Edge e = E[i];
      if (e.tag & kOs3Removed) continue;
      double c12, c21;
      os3_pair_chi2(cam, err_est, inv, e, &c12, &c21);
      if (os3_is_outlier(K, c12, c21)) {
        E[i].tag = e.tag | mark;
        ++bad;
      }
    }
    return red.sum_int(bad);
  }
};

template <bool SPILL>
__global__ __launch_bounds__(kT) void optimize_sim3_kernel(const Os3Args A) {
  __shared__ Os3Edge rec[SPILL ? 1 : kOs3LdsCorr];
  __shared__ uint32_t taken_lds[SPILL ? 1 : kOs3LdsCorr / 32];
  __shared__ BlockSumLds<kW, kOs3Sums> sh;
  __shared__ Os3Est disp[kOs3Disp];
  __shared__ int scan[2][kW];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n1 = clampn(A.n1[p], A.kp_pitch), n2 = clampn(A.n2[p], A.kp_pitch);
  const size_t koff = (size_t)p * A.kp_pitch, moff = (size_t)p * A.mp_pitch;
  const orbx_kp* kps1 = A.kps1 + koff;
  const orbx_kp* kps2 = A.kps2 + koff;
  const orbm_map_point_world* mps1 = A.mps1 + moff;
  const orbm_map_point_world* mps2 = A.mps2 + moff;
  const int* match12 = A.match12 + koff;
  const uint8_t* inlier = A.inlier ? A.inlier + koff : nullptr;
  const int* found12 = A.found12 ? A.found12 + koff : nullptr;
  const int* found21 = A.found21 ? A.found21 + koff : nullptr;
  int* match12_out = A.match12_out ? A.match12_out + koff : nullptr;
  const int words = (A.kp_pitch + 31) / 32, cap = SPILL ? A.kp_pitch : kOs3LdsCorr;
  Os3Edge* E = SPILL ? A.rec_ws + koff : rec;
  uint32_t* taken = SPILL ? A.taken_ws + (size_t)p * words : taken_lds;
  const orbm_camera c1 = A.cam1[p], c2 = A.cam2[p];

  // the KF2 keypoints that kept matches target
  for (int w = tid; w < (n2 + 31) / 32; w += kT) taken[w] = 0u;
  __syncthreads();
  for (int i1 = tid; i1 < n1; i1 += kT)
    if (os3_kept(match12, inlier, i1) && match12[i1] < n2) atomicOr(&taken[match12[i1] >> 5], 1u << (match12[i1] & 31));
  __syncthreads();

  // vpMatches1 and the edge pairs, compacted in i1 order (:1243-1322)
  int ne = 0, bad = 0;
  for (int base = 0, par = 0; base < n1; base += kT, par ^= 1) {
    const int i1 = base + tid;
    bool valid = false;
    int i2 = -1, o1 = 0, o2 = 0;
    if (i1 < n1) {
      i2 = os3_merge(i1, n1, n2, match12, inlier, found12, found21,
                     [&](int k) { return (taken[k >> 5] >> (k & 31)) & 1u; }, &bad);
      if (match12_out) match12_out[i1] = i2;
      if (i2 >= 0 && mps1[i1].valid && mps2[i2].valid) {
        o1 = kps1[i1].octave;
        o2 = kps2[i2].octave;
        valid = o1 >= 0 && o1 < A.nlevels && o2 >= 0 && o2 < A.nlevels;
        bad |= valid ? 0 : 1;
      }
    }
    const uint64_t mask = __ballot(valid);
    int off = mbcnt64(mask);
    if (lane == 0) scan[par][wave] = __popcll(mask);
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int w = 0; w < kW; ++w) {
      const int c = scan[par][w];
      off += (w < wave) ? c : 0;
      total += c;
    }
    off += ne;
    ne += total;
    if (valid && off < cap) {  // off < n1 <= kp_pitch <= cap
      Os3Edge e;
      os3_make_edge(c1, c2, mps1[i1].pos, mps2[i2].pos, kps1[i1], kps2[i2], A.inv_sigma2[o1], A.inv_sigma2[o2], i1, &e);
      E[off] = e;
    }
  }
  ne = ne < cap ? ne : cap;
  if (bad) atomicOr(A.err, kStatusOptSim3Skipped);
  __syncthreads();  // the records are in place

  DeviceCtx ctx;
  ctx.E = E;
  ctx.ne = ne;
  ctx.cam = Os3Cam{(double)c1.fx, (double)c1.fy, (double)c1.cx, (double)c1.cy,
                   (double)c2.fx, (double)c2.fy, (double)c2.cx, (double)c2.cy};
  ctx.K = A.K;
  ctx.fix_scale = A.fix_scale != 0;
  ctx.red.sh = &sh;
  ctx.D = disp;
  ctx.lin = A.lin ? A.lin + (size_t)p * kOs3Sums : nullptr;

  Os3Est S0, S;
  os3_from_float(A.s12[p], A.R12 + (size_t)p * 9, 3, A.t12 + (size_t)p * 3, 1, &S0);
  Os3Stats st;
  os3_run(ctx, S0, ne, &S, &st);

  if (match12_out)
    for (int i = tid; i < ne; i += kT) {
      const Os3Edge e = E[i];
      if (e.tag & (kOs3Removed | kOs3Rejected)) match12_out[e.i1] = -1;
    }
  if (tid == 0) {
    if (ne == 0 && ctx.lin)
      for (int k = 0; k < kOs3Sums; ++k) ctx.lin[k] = 0.0;
    if (A.S12) {
      double* o = A.S12 + (size_t)p * 8;
      for (int k = 0; k < 4; ++k) o[k] = S.q[k];
      for (int k = 0; k < 3; ++k) o[4 + k] = S.t[k];
      o[7] = S.s;
    }
    float Scw[12];
    os3_scw(S, c2.Tcw, Scw);
    if (A.Scw)
      for (int k = 0; k < 12; ++k) A.Scw[(size_t)p * 12 + k] = Scw[k];
    if (A.pose) {
      orbm_pose ps;
      os3_pose(c1, Scw, &ps);
      A.pose[p] = ps;
    }
    if (A.result) A.result[p] = os3_result(st, ne);
  }
}

// the sums of os3_run over host edge pairs, pair after pair in i1 order
struct HostCtx {
  std::vector<Os3Edge>& E;
  Os3Cam cam;
  Os3Huber K;
  bool fix_scale;
  double* lin;
  bool first = true;
  void linearise(const Os3Est& est, bool, double* acc) {
    Os3Est D[kOs3Disp], inv;
    for (int k = 0; k < kOs3Disp / 2; ++k) os3_displace(est, fix_scale, k, &D[2 * k], &D[2 * k + 1]);
    os3_inverse(est, &inv);
    for (int k = 0; k < kOs3Sums; ++k) acc[k] = 0.0;
    for (const Os3Edge& e : E)
      if (!(e.tag & kOs3Removed)) os3_pair_linearise(cam, K, est, inv, D, e, acc);
    if (first && lin) os3_store_lin(acc, lin);
    first = false;
  }
  double robust_chi2(const Os3Est& est, bool) {
    Os3Est inv;
    os3_inverse(est, &inv);
    double s = 0.0;
    for (const Os3Edge& e : E)
      if (!(e.tag & kOs3Removed)) os3_pair_robust_chi2(cam, K, est, inv, e, &s);
    return s;
  }
  int classify(const Os3Est& err_est, uint32_t mark) {
    Os3Est inv;
    os3_inverse(err_est, &inv);
    int bad = 0;
    for (Os3Edge& e : E) {
      if (e.tag & kOs3Removed) continue;
      double c12, c21;
      os3_pair_chi2(cam, err_est, inv, e, &c12, &c21);
      if (os3_is_outlier(K, c12, c21)) {
        e.tag |= mark;
        ++bad;
      }
    }
    return bad;
  }
};

}  // namespace

size_t optsim3_ws_bytes(int kp_pitch, int pairs) {
  if (kp_pitch <= kOs3LdsCorr) return 0;
  const size_t rec = ((size_t)pairs * kp_pitch * sizeof(Os3Edge) + 255) & ~(size_t)255;
  return rec + (size_t)pairs * ((kp_pitch + 31) / 32) * sizeof(uint32_t);
}

int launch_optimize_sim3(const OptSim3Args& P, void* ws, void* stream) {
  Os3Args A{};
  A.kps1 = P.kps1;
  A.kps2 = P.kps2;
  A.n1 = P.n1;
  A.n2 = P.n2;
  A.kp_pitch = P.kp_pitch;
  A.mp_pitch = P.mp_pitch;
  A.mps1 = P.mps1;
  A.mps2 = P.mps2;
  A.cam1 = P.cam1;
  A.cam2 = P.cam2;
  A.match12 = P.match12;
  A.inlier = P.inlier;
  A.found12 = P.found12;
  A.found21 = P.found21;
  for (int l = 0; l < P.nlevels; ++l) A.inv_sigma2[l] = P.inv_sigma2[l];
  A.nlevels = P.nlevels;
  A.s12 = P.s12;
  A.R12 = P.R12;
  A.t12 = P.t12;
  A.K = os3_huber(P.th2);
  A.fix_scale = P.fix_scale;
  A.match12_out = P.match12_out;
  A.S12 = P.S12;
  A.Scw = P.Scw;
  A.pose = P.pose;
  A.result = P.result;
  A.lin = P.lin;
  A.err = P.err;
  hipStream_t s = (hipStream_t)stream;
  if (P.kp_pitch > kOs3LdsCorr) {
    A.rec_ws = (Os3Edge*)ws;
    const size_t rec = ((size_t)P.pairs * P.kp_pitch * sizeof(Os3Edge) + 255) & ~(size_t)255;
    A.taken_ws = (uint32_t*)((uint8_t*)ws + rec);
    hipLaunchKernelGGL(optimize_sim3_kernel<true>, dim3(P.pairs), dim3(kT), 0, s, A);
  } else {
    hipLaunchKernelGGL(optimize_sim3_kernel<false>, dim3(P.pairs), dim3(kT), 0, s, A);
  }
  return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
}

int optimize_sim3_host(const OptSim3Args& P, int n1, int n2, int* status) {
  int bad = 0;
  std::vector<uint8_t> taken(n2 > 0 ? n2 : 1, 0);
  for (int i1 = 0; i1 < n1; ++i1)
    if (os3_kept(P.match12, P.inlier, i1) && P.match12[i1] < n2) taken[P.match12[i1]] = 1;
  std::vector<Os3Edge> E;
  for (int i1 = 0; i1 < n1; ++i1) {
    const int i2 = os3_merge(i1, n1, n2, P.match12, P.inlier, P.found12, P.found21,
                             [&](int k) { return taken[k] != 0; }, &bad);
    if (P.match12_out) P.match12_out[i1] = i2;
    if (i2 < 0 || !P.mps1[i1].valid || !P.mps2[i2].valid) continue;
    const int o1 = P.kps1[i1].octave, o2 = P.kps2[i2].octave;
    if (o1 < 0 || o1 >= P.nlevels || o2 < 0 || o2 >= P.nlevels) {
      bad = 1;
      continue;
    }
    Os3Edge e;
    os3_make_edge(*P.cam1, *P.cam2, P.mps1[i1].pos, P.mps2[i2].pos, P.kps1[i1], P.kps2[i2], P.inv_sigma2[o1],
                  P.inv_sigma2[o2], i1, &e);
    E.push_back(e);
  }
  const int ne = (int)E.size();
  const orbm_camera &c1 = *P.cam1, &c2 = *P.cam2;
  HostCtx ctx{E,
              Os3Cam{(double)c1.fx, (double)c1.fy, (double)c1.cx, (double)c1.cy, (double)c2.fx, (double)c2.fy,
                     (double)c2.cx, (double)c2.cy},
              os3_huber(P.th2), P.fix_scale != 0, P.lin};
  Os3Est S0, S;
  os3_from_float(*P.s12, P.R12, 3, P.t12, 1, &S0);
  Os3Stats st;
  os3_run(ctx, S0, ne, &S, &st);
  if (P.match12_out)
    for (const Os3Edge& e : E)
      if (e.tag & (kOs3Removed | kOs3Rejected)) P.match12_out[e.i1] = -1;
  if (ne == 0 && P.lin)
    for (int k = 0; k < kOs3Sums; ++k) P.lin[k] = 0.0;
  if (P.S12) {
    for (int k = 0; k < 4; ++k) P.S12[k] = S.q[k];
    for (int k = 0; k < 3; ++k) P.S12[4 + k] = S.t[k];
    P.S12[7] = S.s;
  }
  float Scw[12];
  os3_scw(S, c2.Tcw, Scw);
  if (P.Scw)
    for (int k = 0; k < 12; ++k) P.Scw[k] = Scw[k];
  if (P.pose) os3_pose(c1, Scw, P.pose);
  if (P.result) *P.result = os3_result(st, ne);
  if (status) *status = bad ? kStatusOptSim3Skipped : 0;
  return ORBX_OK;
}

}  // namespace orbx
