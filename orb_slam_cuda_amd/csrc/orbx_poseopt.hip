// orbx_poseopt.hip — Optimizer::PoseOptimization (src/Optimizer.cc:334-543),
// one workgroup per frame, the whole solve in one launch.
//
// The workgroup compacts the frame's correspondences (keypoints with a map
// point), in keypoint order, into 32-byte PoEdge records in LDS and never goes
// back to HBM for them: every linearisation, every trial and the four
// classifications read LDS. Thread t owns edges t, t + T, t + 2T, ... (T
// threads): it adds its edges' terms in that order, the wave adds its lanes
// with a fixed DPP tree, and every thread then adds the waves' partial sums
// from LDS in wave order. So a sum's bits depend on the edges' order in the
// frame alone, not on the batch, the slot or the run, and no floating-point
// atomic is involved (BlockSum, orbx_wave.cuh). Two LDS buffers alternate, so a
// reduction costs one barrier. The 6x6 solve, exp and the lambda logic run in every thread on the
// same reduced values (po_run): nobody waits for a thread 0 and a broadcast.
//
// A frame pitch above kPoLdsEdges keeps its edge records in a workspace in
// device memory instead (written once, read by the same workgroup).
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "orbx_poseopt.cuh"
#include "orbx_wave.cuh"

namespace orbx {

namespace {

template <int T, class EdgePtr>
struct DeviceCtx {
  static constexpr int W = T / 64;
  EdgePtr E;
  int ne;
  PoCam cam;
  BlockSum<W, kPoSums> red;  // the reductions' LDS and order (orbx_wave.cuh)

  template <int N>
  __device__ void block_sum(double* v) {
    red.template sum<N>(v);
  }
  __device__ int block_sum_int(int v) { return red.sum_int(v); }

  __device__ void linearise(const PoPose& est, bool robust, double* acc) {
#pragma unroll
    for (int k = 0; k < kPoSums; ++k) acc[k] = 0.0;
    for (int i = threadIdx.x; i < ne; i += T) {
      const PoEdge e = E[i];
      if (!(e.tag & kPoOutlier)) po_edge_linearise(cam, est, e, robust, acc);
    }
    block_sum<kPoSums>(acc);
  }
  __device__ double robust_chi2(const PoPose& est, bool robust) {
    double s = 0.0;
    for (int i = threadIdx.x; i < ne; i += T) {
      const PoEdge e = E[i];
      if (!(e.tag & kPoOutlier)) s += po_edge_robust_chi2(cam, est, e, robust);
    }
    block_sum<1>(&s);
    return s;
  }
  __device__ int classify(const PoPose& est, const PoPose& err_pose) {
    int bad = 0;
    for (int i = threadIdx.x; i < ne; i += T) {
      const PoEdge e = E[i];
      const double chi2 = po_edge_chi2(cam, (e.tag & kPoOutlier) ? est : err_pose, e);
      const bool out = po_is_outlier(e, chi2);
      E[i].tag = out ? (e.tag | kPoOutlier) : (e.tag & ~kPoOutlier);
      bad += out ? 1 : 0;
    }
    return block_sum_int(bad);
  }
};

struct PoArgs {
  const orbx_kp* kps;
  const int* n;
  int kp_pitch;
  const float* uright;  // or null: a monocular frame
  int* assign;
  const orbm_map_point_world* mps;
  const int* nmp;
  int mp_pitch;
  float inv_sigma2[kMaxLevels];
  int nlevels;
  const orbm_camera* cams;
  int flags;
  float* Tcw;               // or null
  orbm_pose* pose;          // or null
  uint8_t* outlier;         // or null
  orbm_poseopt_result* result;  // or null
  int* err;
  PoEdge* spill;  // SPILL: frames x kp_pitch records
};

template <int T, bool SPILL>
__global__ __launch_bounds__(T) void pose_optimization_kernel(const PoArgs A) {
  constexpr int W = T / 64;
  extern __shared__ __align__(16) unsigned char po_lds[];
  __shared__ BlockSumLds<W, kPoSums> sh;
  __shared__ int scan[2][W];
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int n = A.n[f];
  n = n < 0 ? 0 : (n > A.kp_pitch ? A.kp_pitch : n);
  int nmp = A.nmp[f];
  nmp = nmp < 0 ? 0 : (nmp > A.mp_pitch ? A.mp_pitch : nmp);
  const orbx_kp* kps = A.kps + (size_t)f * A.kp_pitch;
  const float* ur = A.uright ? A.uright + (size_t)f * A.kp_pitch : nullptr;
  int* assign = A.assign + (size_t)f * A.kp_pitch;
  const orbm_map_point_world* mps = A.mps + (size_t)f * A.mp_pitch;
  using EdgePtr = PoEdge*;
  EdgePtr E = SPILL ? A.spill + (size_t)f * A.kp_pitch : reinterpret_cast<PoEdge*>(po_lds);

  // the correspondences, compacted in keypoint order (:374-453)
  int ne = 0, bad_input = 0;
  for (int base = 0, par = 0; base < n; base += T, par ^= 1) {
    const int i = base + tid;
    bool valid = false;
    int row = -1, octave = 0;
    if (i < n) {
      row = assign[i];
      if (row >= 0) {
        octave = kps[i].octave;
        valid = row < nmp && octave >= 0 && octave < A.nlevels;
        bad_input |= valid ? 0 : 1;
      }
    }
    const uint64_t mask = __ballot(valid);
    int off = mbcnt64(mask);
    if (W > 1) {
      if (lane == 0) scan[par][wave] = __popcll(mask);
      __syncthreads();
      int total = 0;
#pragma unroll
      for (int w = 0; w < W; ++w) {
        const int c = scan[par][w];
        off += (w < wave) ? c : 0;
        total += c;
      }
      off += ne;
      ne += total;
    } else {
      off += ne;
      ne += __popcll(mask);
    }
    if (valid) {
      const orbm_map_point_world& mp = mps[row];
      const float u = ur ? ur[i] : -1.0f;
      PoEdge e;
      e.X[0] = mp.pos[0];
      e.X[1] = mp.pos[1];
      e.X[2] = mp.pos[2];
      e.obs[0] = kps[i].x;
      e.obs[1] = kps[i].y;
      e.obs[2] = u;
      e.w = A.inv_sigma2[octave];
      e.tag = (uint32_t)i | (u < 0 ? 0u : kPoStereo) | (mp.obs_positive ? kPoObs : 0u);
      E[off] = e;
    }
  }
  if (bad_input) atomicOr(A.err, kStatusPoseOptSkipped);
  __syncthreads();  // the edges are in place

  const orbm_camera cam = A.cams[f];
  DeviceCtx<T, EdgePtr> ctx;
  ctx.E = E;
  ctx.ne = ne;
  ctx.cam = PoCam{(double)cam.fx, (double)cam.fy, (double)cam.cx, (double)cam.cy, (double)cam.mbf};
  ctx.red.sh = &sh;

  PoStats st{0, 0, 0, 0};
  float Tout[12];
  for (int k = 0; k < 12; ++k) Tout[k] = cam.Tcw[k];
  if (ne >= 3) {  // :456
    PoPose T0, est;
    po_from_Tcw(cam.Tcw, &T0);
    po_run(ctx, T0, ne, &est, &st);
    po_to_Tcw(est, Tout);
  }
  // mvbOutlier, the discarded matches of src/Tracking.cc:983-988 and nmatchesMap
  int with_obs = 0;
  for (int i = tid; i < ne; i += T) {
    const uint32_t tag = E[i].tag;
    const int kp = (int)(tag & kPoIndexMask);
    const bool out = (tag & kPoOutlier) != 0;
    if (A.outlier) A.outlier[(size_t)f * A.kp_pitch + kp] = out ? 1 : 0;
    if (out && (A.flags & ORBM_POSEOPT_DISCARD_OUTLIERS)) assign[kp] = -1;
    with_obs += (!out && (tag & kPoObs)) ? 1 : 0;
  }
  with_obs = ctx.block_sum_int(with_obs);
  if (tid == 0) {
    if (A.Tcw)
      for (int k = 0; k < 12; ++k) A.Tcw[(size_t)f * 12 + k] = Tout[k];
    if (A.pose) {
      orbm_pose p;
      pose_from_rt(cam, Tout, &p);
      A.pose[f] = p;
    }
    if (A.result) {
      orbm_poseopt_result r;
      r.ret = ne >= 3 ? ne - st.n_bad : 0;
      r.n_initial = ne;
      r.n_bad = st.n_bad;
      r.n_inliers_with_obs = with_obs;
      r.rounds = st.rounds;
      r.trials = st.trials;
      r.rejected = st.rejected;
      r.reserved = 0;
      A.result[f] = r;
    }
  }
}

template <int T>
int launch_t(const PoArgs& A, int frames, bool spill, size_t lds, hipStream_t s) {
  if (spill) {
    hipLaunchKernelGGL((pose_optimization_kernel<T, true>), dim3(frames), dim3(T), 0, s, A);
  } else {
    if (raise_lds_limit((const void*)pose_optimization_kernel<T, false>, lds)) return ORBX_EDEVICE;
    hipLaunchKernelGGL((pose_optimization_kernel<T, false>), dim3(frames), dim3(T), lds, s, A);
  }
  return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
}

}  // namespace

size_t poseopt_spill_bytes(int kp_pitch, int frames) {
  return kp_pitch > kPoLdsEdges ? (size_t)frames * kp_pitch * sizeof(PoEdge) : 0;
}

int launch_pose_optimization(const PoseOptArgs& P, void* spill, void* stream) {
  PoArgs A{};
  A.kps = P.kps;
  A.n = P.n;
  A.kp_pitch = P.kp_pitch;
  A.uright = P.uright;
  A.assign = P.assign;
  A.mps = P.mps;
  A.nmp = P.nmp;
  A.mp_pitch = P.mp_pitch;
  for (int l = 0; l < P.nlevels; ++l) A.inv_sigma2[l] = P.inv_sigma2[l];
  A.nlevels = P.nlevels;
  A.cams = P.cams;
  A.flags = P.flags;
  A.Tcw = P.Tcw;
  A.pose = P.pose;
  A.outlier = P.outlier;
  A.result = P.result;
  A.err = P.err;
  A.spill = (PoEdge*)spill;
  const bool sp = P.kp_pitch > kPoLdsEdges;
  const size_t lds = sp ? 0 : (size_t)P.kp_pitch * sizeof(PoEdge);
  // diagnostics (tools/poseopt_timing.py): the workgroup sizes measured against the default
  static const int threads = [] {
    const char* e = std::getenv("ORBX_POSEOPT_THREADS");
    const int t = e ? std::atoi(e) : 0;
    return (t == 64 || t == 128) ? t : 256;
  }();
  hipStream_t s = (hipStream_t)stream;
  if (threads == 64) return launch_t<64>(A, P.frames, sp, lds, s);
  if (threads == 128) return launch_t<128>(A, P.frames, sp, lds, s);
  return launch_t<256>(A, P.frames, sp, lds, s);
}

}  // namespace orbx
