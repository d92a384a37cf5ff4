// orbx_sim3.hip — Sim3Solver (src/Sim3Solver.cc): the host form and the kernels
// of orbm_sim3_ransac_batch. The arithmetic is orbx_sim3.cuh's for both.
//
// sim3_solve_count_kernel, grid (hypothesis chunks, pairs), 256 threads: the
// workgroup gathers its pair's correspondences, in i1 order, into LDS (13
// floats each, structure of arrays); lanes 0..kSim3Chunk-1 draw and solve one
// hypothesis each, cv::eigen's work arrays in LDS because a Jacobi rotation's
// rows are run-time indices; then each wave takes every fourth hypothesis of
// the chunk, its lanes stride the list and the flags are added with a DPP
// tree. Count, draws and (s, R, t) of every hypothesis go to the handle's
// workspace (and to the caller's hyp array).
// sim3_select_kernel, one workgroup per pair: the selection rule over the
// counts, the flags of the accepted hypothesis once more, inlier, the result
// and the two orbm_pose records.
// A pair pitch above kSim3LdsCorr gathers once into the workspace
// (sim3_gather_kernel) and both kernels read the list from there.
// Counts are integers and no sum is reordered, so a pair's output bits do not
// depend on the batch, the slot, the run or the split into chunks.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <vector>

#include "orbx_sim3.cuh"
#include "orbx_wave.cuh"

namespace orbx {

namespace {

constexpr int kT = 256, kW = kT / 64;

struct Sim3Args {
  const orbx_kp *kps1, *kps2;
  const int *n1, *n2;
  int kp_pitch, mp_pitch;
  const orbm_map_point_world *mps1, *mps2;
  const orbm_camera *cam1, *cam2;
  const int *match12, *kp_index1;
  float max_err[kMaxLevels];
  int nlevels;
  int min_inliers, max_iterations, fix_scale, first_iteration, best_inliers;
  const int* its_tab;  // [kp_pitch + 1]
  const uint32_t* rand3;
  orbm_sim3_result* result;
  float *s12, *R12, *t12;
  orbm_pose* pose;
  uint8_t* inlier;
  orbm_sim3_hyp* hyp;
  orbm_sim3_hyp* hyp_ws;  // [pairs][max_iterations]
  float* rec_ws;          // spill: [pairs][kSim3Fields][kp_pitch]
  int* n_ws;              // spill: [pairs]
  int* err;
};

__device__ __forceinline__ int clampn(int n, int hi) { return n < 0 ? 0 : (n > hi ? hi : n); }

// The constructor's loop (:62-103) for pair p: the correspondences compacted
// in i1 order into R (room for `cap`). Returns N, the same in every thread.
// scan: [2][kW] ints of LDS. Ends with a barrier: the records are in place.
__device__ int sim3_gather(const Sim3Args& A, int p, const Sim3Recs& R, int cap, int (*scan)[kW]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n1 = clampn(A.n1[p], A.kp_pitch), n2 = clampn(A.n2[p], A.kp_pitch);
  const orbx_kp* kps1 = A.kps1 + (size_t)p * A.kp_pitch;
  const orbx_kp* kps2 = A.kps2 + (size_t)p * A.kp_pitch;
  const orbm_map_point_world* mps1 = A.mps1 + (size_t)p * A.mp_pitch;
  const orbm_map_point_world* mps2 = A.mps2 + (size_t)p * A.mp_pitch;
  const int* match12 = A.match12 + (size_t)p * A.kp_pitch;
  const int* kpi = A.kp_index1 ? A.kp_index1 + (size_t)p * A.kp_pitch : nullptr;
  const orbm_camera c1 = A.cam1[p], c2 = A.cam2[p];
  int N = 0, bad = 0;
  for (int base = 0, par = 0; base < n1; base += kT, par ^= 1) {
    const int i1 = base + tid;
    bool valid = false;
    int i2 = -1, o1 = 0, o2 = 0;
    if (i1 < n1) {
      i2 = match12[i1];
      if (i2 >= 0) {
        if (i2 >= n2) {
          bad = 1;
        } else if (mps1[i1].valid && mps2[i2].valid) {
          const int k1 = kpi ? kpi[i1] : i1;
          if (k1 >= n1) {
            bad = 1;
          } else if (k1 >= 0) {
            o1 = kps1[k1].octave;
            o2 = kps2[i2].octave;
            valid = o1 >= 0 && o1 < A.nlevels && o2 >= 0 && o2 < A.nlevels;
            bad |= valid ? 0 : 1;
          }
        }
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
    off += N;
    N += total;
    if (valid) {
      if (off < cap)
        sim3_make_record(c1, c2, mps1[i1].pos, mps2[i2].pos, A.max_err[o1], A.max_err[o2], i1, R, off);
      else
        bad = 1;
    }
  }
  if (bad) atomicOr(A.err, kStatusSim3Skipped);
  __syncthreads();
  return N < cap ? N : cap;
}

__device__ __forceinline__ int sim3_max_its(const Sim3Args& A, int N) {
  return (N >= A.min_inliers && N >= 3) ? A.its_tab[N] : 0;
}

__global__ __launch_bounds__(kT) void sim3_gather_kernel(const Sim3Args A) {
  __shared__ int scan[2][kW];
  const int p = blockIdx.x;
  const Sim3Recs R{A.rec_ws + (size_t)p * kSim3Fields * A.kp_pitch, A.kp_pitch};
  const int N = sim3_gather(A, p, R, A.kp_pitch, scan);
  if (threadIdx.x == 0) A.n_ws[p] = N;
}

template <bool SPILL>
__global__ __launch_bounds__(kT) void sim3_solve_count_kernel(const Sim3Args A) {
  __shared__ float rec[SPILL ? 1 : kSim3Fields * kSim3LdsCorr];
  __shared__ int scan[2][kW];
  __shared__ Sim3Jacobi jac[kSim3Chunk];
  __shared__ orbm_sim3_hyp hs[kSim3Chunk];
  const int p = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h0 = A.first_iteration + (int)blockIdx.x * kSim3Chunk;
  Sim3Recs R;
  int N;
  if (SPILL) {
    R = Sim3Recs{A.rec_ws + (size_t)p * kSim3Fields * A.kp_pitch, A.kp_pitch};
    N = A.n_ws[p];
  } else {
    R = Sim3Recs{rec, kSim3LdsCorr};
    N = sim3_gather(A, p, R, kSim3LdsCorr, scan);
  }
  const int max_its = sim3_max_its(A, N);
  if (h0 >= max_its) return;  // the whole workgroup
  const int nh = min(kSim3Chunk, max_its - h0);
  if (tid < nh) {
    const int h = h0 + tid;
    const uint32_t* r3 = A.rand3 + ((size_t)p * A.max_iterations + h) * 3;
    const uint32_t r[3] = {r3[0], r3[1], r3[2]};
    orbm_sim3_hyp H;
    sim3_draw(r, N, H.idx);
    float P1[3][3], P2[3][3];
    for (int k = 0; k < 3; ++k)
      for (int c = 0; c < 3; ++c) {
        P1[k][c] = R.at(c, H.idx[k]);
        P2[k][c] = R.at(3 + c, H.idx[k]);
      }
    sim3_solve(P1, P2, A.fix_scale != 0, &jac[tid], &H.s, H.R, H.t);
    H.count = 0;
    hs[tid] = H;
  }
  __syncthreads();
  const orbm_camera c1 = A.cam1[p], c2 = A.cam2[p];
  for (int j = wave; j < nh; j += kW) {
    float S12[12], S21[12];
    sim3_transforms(hs[j].s, hs[j].R, hs[j].t, S12, S21);
    int cnt = 0;
    for (int k = lane; k < N; k += 64) cnt += sim3_is_inlier(S12, S21, c1, c2, R, k) ? 1 : 0;
    cnt = wave_sum_dpp(cnt);
    if (lane == 0) {
      orbm_sim3_hyp H = hs[j];
      H.count = cnt;
      const size_t at = (size_t)p * A.max_iterations + (h0 + j);
      A.hyp_ws[at] = H;
      if (A.hyp) A.hyp[at] = H;
    }
  }
}

template <bool SPILL>
__global__ __launch_bounds__(kT) void sim3_select_kernel(const Sim3Args A) {
  __shared__ float rec[SPILL ? 1 : kSim3Fields * kSim3LdsCorr];
  __shared__ int scan[2][kW];
  __shared__ int counts[kSim3MaxIts];
  __shared__ Sim3Selection sel_sh;
  const int p = blockIdx.x, tid = threadIdx.x;
  const int n1 = clampn(A.n1[p], A.kp_pitch);
  Sim3Recs R;
  int N;
  if (SPILL) {
    R = Sim3Recs{A.rec_ws + (size_t)p * kSim3Fields * A.kp_pitch, A.kp_pitch};
    N = A.n_ws[p];
  } else {
    R = Sim3Recs{rec, kSim3LdsCorr};
    N = sim3_gather(A, p, R, kSim3LdsCorr, scan);
  }
  const int max_its = sim3_max_its(A, N);
  const orbm_sim3_hyp* hyp = A.hyp_ws + (size_t)p * A.max_iterations;
  for (int h = A.first_iteration + tid; h < max_its; h += kT) counts[h] = hyp[h].count;
  __syncthreads();
  if (tid == 0)
    sel_sh = sim3_select(A.first_iteration, max_its, A.min_inliers, A.best_inliers, [&](int h) { return counts[h]; });
  uint8_t* inlier = A.inlier ? A.inlier + (size_t)p * A.kp_pitch : nullptr;
  if (inlier)
    for (int i = tid; i < n1; i += kT) inlier[i] = 0;
  __syncthreads();  // the selection is known, the zeros are ordered before the flags
  const Sim3Selection S = sel_sh;
  const int chosen = S.accepted >= 0 ? S.accepted : S.best_iteration;
  if (S.accepted >= 0 && inlier) {
    const orbm_camera c1 = A.cam1[p], c2 = A.cam2[p];
    float S12[12], S21[12];
    sim3_transforms(hyp[chosen].s, hyp[chosen].R, hyp[chosen].t, S12, S21);
    for (int k = tid; k < N; k += kT)
      if (sim3_is_inlier(S12, S21, c1, c2, R, k)) inlier[s3_f2i(R.at(12, k))] = 1;
  }
  if (tid == 0) {
    if (A.result) A.result[p] = sim3_result(S, S.accepted >= 0 ? counts[S.accepted] : 0, N, max_its, A.first_iteration);
    if (chosen >= 0) {
      const orbm_sim3_hyp H = hyp[chosen];
      if (A.s12) A.s12[p] = H.s;
      if (A.R12)
        for (int k = 0; k < 9; ++k) A.R12[(size_t)p * 9 + k] = H.R[k];
      if (A.t12)
        for (int k = 0; k < 3; ++k) A.t12[(size_t)p * 3 + k] = H.t[k];
      if (A.pose) {
        orbm_pose out[2];
        const orbm_camera c1 = A.cam1[p], c2 = A.cam2[p];
        sim3_match_poses(c1, c1.Tcw, c2.Tcw, H.s, H.R, H.t, out);
        A.pose[2 * (size_t)p] = out[0];
        A.pose[2 * (size_t)p + 1] = out[1];
      }
    }
  }
}

}  // namespace

void sim3_ws_bytes(int kp_pitch, int pairs, int max_iterations, size_t* hyp_bytes, size_t* rec_bytes) {
  *hyp_bytes = ((size_t)pairs * max_iterations * sizeof(orbm_sim3_hyp) + 255) & ~(size_t)255;
  *rec_bytes = kp_pitch > kSim3LdsCorr
                   ? (((size_t)pairs * kSim3Fields * kp_pitch * sizeof(float) + 255) & ~(size_t)255) + 256 +
                         (size_t)pairs * sizeof(int)
                   : 0;
}

int launch_sim3_ransac(const Sim3LaunchArgs& P, void* ws, void* stream) {
  Sim3Args A{};
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
  A.kp_index1 = P.kp_index1;
  for (int l = 0; l < P.nlevels; ++l) A.max_err[l] = sim3_max_error(P.level_sigma2[l]);
  A.nlevels = P.nlevels;
  A.min_inliers = P.params.min_inliers;
  A.max_iterations = P.params.max_iterations;
  A.fix_scale = P.params.fix_scale;
  A.first_iteration = P.params.first_iteration;
  A.best_inliers = P.params.best_inliers;
  A.its_tab = P.its_tab;
  A.rand3 = P.rand3;
  A.result = P.result;
  A.s12 = P.s12;
  A.R12 = P.R12;
  A.t12 = P.t12;
  A.pose = P.pose;
  A.inlier = P.inlier;
  A.hyp = P.hyp;
  A.err = P.err;
  size_t hyp_bytes, rec_bytes;
  sim3_ws_bytes(P.kp_pitch, P.pairs, P.params.max_iterations, &hyp_bytes, &rec_bytes);
  A.hyp_ws = (orbm_sim3_hyp*)ws;
  const bool spill = rec_bytes != 0;
  if (spill) {
    A.rec_ws = (float*)((uint8_t*)ws + hyp_bytes);
    A.n_ws = (int*)((uint8_t*)ws + hyp_bytes + rec_bytes - (size_t)P.pairs * sizeof(int));
  }
  hipStream_t s = (hipStream_t)stream;
  const int left = P.params.max_iterations - P.params.first_iteration;
  const dim3 grid((left + kSim3Chunk - 1) / kSim3Chunk, P.pairs);
  if (spill) {
    hipLaunchKernelGGL(sim3_gather_kernel, dim3(P.pairs), dim3(kT), 0, s, A);
    if (left > 0) hipLaunchKernelGGL(sim3_solve_count_kernel<true>, grid, dim3(kT), 0, s, A);
    hipLaunchKernelGGL(sim3_select_kernel<true>, dim3(P.pairs), dim3(kT), 0, s, A);
  } else {
    if (left > 0) hipLaunchKernelGGL(sim3_solve_count_kernel<false>, grid, dim3(kT), 0, s, A);
    hipLaunchKernelGGL(sim3_select_kernel<false>, dim3(P.pairs), dim3(kT), 0, s, A);
  }
  return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
}

// SetRansacParameters (:125-135) for N correspondences
int sim3_iterations(double probability, int min_inliers, int max_iterations, int N) {
  if (N < min_inliers || N < 3) return 0;
  if (min_inliers == N) return 1;  // max(1, min(1, max_iterations)), max_iterations >= 1
  const float epsilon = (float)min_inliers / N;
  const double v = std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)epsilon, 3)));
  // Limited in double: beyond int's range (N above ~1300 * min_inliers) the reference's conversion to int
  // is undefined; the formula's meaning there is "more than max_iterations". A NaN (probability > 1) gives 1.
  if (v != v) return 1;
  if (v >= (double)max_iterations) return max_iterations;
  return v < 1.0 ? 1 : (int)v;
}

}  // namespace orbx

using namespace orbx;

extern "C" {

int orbm_sim3_rand_fill(uint32_t* out, int iterations) {
  static_assert(RAND_MAX == 2147483647, "the draws assume glibc's RAND_MAX");
  if (!out || iterations < 0) return ORBX_EINVAL;
  for (int k = 0; k < 3 * iterations; ++k) out[k] = (uint32_t)rand();
  return ORBX_OK;
}

int orbm_sim3_limits(int* max_iterations, int* chunk, int* lds_pitch) {
  if (max_iterations) *max_iterations = kSim3MaxIts;
  if (chunk) *chunk = kSim3Chunk;
  if (lds_pitch) *lds_pitch = kSim3LdsCorr;
  return ORBX_OK;
}

int orbm_sim3_iteration_table(double probability, int min_inliers, int max_iterations, int n_max, int* out) {
  if (!out || n_max < 0 || max_iterations < 1) return ORBX_EINVAL;
  for (int N = 0; N <= n_max; ++N) out[N] = sim3_iterations(probability, min_inliers, max_iterations, N);
  return ORBX_OK;
}

}  // extern "C"

namespace orbx {

int sim3_ransac_host(const orbx_kp* kps1, int n1, const orbx_kp* kps2, int n2, const orbm_map_point_world* mps1,
                     const orbm_map_point_world* mps2, const orbm_camera* cam1, const orbm_camera* cam2,
                     const int* match12, const int* kp_index1, const float* level_sigma2, int nlevels,
                     const orbm_sim3_params* params, const uint32_t* rand3, orbm_sim3_result* result, float* s12,
                     float* R12, float* t12, orbm_pose* pose, uint8_t* inlier, orbm_sim3_hyp* hyp, int* status) {
  float max_err[kMaxLevels];
  for (int l = 0; l < nlevels; ++l) max_err[l] = sim3_max_error(level_sigma2[l]);
  // the constructor's gather
  std::vector<float> rec((size_t)kSim3Fields * (n1 > 0 ? n1 : 1));
  const Sim3Recs R{rec.data(), n1 > 0 ? n1 : 1};
  int N = 0, bits = 0;
  for (int i1 = 0; i1 < n1; ++i1) {
    const int i2 = match12[i1];
    if (i2 < 0) continue;
    if (i2 >= n2) {
      bits |= kStatusSim3Skipped;
      continue;
    }
    if (!mps1[i1].valid || !mps2[i2].valid) continue;
    const int k1 = kp_index1 ? kp_index1[i1] : i1;
    if (k1 >= n1) {
      bits |= kStatusSim3Skipped;
      continue;
    }
    if (k1 < 0) continue;
    const int o1 = kps1[k1].octave, o2 = kps2[i2].octave;
    if (o1 < 0 || o1 >= nlevels || o2 < 0 || o2 >= nlevels) {
      bits |= kStatusSim3Skipped;
      continue;
    }
    sim3_make_record(*cam1, *cam2, mps1[i1].pos, mps2[i2].pos, max_err[o1], max_err[o2], i1, R, N++);
  }
  const int first = params->first_iteration;
  const int max_its = sim3_iterations(params->probability, params->min_inliers, params->max_iterations, N);
  std::vector<orbm_sim3_hyp> H(max_its > 0 ? max_its : 1);
  Sim3Jacobi J;
  // without hyp nothing shows the hypotheses after the first accepted one: stop there, as the reference does
  int end = max_its, best = params->best_inliers;
  for (int h = first; h < end; ++h) {
    orbm_sim3_hyp& Hh = H[h];
    sim3_draw(rand3 + (size_t)3 * h, N, Hh.idx);
    float P1[3][3], P2[3][3];
    for (int k = 0; k < 3; ++k)
      for (int c = 0; c < 3; ++c) {
        P1[k][c] = R.at(c, Hh.idx[k]);
        P2[k][c] = R.at(3 + c, Hh.idx[k]);
      }
    sim3_solve(P1, P2, params->fix_scale != 0, &J, &Hh.s, Hh.R, Hh.t);
    float S12[12], S21[12];
    sim3_transforms(Hh.s, Hh.R, Hh.t, S12, S21);
    int cnt = 0;
    for (int k = 0; k < N; ++k) cnt += sim3_is_inlier(S12, S21, *cam1, *cam2, R, k) ? 1 : 0;
    Hh.count = cnt;
    if (hyp) hyp[h] = Hh;
    if (cnt >= best) {
      best = cnt;
      if (!hyp && cnt > params->min_inliers) end = h + 1;
    }
  }
  const Sim3Selection S =
      sim3_select(first, end, params->min_inliers, params->best_inliers, [&](int h) { return H[h].count; });
  const int chosen = S.accepted >= 0 ? S.accepted : S.best_iteration;
  if (inlier) {
    for (int i = 0; i < n1; ++i) inlier[i] = 0;
    if (S.accepted >= 0) {
      float S12[12], S21[12];
      sim3_transforms(H[chosen].s, H[chosen].R, H[chosen].t, S12, S21);
      for (int k = 0; k < N; ++k)
        if (sim3_is_inlier(S12, S21, *cam1, *cam2, R, k)) inlier[s3_f2i(R.at(12, k))] = 1;
    }
  }
  if (result) *result = sim3_result(S, S.accepted >= 0 ? H[S.accepted].count : 0, N, max_its, first);
  if (chosen >= 0) {
    if (s12) *s12 = H[chosen].s;
    if (R12) std::memcpy(R12, H[chosen].R, sizeof H[chosen].R);
    if (t12) std::memcpy(t12, H[chosen].t, sizeof H[chosen].t);
    if (pose) sim3_match_poses(*cam1, cam1->Tcw, cam2->Tcw, H[chosen].s, H[chosen].R, H[chosen].t, pose);
  }
  if (status) *status = bits;
  return ORBX_OK;
}

}  // namespace orbx
