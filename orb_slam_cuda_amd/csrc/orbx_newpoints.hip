// orbx_newpoints.hip — LocalMapping::CreateNewMapPoints' loop over
// vMatchedIndices (src/LocalMapping.cc:317-483): the host form and the kernels
// of orbm_create_new_map_points_batch. The arithmetic is orbx_newpoints.cuh's
// for both.
//
// newpt_kernel, grid (idx1 chunks, pairs), 256 threads: one lane per
// (pair, idx1). The pair record is uniform per workgroup (scalar loads), each
// orbx_kp is read once, the 4x4 Jacobi SVD runs on compile-time indices, so
// its 36 values are registers: no LDS, no scratch. Writes pos and reason.
// newpt_dedup_kernel, one workgroup per pair: the first-pair rule over a
// shared current keyframe (an accepted idx1 that an earlier pair accepted
// becomes DUPLICATE) and the pair's count of accepted matches.
// newpt_emit_kernel, one workgroup per pair: the pair's base is the sum of the
// earlier pairs' counts, its accepted matches get their slots by a ballot scan
// in idx1 order, so d_new is in the reference's creation order in every run;
// the records, the appended map point rows, observation lists and has_mp
// flags are written from there.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "orbx_newpoints.cuh"
#include "orbx_wave.cuh"

namespace orbx {

namespace {

constexpr int kT = 256, kW = kT / 64;

// keypoints of side 1 of pair p that the row of out_pitch entries can hold
__device__ __forceinline__ int side1_count(const NewPtArgs& A, int p) {
  int n = A.n1[A.kp_pitch1 ? p : 0];
  if (A.kp_pitch1 && n > A.kp_pitch1) n = A.kp_pitch1;
  if (n > A.out_pitch) n = A.out_pitch;
  return n < 0 ? 0 : n;
}

__global__ __launch_bounds__(kT) void newpt_kernel(NewPtArgs A, const orbm_newpt_pair* __restrict__ pairs) {
  const int p = blockIdx.y, i = blockIdx.x * kT + threadIdx.x;
  if (i >= side1_count(A, p)) return;
  int n2 = A.n2[p];
  if (n2 > A.kp_pitch2) n2 = A.kp_pitch2;
  const size_t k1 = (size_t)p * A.kp_pitch1, k2 = (size_t)p * A.kp_pitch2, o = (size_t)p * A.out_pitch + i;
  float pos[3];
  bool bad;
  const uint8_t r = newpt_entry(pairs[p], A.kps1 + k1, A.raw1 ? A.raw1 + k1 : nullptr, A.ur1 + k1, A.dp1 + k1, i,
                                A.kps2 + k2, A.raw2 ? A.raw2 + k2 : nullptr, A.ur2 + k2, A.dp2 + k2, n2,
                                A.matches12[o], A.sigma2, A.scale, A.nlevels, pos, &bad);
  A.pos[3 * o] = pos[0];
  A.pos[3 * o + 1] = pos[1];
  A.pos[3 * o + 2] = pos[2];
  A.reason[o] = r;
  if (bad) atomicOr(A.err, kStatusNewPtBad);
}

__global__ __launch_bounds__(kT) void newpt_dedup_kernel(NewPtArgs A) {
  __shared__ int s_cnt;
  const int p = blockIdx.x, tid = threadIdx.x;
  const int n1 = side1_count(A, p);
  const bool shared = A.dedup && A.kp_pitch1 == 0;
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  int cnt = 0;
  for (int i = tid; i < n1; i += kT) {
    const size_t o = (size_t)p * A.out_pitch + i;
    if (!newpt_accepted(A.reason[o])) continue;
    bool dup = false;
    if (shared)
      for (int q = 0; q < p && !dup; ++q) {
        // an earlier pair's DUPLICATE replaced an accepted code: either value says idx1 has its point
        const uint8_t r = ((const volatile uint8_t*)A.reason)[(size_t)q * A.out_pitch + i];
        dup = newpt_accepted(r) || r == kNpDuplicate;
      }
    if (dup) {
      A.reason[o] = kNpDuplicate;
      A.pos[3 * o] = A.pos[3 * o + 1] = A.pos[3 * o + 2] = 0.0f;
    } else {
      ++cnt;
    }
  }
  cnt = wave_sum_dpp(cnt);
  if ((tid & 63) == 0 && cnt) atomicAdd(&s_cnt, cnt);
  __syncthreads();
  if (tid == 0) A.nnew_pair[p] = s_cnt;
}

__global__ __launch_bounds__(kT) void newpt_emit_kernel(NewPtArgs A, const orbm_newpt_pair* __restrict__ pairs) {
  __shared__ int s_w[kW];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int base = 0, total = 0;
  for (int q = 0; q < A.npairs; ++q) {
    const int c = A.nnew_pair[q];
    if (q < p) base += c;
    total += c;
  }
  const int cap = A.capacity;
  const int written = total < cap ? total : cap;
  if (p == 0) {
    if (tid == 0) {
      *A.nnew = written;
      if (total > cap) atomicOr(A.err, kStatusNewPtOverflow);
    }
    if (A.has_emit) {
      const uint32_t kf0 = pairs[0].kf1;
      for (int k = tid; k <= cap; k += kT) {
        A.emit.d_obs_off[k] = 2u * (uint32_t)(k < written ? k : written);
        if (k < cap) A.emit.d_point_ids[k] = A.emit.point_base + (uint32_t)k;
        if (k >= written && k < cap) A.emit.d_ref[k] = orbm_point_refkf{kf0, 0};
      }
    }
  }
  const int n1 = side1_count(A, p);
  const size_t k1 = (size_t)p * A.kp_pitch1, k2 = (size_t)p * A.kp_pitch2;
  int running = base;
  for (int start = 0; start < n1; start += kT) {
    const int i = start + tid;
    const size_t o = (size_t)p * A.out_pitch + i;
    const uint8_t r = i < n1 ? A.reason[o] : (uint8_t)kNpNone;
    const bool flag = newpt_accepted(r);
    const uint64_t b = __ballot(flag);
    if (lane == 0) s_w[w] = __popcll(b);
    __syncthreads();
    int k = running + mbcnt64(b), all = 0;
#pragma unroll
    for (int q = 0; q < kW; ++q) {
      if (q < w) k += s_w[q];
      all += s_w[q];
    }
    running += all;
    __syncthreads();
    if (!flag || k >= cap) continue;
    const orbm_newpt_pair& P = pairs[p];
    const int i2 = A.matches12[o];
    const float x = A.pos[3 * o], y = A.pos[3 * o + 1], z = A.pos[3 * o + 2];
    if (A.out_new) {
      orbm_new_point rec;
      rec.pos[0] = x;
      rec.pos[1] = y;
      rec.pos[2] = z;
      rec.pair = p;
      rec.idx1 = i;
      rec.idx2 = i2;
      rec.kind = r;
      A.out_new[k] = rec;
    }
    if (A.has_emit) {
      orbm_map_point_world* mp = A.emit.d_mps + (size_t)A.emit.point_base + k;
      mp->pos[0] = x;
      mp->pos[1] = y;
      mp->pos[2] = z;
      mp->valid = 1;
      mp->obs_positive = 1;
      const orbm_observation o1{P.kf1, P.desc_base1 + (uint32_t)i}, o2{P.kf2, P.desc_base2 + (uint32_t)i2};
      A.emit.d_obs[2 * (size_t)k] = P.kf2_first ? o2 : o1;
      A.emit.d_obs[2 * (size_t)k + 1] = P.kf2_first ? o1 : o2;
      A.emit.d_ref[k] = orbm_point_refkf{P.kf1, A.kps1[k1 + i].octave};
    }
    if (A.has_mp1) A.has_mp1[k1 + i] = 1;
    if (A.has_mp2) A.has_mp2[k2 + i2] = 1;
  }
}

// cv::invert (DECOMP_LU) of a 3x3 CV_32F matrix: the determinant and every
// cofactor product in double, one rounding per element
void inv3(const float* S, float* D) {
  auto s = [&](int r, int c) { return (double)S[3 * r + c]; };
  double d = s(0, 0) * (s(1, 1) * s(2, 2) - s(1, 2) * s(2, 1)) - s(0, 1) * (s(1, 0) * s(2, 2) - s(1, 2) * s(2, 0)) +
             s(0, 2) * (s(1, 0) * s(2, 1) - s(1, 1) * s(2, 0));
  if (d == 0) {
    for (int k = 0; k < 9; ++k) D[k] = 0.0f;
    return;
  }
  d = 1. / d;
  D[0] = (float)((s(1, 1) * s(2, 2) - s(1, 2) * s(2, 1)) * d);
  D[1] = (float)((s(0, 2) * s(2, 1) - s(0, 1) * s(2, 2)) * d);
  D[2] = (float)((s(0, 1) * s(1, 2) - s(0, 2) * s(1, 1)) * d);
  D[3] = (float)((s(1, 2) * s(2, 0) - s(1, 0) * s(2, 2)) * d);
  D[4] = (float)((s(0, 0) * s(2, 2) - s(0, 2) * s(2, 0)) * d);
  D[5] = (float)((s(0, 2) * s(1, 0) - s(0, 0) * s(1, 2)) * d);
  D[6] = (float)((s(1, 0) * s(2, 1) - s(1, 1) * s(2, 0)) * d);
  D[7] = (float)((s(0, 1) * s(2, 0) - s(0, 0) * s(2, 1)) * d);
  D[8] = (float)((s(0, 0) * s(1, 1) - s(0, 1) * s(1, 0)) * d);
}
// a 3x3 product on gemm's small-matrix path: float dot products left to right
void mul3(const float* A, const float* B, float* C) {
  float T[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) T[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
  std::memcpy(C, T, sizeof T);
}

}  // namespace

// LocalMapping::ComputeF12 (:572-589)
void compute_f12_host(const orbm_camera& c1, const orbm_camera& c2, float* F12) {
  float R1[9], R2t[9], R12[9], t12[3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      R1[3 * r + c] = c1.Tcw[4 * r + c];
      R2t[3 * r + c] = c2.Tcw[4 * c + r];
    }
  mul3(R1, R2t, R12);
  // -R1w*R2w.t()*t2w + t1w: the product's float dot, then t*(-1) + t1w in double
  for (int r = 0; r < 3; ++r) {
    const float t = R12[3 * r] * c2.Tcw[3] + R12[3 * r + 1] * c2.Tcw[7] + R12[3 * r + 2] * c2.Tcw[11];
    t12[r] = (float)((double)t * -1.0 + (double)c1.Tcw[4 * r + 3] * 1.0);
  }
  const float tx[9] = {0.0f, -t12[2], t12[1], t12[2], 0.0f, -t12[0], -t12[1], t12[0], 0.0f};  // SkewSymmetricMatrix
  const float K1t[9] = {c1.fx, 0.0f, 0.0f, 0.0f, c1.fy, 0.0f, c1.cx, c1.cy, 1.0f};
  const float K2[9] = {c2.fx, 0.0f, c2.cx, 0.0f, c2.fy, c2.cy, 0.0f, 0.0f, 1.0f};
  float K1ti[9], K2i[9], M[9];
  inv3(K1t, K1ti);
  inv3(K2, K2i);
  mul3(K1ti, tx, M);
  mul3(M, R12, M);
  mul3(M, K2i, F12);
}

int create_new_map_points_host(const orbm_newpt_pair& P, const orbx_kp* kps1, const orbx_kp* raw1, const float* ur1,
                               const float* dp1, int n1, const orbx_kp* kps2, const orbx_kp* raw2, const float* ur2,
                               const float* dp2, int n2, const float* sigma2, const float* scale, int nlevels,
                               const int* matches12, float* pos, uint8_t* reason, int* nnew, int* status) {
  int cnt = 0, bits = 0;
  for (int i = 0; i < n1; ++i) {
    bool bad;
    const uint8_t r = newpt_entry(P, kps1, raw1, ur1, dp1, i, kps2, raw2, ur2, dp2, n2, matches12[i], sigma2, scale,
                                  nlevels, pos + 3 * (size_t)i, &bad);
    reason[i] = r;
    if (bad) bits |= kStatusNewPtBad;
    if (newpt_accepted(r)) ++cnt;
  }
  if (nnew) *nnew = cnt;
  if (status) *status = bits;
  return ORBX_OK;
}

int launch_new_points(const NewPtArgs& A, const orbm_newpt_pair* d_pairs, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(newpt_kernel, dim3((A.out_pitch + kT - 1) / kT, A.npairs), dim3(kT), 0, s, A, d_pairs);
  hipLaunchKernelGGL(newpt_dedup_kernel, dim3(A.npairs), dim3(kT), 0, s, A);
  hipLaunchKernelGGL(newpt_emit_kernel, dim3(A.npairs), dim3(kT), 0, s, A, d_pairs);
  return (int)hipGetLastError();
}

}  // namespace orbx
