// orbx_wave.cuh — wave64 reductions and scans on DPP (no LDS round trips).
//
// __shfl_xor / __shfl_up lower to ds_bpermute_b32 (an LDS-pipe instruction
// with LDS latency); the serial loops of the matchers run one reduction per
// query, so these use DPP row operations instead: quad_perm, row_half_mirror
// and row_mirror inside 16-lane rows, then row_bcast:15 / row_bcast:31
// across rows (GFX9-family DPP, available on gfx950).
#pragma once
#include <hip/hip_runtime.h>
#include <climits>

namespace orbx {

// popcount of the bits of m below this lane
__device__ __forceinline__ int mbcnt64(uint64_t m) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ int dpp_i(int old, int v) {
  return __builtin_amdgcn_update_dpp(old, v, CTRL, ROW_MASK, 0xf, false);
}

constexpr int kDppQuad1032 = 0xB1;  // quad_perm:[1,0,3,2]
constexpr int kDppQuad2301 = 0x4E;  // quad_perm:[2,3,0,1]
constexpr int kDppHalfMirror = 0x141;
constexpr int kDppMirror = 0x140;
constexpr int kDppBcast15 = 0x142;
constexpr int kDppBcast31 = 0x143;
constexpr int kDppShr1 = 0x111, kDppShr2 = 0x112, kDppShr4 = 0x114, kDppShr8 = 0x118;

// wave-uniform min of v over all 64 lanes (every lane must be active)
__device__ __forceinline__ int wave_min_dpp(int v) {
  v = min(v, dpp_i<kDppQuad1032>(INT_MAX, v));
  v = min(v, dpp_i<kDppQuad2301>(INT_MAX, v));
  v = min(v, dpp_i<kDppHalfMirror>(INT_MAX, v));
  v = min(v, dpp_i<kDppMirror>(INT_MAX, v));
  v = min(v, dpp_i<kDppBcast15, 0xa>(INT_MAX, v));
  v = min(v, dpp_i<kDppBcast31, 0xc>(INT_MAX, v));
  return __builtin_amdgcn_readlane(v, 63);
}

__device__ __forceinline__ int wave_sum_dpp(int v) {
  v += dpp_i<kDppQuad1032>(0, v);
  v += dpp_i<kDppQuad2301>(0, v);
  v += dpp_i<kDppHalfMirror>(0, v);
  v += dpp_i<kDppMirror>(0, v);
  v += dpp_i<kDppBcast15, 0xa>(0, v);
  v += dpp_i<kDppBcast31, 0xc>(0, v);
  return __builtin_amdgcn_readlane(v, 63);
}

template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ double dpp_d(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = dpp_i<CTRL, ROW_MASK>(0, (int)(uint32_t)b);
  const int hi = dpp_i<CTRL, ROW_MASK>(0, (int)(uint32_t)((unsigned long long)b >> 32));
  return __longlong_as_double((long long)(((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo));
}

// the sum of v over the 64 lanes in wave_sum_dpp's fixed order, wave-uniform
__device__ __forceinline__ double wave_sum_f64(double v) {
  v += dpp_d<kDppQuad1032>(v);
  v += dpp_d<kDppQuad2301>(v);
  v += dpp_d<kDppHalfMirror>(v);
  v += dpp_d<kDppMirror>(v);
  v += dpp_d<kDppBcast15, 0xa>(v);
  v += dpp_d<kDppBcast31, 0xc>(v);
  const long long b = __double_as_longlong(v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, 63);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((unsigned long long)b >> 32), 63);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// Sums over a workgroup of W waves in a fixed order: each wave adds its lanes
// (wave_sum_f64 / wave_sum_dpp), every thread then adds the waves' partial
// sums from LDS in wave order, so all threads hold the same bits and a sum
// depends on the lanes' values alone. Two LDS buffers alternate: one barrier
// per reduction. Every thread of the workgroup must call.
template <int W, int N>
struct BlockSumLds {
  double part[2][W][N];
  int ipart[2][W];
};
template <int W, int N>
struct BlockSum {
  BlockSumLds<W, N>* sh;
  int parity = 0, iparity = 0;
  template <int K>
  __device__ void sum(double* v) {
    static_assert(K <= N, "more sums than the LDS buffer holds");
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_sum_f64(v[k]);
    if (W == 1) return;
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int k = 0; k < K; ++k) sh->part[parity][wave][k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
      double s = sh->part[parity][0][k];
#pragma unroll
      for (int w = 1; w < W; ++w) s += sh->part[parity][w][k];
      v[k] = s;
    }
    parity ^= 1;
  }
  __device__ int sum_int(int v) {
    v = wave_sum_dpp(v);
    if (W == 1) return v;
    if ((threadIdx.x & 63) == 0) sh->ipart[iparity][threadIdx.x >> 6] = v;
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) s += sh->ipart[iparity][w];
    iparity ^= 1;
    return s;
  }
};

// inclusive prefix sum over lanes 0..63 (every lane must be active)
__device__ __forceinline__ int wave_incl_scan_dpp(int v) {
  v += dpp_i<kDppShr1>(0, v);
  v += dpp_i<kDppShr2>(0, v);
  v += dpp_i<kDppShr4>(0, v);
  v += dpp_i<kDppShr8>(0, v);
  v += dpp_i<kDppBcast15, 0xa>(0, v);
  v += dpp_i<kDppBcast31, 0xc>(0, v);
  return v;
}

}  // namespace orbx
