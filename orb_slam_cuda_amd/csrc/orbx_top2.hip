// orbx_top2.hip — the dense Hamming best/second search of ORBmatcher for gfx950
// (the inner loop shared by every ORBmatcher search).
//
//   hamming_top2_mfma_kernel  the all-pairs distances as a GEMM on the
//                             block-scaled FP4 MFMA, top-2 on float sort keys
//   hamming_top2_kernel       the VALU version (ORBX_TOP2_VALU=1): lane-per-query,
//                             candidate rows broadcast from LDS, 8 x v_bcnt per pair
#if (defined(ORBX_M_NOMFMA)) && !defined(ORBX_DIAG)
#error "result-changing diagnostic switches need -DORBX_DIAG"
#endif
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "orbx_device.cuh"
#include "orbx_internal.h"

namespace orbx {

// ------------------------------------------------------------ dense top-2
constexpr int kTopQueries = 256;  // queries per workgroup, two per lane
#ifndef ORBX_TOP_SPLIT
#define ORBX_TOP_SPLIT 8
#endif
constexpr int kTopSplit = ORBX_TOP_SPLIT;  // candidate ranges per query (two waves each)
constexpr int kTopThreads = 128 * kTopSplit;
constexpr int kTopChunk = kTopThreads / (2 * kTopSplit);  // candidates per range per staged chunk (64)
// popcount(x) + acc as ONE v_bcnt_u32_b32 (the compiler otherwise splits the
// chain into bcnt(x, 0) and v_add3)
__device__ __forceinline__ int bcnt_acc(uint32_t x, int acc) {
  int r;
  asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
  return r;
}
__device__ __forceinline__ int med3_i32(int a, int b, int c) {
  int r;
  asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

__device__ __forceinline__ uint32_t med3_u32(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t r;
  asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

// Best / second of (distance, candidate) keys: key = d << 16 | j orders by
// distance, then by index, so min() keeps the first candidate on ties and
// med3() the second key (whose distance is the reference's bestDist2, ties
// included). Per pair 8 v_xor + 8 v_bcnt + v_lshl_or + v_min + v_med3.
struct Top2Acc {
  uint4 a0, a1;  // query descriptor
  uint32_t k1, k2;
  __device__ __forceinline__ void score(const uint4& r0, const uint4& r1, int j) {
    int d = bcnt_acc(a0.x ^ r0.x, 0);
    d = bcnt_acc(a0.y ^ r0.y, d);
    d = bcnt_acc(a0.z ^ r0.z, d);
    d = bcnt_acc(a0.w ^ r0.w, d);
    d = bcnt_acc(a1.x ^ r1.x, d);
    d = bcnt_acc(a1.y ^ r1.y, d);
    d = bcnt_acc(a1.z ^ r1.z, d);
    d = bcnt_acc(a1.w ^ r1.w, d);
    const uint32_t key = ((uint32_t)d << 16) | (uint32_t)j;
    k2 = med3_u32(key, k1, k2);
    k1 = min(key, k1);
  }
};
constexpr uint32_t kTopNone = (256u << 16) | 0xFFFFu;  // distance 256, no candidate

// Two queries per lane against wave-uniform candidate rows. The candidates
// are split in kTopSplit contiguous ranges, two waves per range (so that 8
// waves per SIMD are resident); each range stages chunks in LDS (one 16-byte
// load per thread per chunk) that its lanes read back as broadcast loads, one
// pair of row reads serving two queries. A pair costs 8 v_xor + 8 v_bcnt + 3
// top-2 updates on (distance << 16 | index) keys (Top2Acc). The partial
// results merge exactly because the keys carry the index (the earlier
// candidate wins ties, as the sequential scan would).
__global__ __launch_bounds__(kTopThreads) void hamming_top2_kernel(const uint8_t* __restrict__ A, long long a_pitch,
                                                                   const int* __restrict__ nA, int a_cap,
                                                                   const uint8_t* __restrict__ B, long long b_pitch,
                                                                   const int* __restrict__ nB,
                                                                   int* __restrict__ best_idx, int* __restrict__ best,
                                                                   int* __restrict__ second, int* err) {
  __shared__ uint4 sB[kTopSplit][kTopChunk][2];
  __shared__ uint2 part[kTopSplit][kTopQueries];
  const int p = blockIdx.y, tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const int k = wv >> 1, h = wv & 1;
  const int qa = h * 64 + lane, qb = 128 + h * 64 + lane;  // this lane's two queries (of 256)
  const int base = blockIdx.x * kTopQueries;
  // candidate indices live in the low 16 key bits; rows past a_cap have no output slot
  const int na = min(nA[p], a_cap), nb = min(nB[p], 65535);
  if (tid == 0 && blockIdx.x == 0 && (nB[p] > 65535 || nA[p] > a_cap)) atomicOr(err, 16);
  if (base >= na) return;
  const uint4* Ap = (const uint4*)(A + p * a_pitch);
  const uint4* Bp = (const uint4*)(B + p * b_pitch);
  Top2Acc x{make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0), kTopNone, kTopNone};
  Top2Acc y = x;
  if (base + qa < na) {
    x.a0 = Ap[2 * (base + qa)];
    x.a1 = Ap[2 * (base + qa) + 1];
  }
  if (base + qb < na) {
    y.a0 = Ap[2 * (base + qb)];
    y.a1 = Ap[2 * (base + qb) + 1];
  }
  const int per = (nb + kTopSplit - 1) / kTopSplit;
  // wave-uniform range (scalar registers: the key's index operand stays an SGPR)
  const int jb = __builtin_amdgcn_readfirstlane(min(k * per, nb)), je = __builtin_amdgcn_readfirstlane(min(jb + per, nb));
  // loader role of this thread: range lk, row lr, half lh
  const int lk = tid / (2 * kTopChunk), lr = (tid >> 1) % kTopChunk, lh = tid & 1;
  const int ljb = min(lk * per, nb), lje = min(ljb + per, nb);
  for (int c0 = 0; c0 < per; c0 += kTopChunk) {
    __syncthreads();
    if (ljb + c0 + lr < lje) sB[lk][lr][lh] = Bp[2 * (ljb + c0 + lr) + lh];
    __syncthreads();
    const int n = __builtin_amdgcn_readfirstlane(min(kTopChunk, je - (jb + c0)));  // wave-uniform
    int j = 0;
    for (; j + 2 <= n; j += 2) {  // two rows' LDS reads in flight, then four (row, query) pairs
      const uint4 r0 = sB[k][j][0], r1 = sB[k][j][1], r2 = sB[k][j + 1][0], r3 = sB[k][j + 1][1];
      x.score(r0, r1, jb + c0 + j);
      y.score(r0, r1, jb + c0 + j);
      x.score(r2, r3, jb + c0 + j + 1);
      y.score(r2, r3, jb + c0 + j + 1);
    }
    if (j < n) {
      const uint4 r0 = sB[k][j][0], r1 = sB[k][j][1];
      x.score(r0, r1, jb + c0 + j);
      y.score(r0, r1, jb + c0 + j);
    }
  }
  part[k][qa] = make_uint2(x.k1, x.k2);
  part[k][qb] = make_uint2(y.k1, y.k2);
  __syncthreads();
  if (tid >= kTopQueries || base + tid >= na) return;
  // merge the ranges: keys are globally ordered (distance, index), so the
  // best / second keys of the union are min / the second smallest
  uint2 r = part[0][tid];
#pragma unroll
  for (int s = 1; s < kTopSplit; ++s) {
    const uint2 o = part[s][tid];
    r.y = min(min(max(r.x, o.x), r.y), o.y);
    r.x = min(r.x, o.x);
  }
  if (base + tid >= na) return;
  const long long o = (long long)p * a_cap + base + tid;
  const int d1 = (int)(r.x >> 16);
  best_idx[o] = d1 < 256 ? (int)(r.x & 0xFFFFu) : -1;
  best[o] = d1;
  second[o] = (int)(r.y >> 16);
}

// ------------------------------------------------ dense top-2 on the matrix cores
// The all-pairs distance matrix is a GEMM: with bits mapped to +-1, the dot
// product of two descriptors is 256 - 2 * Hamming. The kernel runs it on the
// block-scaled FP4 MFMA (v_mfma_scale_f32_32x32x64_f8f6f4, e2m1 operands:
// 0x2 = +1.0, 0xA = -1.0; 4x the BF16 rate), K = 256 bits in four MFMAs.
//   candidates (A, rows):  bit set -> -1, clear -> +1, block scale 2^14
//   queries    (B, cols):  bit set -> +1, clear -> -1, block scale 2^0
// so A.B = 2^14 * (2h - 256), and with the accumulator seeded with
// 2^22 + 1 + (candidate index within a 32768 block) every result IS the sort
// key 32768 * h + index + 1, an integer in [1, 2^24), exact in f32 whatever the
// accumulation order. Per (candidate, query) value the lane then does one
// v_min_f32 + one v_med3_f32 (the best / second update of Top2Acc). The bit
// order inside K is free as long as A and B use the same one (dot products
// are order-independent): word w of a descriptor goes to the 16-byte
// fragment of MFMA step w >> 1, lane half w & 1, bit 4n + m to nibble n of
// dword m.
// C/D layout (gfx950, 32x32): lane l holds column l & 31 (the query) and
// rows (r & 3) + 8 (r >> 2) + 4 (l >> 5), r = 0..15 (the candidates).
typedef int i32x4_t __attribute__((ext_vector_type(4)));
typedef int i32x8_t __attribute__((ext_vector_type(8)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));
#ifndef ORBX_M_QT
#define ORBX_M_QT 4
#endif
#ifndef ORBX_M_WPE
#define ORBX_M_WPE 2
#endif
#ifndef ORBX_M_CHUNK
#define ORBX_M_CHUNK 128
#endif
constexpr int kMqTiles = ORBX_M_QT;          // 32-query tiles per wave
#ifndef ORBX_M_WAVES
#define ORBX_M_WAVES 2
#endif
#ifndef ORBX_M_HALVES
#define ORBX_M_HALVES 2
#endif
constexpr int kMWaves = ORBX_M_WAVES;        // query waves per candidate range
constexpr int kMHalves = ORBX_M_HALVES;      // candidate ranges per workgroup
constexpr int kMQueries = 32 * kMqTiles * kMWaves;  // 256 queries per workgroup
constexpr int kMChunk = ORBX_M_CHUNK;        // candidates per staged chunk per half (a multiple of 128)
constexpr int kMRowsPerPass = 32 * kMWaves;  // staged rows per pass (two threads per row)
static_assert(kMChunk % kMRowsPerPass == 0, "a chunk is whole staging passes");
constexpr int kMThreads = 64 * kMWaves * kMHalves;
constexpr int kMBlock = 32768;               // candidate indices per float-key block
constexpr float kMNone = 3.0e38f;            // float key of "no candidate"

// 32 descriptor bits -> 32 e2m1 nibbles (bit 4n + m -> nibble n of dword m)
__device__ __forceinline__ i32x4_t fp4_expand(uint32_t w) {
  i32x4_t o;
  o[0] = (int)(((w << 3) & 0x88888888u) | 0x22222222u);
  o[1] = (int)(((w << 2) & 0x88888888u) | 0x22222222u);
  o[2] = (int)(((w << 1) & 0x88888888u) | 0x22222222u);
  o[3] = (int)((w & 0x88888888u) | 0x22222222u);
  return o;
}
__device__ __forceinline__ uint32_t top2_ukey(uint32_t kb, int base) {
  const float k = __builtin_bit_cast(float, kb);
  if (!(k < 1.0e30f)) return kTopNone;
  const int v = (int)k - 1;
  return ((uint32_t)(v >> 15) << 16) | (uint32_t)((v & (kMBlock - 1)) + base);
}
#ifndef ORBX_M_ILV
#define ORBX_M_ILV 1  // MFMA chains of the query tiles interleaved (0: tile-major, for A/B and the timing experiments)
#endif
#ifndef ORBX_M_PAIRS
#define ORBX_M_PAIRS 1  // top-2 update on pairs of results (0: one result per step, for A/B)
#endif
__device__ __forceinline__ void top2_merge(uint32_t& u1, uint32_t& u2, uint32_t x1, uint32_t x2) {
  u2 = min(min(max(u1, x1), u2), x2);
  u1 = min(u1, x1);
}

__global__ __launch_bounds__(kMThreads) __attribute__((amdgpu_waves_per_eu(ORBX_M_WPE))) void hamming_top2_mfma_kernel(
    const uint8_t* __restrict__ A, long long a_pitch, const int* __restrict__ nA, int a_cap,
    const uint8_t* __restrict__ B, long long b_pitch, const int* __restrict__ nB, int* __restrict__ best_idx,
    int* __restrict__ best, int* __restrict__ second, int* err) {
  __shared__ __attribute__((aligned(16))) i32x4_t sC[2][kMHalves][kMChunk / 32][4][64];  // [buffer][half][tile][step][lane]
  __shared__ uint2 part[kMHalves > 1 ? kMHalves - 1 : 1][kMQueries];
  // XCD-aware order: a pair's query blocks are consecutive logical ids, which
  // xcd_remap keeps on one XCD, so its candidates are fetched into one L2
  const int lg = xcd_remap(blockIdx.x + blockIdx.y * gridDim.x, gridDim.x * gridDim.y);
  const int p = lg / gridDim.x, tid = threadIdx.x, lane = tid & 63;
  const int hf = tid / (64 * kMWaves), wv = (tid >> 6) % kMWaves, ht = tid % (64 * kMWaves);
  const int base = (lg % gridDim.x) * kMQueries;
  // final keys hold the index in 16 bits; rows past a_cap have no output slot
  const int na = min(nA[p], a_cap), nb = min(nB[p], 65535);
  if (tid == 0 && (lg % gridDim.x) == 0 && (nB[p] > 65535 || nA[p] > a_cap)) atomicOr(err, 16);
  if (base >= na) return;
  // queries (the B operand), this wave's kMqTiles tiles, held for the whole kernel
  const uint4* Ap = (const uint4*)(A + p * a_pitch);
  const uint4* Bp = (const uint4*)(B + p * b_pitch);
  const int hl = lane >> 5;
  i32x4_t qf[kMqTiles][4];
#pragma unroll
  for (int q = 0; q < kMqTiles; ++q) {
    const int qi = min(base + wv * 32 * kMqTiles + q * 32 + (lane & 31), na - 1);
    const uint4 d0 = Ap[2 * qi], d1 = Ap[2 * qi + 1];
    const uint32_t w[4] = {hl ? d0.y : d0.x, hl ? d0.w : d0.z, hl ? d1.y : d1.x, hl ? d1.w : d1.z};
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[q][s] = fp4_expand(~w[s]);
  }
  // running row keys: 2^22 + 1 + (index of this lane's row r in the next tile - blk);
  // the + 1 keeps every key >= 1, so no result is a signed zero (whose bit
  // pattern would order last)
  f32x16_t rk;
  auto rk_reset = [&]() {
#pragma unroll
    for (int r = 0; r < 16; ++r) rk[r] = 4194305.0f + (float)((r & 3) + 8 * (r >> 2) + 4 * hl);
  };
  rk_reset();
  uint32_t k1[kMqTiles], k2[kMqTiles];  // float keys as bit patterns
  uint32_t u1[kMqTiles], u2[kMqTiles];
  const uint32_t kNoneBits = __builtin_bit_cast(uint32_t, kMNone);
#pragma unroll
  for (int q = 0; q < kMqTiles; ++q) {
    k1[q] = k2[q] = kNoneBits;
    u1[q] = u2[q] = kTopNone;
  }
  const int per = (nb + kMHalves - 1) / kMHalves;
  const int jb = min(hf * per, nb), je = min(jb + per, nb);  // this half's candidates
  const int nchunks = (per + kMChunk - 1) / kMChunk;         // the same for both halves (barriers)
  int blk = jb;                                              // first index of the current key block
  const int sr = ht >> 1, spart = ht & 1;                    // staging role: row, 16-byte half
  // double-buffered staging: chunk c+1's global load is in flight while chunk
  // c is computed; one barrier per chunk (a wave writing buffer c & 1 has
  // passed the barrier every wave reaches only after computing chunk c - 2)
  constexpr int kRep = kMChunk / kMRowsPerPass;  // staged rows per thread per chunk
  uint4 pre[kRep];
#pragma unroll
  for (int i = 0; i < kRep; ++i) pre[i] = jb < je ? Bp[2 * min(jb + sr + kMRowsPerPass * i, je - 1) + spart] : make_uint4(0, 0, 0, 0);
  // top-2 update of query tile q with one tile's 16 results per lane: results
  // in pairs; with k1 <= k2, the second smallest of {k1, k2, x0, x1} is
  // min(med3(k1, x0, x1), k2) and the smallest min3(k1, x0, x1); two pairs
  // share one min3 into k2, so four values cost 5 integer VALU instead of 8
  // (positive floats order as their bit patterns; the medians as v_med3_f32,
  // so no integer min is shared with the new minimum's and each folds into
  // one v_min3_u32)
  auto top2_update = [&](int q, const f32x16_t& acc) {
#pragma unroll
    for (int r = 0; r < 16; r += 4) {
      const float xf0 = acc[r], xf1 = acc[r + 1], xf2 = acc[r + 2], xf3 = acc[r + 3];
      const uint32_t x0 = __float_as_uint(xf0), x1 = __float_as_uint(xf1);
      const uint32_t x2 = __float_as_uint(xf2), x3 = __float_as_uint(xf3);
      const uint32_t t0 = __float_as_uint(__builtin_amdgcn_fmed3f(xf0, xf1, __uint_as_float(k1[q])));
      const uint32_t m = min(min(k1[q], x0), x1);
      const uint32_t t1 = __float_as_uint(__builtin_amdgcn_fmed3f(xf2, xf3, __uint_as_float(m)));
      k1[q] = min(min(m, x2), x3);
      k2[q] = min(min(t0, t1), k2[q]);
    }
  };
  auto top2_tile = [&](const i32x8_t (&af)[4], const f32x16_t& rkt) {
#if ORBX_M_ILV && !defined(ORBX_M_NOMFMA) && !defined(ORBX_M_NOTOP2)
    // step-major: the four query tiles' accumulation chains interleaved
    // (34.3 -> 33.1 us per 64 pairs alone against tile-major chains)
    f32x16_t accs[kMqTiles];
#pragma unroll
    for (int q = 0; q < kMqTiles; ++q) accs[q] = rkt;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
      for (int q = 0; q < kMqTiles; ++q) {
        const i32x8_t bf = (i32x8_t){qf[q][s][0], qf[q][s][1], qf[q][s][2], qf[q][s][3], 0, 0, 0, 0};
        accs[q] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af[s], bf, accs[q], 4, 4, 0, 141, 0, 127);
      }
    }
#pragma unroll
    for (int q = 0; q < kMqTiles; ++q) top2_update(q, accs[q]);
    return;
#endif
#pragma unroll
    for (int q = 0; q < kMqTiles; ++q) {
      f32x16_t acc = rkt;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const i32x8_t bf = (i32x8_t){qf[q][s][0], qf[q][s][1], qf[q][s][2], qf[q][s][3], 0, 0, 0, 0};
#if defined(ORBX_M_NOMFMA)  // timing experiment only: the top-2 update without MFMA
        acc[s] += __builtin_bit_cast(float, af[s][0] ^ bf[0]);
#else
        acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af[s], bf, acc, 4, 4, 0, 141, 0, 127);
#endif
      }
#if defined(ORBX_M_NOTOP2)  // timing experiment only: MFMA without the top-2 update
      const float x0 = acc[0];
      k1[q] = min(__float_as_uint(x0), k1[q]);
#elif ORBX_M_PAIRS
      top2_update(q, acc);
#else
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        // positive floats order as their bit patterns: the best key is an
        // integer v_min_u32 and the second a v_med3_f32 (the target builtin);
        // fminf would first canonicalise every MFMA result with a v_max_f32.
        // (__float_as_uint of a float copy: ROCm 7.2 clang lowers
        // __builtin_bit_cast(uint32_t, acc[r]) of an ext_vector element to a
        // read of element 0)
        const float xf = acc[r];
        k2[q] = __float_as_uint(__builtin_amdgcn_fmed3f(xf, __uint_as_float(k1[q]), __uint_as_float(k2[q])));
        k1[q] = min(__float_as_uint(xf), k1[q]);
      }
#endif
    }
  };
  for (int c = 0; c < nchunks; ++c) {
    const int c0 = jb + c * kMChunk, buf = c & 1;
    if (c0 < je) {
#pragma unroll
      for (int k = 0; k < kRep; ++k) {
        const int row = sr + kMRowsPerPass * k;
        const uint32_t w[4] = {pre[k].x, pre[k].y, pre[k].z, pre[k].w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int wi = 4 * spart + i;
          sC[buf][hf][row >> 5][wi >> 1][(row & 31) + 32 * (wi & 1)] = fp4_expand(w[i]);
        }
      }
      if (c0 + kMChunk < je) {
#pragma unroll
        for (int k = 0; k < kRep; ++k) pre[k] = Bp[2 * min(c0 + kMChunk + sr + kMRowsPerPass * k, je - 1) + spart];
      }
    }
    __syncthreads();
    if (c0 >= je) continue;
    if (c0 - blk >= kMBlock) {  // key block full: fold the float keys into the index keys
#pragma unroll
      for (int q = 0; q < kMqTiles; ++q) {
        top2_merge(u1[q], u2[q], top2_ukey(k1[q], blk), top2_ukey(k2[q], blk));
        k1[q] = k2[q] = kNoneBits;
      }
      blk = c0;
      rk_reset();
    }
    const int nval = min(kMChunk, je - c0);
#ifdef ORBX_M_PREF
    // the next tile's candidate fragments are read while this tile computes
    const int ntile = (nval + 31) >> 5;
    i32x4_t nx[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) nx[s] = sC[buf][hf][0][s][lane];
#endif
    for (int t = 0; t * 32 < nval; ++t) {
      i32x8_t af[4];
#ifdef ORBX_M_PREF
#pragma unroll
      for (int s = 0; s < 4; ++s) af[s] = (i32x8_t){nx[s][0], nx[s][1], nx[s][2], nx[s][3], 0, 0, 0, 0};
      const int tn = min(t + 1, ntile - 1);
#pragma unroll
      for (int s = 0; s < 4; ++s) nx[s] = sC[buf][hf][tn][s][lane];
#else
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const i32x4_t v = sC[buf][hf][t][s][lane];
        af[s] = (i32x8_t){v[0], v[1], v[2], v[3], 0, 0, 0, 0};
      }
#endif
      const int nrow = nval - 32 * t;  // valid rows of this tile
      if (nrow >= 32) {
        top2_tile(af, rk);
      } else {  // ragged last tile: rows past the end never win
        f32x16_t rkt;
#pragma unroll
        for (int r = 0; r < 16; ++r) rkt[r] = (r & 3) + 8 * (r >> 2) + 4 * hl < nrow ? rk[r] : kMNone;
        top2_tile(af, rkt);
      }
      rk += 32.0f;
    }
  }
  // fold the last block, then merge the two lane halves (rows 0-3 / 4-7 of each 8)
#pragma unroll
  for (int q = 0; q < kMqTiles; ++q) {
    top2_merge(u1[q], u2[q], top2_ukey(k1[q], blk), top2_ukey(k2[q], blk));
    const uint32_t o1 = __shfl_xor(u1[q], 32), o2 = __shfl_xor(u2[q], 32);
    top2_merge(u1[q], u2[q], o1, o2);
  }
  const int qloc = wv * 32 * kMqTiles + (lane & 31);
  if (hf >= 1 && lane < 32) {
#pragma unroll
    for (int q = 0; q < kMqTiles; ++q) part[hf - 1][qloc + 32 * q] = make_uint2(u1[q], u2[q]);
  }
  if (kMHalves > 1) __syncthreads();
  if (hf != 0 || lane >= 32) return;
#pragma unroll
  for (int q = 0; q < kMqTiles; ++q) {
    const int qi = base + qloc + 32 * q;
    if (qi >= na) continue;
    for (int h = 0; h + 1 < kMHalves; ++h) {  // ranges in index order: keys merge exactly in any order
      const uint2 o = part[h][qloc + 32 * q];
      top2_merge(u1[q], u2[q], o.x, o.y);
    }
    const long long oi = (long long)p * a_cap + qi;
    const int d1 = (int)(u1[q] >> 16);
    best_idx[oi] = d1 < 256 ? (int)(u1[q] & 0xFFFFu) : -1;
    best[oi] = d1;
    second[oi] = (int)(u2[q] >> 16);
  }
}

// ------------------------------------------------------------ launchers
int launch_hamming_top2(const uint8_t* A, size_t a_pitch, const int* nA, int a_cap, const uint8_t* B,
                        size_t b_pitch, const int* nB, int pairs, int* best_idx, int* best, int* second,
                        int* err, void* stream) {
  // ORBX_TOP2_VALU=1 selects the VALU kernel (A/B timing and the cross-check
  // in tests/test_gpu_match.py; read per call so a test can switch it)
  const char* ev = getenv("ORBX_TOP2_VALU");
  const bool valu = ev && ev[0] == '1';
  if (!valu) {
    dim3 grid((a_cap + kMQueries - 1) / kMQueries, pairs);
    hipLaunchKernelGGL(hamming_top2_mfma_kernel, grid, dim3(kMThreads), 0, (hipStream_t)stream, A, (long long)a_pitch,
                       nA, a_cap, B, (long long)b_pitch, nB, best_idx, best, second, err);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
  }
  dim3 grid((a_cap + kTopQueries - 1) / kTopQueries, pairs);
  hipLaunchKernelGGL(hamming_top2_kernel, grid, dim3(kTopThreads), 0, (hipStream_t)stream, A, (long long)a_pitch, nA, a_cap,
                     B, (long long)b_pitch, nB, best_idx, best, second, err);
  return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
}

}  // namespace orbx
