// orbx_top2.hip — the dense Hamming best/second search of ORBmatcher for gfx950
// (the inner loop shared by every ORBmatcher search).
//
//   hamming_top2_mfma_kernel  the all-pairs distances as a GEMM on the
//                             block-scaled FP4 MFMA, top-2 on float sort keys
//   hamming_top2_kernel       the VALU version (ORBX_TOP2_VALU=1): lane-per-query,
//                             candidate rows broadcast from LDS, 8 x v_bcnt per pair
//
// Compile-time switches of the MFMA kernel (A/B builds with tools/variant.sh):
//   ORBX_M_QT, ORBX_M_WPE   query tiles per wave, waves per SIMD asked for
//   (ORBX_M_WAVES, ORBX_M_HALVES, ORBX_M_CHUNK stay 2, 2, 128: the staging
//   inside the tile loop and the single float-key block are laid out for them)
//   ORBX_M_NOTOP2, ORBX_M_NOMFMA, ORBX_M_NOSTAGE   timing only, WRONG results:
//                      the loop without the top-2 update / without the MFMAs /
//                      without the candidates' staging (loads, fp4_expand, LDS writes;
//                      the fragment reads, their waits and the barriers stay)
#if (defined(ORBX_M_NOMFMA) || defined(ORBX_M_NOTOP2) || defined(ORBX_M_NOSTAGE)) && !defined(ORBX_DIAG)
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
// A half's candidates fit one float-key block (nb <= 65535), so the keys are
// folded into index keys once, after the chunk loop, never inside it.
static_assert((65535 + kMHalves - 1) / kMHalves <= kMBlock, "a candidate half spans more than one float-key block");
static_assert(kMqTiles >= 2, "the tile loop alternates two groups of query tiles");
constexpr int kMGroupX = (kMqTiles + 1) / 2;  // query tiles [0, kMGroupX) are group X, the rest group Y
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
  // running row keys: 2^22 + 1 + (index of this lane's row r in the next tile - jb);
  // the + 1 keeps every key >= 1, so no result is a signed zero (whose bit
  // pattern would order last)
  f32x16_t rk;
#pragma unroll
  for (int r = 0; r < 16; ++r) rk[r] = 4194305.0f + (float)((r & 3) + 8 * (r >> 2) + 4 * hl);
  uint32_t k1[kMqTiles], k2[kMqTiles];  // float keys as bit patterns
  const uint32_t kNoneBits = __builtin_bit_cast(uint32_t, kMNone);
  // the results of the candidate tile in flight, held from the MFMAs that write
  // them to the update that reads them half a tile later (group Y's across the
  // chunk barrier); "no candidate" until then, which an update leaves alone
  f32x16_t acc[kMqTiles];
#pragma unroll
  for (int q = 0; q < kMqTiles; ++q) {
    k1[q] = k2[q] = kNoneBits;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[q][r] = kMNone;
  }
  const int per = (nb + kMHalves - 1) / kMHalves;
  // this half's candidates (wave-uniform: the tile loop's branches are scalar)
  const int jb = __builtin_amdgcn_readfirstlane(min(hf * per, nb)), je = __builtin_amdgcn_readfirstlane(min(jb + per, nb));
  const int nchunks = (per + kMChunk - 1) / kMChunk;  // the same for both halves (barriers)
  const int sr = ht >> 1, spart = ht & 1;                    // staging role: row, 16-byte half
  // Double-buffered staging off the barrier: while chunk c is computed from
  // buffer c & 1, chunk c+1 is expanded and written to the other buffer, a
  // share of it inside each of chunk c's tiles, and chunk c+2's global loads
  // follow into the registers that frees. One barrier per chunk, at its end:
  // it publishes chunk c+1, and a wave that writes buffer (c+1) & 1 during
  // chunk c has passed the barrier at the end of chunk c-1, which every wave
  // reaches only after its last read of chunk c-1 from that buffer.
  constexpr int kRep = kMChunk / kMRowsPerPass;  // staged rows per thread per chunk
  // the tile loop stages one candidate row per thread per two tiles
  static_assert(kRep == 2 && kMChunk == 128, "the tile loop stages a chunk as two rows per thread over four tiles");
#ifndef ORBX_M_NOSTAGE
  auto cand_row = [&](int first, int k) { return Bp[2 * min(first + sr + kMRowsPerPass * k, je - 1) + spart]; };
  uint4 pre[kRep];
#pragma unroll
  for (int k = 0; k < kRep; ++k) pre[k] = jb < je ? cand_row(jb, k) : make_uint4(0, 0, 0, 0);
#endif
  // word i of this thread's 16 bytes of candidate row `row` of a chunk, expanded into buffer b
  auto stage_word = [&](int b, int row, int i, uint32_t w) {
#ifndef ORBX_M_NOSTAGE
    const int wi = 4 * spart + i;
    sC[b][hf][row >> 5][wi >> 1][(row & 31) + 32 * (wi & 1)] = fp4_expand(w);
#endif
  };
  // top-2 update of query tiles [q0, q1) with their 16 results per lane, four
  // results at a time: with k1 <= k2, the second smallest of {k1, k2, x0, x1} is
  // min(med3(k1, x0, x1), k2) and the smallest min3(k1, x0, x1); two pairs
  // share one min3 into k2, so four values cost 5 integer VALU instead of 8
  // (positive floats order as their bit patterns; the medians as v_med3_f32,
  // so no integer min is shared with the new minimum's and each folds into
  // one v_min3_u32). The tiles' dependent chains alternate.
  // (__float_as_uint of a float copy: ROCm 7.2 clang lowers
  // __builtin_bit_cast(uint32_t, acc[r]) of an ext_vector element to a read
  // of element 0)
  auto update_group = [&](int q0, int q1) {
#if defined(ORBX_M_NOTOP2)  // timing experiment only: MFMA without the top-2 update
#pragma unroll
    for (int q = q0; q < q1; ++q) {
      const float x0 = acc[q][0];
      k1[q] = min(__float_as_uint(x0), k1[q]);
    }
#else
#pragma unroll
    for (int r = 0; r < 16; r += 4) {
#pragma unroll
      for (int q = q0; q < q1; ++q) {
        const float xf0 = acc[q][r], xf1 = acc[q][r + 1], xf2 = acc[q][r + 2], xf3 = acc[q][r + 3];
        const uint32_t x0 = __float_as_uint(xf0), x1 = __float_as_uint(xf1);
        const uint32_t x2 = __float_as_uint(xf2), x3 = __float_as_uint(xf3);
        const uint32_t t0 = __float_as_uint(__builtin_amdgcn_fmed3f(xf0, xf1, __uint_as_float(k1[q])));
        const uint32_t m = min(min(k1[q], x0), x1);
        const uint32_t t1 = __float_as_uint(__builtin_amdgcn_fmed3f(xf2, xf3, __uint_as_float(m)));
        k1[q] = min(min(m, x2), x3);
        k2[q] = min(min(t0, t1), k2[q]);
      }
    }
#endif
  };
  // the candidate tile af against query tiles [q0, q1): K = 256 in four steps,
  // step-major so that the tiles' accumulation chains alternate; the row keys
  // are the first step's addend
  auto mfma_group = [&](int q0, int q1, const i32x8_t (&af)[4]) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
      for (int q = q0; q < q1; ++q) {
        const i32x8_t bf = (i32x8_t){qf[q][s][0], qf[q][s][1], qf[q][s][2], qf[q][s][3], 0, 0, 0, 0};
#if defined(ORBX_M_NOMFMA)  // timing experiment only: the top-2 update without MFMA
        if (s == 0) acc[q] = rk;
        acc[q][s] += __builtin_bit_cast(float, af[s][0] ^ bf[0]);
#else
        acc[q] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af[s], bf, s == 0 ? rk : acc[q], 4, 4, 0, 141, 0, 127);
#endif
      }
    }
  };
  // ragged last tile: rows past the end never win
  auto mask_group = [&](int q0, int q1, int nrow) {
    int lim = nrow - 4 * hl;  // one register, compared with constants (not 16 row numbers kept live)
    asm volatile("" : "+v"(lim));
#pragma unroll
    for (int q = q0; q < q1; ++q) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[q][r] = (r & 3) + 8 * (r >> 2) < lim ? (float)acc[q][r] : kMNone;
    }
  };
  // One candidate tile. Within a wave an MFMA group and the other group's
  // update issue together: X's MFMAs of this tile with Y's update of the tile
  // before, then Y's MFMAs with X's update. A group's accumulators are free
  // for its next MFMAs exactly when its update has read them, which this
  // order guarantees; the placement (one MFMA, then a share of the update's
  // VALU) is held by the scheduling group barriers.
  constexpr int kNX = kMGroupX, kNY = kMqTiles - kMGroupX;
  // (an update is 20 VALU per query tile; + 8: the word a region stages)
  constexpr int kValuX = (21 * kNY + 8 + 4 * kNX - 1) / (4 * kNX);  // VALU per MFMA of X: Y's update
  constexpr int kValuY = (21 * kNX + 8 + 4 * kNY - 1) / (4 * kNY);  // VALU per MFMA of Y: X's update
  // (The compiler moves the update and the MFMAs, which have no side effects,
  // across a sched_barrier before the machine scheduler runs; the empty asm
  // statements tie the inputs of a region to its head and its results to its
  // end, as orbx_fast.hip does.)
  auto pin_acc = [&](int q0, int q1) {
#pragma unroll
    for (int q = q0; q < q1; ++q) asm volatile("" : "+v"(acc[q]));
  };
  auto pin_keys = [&](int q0, int q1) {
#pragma unroll
    for (int q = q0; q < q1; ++q) asm volatile("" : "+v"(k1[q]), "+v"(k2[q]));
  };
  // nst: words [i0, i0 + 2 nst) of row `row` of the next chunk (w) go to buffer sb on the way
  auto tile = [&](const i32x8_t (&af)[4], int nrow, int nst, int sb, int row, int i0, const uint4& w) __attribute__((always_inline)) {
    const uint32_t wv4[4] = {w.x, w.y, w.z, w.w};
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" : "+v"(rk));
    pin_acc(kNX, kMqTiles);
    mfma_group(0, kNX, af);
    update_group(kNX, kMqTiles);
#pragma unroll
    for (int i = i0; i < i0 + nst; ++i) stage_word(sb, row, i, wv4[i]);
#pragma unroll
    for (int i = 0; i < 4 * kNX; ++i) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, kValuX, 0);
    }
    pin_acc(0, kNX);
    pin_keys(kNX, kMqTiles);
    __builtin_amdgcn_sched_barrier(0);
    if (nrow < 32) mask_group(0, kNX, nrow);
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" : "+v"(rk));
    pin_acc(0, kNX);
    mfma_group(kNX, kMqTiles, af);
    update_group(0, kNX);
#pragma unroll
    for (int i = i0 + nst; i < i0 + 2 * nst; ++i) stage_word(sb, row, i, wv4[i]);
#pragma unroll
    for (int i = 0; i < 4 * kNY; ++i) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, kValuY, 0);
    }
    pin_acc(kNX, kMqTiles);
    pin_keys(0, kNX);
    __builtin_amdgcn_sched_barrier(0);
    rk += 32.0f;
    if (nrow < 32) mask_group(kNX, kMqTiles, nrow);
    __builtin_amdgcn_sched_barrier(0);
  };
  auto frags = [&](i32x8_t (&af)[4], int buf, int t) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const i32x4_t v = sC[buf][hf][t][s][lane];
      af[s] = (i32x8_t){v[0], v[1], v[2], v[3], 0, 0, 0, 0};
    }
  };
  // chunk 0 is staged whole, in front of the first barrier
#ifdef ORBX_M_NOSTAGE
  // nothing writes sC in this build: hand its address to an asm that may have,
  // so that the array, the fragment reads and their waits stay
  asm volatile("" : : "v"(&sC[0][0][0][0][0]) : "memory");
  (void)Bp;
  (void)spart;
#else
  if (jb < je) {
#pragma unroll
    for (int k = 0; k < kRep; ++k) {
      stage_word(0, sr + kMRowsPerPass * k, 0, pre[k].x);
      stage_word(0, sr + kMRowsPerPass * k, 1, pre[k].y);
      stage_word(0, sr + kMRowsPerPass * k, 2, pre[k].z);
      stage_word(0, sr + kMRowsPerPass * k, 3, pre[k].w);
      pre[k] = cand_row(jb + kMChunk, k);
    }
  }
#endif
  __syncthreads();
  for (int c = 0; c < nchunks; ++c) {
    const int c0 = jb + c * kMChunk, buf = c & 1;
    if (c0 < je) {
      const int nval = min(kMChunk, je - c0), last = (nval - 1) >> 5;
      // the candidate fragments are read one tile ahead, in two register sets:
      // a set is reloaded with the tile after next as soon as its tile's last
      // MFMA has issued. The first reads of a chunk wait behind its barrier.
      // (A read past the chunk's last tile repeats that tile and is not used.)
      i32x8_t fa[4], fb[4];
      frags(fa, buf, 0);
      frags(fb, buf, min(1, last));
      // Two tiles a turn, one from each set; a turn stages one of the thread's
      // two rows of the next chunk on the way and then loads that row of the
      // chunk after next into the registers that frees (two tiles and a
      // barrier ahead of its use). The turns are written out, not looped, so
      // that each load lands in its row's registers and is waited for only
      // where it is used. Where there is no next chunk (only then can a chunk
      // have fewer than four tiles) the writes go to the free buffer and the
      // loads to the half's last row, neither used (a scalar guard around the
      // loads measured 0.2 to 0.4 us slower in three of three pairs).
      int t = 0;
#ifdef ORBX_M_NOSTAGE
      const uint4 pre[kRep] = {};
#endif
      if (last >= 1) {
        tile(fa, 32, 1, buf ^ 1, sr, 0, pre[0]);
        frags(fa, buf, min(2, last));
        tile(fb, nval - 32, 1, buf ^ 1, sr, 2, pre[0]);
        frags(fb, buf, min(3, last));
#ifndef ORBX_M_NOSTAGE
        pre[0] = cand_row(c0 + 2 * kMChunk, 0);
#endif
        t = 2;
        if (last >= 3) {
          tile(fa, 32, 1, buf ^ 1, sr + kMRowsPerPass, 0, pre[1]);
          tile(fb, nval - 96, 1, buf ^ 1, sr + kMRowsPerPass, 2, pre[1]);
#ifndef ORBX_M_NOSTAGE
          pre[1] = cand_row(c0 + 2 * kMChunk, 1);
#endif
          t = 4;
        }
      }
      if (t == last) tile(fa, nval - 32 * t, 0, 0, 0, 0, pre[0]);
    }
    if (c + 1 < nchunks) __syncthreads();
  }
  // drain: group Y's update of the last tile
  update_group(kNX, kMqTiles);
  // float keys -> (distance << 16 | index) keys, then merge the two lane halves
  // (rows 0-3 / 4-7 of each 8)
  uint32_t u1[kMqTiles], u2[kMqTiles];
#pragma unroll
  for (int q = 0; q < kMqTiles; ++q) {
    u1[q] = top2_ukey(k1[q], jb);
    u2[q] = top2_ukey(k2[q], jb);
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
