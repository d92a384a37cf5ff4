// orbx_pyramid.hip — ComputePyramid (src/ORBextractor.cc:1837-1863).
//
// Level l = cv::resize(level l-1, size_l, INTER_LINEAR), chained. OpenCV 3.x
// evaluates INTER_LINEAR on u8 in fixed point: 11-bit horizontal and vertical
// coefficients (tables built on the host from the same float expressions,
// orbx_plan.hip resize_tables), an int32 horizontal pass, and the vertical
// pass (D0*b0 + D1*b1 + 2^21) >> 22; columns at or beyond `xmax` replicate
// the source pixel (x2048). An exact 2x downscale switches to the 2x2 area
// mean, as cv::resize does. The 19-px border the reference pads each level
// with is never read by extraction and is not built.
//
// pyr_resize_kernel: one launch per level (each level depends on the
// previous), used when a level's band does not fit LDS. A 256-thread
// block produces a 16-row x 256-column output tile: the source rows/columns
// the tile touches are staged in LDS with 16-byte loads, then each thread
// computes a 4x4 output block from LDS and writes 4 x 32-bit stores.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "orbx_device.cuh"

namespace orbx {

constexpr int kPyrTW = 256, kPyrTH = 16;
constexpr int kPyrMaxSrcW = 576;  // >= 256 * 2 (scale <= 2) + 2 + 16 alignment + 16 slack
constexpr int kPyrMaxSrcH = 36;   // >= 16 * 2 + 2 + slack

__global__ __launch_bounds__(256) void pyr_resize_kernel(
    const uint8_t* __restrict__ src, long long src_fs, int src_pitch, int sw, int sh, uint8_t* __restrict__ dst,
    long long dst_fs, int dst_pitch, int dw, int dh, const int2* __restrict__ xtab, const int2* __restrict__ ytab,
    int xmax, int area2x, int src_aligned16) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[kPyrMaxSrcH][kPyrMaxSrcW];
  __shared__ int2 s_xt[kPyrTW];
  __shared__ int2 s_yt[kPyrTH];
  const int wg = xcd_remap(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z),
                           gridDim.x * gridDim.y * gridDim.z);
  const int f = wg / (gridDim.x * gridDim.y), tid = threadIdx.x;
  const int x0 = (wg % gridDim.x) * kPyrTW, y0 = ((wg / gridDim.x) % gridDim.y) * kPyrTH;
  const int nx = min(kPyrTW, dw - x0), ny = min(kPyrTH, dh - y0);
  const uint8_t* S = src + f * src_fs;
  // source footprint of the tile
  int sx_lo, sx_hi, sy_lo, sy_hi;  // inclusive
  if (area2x) {
    if (tid < nx) s_xt[tid] = make_int2(2 * (x0 + tid), 0);
    if (tid < ny) s_yt[tid] = make_int2(2 * (y0 + tid) | ((2 * (y0 + tid) + 1) << 16), 0);
    sx_lo = 2 * x0;
    sx_hi = 2 * (x0 + nx - 1) + 1;
    sy_lo = 2 * y0;
    sy_hi = 2 * (y0 + ny - 1) + 1;
  } else {
    if (tid < nx) s_xt[tid] = xtab[x0 + tid];
    if (tid < ny) s_yt[tid] = ytab[y0 + tid];
    sx_lo = xtab[x0].x;
    sx_hi = min(xtab[x0 + nx - 1].x + 1, sw - 1);
    sy_lo = ytab[y0].x & 0xFFFF;
    sy_hi = ytab[y0 + ny - 1].x >> 16;
  }
  const int a0 = src_aligned16 ? (sx_lo & ~15) : sx_lo;
  const int nrow = sy_hi - sy_lo + 1;
  // stage source rows [sy_lo, sy_hi], columns [a0, sx_hi]
  if (src_aligned16) {
    const int nch = (sx_hi - a0 + 16) >> 4;
    for (int i = tid; i < nrow * nch; i += 256) {
      const int r = i / nch, ch = i - r * nch;
      const uint8_t* g = S + (long long)(sy_lo + r) * src_pitch + a0 + ch * 16;
      if (a0 + ch * 16 + 16 <= src_pitch) {
        *(uint4*)&tile[r][ch * 16] = *(const uint4*)g;
      } else {  // never read past the row's pitch (the last row may end the buffer)
        for (int k = 0; k < 16 && a0 + ch * 16 + k < sw; ++k) tile[r][ch * 16 + k] = g[k];
      }
    }
  } else {
    const int ncol = sx_hi - a0 + 1;
    for (int i = tid; i < nrow * ncol; i += 256) {
      const int r = i / ncol, c = i - r * ncol;
      tile[r][c] = S[(long long)(sy_lo + r) * src_pitch + a0 + c];
    }
  }
  __syncthreads();
  // thread -> 4 columns x 4 rows
  const int cx = (tid & 63) * 4, ry = (tid >> 6) * 4;
  if (cx >= nx) return;
  int sxl[4], a0v[4], a1v[4], rep[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c = min(cx + q, nx - 1);
    const int2 xt = s_xt[c];
    sxl[q] = xt.x - a0;
    a0v[q] = (short)(xt.y & 0xFFFF);
    a1v[q] = (short)(xt.y >> 16);
    rep[q] = area2x ? 0 : (x0 + c >= xmax);
  }
  uint8_t* D = dst + f * dst_fs + (long long)(y0 + ry) * dst_pitch + x0 + cx;
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    if (ry + rr >= ny) break;
    const int2 yt = s_yt[ry + rr];
    const uint8_t* r0 = tile[(yt.x & 0xFFFF) - sy_lo];
    const uint8_t* r1 = tile[(yt.x >> 16) - sy_lo];
    int v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int s = sxl[q];
      if (area2x) {
        v[q] = (r0[s] + r0[s + 1] + r1[s] + r1[s + 1] + 2) >> 2;
      } else {
        int D0, D1;
        if (!rep[q]) {
          D0 = __mul24((int)r0[s], a0v[q]) + __mul24((int)r0[s + 1], a1v[q]);
          D1 = __mul24((int)r1[s], a0v[q]) + __mul24((int)r1[s + 1], a1v[q]);
        } else {
          D0 = r0[s] * 2048;
          D1 = r1[s] * 2048;
        }
        const int b0 = (short)(yt.y & 0xFFFF), b1 = (short)(yt.y >> 16);
        v[q] = sat_u8((__mul24(D0, b0) + __mul24(D1, b1) + (1 << 21)) >> 22);
      }
    }
    const uint32_t packed = pack4_u8(v[0], v[1], v[2], v[3]);
    uint8_t* drow = D + (long long)rr * dst_pitch;
    if (cx + 4 <= nx) {
      *(uint32_t*)drow = packed;  // dst pitch, x0 and cx are multiples of 4
    } else {
      for (int q = 0; cx + q < nx; ++q) drow[q] = (uint8_t)(packed >> (8 * q));
    }
  }
}

// ---------------------------------------------------------------- band pyramid
// All levels in ONE launch: a workgroup owns a tile of the last level (a
// band of rows x a column tile) and, walking the chain back, the rows and
// columns of every level that tile depends on. It stages the level-0 tile
// once (16-byte loads, all in flight), then builds level 1, 2, ... in LDS,
// each from the previous level's tile in LDS, and writes to HBM only the rows
// and columns it owns at each level (tiles partition every level; the few
// source rows and columns two tiles share are recomputed by both instead of
// exchanged). Ranges per (band, level) and (column tile, level) come from the
// host (orbx_plan.hip plan_band_pyramid / plan_pyr_cols): comp = computed,
// own = written. Column tiles let a single frame (or a small batch) spread
// over more workgroups than row bands alone allow, at a few recomputed
// columns per tile edge.
#ifndef ORBX_PYR_THREADS
#define ORBX_PYR_THREADS 512
#endif
constexpr int kPyrBandThreads = ORBX_PYR_THREADS;
// (the 2x2 area mean runs through the bilinear loop, band_row, with the
// coefficients a0 = a1 = 2048 and 4*b0 = 4*b1 = 2048 in the host's column
// records and row entries)
// waves per SIMD the band kernel is compiled for (5: <= 96 VGPRs, two
// 512-thread workgroups per CU; 6 would allow three at <= 53 KB of LDS)
#ifndef ORBX_PYR_WPE
#define ORBX_PYR_WPE 5
#endif

// A thread's 8 output columns are 4 runs of 2: run k starts at column
// 2 * (gi + k * G), G = ceil(w / 8). The 32 lanes of an LDS half-wave then read
// source bytes within ~77 bytes (20 dwords, distinct banks).
__device__ __forceinline__ int pyr_col(int gi, int G, int q) { return 2 * (gi + (q >> 1) * G) + (q & 1); }

typedef unsigned short pyr_us2_t __attribute__((ext_vector_type(2)));

// i / d for 0 <= i < 2^21, d >= 1, given rcp = v_rcp_f32(d), without the ~35
// instructions of an integer division: (i + 0.5) / d lies at least 0.5 / d from
// an integer, and the reciprocal's and the product's rounding (relative 2^-22
// together) move it by at most i / d * 2^-22 < 0.5 / d.
__device__ __forceinline__ int band_div(int i, float rcp) { return (int)(((float)i + 0.5f) * rcp); }

// Horizontal pass of one source row for a thread's 8 columns. A run's two
// columns read source bytes sx0, sx0 + 1 and sx1, sx1 + 1 with sx0 <= sx1 <=
// sx0 + 3 (a scale of at most 2 steps 2 or 3 source columns; a column clamped
// to the level's last repeats it), all inside the two aligned dwords from
// sx0 & ~3: one ds_read2_b32 per run (band_load) instead of a byte read per
// pixel, one v_perm_b32 per column that spreads its pixel pair to u16 x 2
// (byte selectors fixed per level, BandCols), and one v_dot2_u32_u16 with the
// column's {a0, a1} (non-negative 11-bit values: the unsigned dot is exact,
// D <= 255 * 2048 < 2^20). The pair read reaches bytes sx0 & ~3 .. + 7, up to
// 6 bytes past the last byte a column uses: into the row's padding, the next
// row, or (from the last row of one buffer) the first bytes of the other
// buffer or of the staged y entries, which other lanes may be writing. The
// selectors never pick those bytes, and the kernel's LDS block ends 16 bytes
// after the y entries, so every read stays inside it. The dword alignment
// rests on the plan: every LDS row pitch and pyr_lds_a are multiples of 4
// (plan_pyr_cols rounds pitches to 16; ORBX_PYR_PADMOD steps by 4 or 16). A
// 16-bit read at the pair's own byte is no
// substitute: at odd addresses it runs the LDS at a third of the speed
// (109 us per 32 KITTI frames against 37).
struct BandCols {
  int off[4];       // run k: LDS-relative byte offset of its dword pair in a source row (a multiple of 4)
  uint32_t sel[8];  // column q: v_perm_b32 selector {o, zero, o + 1, zero}, o = the column's byte in the pair
  uint32_t a01[8];  // column q: a0 | a1 << 16
};
__device__ __forceinline__ void band_load(const uint8_t* row, const BandCols& bc, uint32_t (&p)[8]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t* d = (const uint32_t*)(row + bc.off[k]);
    p[2 * k] = d[0];
    p[2 * k + 1] = d[1];
  }
}
__device__ __forceinline__ void band_hpass(const uint32_t (&p)[8], const BandCols& bc, uint32_t (&D)[8]) {
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const uint32_t pp = __builtin_amdgcn_perm(p[q | 1], p[q & ~1], bc.sel[q]);
    D[q] = __builtin_amdgcn_udot2(__builtin_bit_cast(pyr_us2_t, pp), __builtin_bit_cast(pyr_us2_t, bc.a01[q]), 0u, false);
  }
}

// a * b + c for a, b < 2^24 as one v_mad_u32_u24 (from __umul24 and adds the
// compiler makes two multiplies and a three-operand add per pixel)
__device__ __forceinline__ uint32_t band_mad24(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t d;
  asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}

// One output row from the horizontal results Da (source row y0; kept from the
// previous output row where that row's second source row was y0) and Db
// (source row y1, always new; it is the next row's candidate for Da).
// Vertical pass: b0 and b1 arrive x4 (yt.y), so the rounded value
// (D0*b0 + D1*b1 + 2^21) >> 22 is the top byte of D0*4b0 + D1*4b1 + 2^23:
// a0 + a1 and b0 + b1 are at most 2049, so the sum is at most
// 4 * (255 * 2049 * 2049 + 2^21) = 4 290 757 628 < 2^32 with every term >= 0,
// and its top byte is at most 255: no clamp. The 2x2 area mean runs through the
// same code with a0 = a1 = 2048 and 4b0 = 4b1 = 2048 (the host's tables):
// ((p00 + p01 + p10 + p11) * 2^22 + 2^23) >> 24 = (sum + 2) >> 2.
struct BandRowCtx {
  const uint8_t* src;   // the source level's LDS tile, row src_lo first
  uint8_t* dst;         // this level's LDS tile
  uint8_t* g[4];        // the level's plane in HBM + the tile's column origin + 2kG (uniform)
  const int2* yt;       // staged row entries, row cd.x first
  int spitch, dpitch, gpitch, src_lo, row0;
  unsigned own_lo, own_n;  // owned rows: r - own_lo < own_n
  // hoisted out of the row loop: run k is owned whole by the tile / only its
  // first column is (the level's last column), and whether any run is such
  bool st2[4], st1[4], any1;
};
__device__ __forceinline__ void band_row(const BandRowCtx& c, int r, uint32_t loff, uint32_t goff, int& have,
                                         const BandCols& bc, int G, uint32_t (&Da)[8], uint32_t (&Db)[8]) {
  const int2 yt = c.yt[r - c.row0];
  const int y0 = yt.x & 0xFFFF, y1 = yt.x >> 16;
  const uint8_t* const row1 = c.src + __mul24(y1 - c.src_lo, c.spitch);
  uint32_t p1[8];
  if (y0 != have) {
    // the second source row's reads are in flight while the first is redone
    uint32_t p0[8];
    band_load(c.src + __mul24(y0 - c.src_lo, c.spitch), bc, p0);
    band_load(row1, bc, p1);
    band_hpass(p0, bc, Da);
  } else {
    band_load(row1, bc, p1);
  }
  band_hpass(p1, bc, Db);
  have = y1;
  const uint32_t b0 = (uint32_t)yt.y & 0xFFFFu, b1 = (uint32_t)yt.y >> 16;
  const bool owned = (unsigned)r - c.own_lo < c.own_n;
  uint32_t pk[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t va = band_mad24(Da[2 * k], b0, band_mad24(Db[2 * k], b1, 1u << 23));
    const uint32_t vb = band_mad24(Da[2 * k + 1], b0, band_mad24(Db[2 * k + 1], b1, 1u << 23));
    pk[k] = __builtin_amdgcn_perm(vb, va, 0x0c0c0703u);  // {va byte 3, vb byte 3, 0, 0}
    *(uint16_t*)(c.dst + loff + 2 * k * G) = (uint16_t)pk[k];  // the LDS row holds the run even past the computed columns
    // owned ranges start at even columns (plan_pyr_cols), so a run is owned
    // whole or not at all, but at the level's last column (below)
    if (owned && c.st2[k]) *(uint16_t*)(c.g[k] + goff) = (uint16_t)pk[k];
  }
  if (c.any1 && owned) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (c.st1[k]) c.g[k][goff] = (uint8_t)pk[k];
  }
}

// Diagnostics (tools/variant.sh; wrong pixels, timing only): the bound of what
// building level 1 from global memory, without the level-0 tile in LDS, could
// save. ORBX_PYR_NOSTAGE skips the level-0 staging
// altogether; ORBX_PYR_STAGE_NOLDS issues its loads but does not write them to LDS.
#if (defined(ORBX_PYR_NOSTAGE) || defined(ORBX_PYR_STAGE_NOLDS)) && !defined(ORBX_DIAG)
#error "result-changing diagnostic switches need -DORBX_DIAG (tools/variant.sh)"
#endif

__global__ __launch_bounds__(kPyrBandThreads) __attribute__((amdgpu_waves_per_eu(ORBX_PYR_WPE))) void pyr_band_kernel(ExtractParams P, LevelPtrs lp,
                                                                   const int2* __restrict__ rtab, int* dbg) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const unsigned long long t_begin = __builtin_amdgcn_s_memtime();
  const int nb = P.pyr_nbands, nct = P.pyr_nct, L = P.L, tid = threadIdx.x;
  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  const int f = wg / (nb * nct), tile = wg - f * (nb * nct), band = tile / nct, ct = tile - band * nct;
  const int2* bt = rtab + P.pyr_bands + (long long)band * L * 2;  // {comp}, {own} rows per level
  const int2* xt = rtab + P.pyr_ctiles + (long long)ct * L * 4;   // {comp}, {own} columns, {LDS pitch, origin}, {records}
  uint8_t* const bufA = smem;
  uint8_t* const bufB = smem + P.pyr_lds_a;
  // the band's row coefficients of every level, staged once: a global load
  // per output row would put one memory latency on every row iteration
  int2* const s_yt = (int2*)(smem + P.pyr_lds_a + P.pyr_lds_b);
  // one staged row entry per thread, {sy0 | sy1 << 16, 4*b0 | 4*b1 << 16}
  // (band_row; 4 * 2048 fits 16 bits): the band's rows of levels 1..L-1
  // flattened, a list the host makes per band (plan_band_pyramid; the band
  // table's level-0 own entry holds {its offset, its length}). Bands hold far
  // fewer than kPyrBandThreads rows, larger ones loop. The load is issued
  // before the level-0 loads so that both are in flight together.
  const int2 yh = bt[1];
  const int ytot = yh.y;
  int2 yval = make_int2(0, 0);
  if (tid < ytot) yval = rtab[yh.x + tid];
  for (int i = tid + kPyrBandThreads; i < ytot; i += kPyrBandThreads) s_yt[i] = rtab[yh.x + i];  // very tall bands only

  // ---- stage level-0 rows [comp_lo, comp_hi] x the tile's columns, 4 loads in flight per thread
  {
    const int2 c0 = bt[0], x0c = xt[0], x0p = xt[2];
    const int rows = c0.y - c0.x + 1, lp0 = x0p.x, org = x0p.y, pitch = lp.pitch[0];
    // the last staged column: the tile's last computed one, inside the image
    // (a source column past it is only read with weight 0)
    const int xe = min(x0c.y, P.lv[0].w - 1);
    const uint8_t* S = lp.base[0] + f * lp.fstride[0] + (long long)c0.x * pitch + org;
    if (lp.aligned16[0]) {
      typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
      const int nch = ((xe - org) >> 4) + 1, total = rows * nch;  // at most a CU's LDS / 16
      const float rnch = __builtin_amdgcn_rcpf((float)nch);
      // unpredicated (indices past the end repeat the last chunk)
#ifdef ORBX_PYR_NOSTAGE
      for (int i0 = tid; i0 < 0; i0 += 4 * kPyrBandThreads) {
#else
      for (int i0 = tid; i0 < total; i0 += 4 * kPyrBandThreads) {
#endif
        u32x4 v[4];
        int so[4], lo[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int i = min(i0 + q * kPyrBandThreads, total - 1);
          const int r = band_div(i, rnch), ch = i - r * nch;
          lo[q] = r * pitch + ch * 16;
          so[q] = r * lp0 + ch * 16;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = *(const u32x4*)(S + lo[q]);
        if (i0 == tid && tid < ytot) s_yt[tid] = yval;
#ifdef ORBX_PYR_STAGE_NOLDS
#pragma unroll
        for (int q = 0; q < 4; ++q) asm volatile("" ::"v"(v[q]));  // the loads stay, their LDS writes go
#else
#pragma unroll
        for (int q = 0; q < 4; ++q) *(u32x4*)(bufA + so[q]) = v[q];
#endif
      }
#ifdef ORBX_PYR_NOSTAGE
      if (tid < ytot) s_yt[tid] = yval;
#else
      if (tid >= total && tid < ytot) s_yt[tid] = yval;
#endif
    } else {
      if (tid < ytot) s_yt[tid] = yval;
      const int ncol = xe - org + 1;
      for (int r = 0; r < rows; ++r)
        for (int c = tid; c < ncol; c += kPyrBandThreads) bufA[r * lp0 + c] = S[(long long)r * pitch + c];
    }
  }

  // the thread's column record (BandCols and its store flags, made on the
  // host: plan_band_pyramid): level l+1's is fetched while level l is computed
  typedef unsigned int rec4_t __attribute__((ext_vector_type(4)));
  rec4_t nxt[5];
  uint32_t nxt_flags = 0;
  int nxt_gi = 0, nxt_ra = 0, nxt_rb = -1;  // the thread's column group and rows [ra, rb] at that level
  // a thread's 8 columns are 4 runs of 2 (pyr_col) with G = ceil(width/8)
  // over the tile's computed columns: neighbouring lanes read source bytes a
  // run's width x 1.2 apart
  auto fetch_cols = [&](int l) {
    const int2 xc = xt[4 * l];
    const int G = (xc.y - xc.x + 1 + 7) >> 3;
    const float rG = __builtin_amdgcn_rcpf((float)G);
    const int chunk = band_div(tid, rG), gi = tid - chunk * G;
    // Rows per thread: the level's rows over the kPyrBandThreads / G row chunks
    // (G <= kPyrBandThreads, so nchunks >= 1: plan_pyr_cols refuses wider
    // tiles). Chunks differ by at most one row and the longer ones come first,
    // so the spare rows fill whole waves (a wave takes as long as its longest
    // lane) and every chunk is used, as when rows were strided. Worked out
    // here, a level ahead and without integer divisions: two dependent scalar
    // divisions at the top of a level were ~300 of a short level's ~3 k clocks.
    const int2 cd = bt[2 * l];
    const int nrows = cd.y - cd.x + 1, nchunks = band_div(kPyrBandThreads, rG);
    const int len = band_div(nrows, __builtin_amdgcn_rcpf((float)nchunks)), rem = nrows - len * nchunks;
    nxt_gi = gi;
    nxt_ra = cd.x + chunk * len + min(chunk, rem);
    nxt_rb = chunk < nchunks ? nxt_ra + len - (chunk < rem ? 0 : 1) : nxt_ra - 1;
    const rec4_t* rec = (const rec4_t*)(rtab + xt[4 * l + 3].x) + __mul24(gi, 6);
#pragma unroll
    for (int i = 0; i < 5; ++i) nxt[i] = rec[i];
    nxt_flags = ((const uint32_t*)rec)[20];
  };
  fetch_cols(1);
  lds_sync();  // LDS only: the owned rows written to HBM are not read back here
  if (dbg && tid == 0) dbg[blockIdx.x * 16] = (int)(__builtin_amdgcn_s_memtime() - t_begin);

  // ---- levels 1 .. L-1: thread -> 8 output columns (runs of 2) x a contiguous
  // chunk of the level's computed rows. Walking the chunk, the horizontal
  // result of a row's second source row stays in registers and serves as the
  // next row's first whenever the staged y entries say it is the same source
  // row (four rows out of five at scale 1.2; never on the 2x2 area path, on the
  // first row of a chunk or after a step of two source rows).
  int yoff = 0;
  for (int l = 1; l < L; ++l) {
    const int2 cs = bt[2 * (l - 1)], cd = bt[2 * l], own = bt[2 * l + 1];
    const int2 xc = xt[4 * l], sp = xt[4 * (l - 1) + 2], dp = xt[4 * l + 2];
    const int G = (xc.y - xc.x + 1 + 7) >> 3, gi = nxt_gi, ra = nxt_ra, rb = nxt_rb;
    BandCols bc;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      bc.off[q] = (int)nxt[0][q];
      bc.sel[q] = nxt[1][q], bc.sel[4 + q] = nxt[2][q];
      bc.a01[q] = nxt[3][q], bc.a01[4 + q] = nxt[4][q];
    }
    const uint32_t flags = nxt_flags;
    if (l + 1 < L) fetch_cols(l + 1);
    BandRowCtx c;
    c.src = (l & 1) ? bufA : bufB;
    c.dst = (l & 1) ? bufB : bufA;
    c.yt = s_yt + yoff;
    c.spitch = sp.x, c.dpitch = dp.x, c.gpitch = lp.pitch[l], c.src_lo = cs.x, c.row0 = cd.x;
    c.own_lo = (unsigned)own.x, c.own_n = (unsigned)(own.y - own.x + 1);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      c.g[k] = (uint8_t*)lp.base[l] + f * lp.fstride[l] + xc.x + 2 * k * G;
      c.st2[k] = (flags >> k) & 1u;
      c.st1[k] = (flags >> (4 + k)) & 1u;
    }
    c.any1 = (flags & 0xF0u) != 0;
    // 32-bit offsets of the thread's first run in the LDS tile and in the
    // level's plane (level sides are at most 4096), advanced by a pitch per row
    uint32_t loff = (uint32_t)(__mul24(ra - cd.x, c.dpitch) + 2 * gi);
    uint32_t goff = (uint32_t)(ra * c.gpitch + 2 * gi);
    uint32_t Da[8], Db[8];
    int have = -1;  // the source row whose horizontal result the next row's Da holds
    for (int r = ra; r <= rb; r += 2) {
      band_row(c, r, loff, goff, have, bc, G, Da, Db);
      loff += c.dpitch, goff += c.gpitch;
      if (r + 1 <= rb) band_row(c, r + 1, loff, goff, have, bc, G, Db, Da);
      loff += c.dpitch, goff += c.gpitch;
    }
    yoff += cd.y - cd.x + 1;
    lds_sync();
    if (dbg && tid == 0) dbg[blockIdx.x * 16 + l] = (int)(__builtin_amdgcn_s_memtime() - t_begin);
  }
}

size_t pyr_band_lds_bytes(const ExtractParams& P) { return (size_t)P.pyr_lds_a + P.pyr_lds_b + P.pyr_lds_y + 16; }
const void* pyr_band_kernel_ptr() { return (const void*)pyr_band_kernel; }
int pyr_band_occupancy(size_t lds) {
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, pyr_band_kernel, kPyrBandThreads, lds) != hipSuccess) return 1;
  return std::max(1, n);
}

static int launch_band(const ExtractParams& P, const LevelPtrs& lp, const int2* rtab, int batch, hipStream_t s) {
  static int* dbg = nullptr;  // diagnostics only: per-workgroup phase cycles (ORBX_PYR_PROF=1)
  static int dbg_cap = 0;
  static const bool prof = getenv("ORBX_PYR_PROF") && getenv("ORBX_PYR_PROF")[0] == '1';
  const int nwg = P.pyr_nbands * P.pyr_nct * batch;
  if (prof && nwg > dbg_cap) {
    if (dbg) (void)hipFree(dbg);
    (void)hipMalloc(&dbg, (size_t)nwg * 16 * 4);
    dbg_cap = nwg;
  }
  hipLaunchKernelGGL(pyr_band_kernel, dim3(nwg), dim3(kPyrBandThreads), pyr_band_lds_bytes(P), s, P, lp, rtab,
                     prof ? dbg : nullptr);
  if (prof) {
    std::vector<int> h((size_t)nwg * 16);
    (void)hipStreamSynchronize(s);
    (void)hipMemcpy(h.data(), dbg, h.size() * 4, hipMemcpyDeviceToHost);
    double avg[16] = {0};
    int mx[16] = {0};
    for (int w = 0; w < nwg; ++w)
      for (int k = 0; k < P.L; ++k) {
        avg[k] += h[w * 16 + k];
        mx[k] = std::max(mx[k], h[w * 16 + k]);
      }
    fprintf(stderr, "pyr_band plans (bands x tiles/cost/lds):");
    for (int i = 0; i < P.pyr_nplans; ++i)
      fprintf(stderr, " %dx%d/%d/%d", P.pyr_plan[i].nbands, P.pyr_plan[i].nct, P.pyr_plan[i].cost,
              P.pyr_plan[i].lds_a + P.pyr_plan[i].lds_b + P.pyr_plan[i].lds_y + 16);
    fprintf(stderr, "\n");
    fprintf(stderr, "pyr_band: %d WGs (%d bands x %d tiles); phase cycles avg/max:", nwg, P.pyr_nbands, P.pyr_nct);
    for (int k = 0; k < P.L; ++k) fprintf(stderr, " [%d] %.0f/%d", k, avg[k] / nwg, mx[k]);
    fprintf(stderr, "\n");
  }
  return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
}

int launch_pyramid(const ExtractParams& P, const LevelPtrs& lp, const int2* rtab, int batch, hipStream_t s) {
  if (P.L < 2) return ORBX_OK;
  if (P.pyr_fused) {
    // each plan's resident workgroups per CU (LDS and the kernel's registers)
    // were found at plan time
    static const int cus = [] {
      int dev = 0, n = 256;
      (void)hipGetDevice(&dev);
      (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
      return n;
    }();
    // experiments and the per-plan parity test: read per launch (a captured
    // graph keeps the plan it was captured with)
    const char* fp = getenv("ORBX_PYR_PLAN");
    const int forced = fp ? atoi(fp) : -1;
    ExtractParams Q = P;
    select_pyr_plan(Q, forced >= 0 && forced < P.pyr_nplans
                           ? forced
                           : pick_pyr_plan(P, batch, cus));
    return launch_band(Q, lp, rtab, batch, s);
  }
  for (int l = 1; l < P.L; ++l) {
    const LevelGeom& sg = P.lv[l - 1];
    const LevelGeom& d = P.lv[l];
    dim3 grid((d.w + kPyrTW - 1) / kPyrTW, (d.h + kPyrTH - 1) / kPyrTH, batch);
    hipLaunchKernelGGL(pyr_resize_kernel, grid, dim3(256), 0, s, lp.base[l - 1], lp.fstride[l - 1], lp.pitch[l - 1],
                       sg.w, sg.h, (uint8_t*)lp.base[l], lp.fstride[l], lp.pitch[l], d.w, d.h, rtab + d.xtab,
                       rtab + d.ytab, d.xmax, d.area2x, lp.aligned16[l - 1]);
  }
  return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
}

}  // namespace orbx
