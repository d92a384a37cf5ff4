// orbx_blur.hip — GaussianBlur(level, 7x7, sigma 2, BORDER_REFLECT_101)
// (src/ORBextractor.cc:1735-1749), OpenCV 3.x 8U fixed point: kernel taps
// round(256*g) = [18,34,49,55,49,34,18] (sum 257), result (acc + 2^15) >> 16
// (the 8U smooth-symmetric branch of createSeparableLinearFilter). The blurred
// levels feed the rBRIEF tests.
//
// The reference filters rows, then columns, in integers without intermediate
// rounding, so columns-then-rows gives the same bytes; a column sum is at most
// 257 * 255 = 65535 and fits u16 exactly. This kernel streams columns first,
// in registers: no LDS, no barrier.
//   A wave owns a strip of a level: lane i holds the 4 pixels of dword column
//   x0 - 4 + 4i of the current source row (one coalesced dword load per lane
//   and row); lanes 1..62 produce the strip's 248 output columns, lanes 0 and
//   63 are the +-3 halo. The wave walks down a segment of R rows (R + 6 source
//   rows), with the loads of the next 7 rows in flight.
//   column pass: the dword unpacked to two u16 pairs (2 v_perm_b32), a rolling
//                window of 7 unpacked rows (14 VGPRs), 3 v_pk_add_u16 + 4
//                v_pk_mul/mad_u16 per pair by the taps' symmetry,
//   row pass:    the neighbour lanes' column sums by DPP wave shifts (4 moves),
//                16 v_dot2_u32_u16 per 4 outputs on the even-aligned pairs only
//                (an output at an odd offset takes its first or last tap as a
//                pair (0, k0) / (k6, 0)), seeded with 2^15; min, pack, one
//                dword store per lane and row.
// BORDER_REFLECT_101 is applied at load time only: row indices are reflected
// for the loads (scalar), and in a strip that touches the level's left or
// right edge a lane picks its 4 bytes out of two aligned dwords of the
// reflected source columns with a per-lane v_perm_b32 selector. A level that
// is not 16-byte aligned (level 0 can be: the caller's frame) loads bytes.
#include "orbx_device.cuh"

namespace orbx {

constexpr int kBlurStrip = 4 * 62;  // output columns of a strip (lanes 1..62)
// rows of a segment: the halo rows cost a load and an unpack each (no
// arithmetic), so short segments are cheap. Alone, 32 KITTI frames take the
// same time with 16, 24 and 32 rows and longer with 48 and 64; a single frame
// takes the short ones, ~1760 waves instead of 228 (its blur stage: 4 rows as
// fast as the tile kernel it replaced, 2, 3, 5, 6 and 8 rows 0.2-0.4 us slower)
#ifndef ORBX_BLUR_R
#define ORBX_BLUR_R 32
#endif
#ifndef ORBX_BLUR_RS
#define ORBX_BLUR_RS 4
#endif
constexpr int kBlurR = ORBX_BLUR_R, kBlurRs = ORBX_BLUR_RS;

typedef unsigned short us2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t dot2(us2_t pair, uint32_t taps, uint32_t acc) {
  return __builtin_amdgcn_udot2(pair, __builtin_bit_cast(us2_t, taps), acc, false);
}
// the value of the lane below / above (wave_shr:1 / wave_shl:1); undefined in
// lane 0 / 63, the halo lanes, which store nothing
__device__ __forceinline__ us2_t from_lane_below(us2_t v) {
  return __builtin_bit_cast(us2_t, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ us2_t from_lane_above(us2_t v) {
  return __builtin_bit_cast(us2_t, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x130, 0xf, 0xf, false));
}

// One strip segment. MODE 0: every lane's dword lies inside the level's rows
// (one aligned dword load); 1: a strip at the level's left or right edge (two
// aligned dwords and a byte selector); 2: byte loads (unaligned level).
// TAIL: the strip holds the dword that straddles W (W mod 4 != 0), whose
// columns below W are stored as bytes.
// Loads and stores are issued by every lane in every row, outside any
// branch, so that the compiler's counted vmcnt waits see them all and a
// row's unpack waits for its own load only (7 rows back), not for the stores
// of the rows between: a lane with nothing to store gets an offset past the
// buffer's range, which drops the store.
template <int MODE, bool TAIL>
__device__ __forceinline__ void blur_strip(const int* __restrict__ k, int W, int H, int x0, int y0, int rows,
                                           const uint8_t* S, int pitch, uint8_t* D, int dpitch, long long dplane) {
  constexpr int kRaw = MODE == 0 ? 1 : MODE == 1 ? 2 : 4;
  const int lane = threadIdx.x & 63;
  const int c = x0 - 4 + 4 * lane;  // this lane's first column
  // readable bytes of the level: level 0's rows only up to ceil16(W) (orbx_c.h)
  const int srange = (H - 1) * pitch + min(pitch, (W + 15) & ~15);
  const __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc((void*)S, (short)0, srange, 0x00020000);
  int voff[kRaw];
  uint32_t sel = 0;
  if constexpr (MODE == 0) {
    voff[0] = c;
  } else {
    int sx[4], lo = W;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      sx[j] = reflect101_clamped(c + j, W);
      lo = min(lo, sx[j]);
    }
    if constexpr (MODE == 1) {
      // the 4 source columns span at most 4 columns: inside the aligned dwords at a and a + 4
      const int a = lo & ~3;
#pragma unroll
      for (int j = 0; j < 4; ++j) sel |= (uint32_t)min(sx[j] - a, 7) << (8 * j);
      voff[0] = a;
      voff[1] = min(a + 4, (W - 1) & ~3);  // the row's last dword: then no selector reaches the second one
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) voff[j] = sx[j];
    }
  }
  struct Raw {
    uint32_t v[kRaw];
  };
  auto issue = [&](int r) {  // source row y0 - 3 + r, reflected
    const int soff = reflect101_clamped(y0 - 3 + r, H) * pitch;
    Raw q;
#pragma unroll
    for (int j = 0; j < kRaw; ++j)
      q.v[j] = MODE == 2 ? (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(srs, voff[j], soff, 0)
                         : (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(srs, voff[j], soff, 0);
    return q;
  };
  auto pixels = [&](const Raw& q) -> uint32_t {
    if constexpr (MODE == 0) return q.v[0];
    else if constexpr (MODE == 1) return __builtin_amdgcn_perm(q.v[1], q.v[0], sel);
    else return q.v[0] | (q.v[1] << 8) | (q.v[2] << 16) | (q.v[3] << 24);
  };
  const us2_t k0 = {(unsigned short)k[0], (unsigned short)k[0]}, k1 = {(unsigned short)k[1], (unsigned short)k[1]};
  const us2_t k2 = {(unsigned short)k[2], (unsigned short)k[2]}, k3 = {(unsigned short)k[3], (unsigned short)k[3]};
  // tap pairs of the row pass, (low | high << 16)
  const uint32_t t_0 = k[0] << 16, t01 = k[0] | (k[1] << 16), t12 = k[1] | (k[2] << 16), t23 = k[2] | (k[3] << 16);
  const uint32_t t34 = k[3] | (k[4] << 16), t45 = k[4] | (k[5] << 16), t56 = k[5] | (k[6] << 16), t6_ = k[6];
  const int nsrc = rows + 6;
  Raw q[7];
  us2_t wl[7], wh[7];  // the window: source row r in slot r % 7, columns {c, c+1} and {c+2, c+3} as u16
  auto unpack = [&](int slot) {
    const uint32_t p = pixels(q[slot]);
    wl[slot] = __builtin_bit_cast(us2_t, __builtin_amdgcn_perm(0u, p, 0x0c010c00u));
    wh[slot] = __builtin_bit_cast(us2_t, __builtin_amdgcn_perm(0u, p, 0x0c030c02u));
  };
#pragma unroll
  for (int r = 0; r < 7; ++r) q[r] = issue(r);
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    unpack(r);
    q[r] = issue(min(r + 7, nsrc - 1));
  }
  const __amdgpu_buffer_rsrc_t drs = __builtin_amdgcn_make_buffer_rsrc((void*)D, (short)0, (int)dplane, 0x00020000);
  const bool owner = lane >= 1 && lane <= 62 && c < W;
  constexpr int kDrop = 0x40000000;
  const int st4 = owner && c + 4 <= W ? c : kDrop;
  int st1[3];
#pragma unroll
  for (int b = 0; b < 3; ++b) st1[b] = owner && c + 4 > W && c + b < W ? c + b : kDrop;
#pragma unroll 1
  for (int i0 = 0; i0 < rows; i0 += 7) {
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      const int i = i0 + j;  // output row y0 + i from source rows i .. i + 6: slots (j + t) % 7
      if (i >= rows) break;
      unpack((j + 6) % 7);
      q[(j + 6) % 7] = issue(min(i + 13, nsrc - 1));
      const us2_t al = wl[j] + wl[(j + 6) % 7], ah = wh[j] + wh[(j + 6) % 7];
      const us2_t bl = wl[(j + 1) % 7] + wl[(j + 5) % 7], bh = wh[(j + 1) % 7] + wh[(j + 5) % 7];
      const us2_t cl = wl[(j + 2) % 7] + wl[(j + 4) % 7], ch = wh[(j + 2) % 7] + wh[(j + 4) % 7];
      const us2_t vl = al * k0 + bl * k1 + cl * k2 + wl[(j + 3) % 7] * k3;
      const us2_t vh = ah * k0 + bh * k1 + ch * k2 + wh[(j + 3) % 7] * k3;
      // columns c-4 .. c+7 as pairs: ll lh | vl vh | rl rh
      const us2_t ll = from_lane_below(vl), lh = from_lane_below(vh);
      const us2_t rl = from_lane_above(vl), rh = from_lane_above(vh);
      const uint32_t o0 = dot2(vh, t56, dot2(vl, t34, dot2(lh, t12, dot2(ll, t_0, 1u << 15))));
      const uint32_t o1 = dot2(rl, t6_, dot2(vh, t45, dot2(vl, t23, dot2(lh, t01, 1u << 15))));
      const uint32_t o2 = dot2(rl, t56, dot2(vh, t34, dot2(vl, t12, dot2(lh, t_0, 1u << 15))));
      const uint32_t o3 = dot2(rh, t6_, dot2(rl, t45, dot2(vh, t23, dot2(vl, t01, 1u << 15))));
      // o >> 16 of two outputs as a u16 pair, clamped to 255 (257 at most), the four low bytes packed
      const us2_t hi = {255, 255};
      const us2_t m01 = __builtin_elementwise_min(__builtin_bit_cast(us2_t, __builtin_amdgcn_perm(o1, o0, 0x07060302u)), hi);
      const us2_t m23 = __builtin_elementwise_min(__builtin_bit_cast(us2_t, __builtin_amdgcn_perm(o3, o2, 0x07060302u)), hi);
      const uint32_t packed =
          __builtin_amdgcn_perm(__builtin_bit_cast(uint32_t, m23), __builtin_bit_cast(uint32_t, m01), 0x06040200u);
      const int soff = (y0 + i) * dpitch;
      __builtin_amdgcn_raw_buffer_store_b32(packed, drs, st4, soff, 0);
      if constexpr (TAIL) {
#pragma unroll
        for (int b = 0; b < 3; ++b)
          __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(packed >> (8 * b)), drs, st1[b], soff, 0);
      }
    }
  }
}

// BYTES0: level 0 (the caller's frames) is not 16-byte aligned
template <bool BYTES0>
__global__ __launch_bounds__(256) void blur_kernel(ExtractParams P, LevelPtrs lp, const int2* __restrict__ rtab,
                                                   int items, int nitems, int nwg, unsigned magic,
                                                   uint8_t* __restrict__ blur) {
  const int wg = xcd_remap(blockIdx.x + blockIdx.y * gridDim.x, gridDim.x * gridDim.y);
  // the frame by a multiply-high (exact for every id of the plan's batch,
  // checked at plan time), the wave's level, strip and segment by one table load
  const int f = magic ? (int)__umulhi((unsigned)wg, magic) : wg / nwg;
  const int it = (wg - f * nwg) * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (it >= nitems) return;
  const int2 e = rtab[items + it];
  const int l = e.x & 15, x0 = (e.x >> 4) & 0xFFF, y0 = e.x >> 16, rows = e.y;
  const LevelGeom& g = P.lv[l];
  const int W = g.w, H = g.h;
  const uint8_t* S = lp.base[l] + f * lp.fstride[l];
  uint8_t* D = blur + g.off + f * g.plane;
  if (BYTES0 && l == 0)
    blur_strip<2, true>(P.gauss, W, H, x0, y0, rows, S, lp.pitch[l], D, g.pitch, g.plane);
  else if ((W & 3) && x0 + kBlurStrip >= W)
    blur_strip<1, true>(P.gauss, W, H, x0, y0, rows, S, lp.pitch[l], D, g.pitch, g.plane);
  else if (x0 == 0 || x0 + kBlurStrip + 4 > W)
    blur_strip<1, false>(P.gauss, W, H, x0, y0, rows, S, lp.pitch[l], D, g.pitch, g.plane);
  else
    blur_strip<0, false>(P.gauss, W, H, x0, y0, rows, S, lp.pitch[l], D, g.pitch, g.plane);
}

void blur_strip_dims(int small, int* strip, int* rows) {
  *strip = kBlurStrip;
  *rows = small ? kBlurRs : kBlurR;
}

int launch_blur(const ExtractParams& P, const LevelPtrs& lp, const int2* rtab, uint8_t* blur, int batch,
                hipStream_t s) {
  static const int cus = [] {
    int dev = 0, n = 256;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    return n;
  }();
  // the long segments once they give every SIMD two waves
  const int v = (long long)P.blur_ntiles[0] * batch >= 8ll * cus ? 0 : 1;
  const int nwg = (P.blur_ntiles[v] + 3) / 4;
  if (lp.aligned16[0])
    hipLaunchKernelGGL(blur_kernel<false>, dim3(nwg, batch), dim3(256), 0, s, P, lp, rtab, P.blur_tiles[v],
                       P.blur_ntiles[v], nwg, P.blur_magic[v], blur);
  else
    hipLaunchKernelGGL(blur_kernel<true>, dim3(nwg, batch), dim3(256), 0, s, P, lp, rtab, P.blur_tiles[v],
                       P.blur_ntiles[v], nwg, P.blur_magic[v], blur);
  return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
}

}  // namespace orbx
