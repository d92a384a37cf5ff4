// orbx_initializer.hip — Initializer (src/Initializer.cc): the host form and the
// kernels of orbm_initialize_batch. The arithmetic is orbx_initializer.cuh's
// for both. (orbx_init.hip is the search that precedes it.)
//
// iz_gather_kernel, one workgroup per pair: the gathered list (i1,
// matches12[i1]) compacted in i1 order into the handle's workspace (ballot and
// mbcnt per wave, a running base across tiles), then Normalize of both frames:
// lane 0 of waves 0..3 each runs one of the four serial float sums over tiles
// of 256 coordinates staged in LDS, once for the means and once for the
// deviations. T1, T2 and T2inv go to the pair's header.
// iz_solve_score_kernel, grid (hypothesis chunks, {H, F}, pairs), 256 threads:
// lanes 0..kInitzChunk-1 draw and solve one hypothesis each, the Jacobi work
// arrays in LDS laid out [word][lane] because its row indices are run-time
// values; then each wave takes every fourth hypothesis of the chunk, its lanes
// compute the two score terms of 64 matches at a time and every lane adds the
// 128 terms in match order (v_readlane of a constant lane), which is the
// reference's sequential float sum.
// iz_select_kernel, one workgroup per pair: first-strictly-greater argmax of
// both score lists, the winners' inlier flags once more, the model choice and
// the 3x3 decompositions (thread 0, work arrays in LDS), one CheckRT pass per
// candidate (a match per lane, integer counts by DPP, the cosine order
// statistic by a 4 x 8-bit radix select over integer histograms), the
// acceptance rule, and the winner's pass once more for the outputs.
// Counts are integers and no float sum is reordered, so a pair's output bits
// do not depend on the batch, the slot, the run, the pitch or the chunking.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "orbx_initializer.cuh"
#include "orbx_wave.cuh"

namespace orbx {

namespace {

constexpr int kT = 256, kW = kT / 64;

// a pair's header in the workspace
struct IzHdr {
  int N, pad[3];
  IzNorm n1, n2;
  float T1[9], T2[9], T2inv[9];
  float pad2[64 - 4 - 8 - 27];
};
static_assert(sizeof(IzHdr) == 256, "one header per 256 bytes");

struct IzArgs {
  const orbx_kp *kps1, *kps2;
  const int *n1, *n2;
  int kp_pitch, max_its;
  const int* matches12;
  const orbm_camera* cam;
  orbm_init_params P;
  const uint32_t* rand8;
  orbm_init_result* result;
  float *R21, *t21, *Tcw, *p3d;
  uint8_t* triangulated;
  int* matches12_out;
  uint8_t *inlier_h, *inlier_f;
  float *T1, *T2, *H21, *F21;
  orbm_init_hyp* hyp;
  orbm_init_rt* rt;
  // workspace
  IzHdr* hdr;             // [pairs]
  float* lf;              // [pairs][4][kp_pitch]: u1, v1, u2, v2 of the gathered list
  int* li;                // [pairs][2][kp_pitch]: i1, i2
  orbm_init_hyp* hyp_ws;  // [pairs][2][max_its]
  uint8_t* flags;         // [pairs][3][kp_pitch]: inlier of H, of F, counted by the current CheckRT pass
  uint32_t* keys;         // [pairs][kp_pitch]: cosine keys of the current CheckRT pass
  int* err;
};

__device__ __forceinline__ int clampn(int n, int hi) { return n < 0 ? 0 : (n > hi ? hi : n); }

// one of Normalize's sums over `n` staged values, in index order
__device__ __forceinline__ float iz_chain(const float* v, int n, float acc, float mean, bool dev) {
  for (int k = 0; k < n; ++k) acc = iz_fadd(acc, dev ? iz_norm_dev(v[k], mean) : v[k]);
  return acc;
}

__global__ __launch_bounds__(kT) void iz_gather_kernel(const IzArgs A) {
  __shared__ int scan[2][kW];
  __shared__ float tile[4][kT];
  __shared__ float red[4];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n1 = clampn(A.n1[p], A.kp_pitch), n2 = clampn(A.n2[p], A.kp_pitch);
  const orbx_kp* kps1 = A.kps1 + (size_t)p * A.kp_pitch;
  const orbx_kp* kps2 = A.kps2 + (size_t)p * A.kp_pitch;
  const int* m12 = A.matches12 + (size_t)p * A.kp_pitch;
  float* lf = A.lf + (size_t)p * 4 * A.kp_pitch;
  int* li = A.li + (size_t)p * 2 * A.kp_pitch;
  // :51-63
  int N = 0, bad = 0;
  for (int base = 0, par = 0; base < n1; base += kT, par ^= 1) {
    const int i1 = base + tid;
    int i2 = -1;
    if (i1 < n1) {
      i2 = m12[i1];
      if (i2 >= n2) bad = 1, i2 = -1;
    }
    const bool valid = i2 >= 0;
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
    if (valid) {  // off < n1 <= kp_pitch
      lf[off] = kps1[i1].x;
      lf[A.kp_pitch + off] = kps1[i1].y;
      lf[2 * A.kp_pitch + off] = kps2[i2].x;
      lf[3 * A.kp_pitch + off] = kps2[i2].y;
      li[off] = i1;
      li[A.kp_pitch + off] = i2;
    }
  }
  if (bad) atomicOr(A.err, kStatusInitSkipped);
  IzHdr* H = A.hdr + p;
  if (N < 8) {  // the whole workgroup
    if (tid == 0) H->N = N;
    return;
  }
  // Normalize (:749-795) of mvKeys1 and mvKeys2: chain c = wave: x1, y1, x2, y2
  const int nmax = n1 > n2 ? n1 : n2;
  const int nc = wave < 2 ? n1 : n2;
  float mean = 0.0f, acc = 0.0f;
  for (int pass = 0; pass < 2; ++pass) {
    acc = 0.0f;
    for (int base = 0; base < nmax; base += kT) {
      const int i = base + tid;
      if (i < n1) tile[0][tid] = kps1[i].x, tile[1][tid] = kps1[i].y;
      if (i < n2) tile[2][tid] = kps2[i].x, tile[3][tid] = kps2[i].y;
      __syncthreads();
      if (lane == 0) {
        const int left = nc - base;
        acc = iz_chain(tile[wave], left < 0 ? 0 : (left > kT ? kT : left), acc, mean, pass == 1);
      }
      __syncthreads();
    }
    if (lane == 0) {
      const float m = iz_norm_mean(acc, nc);
      if (pass == 0) mean = m;
      red[wave] = m;
    }
    __syncthreads();
    if (tid == 0) {
      if (pass == 0) {
        H->n1.mx = red[0], H->n1.my = red[1], H->n2.mx = red[2], H->n2.my = red[3];
      } else {
        H->n1.sx = iz_norm_scale(red[0]), H->n1.sy = iz_norm_scale(red[1]);
        H->n2.sx = iz_norm_scale(red[2]), H->n2.sy = iz_norm_scale(red[3]);
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    const IzNorm a = H->n1, b = H->n2;
    float T1[9], T2[9], T2inv[9];
    iz_norm_T(a, T1);
    iz_norm_T(b, T2);
    iz_invert3(T2, T2inv);  // :134
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      H->T1[k] = T1[k], H->T2[k] = T2[k], H->T2inv[k] = T2inv[k];
      if (A.T1) A.T1[(size_t)p * 9 + k] = T1[k];
      if (A.T2) A.T2[(size_t)p * 9 + k] = T2[k];
    }
    H->N = N;
  }
}

__device__ __forceinline__ float readlane_f(float v, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}

__global__ __launch_bounds__(kT) void iz_solve_score_kernel(const IzArgs A) {
  __shared__ float svdF[kInitzSvdFloats * kInitzChunk];
  __shared__ double svdW[kInitzSvdDoubles * kInitzChunk];
  __shared__ orbm_init_hyp hs[kInitzChunk];
  __shared__ float inv12[kInitzChunk][9];
  const int p = blockIdx.z, isF = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h0 = (int)blockIdx.x * kInitzChunk;
  const IzHdr* H = A.hdr + p;
  const int N = H->N;
  if (N < 8) return;  // the whole workgroup
  const int nh = min(kInitzChunk, A.max_its - h0);
  const float* lf = A.lf + (size_t)p * 4 * A.kp_pitch;
  const int P = A.kp_pitch;
  if (tid < nh) {
    const int h = h0 + tid;
    const uint32_t* r8 = A.rand8 + ((size_t)p * A.max_its + h) * 8;
    uint32_t r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = r8[j];
    orbm_init_hyp hyp;
    iz_draw(r, N, hyp.idx);
    const IzNorm a = H->n1, b = H->n2;
    float x1[8], y1[8], x2[8], y2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {  // :151-157
      const int k = hyp.idx[j];
      x1[j] = iz_norm_pt(lf[k], a.mx, a.sx);
      y1[j] = iz_norm_pt(lf[P + k], a.my, a.sy);
      x2[j] = iz_norm_pt(lf[2 * P + k], b.mx, b.sx);
      y2[j] = iz_norm_pt(lf[3 * P + k], b.my, b.sy);
    }
    float T1[9], T2[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) T1[k] = H->T1[k];
    float H12[9];
    if (isF) {
#pragma unroll
      for (int k = 0; k < 9; ++k) T2[k] = H->T2[k];
      iz_solve_f(x1, y1, x2, y2, T1, T2, svdF + tid, svdW + tid, kInitzChunk, hyp.M);
#pragma unroll
      for (int k = 0; k < 9; ++k) H12[k] = 0.0f;
    } else {
#pragma unroll
      for (int k = 0; k < 9; ++k) T2[k] = H->T2inv[k];
      iz_solve_h(x1, y1, x2, y2, T1, T2, svdF + tid, svdW + tid, kInitzChunk, hyp.M, H12);
    }
    hyp.score = 0.0f;
    hs[tid] = hyp;
#pragma unroll
    for (int k = 0; k < 9; ++k) inv12[tid][k] = H12[k];
  }
  __syncthreads();
  const float invs2 = iz_inv_sigma2(A.P.sigma);
  for (int j = wave; j < nh; j += kW) {
    float M[9], M12[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) M[k] = hs[j].M[k], M12[k] = inv12[j][k];
    float score = 0.0f;
    for (int base = 0; base < N; base += 64) {
      const int k = base + lane;
      float t1 = 0.0f, t2 = 0.0f;
      if (k < N) {
        const float u1 = lf[k], v1 = lf[P + k], u2 = lf[2 * P + k], v2 = lf[3 * P + k];
        if (isF)
          (void)iz_check_f(M, invs2, u1, v1, u2, v2, &t1, &t2);
        else
          (void)iz_check_h(M, M12, invs2, u1, v1, u2, v2, &t1, &t2);
      }
      // the sequential sum (:363, :379 / :441, :459): every lane adds the tile's terms in match order
#pragma unroll
      for (int l = 0; l < 64; ++l) {
        score = iz_fadd(score, readlane_f(t1, l));
        score = iz_fadd(score, readlane_f(t2, l));
      }
    }
    if (lane == 0) {
      orbm_init_hyp hyp = hs[j];
      hyp.score = score;
      const size_t at = ((size_t)p * 2 + isF) * A.max_its + (h0 + j);
      A.hyp_ws[at] = hyp;
      if (A.hyp) A.hyp[at] = hyp;
    }
  }
}

struct IzSel {
  int best[2];
  float score[2];
  int model, ncand, n_inl, degenerate;
  float RH;
  IzVerdict v;
  int bin, kk;
};

__global__ __launch_bounds__(kT) void iz_select_kernel(const IzArgs A) {
  __shared__ float sc[2 * kInitzMaxIts];
  __shared__ IzSel S;
  __shared__ float svdF[18];
  __shared__ double svdW[3];
  __shared__ orbm_init_rt rts[8];
  __shared__ IzRt prep;
  __shared__ int hist[256];
  __shared__ int wsum[2][kW];
  __shared__ int n_good[8];
  __shared__ float parallax[8];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const IzHdr* H = A.hdr + p;
  const int N = H->N, P = A.kp_pitch;
  orbm_init_result* res = A.result ? A.result + p : nullptr;
  if (N < 8) {  // the whole workgroup: nothing but the result is written
    if (tid == 0 && res) {
      orbm_init_result r{};
      r.code = kIzTooFewMatches;
      r.n = N;
      r.best_h = r.best_f = r.best_rt = -1;
      *res = r;
    }
    return;
  }
  const int n1 = clampn(A.n1[p], P);
  const float* lf = A.lf + (size_t)p * 4 * P;
  const int* li = A.li + (size_t)p * 2 * P;
  const orbm_init_hyp* hyp = A.hyp_ws + (size_t)p * 2 * A.max_its;
  uint8_t* flags = A.flags + (size_t)p * 3 * P;
  uint32_t* keys = A.keys + (size_t)p * P;
  const orbm_camera cam = A.cam[p];
  // :165 / :216: the first strictly greater score wins, from 0
  for (int h = tid; h < 2 * A.max_its; h += kT) sc[h] = hyp[h].score;
  __syncthreads();
  if (wave < 2) {
    const float* s = sc + wave * A.max_its;
    float bs = 0.0f;
    int bi = -1;
    for (int h = lane; h < A.max_its; h += 64)
      if (s[h] > bs) bs = s[h], bi = h;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const float os = __shfl_xor(bs, off);
      const int oi = __shfl_xor(bi, off);
      if (oi >= 0 && (bi < 0 || os > bs || (os == bs && oi < bi))) bs = os, bi = oi;
    }
    if (lane == 0) S.best[wave] = bi, S.score[wave] = bs;
  }
  // the per-keypoint outputs of a pair that is not accepted
  {
    const int* m12 = A.matches12 + (size_t)p * P;
    for (int i = tid; i < n1; i += kT) {
      if (A.p3d) {
        float* q = A.p3d + ((size_t)p * P + i) * 3;
        q[0] = q[1] = q[2] = 0.0f;
      }
      if (A.triangulated) A.triangulated[(size_t)p * P + i] = 0;
      if (A.matches12_out) {
        const int m = m12[i];
        A.matches12_out[(size_t)p * P + i] = m < 0 ? m : -1;
      }
    }
  }
  __syncthreads();
  // the winners' flags once more
  const float invs2 = iz_inv_sigma2(A.P.sigma);
  {
    const int bh = S.best[0], bf = S.best[1];
    float Hm[9], H12[9], Fm[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      Hm[k] = bh >= 0 ? hyp[bh].M[k] : 0.0f;
      Fm[k] = bf >= 0 ? hyp[A.max_its + bf].M[k] : 0.0f;
    }
    iz_invert3(Hm, H12);  // :161
    int ch = 0, cf = 0;
    for (int k = tid; k < N; k += kT) {
      const float u1 = lf[k], v1 = lf[P + k], u2 = lf[2 * P + k], v2 = lf[3 * P + k];
      float t1, t2;
      const bool ih = bh >= 0 && iz_check_h(Hm, H12, invs2, u1, v1, u2, v2, &t1, &t2);
      const bool jf = bf >= 0 && iz_check_f(Fm, invs2, u1, v1, u2, v2, &t1, &t2);
      flags[k] = ih;
      flags[P + k] = jf;
      if (A.inlier_h) A.inlier_h[(size_t)p * P + k] = ih;
      if (A.inlier_f) A.inlier_f[(size_t)p * P + k] = jf;
      ch += ih, cf += jf;
    }
    ch = wave_sum_dpp(ch);
    cf = wave_sum_dpp(cf);
    if (lane == 0) wsum[0][wave] = ch, wsum[1][wave] = cf;
  }
  __syncthreads();
  if (tid == 0) {
    const int bh = S.best[0], bf = S.best[1];
    float RH;
    const int model = iz_choose_model(S.score[0], S.score[1], bh, bf, &RH);
    S.model = model;
    S.RH = RH;
    S.degenerate = 0;
    S.ncand = 0;
    S.n_inl = 0;
    for (int k = 0; k < 8; ++k) {
      n_good[k] = 0;
      parallax[k] = 0.0f;
      for (int q = 0; q < 9; ++q) rts[k].R[q] = 0.0f;
      for (int q = 0; q < 3; ++q) rts[k].t[q] = 0.0f;
    }
    float M[9];
    if (bh >= 0) {
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        M[k] = hyp[bh].M[k];
        if (A.H21) A.H21[(size_t)p * 9 + k] = M[k];
      }
    }
    if (model == kIzModelH) {
      S.n_inl = wsum[0][0] + wsum[0][1] + wsum[0][2] + wsum[0][3];
      if (iz_candidates_h(M, cam, svdF, svdW, 1, rts))
        S.ncand = 8;
      else
        S.degenerate = 1;
    }
    if (bf >= 0) {
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        M[k] = hyp[A.max_its + bf].M[k];
        if (A.F21) A.F21[(size_t)p * 9 + k] = M[k];
      }
    }
    if (model == kIzModelF) {
      S.n_inl = wsum[1][0] + wsum[1][1] + wsum[1][2] + wsum[1][3];
      iz_candidates_f(M, cam, svdF, svdW, 1, rts);
      S.ncand = 4;
    }
    if (model != kIzModelNone && A.rt)
      for (int k = 0; k < 8; ++k) A.rt[(size_t)p * 8 + k] = rts[k];
  }
  __syncthreads();
  const int model = S.model, ncand = S.ncand;
  const uint8_t* inl = flags + (model == kIzModelF ? P : 0);
  uint8_t* counted = flags + 2 * P;
  const float th2 = iz_th2(A.P.sigma);
  // one CheckRT pass per candidate (:494-497, :698-718); pass ncand is the winner's once more, for the outputs
  for (int c = 0; c <= ncand; ++c) {
    if (c == ncand) {
      if (tid == 0) {
        S.v = model == kIzModelF ? iz_accept_f(n_good, parallax, S.n_inl, A.P.min_parallax, A.P.min_triangulated)
                                 : iz_accept_h(n_good, parallax, S.n_inl, A.P.min_parallax, A.P.min_triangulated);
      }
      __syncthreads();
      if (!S.v.ok) break;
    }
    const int cand = c == ncand ? S.v.best : c;
    if (tid == 0) iz_prepare_rt(cam, rts[cand], &prep);
    __syncthreads();
    const IzRt C = prep;
    int cnt = 0;
    for (int k = tid; k < N; k += kT) {
      bool ok = false;
      if (inl[k]) {
        float q[3], cosp;
        bool good;
        ok = iz_check_rt(cam, C, th2, lf[k], lf[P + k], lf[2 * P + k], lf[3 * P + k], q, &cosp, &good);
        if (ok && c == ncand) {  // :889-893
          const int i1 = li[k];
          if (A.p3d) {
            float* o = A.p3d + ((size_t)p * P + i1) * 3;
            o[0] = q[0], o[1] = q[1], o[2] = q[2];
          }
          if (good) {
            if (A.triangulated) A.triangulated[(size_t)p * P + i1] = 1;
            if (A.matches12_out) A.matches12_out[(size_t)p * P + i1] = li[P + k];
          }
        }
        if (ok) keys[k] = iz_cos_key(cosp);
      }
      counted[k] = ok;
      cnt += ok;
    }
    if (c == ncand) break;
    cnt = wave_sum_dpp(cnt);
    if (lane == 0) wsum[0][wave] = cnt;
    __syncthreads();  // the counts, keys and counted flags of this pass
    const int nGood = wsum[0][0] + wsum[0][1] + wsum[0][2] + wsum[0][3];
    // :896-904: element min(50, size - 1) of the sorted cosines, by four 8-bit digits from the top
    uint32_t prefix = 0, maskv = 0;
    int kk = nGood - 1 < 50 ? nGood - 1 : 50;
    if (nGood > 0) {
      for (int shift = 24; shift >= 0; shift -= 8) {
        hist[tid] = 0;
        __syncthreads();
        for (int k = tid; k < N; k += kT)
          if (counted[k] && (keys[k] & maskv) == prefix) atomicAdd(&hist[(keys[k] >> shift) & 255u], 1);
        __syncthreads();
        if (wave == 0) {
          const int c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
          const int s4 = c0 + c1 + c2 + c3;
          const int incl = wave_incl_scan_dpp(s4), excl = incl - s4;
          if (kk >= excl && kk < incl) {
            int r = kk - excl, b = 0;
            if (r >= c0) {
              r -= c0, b = 1;
              if (r >= c1) {
                r -= c1, b = 2;
                if (r >= c2) r -= c2, b = 3;
              }
            }
            S.bin = 4 * lane + b;
            S.kk = r;
          }
        }
        __syncthreads();
        prefix |= (uint32_t)S.bin << shift;
        maskv |= 255u << shift;
        kk = S.kk;
      }
    }
    if (tid == 0) {
      n_good[c] = nGood;
      parallax[c] = nGood > 0 ? iz_parallax(iz_key_cos(prefix)) : 0.0f;
    }
    __syncthreads();
  }
  if (tid == 0) {
    IzVerdict v;
    if (model == kIzModelNone)
      v = IzVerdict{0, kIzNoScore, -1};
    else if (S.degenerate)
      v = IzVerdict{0, kIzDegenerate, -1};
    else
      v = S.v;
    if (v.ok) {
      const orbm_init_rt w = rts[v.best];
      for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) {
          if (A.R21) A.R21[(size_t)p * 9 + 3 * r + k] = w.R[3 * r + k];
          if (A.Tcw) A.Tcw[(size_t)p * 12 + 4 * r + k] = w.R[3 * r + k];
        }
        if (A.t21) A.t21[(size_t)p * 3 + r] = w.t[r];
        if (A.Tcw) A.Tcw[(size_t)p * 12 + 4 * r + 3] = w.t[r];
      }
    }
    if (res) {
      orbm_init_result r{};
      r.ok = v.ok;
      r.code = v.code;
      r.n = N;
      r.model = model;
      r.SH = S.score[0];
      r.SF = S.score[1];
      r.RH = S.RH;
      r.best_h = S.best[0];
      r.best_f = S.best[1];
      r.best_rt = v.best;
      for (int k = 0; k < 8; ++k) r.n_good[k] = n_good[k], r.parallax[k] = parallax[k];
      r.n_inliers = S.n_inl;
      *res = r;
    }
  }
}

size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

size_t initializer_ws_bytes(int kp_pitch, int pairs, int max_iterations) {
  const size_t pp = (size_t)pairs * kp_pitch;
  return up256((size_t)pairs * sizeof(IzHdr)) + up256(pp * 4 * sizeof(float)) + up256(pp * 2 * sizeof(int)) +
         up256((size_t)pairs * 2 * max_iterations * sizeof(orbm_init_hyp)) + up256(pp * 3) + up256(pp * sizeof(uint32_t));
}

int launch_initialize(const InitzLaunchArgs& L, void* ws, void* stream) {
  IzArgs A{};
  A.kps1 = L.kps1;
  A.kps2 = L.kps2;
  A.n1 = L.n1;
  A.n2 = L.n2;
  A.kp_pitch = L.kp_pitch;
  A.max_its = L.params.max_iterations;
  A.matches12 = L.matches12;
  A.cam = L.cam;
  A.P = L.params;
  A.rand8 = L.rand8;
  A.result = L.result;
  A.R21 = L.R21;
  A.t21 = L.t21;
  A.Tcw = L.Tcw;
  A.p3d = L.p3d;
  A.triangulated = L.triangulated;
  A.matches12_out = L.matches12_out;
  A.inlier_h = L.inlier_h;
  A.inlier_f = L.inlier_f;
  A.T1 = L.T1;
  A.T2 = L.T2;
  A.H21 = L.H21;
  A.F21 = L.F21;
  A.hyp = L.hyp;
  A.rt = L.rt;
  A.err = L.err;
  const size_t pp = (size_t)L.pairs * L.kp_pitch;
  uint8_t* w = (uint8_t*)ws;
  A.hdr = (IzHdr*)w;
  w += up256((size_t)L.pairs * sizeof(IzHdr));
  A.lf = (float*)w;
  w += up256(pp * 4 * sizeof(float));
  A.li = (int*)w;
  w += up256(pp * 2 * sizeof(int));
  A.hyp_ws = (orbm_init_hyp*)w;
  w += up256((size_t)L.pairs * 2 * A.max_its * sizeof(orbm_init_hyp));
  A.flags = w;
  w += up256(pp * 3);
  A.keys = (uint32_t*)w;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((A.max_its + kInitzChunk - 1) / kInitzChunk, 2, L.pairs);
  hipLaunchKernelGGL(iz_gather_kernel, dim3(L.pairs), dim3(kT), 0, s, A);
  hipLaunchKernelGGL(iz_solve_score_kernel, grid, dim3(kT), 0, s, A);
  hipLaunchKernelGGL(iz_select_kernel, dim3(L.pairs), dim3(kT), 0, s, A);
  return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
}

// The host form: Initializer::Initialize (:44-121) as the reference runs it, one hypothesis after the other.
int initialize_host(const orbx_kp* kps1, int n1, const orbx_kp* kps2, int n2, const int* matches12,
                    const orbm_camera* cam, const orbm_init_params* P, const uint32_t* rand8, orbm_init_result* result,
                    float* R21, float* t21, float* Tcw, float* p3d, uint8_t* triangulated, int* matches12_out,
                    uint8_t* inlier_h, uint8_t* inlier_f, float* T1o, float* T2o, float* H21o, float* F21o,
                    orbm_init_hyp* hyp, orbm_init_rt* rt, int* status) {
  // :51-63
  std::vector<int> I1, I2;
  std::vector<float> U1, V1, U2, V2;
  int bits = 0;
  for (int i1 = 0; i1 < n1; ++i1) {
    const int i2 = matches12[i1];
    if (i2 < 0) continue;
    if (i2 >= n2) {
      bits |= kStatusInitSkipped;
      continue;
    }
    I1.push_back(i1);
    I2.push_back(i2);
    U1.push_back(kps1[i1].x);
    V1.push_back(kps1[i1].y);
    U2.push_back(kps2[i2].x);
    V2.push_back(kps2[i2].y);
  }
  if (status) *status = bits;
  const int N = (int)I1.size();
  orbm_init_result res{};
  res.n = N;
  res.best_h = res.best_f = res.best_rt = -1;
  if (N < 8) {
    res.code = kIzTooFewMatches;
    if (result) *result = res;
    return ORBX_OK;
  }
  // Normalize (:749-795)
  IzNorm nm[2];
  for (int f = 0; f < 2; ++f) {
    const orbx_kp* k = f ? kps2 : kps1;
    const int n = f ? n2 : n1;
    float sx = 0, sy = 0;
    for (int i = 0; i < n; ++i) sx = iz_fadd(sx, k[i].x), sy = iz_fadd(sy, k[i].y);
    nm[f].mx = iz_norm_mean(sx, n);
    nm[f].my = iz_norm_mean(sy, n);
    float dx = 0, dy = 0;
    for (int i = 0; i < n; ++i) dx = iz_fadd(dx, iz_norm_dev(k[i].x, nm[f].mx)), dy = iz_fadd(dy, iz_norm_dev(k[i].y, nm[f].my));
    nm[f].sx = iz_norm_scale(iz_norm_mean(dx, n));
    nm[f].sy = iz_norm_scale(iz_norm_mean(dy, n));
  }
  float T1[9], T2[9], T2inv[9];
  iz_norm_T(nm[0], T1);
  iz_norm_T(nm[1], T2);
  iz_invert3(T2, T2inv);
  if (T1o) std::memcpy(T1o, T1, sizeof T1);
  if (T2o) std::memcpy(T2o, T2, sizeof T2);
  // FindHomography (:124-172) and FindFundamental (:175-223)
  const int its = P->max_iterations;
  const float invs2 = iz_inv_sigma2(P->sigma);
  float svdF[kInitzSvdFloats];
  double svdW[kInitzSvdDoubles];
  float best[2][9] = {}, bestScore[2] = {0.0f, 0.0f};
  int bestIt[2] = {-1, -1};
  for (int f = 0; f < 2; ++f)
    for (int it = 0; it < its; ++it) {
      orbm_init_hyp h;
      iz_draw(rand8 + (size_t)8 * it, N, h.idx);
      float x1[8], y1[8], x2[8], y2[8];
      for (int j = 0; j < 8; ++j) {
        const int k = h.idx[j];
        x1[j] = iz_norm_pt(U1[k], nm[0].mx, nm[0].sx);
        y1[j] = iz_norm_pt(V1[k], nm[0].my, nm[0].sy);
        x2[j] = iz_norm_pt(U2[k], nm[1].mx, nm[1].sx);
        y2[j] = iz_norm_pt(V2[k], nm[1].my, nm[1].sy);
      }
      float H12[9];
      if (f)
        iz_solve_f(x1, y1, x2, y2, T1, T2, svdF, svdW, 1, h.M);
      else
        iz_solve_h(x1, y1, x2, y2, T1, T2inv, svdF, svdW, 1, h.M, H12);
      float score = 0;
      for (int k = 0; k < N; ++k) {
        float t1, t2;
        if (f)
          (void)iz_check_f(h.M, invs2, U1[k], V1[k], U2[k], V2[k], &t1, &t2);
        else
          (void)iz_check_h(h.M, H12, invs2, U1[k], V1[k], U2[k], V2[k], &t1, &t2);
        score = iz_fadd(score, t1);
        score = iz_fadd(score, t2);
      }
      h.score = score;
      if (hyp) hyp[(size_t)f * its + it] = h;
      if (score > bestScore[f]) {  // :165 / :216
        bestScore[f] = score;
        bestIt[f] = it;
        std::memcpy(best[f], h.M, sizeof h.M);
      }
    }
  std::vector<uint8_t> inl[2];
  int ninl[2] = {0, 0};
  {
    float H12[9];
    iz_invert3(best[0], H12);
    for (int f = 0; f < 2; ++f) {
      inl[f].assign(N, 0);
      for (int k = 0; k < N && bestIt[f] >= 0; ++k) {
        float t1, t2;
        inl[f][k] = f ? iz_check_f(best[1], invs2, U1[k], V1[k], U2[k], V2[k], &t1, &t2)
                      : iz_check_h(best[0], H12, invs2, U1[k], V1[k], U2[k], V2[k], &t1, &t2);
        ninl[f] += inl[f][k];
      }
    }
  }
  if (inlier_h) std::memcpy(inlier_h, inl[0].data(), N);
  if (inlier_f) std::memcpy(inlier_f, inl[1].data(), N);
  if (bestIt[0] >= 0 && H21o) std::memcpy(H21o, best[0], sizeof best[0]);
  if (bestIt[1] >= 0 && F21o) std::memcpy(F21o, best[1], sizeof best[1]);
  for (int i = 0; i < n1; ++i) {
    if (p3d) p3d[3 * i] = p3d[3 * i + 1] = p3d[3 * i + 2] = 0.0f;
    if (triangulated) triangulated[i] = 0;
    if (matches12_out) matches12_out[i] = matches12[i] < 0 ? matches12[i] : -1;
  }
  res.SH = bestScore[0];
  res.SF = bestScore[1];
  res.best_h = bestIt[0];
  res.best_f = bestIt[1];
  // :112-118
  const int model = iz_choose_model(res.SH, res.SF, bestIt[0], bestIt[1], &res.RH);
  res.model = model;
  IzVerdict v{0, kIzNoScore, -1};
  orbm_init_rt rts[8] = {};
  int ncand = 0;
  if (model == kIzModelH) {
    res.n_inliers = ninl[0];
    if (iz_candidates_h(best[0], *cam, svdF, svdW, 1, rts))
      ncand = 8;
    else
      v = IzVerdict{0, kIzDegenerate, -1};
  } else if (model == kIzModelF) {
    res.n_inliers = ninl[1];
    iz_candidates_f(best[1], *cam, svdF, svdW, 1, rts);
    ncand = 4;
  }
  if (model != kIzModelNone && rt) std::memcpy(rt, rts, sizeof rts);
  if (ncand) {
    const std::vector<uint8_t>& in = inl[model == kIzModelF ? 1 : 0];
    const float th2 = iz_th2(P->sigma);
    std::vector<uint32_t> keys;
    for (int c = 0; c <= ncand; ++c) {
      if (c == ncand) {
        v = model == kIzModelF ? iz_accept_f(res.n_good, res.parallax, res.n_inliers, P->min_parallax, P->min_triangulated)
                               : iz_accept_h(res.n_good, res.parallax, res.n_inliers, P->min_parallax, P->min_triangulated);
        if (!v.ok) break;
      }
      const int cand = c == ncand ? v.best : c;
      IzRt C;
      iz_prepare_rt(*cam, rts[cand], &C);
      keys.clear();
      for (int k = 0; k < N; ++k) {
        if (!in[k]) continue;
        float q[3], cosp;
        bool good;
        if (!iz_check_rt(*cam, C, th2, U1[k], V1[k], U2[k], V2[k], q, &cosp, &good)) continue;
        keys.push_back(iz_cos_key(cosp));
        if (c == ncand) {
          const int i1 = I1[k];
          if (p3d) p3d[3 * i1] = q[0], p3d[3 * i1 + 1] = q[1], p3d[3 * i1 + 2] = q[2];
          if (good) {
            if (triangulated) triangulated[i1] = 1;
            if (matches12_out) matches12_out[i1] = I2[k];
          }
        }
      }
      if (c == ncand) break;
      const int nGood = (int)keys.size();
      res.n_good[c] = nGood;
      res.parallax[c] = 0.0f;
      if (nGood > 0) {  // :896-904
        const int idx = std::min(50, nGood - 1);
        std::nth_element(keys.begin(), keys.begin() + idx, keys.end());
        res.parallax[c] = iz_parallax(iz_key_cos(keys[idx]));
      }
    }
  }
  res.ok = v.ok;
  res.code = v.code;
  res.best_rt = v.best;
  if (v.ok) {
    const orbm_init_rt& w = rts[v.best];
    for (int r = 0; r < 3; ++r) {
      for (int k = 0; k < 3; ++k) {
        if (R21) R21[3 * r + k] = w.R[3 * r + k];
        if (Tcw) Tcw[4 * r + k] = w.R[3 * r + k];
      }
      if (t21) t21[r] = w.t[r];
      if (Tcw) Tcw[4 * r + 3] = w.t[r];
    }
  }
  if (result) *result = res;
  return ORBX_OK;
}

}  // namespace orbx

using namespace orbx;

extern "C" {

int orbm_initializer_rand_fill(uint32_t* out, int iterations) {
  static_assert(RAND_MAX == 2147483647, "the draws assume glibc's RAND_MAX");
  if (!out || iterations < 0) return ORBX_EINVAL;
  for (int k = 0; k < 8 * iterations; ++k) out[k] = (uint32_t)rand();
  return ORBX_OK;
}

int orbm_initializer_limits(int* max_iterations, int* chunk, int* lds_pitch) {
  if (max_iterations) *max_iterations = kInitzMaxIts;
  if (chunk) *chunk = kInitzChunk;
  if (lds_pitch) *lds_pitch = 0;
  return ORBX_OK;
}

}  // extern "C"
