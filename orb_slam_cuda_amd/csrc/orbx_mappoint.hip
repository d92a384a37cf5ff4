// orbx_mappoint.hip — MapPoint::ComputeDistinctiveDescriptors
// (src/MapPoint.cc:247-312) and MapPoint::UpdateNormalAndDepth (:335-376) for a
// list of map points, in place on the device: the point's descriptor becomes
// the observation with the least median Hamming distance to the others, its
// normal the mean viewing direction, its distance range the reference
// keyframe's. The arithmetic is in orbx_mappoint.cuh (shared with the host).
//
// Most points have a handful of observations and a few have hundreds, so the
// points are sorted into classes by observation count N first:
//
//   refresh_prep_kernel   one thread per point: N from the offsets, the point
//                         appended to its class's list (one atomic counter per
//                         class; the order inside a list does not matter, every
//                         output is indexed by point). N = 0 ends here.
//   refresh_wave_kernel   N <= 64. A wave takes 8, 4, 2 or 1 points of the
//                         classes N <= 8, 16, 32, 64, in groups of 8, 16, 32 or
//                         64 lanes; lane i holds observation i and its
//                         descriptor (8 registers). Descriptor j is broadcast
//                         (v_readlane in the 64-lane class, ds_bpermute in a
//                         group), the distance row goes to LDS as u16 at
//                         [j][lane] (a lane only reads its own column), and the
//                         median is found by bisecting the value range 0..256
//                         (9 counts of the row, no sort). The winner is the
//                         group minimum of (median << 16 | lane): least median,
//                         then first index. An observation on a bad keyframe
//                         keeps its lane and is masked out of rows and columns.
//   refresh_block_kernel  N > 64: a 1024-thread workgroup per point. A table of
//                         descriptor rows (or "not kept") for the first 2048
//                         observations and, up to N = 1024, the descriptors sit
//                         in LDS; past those sizes they are read from global
//                         memory. A row takes 16 lanes (each counts a sixteenth
//                         of the columns), 64 rows a round; a row
//                         bisects below the best median of the rounds before it
//                         only, after one count that tells whether it can win
//                         at all (a later row must be strictly smaller).
//                         Distances are recomputed at every step. The key is
//                         (median << 32 | index) in 64 bits: exact for every N.
//
// The normal is an ordered float sum (a dependent chain, like the database's
// ordered score sum): every lane computes its observation's unit vector, then
// the terms are added one at a time in list order (lane reads in a wave, LDS
// and one thread in a workgroup).
#include "orbx_mappoint.cuh"
#include "orbx_wave.cuh"

namespace orbx {

constexpr int kRefThreads = 256, kRefWaves = kRefThreads / 64;
constexpr int kRefBlockThreads = 1024;  // block kernel: four waves per SIMD keep the vector issue busy
constexpr int kRefRowLanes = 16;        // block kernel: lanes that share a row (one DPP row)
constexpr int kRefRows = kRefBlockThreads / kRefRowLanes;  // rows per round
constexpr int kRefLdsDesc = 1024;  // block kernel: descriptors in LDS up to this N
constexpr int kRefLdsRows = 2048;  // block kernel: row-table entries in LDS
constexpr uint32_t kNoRow = 0xFFFFFFFFu;  // never a valid row: desc_row < desc_rows <= 2^32 - 1

static_assert(sizeof(orbm_observation) == 8 && sizeof(orbm_keyframe_ref) == 16 && sizeof(orbm_point_refkf) == 8,
              "record layouts");

__device__ __forceinline__ int refresh_class(uint32_t N) {
  return N <= 8 ? 0 : N <= 16 ? 1 : N <= 32 ? 2 : N <= 64 ? 3 : 4;
}

__device__ __forceinline__ uint32_t obs_count(const RefreshArgs& A, int p, uint32_t* o0) {
  const uint32_t a = A.off[p], b = A.off[p + 1];
  *o0 = a;
  return b > a ? b - a : 0u;
}

__device__ __forceinline__ bool ref_out_of_range(const RefreshArgs& A, const orbm_point_refkf& r) {
  return r.kf >= A.n_kfs || r.octave < 0 || r.octave >= A.nlevels;
}

// A.scale[l] without a dynamically indexed copy of the arguments
__device__ __forceinline__ float scale_of(const RefreshArgs& A, int l) {
  float s = A.scale[0];
#pragma unroll
  for (int k = 1; k < kMaxLevels; ++k) s = k == l ? A.scale[k] : s;
  return s;
}

// normal, min_distance, max_distance of record q: 5 floats from byte 12 on
__device__ __forceinline__ void store_normal_depth(const RefreshArgs& A, uint32_t q, const float* sum, uint32_t n,
                                                   const float* pos, const orbm_point_refkf& rf) {
  const orbm_keyframe_ref kr = A.kfs[rf.kf];
  float out[5];
  mp_finish(sum, n, pos, kr.Ow, scale_of(A, rf.octave), scale_of(A, A.nlevels - 1), out);
  float* dst = A.mps[q].normal;
#pragma unroll
  for (int k = 0; k < 5; ++k) dst[k] = out[k];
}

__global__ __launch_bounds__(kRefThreads) void refresh_prep_kernel(RefreshArgs A) {
  const int p = blockIdx.x * kRefThreads + threadIdx.x;
  int c = -1;
  if (p < A.points) {
    uint32_t o0;
    const uint32_t N = obs_count(A, p, &o0);
    if (N == 0) {
      if (A.best) A.best[p] = -1;
      if (A.median) A.median[p] = -1;
    } else {
      c = refresh_class(N);
    }
  }
  // one atomic per wave and class; a list entry is < points, every point is listed once
#pragma unroll
  for (int k = 0; k < kRefreshClasses; ++k) {
    const uint64_t m = __ballot(c == k);
    if (!m) continue;  // uniform
    const int leader = __ffsll((long long)m) - 1;
    int first = 0;
    if ((int)(threadIdx.x & 63) == leader) first = atomicAdd(&A.counts[k], __popcll(m));
    first = __builtin_amdgcn_readlane(first, leader);
    if (c == k) A.lists[(size_t)k * A.points + first + mbcnt64(m)] = p;
  }
}

// minimum over each group of G lanes, in every lane of the group (all 64 lanes active)
template <int G>
__device__ __forceinline__ int group_min(int v) {
  v = min(v, dpp_i<kDppQuad1032>(INT_MAX, v));
  v = min(v, dpp_i<kDppQuad2301>(INT_MAX, v));
  v = min(v, dpp_i<kDppHalfMirror>(INT_MAX, v));
  if (G >= 16) v = min(v, dpp_i<kDppMirror>(INT_MAX, v));
  if (G >= 32) v = min(v, __shfl_xor(v, 16));
  if (G >= 64) v = min(v, __shfl_xor(v, 32));
  return v;
}

// lane (group base + j)'s value; j is uniform over the wave
template <int G>
__device__ __forceinline__ int group_bcast(int v, int j) {
  if (G == 64) return __builtin_amdgcn_readlane(v, j);
  return __shfl(v, (int)((threadIdx.x & 63 & ~(G - 1)) + j));
}

// One wave item of the class with groups of G lanes: 64 / G points, `item`
// counting the class's list in steps of that many. Every lane of the wave
// stays on one path (ballots, DPP and lane reads need them all).
template <int G>
__device__ __forceinline__ void refresh_groups(const RefreshArgs& A, const int* __restrict__ list, int cnt, int item,
                                               uint16_t* s_row) {
  constexpr int kPer = 64 / G;
  constexpr int kShift = G == 8 ? 3 : G == 16 ? 4 : G == 32 ? 5 : 6;
  const int lane = threadIdx.x & 63, g = lane >> kShift, l = lane & (G - 1);
  const int idx = item * kPer + g;
  const bool has = idx < cnt;
  const int p = has ? list[idx] : 0;
  uint32_t o0 = 0, N = 0;
  if (has) N = min(obs_count(A, p, &o0), (uint32_t)G);
  const uint32_t q = has ? (A.ids ? A.ids[p] : (uint32_t)p) : 0u;
  const bool active = has && (uint32_t)l < N;
  orbm_observation ob{0u, 0u};
  if (active) ob = A.obs[(size_t)o0 + l];
  bool bad_arg = active && (ob.kf >= A.n_kfs || ob.desc_row >= A.desc_rows);
  orbm_point_refkf rf{0u, 0};
  if (has && A.mps) {
    rf = A.ref[p];
    bad_arg |= l == 0 && ref_out_of_range(A, rf);
  }
  uint64_t gmask = ~0ull;
  if (G < 64) gmask = ((1ull << (G & 63)) - 1) << (g * (G & 63));
  const int gsh = G < 64 ? g * G : 0;
  const bool skip = (__ballot(bad_arg) & gmask) != 0;  // the whole point is left untouched
  const bool live = active && !skip;
  orbm_keyframe_ref kr{{0.f, 0.f, 0.f}, 1u};
  if (live) kr = A.kfs[ob.kf];
  const bool want_desc = A.mpdesc || A.best || A.median;
  const bool keep = live && want_desc && kr.bad == 0;
  // the longest list of the wave's groups bounds the uniform loops
  uint64_t am = __ballot(active);
  if (G < 64) am |= am >> 32;
  if (G < 32) am |= am >> 16;
  if (G < 16) am |= am >> 8;
  if (G < 64) am &= (1ull << (G & 63)) - 1;
  const int nmax = am ? 64 - __clzll((long long)am) : 0;

  if (want_desc) {
    uint32_t d[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    if (keep) {
      const uint4* src = (const uint4*)(A.desc + (size_t)ob.desc_row * 32);
      const uint4 a = src[0], b = src[1];
      d[0] = a.x, d[1] = a.y, d[2] = a.z, d[3] = a.w;
      d[4] = b.x, d[5] = b.y, d[6] = b.z, d[7] = b.w;
    }
    const uint64_t keepb = __ballot(keep);
    const uint64_t gkeep = (keepb & gmask) >> gsh;  // the group's kept observations, bit = position
    const int K = __popcll(gkeep);
    int key = INT_MAX;
    if (keepb) {  // uniform
      for (int j = 0; j < nmax; ++j) {
        uint32_t b[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) b[k] = (uint32_t)group_bcast<G>((int)d[k], j);
        const int dist = mp_hamming(d, b);
        s_row[j * 64 + lane] = ((gkeep >> j) & 1) ? (uint16_t)dist : (uint16_t)0xFFFF;
      }
      // vDists[(N-1)/2] of the sorted row: the least v with need entries <= v
      const int need = ((K - 1) >> 1) + 1;
      int lo = 0, hi = 256;
      for (int step = 0; step < 9; ++step) {  // 257 values: 9 halvings; lo == hi stays put
        const int mid = (lo + hi) >> 1;
        int c = 0;
        for (int j = 0; j < nmax; ++j) c += (int)s_row[j * 64 + lane] <= mid ? 1 : 0;
        if (c >= need) hi = mid; else lo = mid + 1;
      }
      key = keep ? (lo << 16) | l : INT_MAX;
      key = group_min<G>(key);
    }
    if (has && K > 0) {
      const int wl = key & 0xffff;
      if (keep && l == wl) {
        if (A.mpdesc) {
          uint4* dst = (uint4*)(A.mpdesc + (size_t)q * 32);
          dst[0] = make_uint4(d[0], d[1], d[2], d[3]);
          dst[1] = make_uint4(d[4], d[5], d[6], d[7]);
        }
        if (A.best) A.best[p] = __popcll(gkeep & ((1ull << wl) - 1));
        if (A.median) A.median[p] = key >> 16;
      }
    } else if (has && l == 0) {
      if (A.best) A.best[p] = -1;
      if (A.median) A.median[p] = -1;
    }
  }
  if (has && skip && l == 0) atomicOr(A.err, kStatusRefreshSkipped);

  if (A.mps) {
    float pos[3] = {0.f, 0.f, 0.f}, t[3] = {0.f, 0.f, 0.f};
    if (live) {
      const float* ps = A.mps[q].pos;
      pos[0] = ps[0], pos[1] = ps[1], pos[2] = ps[2];
      mp_normal_term(pos, kr.Ow, t);
    }
    float sum[3] = {0.f, 0.f, 0.f};
    for (int j = 0; j < nmax; ++j) {
      float tj[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) tj[k] = __int_as_float(group_bcast<G>(__float_as_int(t[k]), j));
      if ((uint32_t)j < N) mp_normal_add(sum, tj);
    }
    if (live && l == 0) store_normal_depth(A, q, sum, N, pos, rf);
  }
}

__global__ __launch_bounds__(kRefThreads) void refresh_wave_kernel(RefreshArgs A) {
  __shared__ uint16_t s_rows[kRefWaves][64 * 64];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int c0 = min(A.counts[0], A.points), c1 = min(A.counts[1], A.points), c2 = min(A.counts[2], A.points),
            c3 = min(A.counts[3], A.points);
  const int i0 = (c0 + 7) >> 3, i1 = i0 + ((c1 + 3) >> 2), i2 = i1 + ((c2 + 1) >> 1), i3 = i2 + c3;
  const int* L = A.lists;
  const size_t P = (size_t)A.points;
  for (int it = blockIdx.x * kRefWaves + wave; it < i3; it += gridDim.x * kRefWaves) {
    if (it < i0) refresh_groups<8>(A, L, c0, it, s_rows[wave]);
    else if (it < i1) refresh_groups<16>(A, L + P, c1, it - i0, s_rows[wave]);
    else if (it < i2) refresh_groups<32>(A, L + 2 * P, c2, it - i1, s_rows[wave]);
    else refresh_groups<64>(A, L + 3 * P, c3, it - i2, s_rows[wave]);
  }
}

__global__ __launch_bounds__(kRefBlockThreads) void refresh_block_kernel(RefreshArgs A) {
  __shared__ uint4 s_desc[kRefLdsDesc * 2];
  __shared__ uint32_t s_tab[kRefLdsRows];
  __shared__ float s_term[kRefBlockThreads * 3];
  __shared__ unsigned long long s_key;
  __shared__ int s_kept, s_rank;
  const int tid = threadIdx.x;
  const int cnt = min(A.counts[4], A.points);
  const int* list = A.lists + (size_t)4 * A.points;
  const bool want_desc = A.mpdesc || A.best || A.median;
  for (int it = blockIdx.x; it < cnt; it += gridDim.x) {
    const int p = list[it];
    uint32_t o0;
    const uint32_t N = obs_count(A, p, &o0);
    const uint32_t q = A.ids ? A.ids[p] : (uint32_t)p;
    const orbm_observation* obs = A.obs + (size_t)o0;
    if (tid == 0) {
      s_key = ~0ull;
      s_kept = 0;
      s_rank = 0;
    }
    __syncthreads();  // also: the point before this one is done with the shared arrays
    // the ranges of the whole list first; the table of kept rows on the way
    bool bad_arg = false;
    int kept = 0;
    for (uint32_t j = tid; j < N; j += kRefBlockThreads) {
      const orbm_observation ob = obs[j];
      const bool ok = ob.kf < A.n_kfs && ob.desc_row < A.desc_rows;
      bad_arg |= !ok;
      uint32_t row = kNoRow;
      if (ok && want_desc && A.kfs[ob.kf].bad == 0) {
        row = ob.desc_row;
        ++kept;
      }
      if (j < (uint32_t)kRefLdsRows) s_tab[j] = row;
    }
    orbm_point_refkf rf{0u, 0};
    if (A.mps) {
      rf = A.ref[p];
      bad_arg |= ref_out_of_range(A, rf);
    }
    if (kept) atomicAdd(&s_kept, kept);
    if (__syncthreads_or(bad_arg ? 1 : 0)) {  // uniform: the whole point is left untouched
      if (tid == 0) {
        atomicOr(A.err, kStatusRefreshSkipped);
        if (A.best) A.best[p] = -1;
        if (A.median) A.median[p] = -1;
      }
      continue;
    }
    const int K = s_kept;
    const bool in_lds = N <= (uint32_t)kRefLdsDesc;
    // row of observation j, kNoRow when its keyframe is bad (ranges checked above)
    auto row_of = [&](uint32_t j) -> uint32_t {
      if (j < (uint32_t)kRefLdsRows) return s_tab[j];
      const orbm_observation ob = obs[j];
      return A.kfs[ob.kf].bad == 0 ? ob.desc_row : kNoRow;
    };
    auto load_desc = [&](uint32_t j, uint32_t row, uint32_t* d) {
      uint4 a, b;
      if (in_lds) {
        a = s_desc[2 * j];
        b = s_desc[2 * j + 1];
      } else {
        const uint4* src = (const uint4*)(A.desc + (size_t)row * 32);
        a = src[0];
        b = src[1];
      }
      d[0] = a.x, d[1] = a.y, d[2] = a.z, d[3] = a.w;
      d[4] = b.x, d[5] = b.y, d[6] = b.z, d[7] = b.w;
    };
    if (want_desc && K > 0) {
      if (in_lds) {
        for (uint32_t j = tid; j < N; j += kRefBlockThreads) {
          const uint32_t row = s_tab[j];
          if (row == kNoRow) continue;
          const uint4* src = (const uint4*)(A.desc + (size_t)row * 32);
          s_desc[2 * j] = src[0];
          s_desc[2 * j + 1] = src[1];
        }
        __syncthreads();
      }
      const int need = ((K - 1) >> 1) + 1;
      // a row per 16 lanes, 64 rows a round: lane `sub` of the 16 counts columns sub, sub + 16, ...
      const uint32_t sub = tid & (kRefRowLanes - 1), n_tab = min(N, (uint32_t)kRefLdsRows);
      for (uint32_t base = 0; base < N; base += kRefRows) {  // uniform rounds
        const int bound = (int)(s_key >> 32);  // best median of the rounds before; 0xFFFFFFFF (< 0) = none yet
        __syncthreads();  // every thread has read it before this round's rows lower it
        const uint32_t i = base + tid / kRefRowLanes;
        const uint32_t ri = i < N ? row_of(i) : kNoRow;
        if (ri != kNoRow && bound != 0) {  // the same in the row's 16 lanes, like every branch below
          uint32_t di[8];
          load_desc(i, ri, di);
          // entries of row i at or below v. No branch around the loads, so that the compiler keeps
          // several columns' reads in flight: a column that is not kept reads a valid address (its LDS
          // slot, or row i's descriptor) and is left out of the count.
          auto count_le = [&](int v) {
            int c = 0;
#pragma unroll 4
            for (uint32_t j = sub; j < n_tab; j += kRefRowLanes) {
              const uint32_t rj = s_tab[j];
              uint32_t dj[8];
              load_desc(j, rj == kNoRow ? ri : rj, dj);
              c += (rj != kNoRow && mp_hamming(di, dj) <= v) ? 1 : 0;
            }
            for (uint32_t j = (uint32_t)kRefLdsRows + sub; j < N; j += kRefRowLanes) {  // past the table
              const uint32_t rj = row_of(j);
              uint32_t dj[8];
              load_desc(j, rj == kNoRow ? ri : rj, dj);
              c += (rj != kNoRow && mp_hamming(di, dj) <= v) ? 1 : 0;
            }
            c += dpp_i<kDppQuad1032>(0, c);
            c += dpp_i<kDppQuad2301>(0, c);
            c += dpp_i<kDppHalfMirror>(0, c);
            c += dpp_i<kDppMirror>(0, c);
            return c;
          };
          // a row of a later round wins only with a strictly smaller median
          int lo = 0, hi = 256;
          bool can_win = true;
          if (bound > 0) {
            hi = bound - 1;
            can_win = count_le(hi) >= need;
          }
          if (can_win) {
            while (lo < hi) {
              const int mid = (lo + hi) >> 1;
              if (count_le(mid) >= need) hi = mid; else lo = mid + 1;
            }
            if (sub == 0) atomicMin(&s_key, ((unsigned long long)lo << 32) | i);
          }
        }
        __syncthreads();
      }
      const unsigned long long key = s_key;
      const uint32_t wi = min((uint32_t)key, N - 1);  // (the first kept row always enters a key: wi < N)
      int before = 0;  // kept observations ahead of the winner: its position among them
      for (uint32_t j = tid; j < wi; j += kRefBlockThreads) before += row_of(j) != kNoRow ? 1 : 0;
      if (before) atomicAdd(&s_rank, before);
      __syncthreads();
      if (tid < 2 && A.mpdesc) {
        const uint4* src = (const uint4*)(A.desc + (size_t)row_of(wi) * 32);
        ((uint4*)(A.mpdesc + (size_t)q * 32))[tid] = src[tid];
      }
      if (tid == 0) {
        if (A.best) A.best[p] = s_rank;
        if (A.median) A.median[p] = (int)(key >> 32);
      }
    } else if (tid == 0) {
      if (A.best) A.best[p] = -1;
      if (A.median) A.median[p] = -1;
    }
    if (A.mps) {
      const float* ps = A.mps[q].pos;
      const float pos[3] = {ps[0], ps[1], ps[2]};
      float sum[3] = {0.f, 0.f, 0.f};
      for (uint32_t base = 0; base < N; base += kRefBlockThreads) {
        const uint32_t j = base + tid;
        if (j < N) {
          const orbm_keyframe_ref kr = A.kfs[obs[j].kf];
          float t[3];
          mp_normal_term(pos, kr.Ow, t);
          s_term[3 * tid] = t[0];
          s_term[3 * tid + 1] = t[1];
          s_term[3 * tid + 2] = t[2];
        }
        __syncthreads();
        if (tid == 0) {
          const uint32_t m = min((uint32_t)kRefBlockThreads, N - base);
          for (uint32_t k = 0; k < m; ++k) mp_normal_add(sum, &s_term[3 * k]);
        }
        __syncthreads();
      }
      if (tid == 0) store_normal_depth(A, q, sum, N, pos, rf);
    }
  }
}

size_t refresh_ws_bytes(int points) { return 256 + (size_t)kRefreshClasses * (size_t)points * 4; }

int launch_refresh_map_points(const RefreshArgs& A, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(A.counts, 0, 32, s) != hipSuccess) return ORBX_EDEVICE;
  const int nb = (A.points + kRefThreads - 1) / kRefThreads;
  hipLaunchKernelGGL(refresh_prep_kernel, dim3(nb), dim3(kRefThreads), 0, s, A);
  // the class sizes stay on the device: both grids are sized for the worst case and stride over their lists
  // (at most one wave item per point; a point in a thousand has more than 64 observations)
  hipLaunchKernelGGL(refresh_block_kernel, dim3(std::min(A.points, 512)), dim3(kRefBlockThreads), 0, s, A);
  hipLaunchKernelGGL(refresh_wave_kernel, dim3(std::min((A.points + kRefWaves - 1) / kRefWaves, 2048)),
                     dim3(kRefThreads), 0, s, A);
  return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
}

}  // namespace orbx
