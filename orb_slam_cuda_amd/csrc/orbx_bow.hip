// orbx_bow.hip — SearchByBoW (KF-F src/ORBmatcher.cc:159-288, KF-KF :522-655) for gfx950.
//
// The reference resolves matches greedily in a fixed order (matched features
// drop out of SearchByBoW :205-210). The kernels keep that order exactly:
// candidate lists and all 256-bit distances are computed in parallel; the
// per-node greedy loops run as parallel rounds to a fixed point (with a
// sequential pass as the fallback), or one wavefront per node with the
// best/second reduction across lanes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "orbx_device.cuh"
#include "orbx_internal.h"
#include "orbx_wave.cuh"

namespace orbx {

constexpr int kHistoLength = 30;
constexpr int kThLow = 50;

__device__ __forceinline__ int hamming256(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
  return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
         __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// ------------------------------------------------------------ wave helpers
__device__ __forceinline__ int wave_min(int v) { return wave_min_dpp(v); }
__device__ __forceinline__ int wave_sum_i(int v) { return wave_sum_dpp(v); }

// best / second of the multiset of valid distances, first position wins ties
// (the sequential "if(d<best){second=best;best=d;idx=i} else if(d<second)"
// loop computes exactly this). Returns wave-uniform values.
struct Top2 {
  int best, pos, second;
};
__device__ __forceinline__ Top2 wave_top2(bool valid, int dist, int pos) {
  const int BIG = INT_MAX;
  const int d = valid ? dist : BIG;
  const int b = wave_min(d);
  const uint64_t eq = __ballot(valid && d == b);
  Top2 r;
  r.best = b;
  if (eq == 0) {
    r.pos = -1;
    r.second = BIG;
    return r;
  }
  const int first_lane = __ffsll((long long)eq) - 1;
  r.pos = __builtin_amdgcn_readlane(pos, first_lane);
  if (__popcll(eq) >= 2) {
    r.second = b;
  } else {
    const int lane = threadIdx.x & 63;
    r.second = wave_min(lane == first_lane ? BIG : d);
  }
  return r;
}

// ------------------------------------------------------------ SearchByBoW
// Grid: pairs x G workgroups; workgroup g of a pair takes the pair's A nodes
// [g*nnA/G, (g+1)*nnA/G). Shared vocabulary nodes are independent: DBoW2 puts
// every feature in exactly one node, so a node's B features are touched by
// that node's A features only, the taken bits of a workgroup's nodes are
// private to it, and only the rotation histogram and the match count are the
// pair's (global atomics: hist[0..29] bins, hist[30] count;
// search_bow_finalize_kernel applies ComputeThreeMaxima after). An accepted
// match goes to the pair's row record, bin << 16 | matched index (16 bits: the
// entry points bound both frames' counts by 65536), in a
// scratch that is all -1 between calls (finalize writes `out` from it and
// resets it and the histogram, so no fill launches precede the kernel).
//
// Inside a node the reference is greedy (src/ORBmatcher.cc:186-262): A rows in
// node order, each taking the best untaken B row. The workgroup splits that
// into
//  (1) a data-parallel pass, one lane per A row: the node's B rows (staged in
//      LDS in node order, static filter applied) are scanned once and the
//      row's K smallest keys (distance << 16 | position in the node) kept;
//  (2) the greedy pass, one lane per node, in A order: the first two untaken
//      keys of the row's list ARE the reference's bestDist1/bestIdx and
//      bestDist2 (keys order ties by node position, as the strict `<` of
//      :211-226 does), so the pass is a few register operations per row; a
//      row whose list has fewer than two untaken keys left while it had more
//      than K candidates rescans its node (rare).
// A workgroup whose node range does not fit the LDS tables falls back to the
// per-wave greedy (a wave per node, the best/second reduced across lanes).

#ifndef ORBX_BOW_GROUPS
#define ORBX_BOW_GROUPS 24
#endif
#ifndef ORBX_BOW_BALANCE
#define ORBX_BOW_BALANCE 1  // node ranges of equal estimated work (0: equal node counts)
#endif
// Workgroup shape (C3 + BoW bench, 64 KITTI pairs): alone, 8 ranges of <= 768
// rows on 512 threads are fastest (34.9 us; 256 threads 40.8 us), but in the
// pipelined step those 71 KB-LDS workgroups wait for CUs the extraction
// kernels hold (0.24 ms of event time per batch); 24 ranges of <= 256 rows
// (~26 KB) on 256 threads fit beside them: 0.135 ms, 106 k -> 118 k frames/s.
// Ranges past the caps take the per-wave fallback.
constexpr int kBowGroups = ORBX_BOW_GROUPS;  // workgroups per pair (node ranges)
#ifndef ORBX_BOW_THREADS
#define ORBX_BOW_THREADS 256
#endif
constexpr int kBowThreads = ORBX_BOW_THREADS;
constexpr int kBowK = 8;         // smallest keys kept per A row
#ifndef ORBX_BOW_CAP
#define ORBX_BOW_CAP 256
#endif
constexpr int kBowCapB = ORBX_BOW_CAP;      // B rows staged per workgroup
constexpr int kBowCapA = ORBX_BOW_CAP;      // A rows per workgroup
constexpr int kBowCapN = ORBX_BOW_CAP / 3;  // nodes per workgroup
constexpr int kBowMaxB = 256;    // fallback: B features of a node held in registers (4 chunks of 64 lanes)
constexpr uint32_t kBowNone = 0xFFFFFFFFu;
#ifndef ORBX_BOW_ROWCOST
#define ORBX_BOW_ROWCOST 64
#endif
constexpr int kBowRowCost = ORBX_BOW_ROWCOST;  // a row's fixed cost in candidate scans (range balance)
#ifndef ORBX_BOW_ROUNDS
#define ORBX_BOW_ROUNDS 16
#endif
constexpr int kBowRounds = ORBX_BOW_ROUNDS;  // default greedy fixed-point rounds before the sequential pass
// (ORBX_BOW_ROUNDS=<n> in the environment overrides it per call; 0: the sequential pass only; results are the same)

struct BowTables {  // the two-pass layout
  uint32_t bdesc[kBowCapB][8];  // the range's B rows, node by node
  int bidx[kBowCapB];           // their feature index, -1 = not a candidate (KF-KF without a good MapPoint)
  uint4 top[kBowCapA][2];       // per A row its kBowK = 8 smallest keys, ascending (kBowNone = empty)
  int nv[kBowCapA];             // candidates the row saw, -1 = row skipped (no good MapPoint);
                                // after the greedy pass: the matched staged position, or -1
  int match[kBowCapA];          // greedy rounds: the row's current choice (staged position, -1 = none)
  int claim[kBowCapB];          // greedy rounds: first row (in range order) choosing the position
  int rq[kBowCapA];             // the row's node: B rows [rq & 0xFFFF, rq >> 16)
  int boff[kBowCapN + 1];       // node j's B rows at [boff[j], boff[j+1])
  int aoff[kBowCapN + 1];       // node j's A rows at [aoff[j], aoff[j+1]) (relative to the range)
  int bsrc[kBowCapN];           // node j's B CSR start
  int sstart[kBowCapN + 1];     // phase (1) lane slots: the k-th node in slot order starts at sstart[k]
  int snode[kBowCapN];          // ... and is node snode[k]
  int rescan[kBowCapA];         // greedy rounds: rows whose list ran out, rescanned by whole waves
  uint32_t taken[kBowCapB / 32];  // by staged position
};
struct BowFallback {  // the per-wave layout
  uint32_t taken[2048];  // one bit per B feature
  uint32_t adesc[kBowThreads / 64][64][8];
  int aidx[kBowThreads / 64][64];
  int bidx[kBowThreads / 64][kBowMaxB];
};
union BowLds {
  BowTables t;
  BowFallback f;
};

template <int NT>
__global__ __launch_bounds__(NT) void search_bow_kernel(BowSide A, BowSide B, float nnratio, int check_ori,
                                                        int kf_vs_kf, int G, int max_rounds, long long out_pitch,
                                                        int* __restrict__ rec_all, int* __restrict__ hist_all,
                                                        int* __restrict__ err, int* dbg) {
  constexpr int kWaves = NT / 64;
  const unsigned long long t_begin = __builtin_amdgcn_s_memtime();
  auto stamp = [&](int k, int v) {  // diagnostics only (ORBX_BOW_PROF=1): per-workgroup phase cycles
    if (dbg && threadIdx.x == 0) dbg[blockIdx.x * 8 + k] = v < 0 ? (int)(__builtin_amdgcn_s_memtime() - t_begin) : v;
  };
  __shared__ BowLds S;
  __shared__ int s_scan[kWaves + 1];
  __shared__ int s_hist[32];
  __shared__ int s_queue;
  const int p = blockIdx.x / G, g = blockIdx.x - p * G;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nnA = A.nn[p], nnB = B.nn[p];
  const int* offA0 = A.off + p * (A.node_pitch + 1);
#if ORBX_BOW_BALANCE
  // The pair's nodes split into G contiguous ranges of equal estimated work
  // rather than equal node counts (node sizes are skewed: a few nodes hold
  // hundreds of features, and a range's time follows its largest nodes). A
  // node of n A rows costs about n x (n + kBowRowCost): the candidate scans
  // plus each row's fixed part (its node lookup and two dependent global
  // loads, worth ~64 candidates; with n x (n + 4) the first range of a pair
  // took ~540 rows, two passes of the workgroup's lanes). B's node sizes
  // follow A's in consecutive frames, so no B lookup is needed here: node j
  // goes to workgroup floor(excl_j x G / total), non-decreasing in j.
  int k0, k1;
  {
    // n clamped at 4096 in the estimate (it only drives the balance): with at
    // most 65536 rows per frame every sum below then stays far inside 32 bits
    auto work = [&](int j) {
      const int n = min(offA0[j + 1] - offA0[j], 4096);
      return n * (n + kBowRowCost);
    };
    int tot = 0;
    for (int j = tid; j < nnA; j += NT) tot += work(j);
    tot = wave_sum_dpp(tot);
    if (lane == 0) s_scan[wv] = tot;
    __syncthreads();
    long long W = 0;
    for (int w = 0; w < kWaves; ++w) W += s_scan[w];
    __syncthreads();
    int lt = 0, le = 0;
    long long carry = 0;
    for (int j0 = 0; j0 < nnA; j0 += NT) {
      const int j = j0 + tid;
      const int wj = j < nnA ? work(j) : 0;
      const int incl = wave_incl_scan_dpp(wj);
      if (lane == 63) s_scan[wv] = incl;
      __syncthreads();
      long long before = carry;
      for (int w = 0; w < wv; ++w) before += s_scan[w];
      const long long excl = before + incl - wj;
      if (j < nnA) {
        const int owner = W > 0 ? (int)min((long long)(G - 1), excl * G / W) : 0;
        lt += owner < g;
        le += owner <= g;
      }
      for (int w = 0; w < kWaves; ++w) carry += s_scan[w];
      __syncthreads();
    }
    lt = wave_sum_dpp(lt);
    le = wave_sum_dpp(le);
    if (lane == 0) {
      s_scan[wv] = lt;
      s_hist[wv] = le;
    }
    __syncthreads();
    k0 = k1 = 0;
    for (int w = 0; w < kWaves; ++w) {
      k0 += s_scan[w];
      k1 += s_hist[w];
    }
    __syncthreads();
  }
  const int nk = k1 - k0;
#else
  const int k0 = (int)((long long)g * nnA / G), k1 = (int)((long long)(g + 1) * nnA / G), nk = k1 - k0;
#endif
  const uint8_t* descA = A.desc + p * A.kp_pitch * 32;
  const uint8_t* descB = B.desc + p * B.kp_pitch * 32;
  const float* angA = A.angle + p * A.kp_pitch * A.angle_stride;
  const float* angB = B.angle + p * B.kp_pitch * B.angle_stride;
  const uint8_t* mpA = A.mp ? A.mp + p * A.kp_pitch : nullptr;
  const uint8_t* mpB = B.mp ? B.mp + p * B.kp_pitch : nullptr;
  const uint32_t* nodesA = A.nodes + p * A.node_pitch;
  const uint32_t* nodesB = B.nodes + p * B.node_pitch;
  const int* offA = A.off + p * (A.node_pitch + 1);
  const int* offB = B.off + p * (B.node_pitch + 1);
  const int* idxA = A.idx + p * A.node_pitch;
  const int* idxB = B.idx + p * B.node_pitch;
  int* rec = rec_all + p * out_pitch;
  int* hist = hist_all + p * 32;
  if (nk <= 0) return;
  // feature indices come from device CSR arrays the host cannot check: an
  // index outside [0, min(n, kp_pitch)) is not a candidate and sets status
  // bit 32 (it would address the next pair's rows or past the buffers)
  // (a side's pitch is 0 for the single-pair host entry; out rows are indexed by
  // the A feature for KF-KF and by the B feature for KF-F)
  auto extent = [&](const BowSide& X, bool out_side) {
    long long e = X.n[p];
    if (X.kp_pitch > 0) e = min(e, X.kp_pitch);
    if (out_side) e = min(e, out_pitch);
    return (int)e;
  };
  const int nAp = extent(A, kf_vs_kf), nBp = extent(B, !kf_vs_kf);
  if (tid == 0 && g == 0 && (A.n[p] > nAp || B.n[p] > nBp)) atomicOr(err, 32);
  auto in_a = [&](int i) {
    const bool ok = (unsigned)i < (unsigned)nAp;
    if (!ok) atomicOr(err, 32);
    return ok;
  };
  auto in_b = [&](int i) {
    const bool ok = (unsigned)i < (unsigned)nBp;
    if (!ok) atomicOr(err, 32);
    return ok;
  };
  const float factor = 1.0f / kHistoLength;
  // an accepted match: output, the pair's count and rotation histogram
  auto accept = [&](int idx1, int bestIdx2, int* h) {
    int bin = 0;
    atomicAdd(&h[30], 1);
    if (check_ori) {
      float rot = __fsub_rn(angA[(long long)idx1 * A.angle_stride], angB[(long long)bestIdx2 * B.angle_stride]);
      if (rot < 0.0f) rot = __fadd_rn(rot, 360.0f);
      bin = (int)roundf(__fmul_rn(rot, factor));
      if (bin == kHistoLength) bin = 0;
      atomicAdd(&h[bin], 1);
    }
    if (kf_vs_kf) rec[idx1] = bin << 16 | bestIdx2;
    else rec[bestIdx2] = bin << 16 | idx1;
  };
  // lower_bound of a node id in B's node list (the lock-step walk of :180-264
  // meets exactly the shared ids); -1 when B lacks it
  auto find_b = [&](uint32_t id) {
    int lo = 0, hi = nnB;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (nodesB[mid] < id) lo = mid + 1;
      else hi = mid;
    }
    return (lo < nnB && nodesB[lo] == id) ? lo : -1;
  };
  const int a_base = offA[k0], na = offA[k1] - a_base;

  // ---- node table: B node per A node, staged B offsets (block scan of counts)
  bool fits = nk <= kBowCapN && na <= kBowCapA;
  if (fits) {
    // B's node list in LDS (the claim table is free until the greedy rounds):
    // the per-node lower_bound then waits on LDS, not on ~7 dependent global loads
    const bool nodes_lds = nnB <= kBowCapB;
    uint32_t* const snb = (uint32_t*)S.t.claim;
    if (nodes_lds)
      for (int i = tid; i < nnB; i += NT) snb[i] = nodesB[i];
    __syncthreads();
    auto find_b_lds = [&](uint32_t id) {
      int lo = 0, hi = nnB;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (snb[mid] < id) lo = mid + 1;
        else hi = mid;
      }
      return (lo < nnB && snb[lo] == id) ? lo : -1;
    };
    int carry = 0;
    for (int j0 = 0; j0 < nk; j0 += NT) {
      const int j = j0 + tid;
      int cnt = 0, src = 0;
      if (j < nk) {
        const uint32_t id = nodesA[k0 + j];
        const int kb = nodes_lds ? find_b_lds(id) : find_b(id);
        if (kb >= 0) {
          src = offB[kb];
          cnt = offB[kb + 1] - src;
        }
        S.t.bsrc[j] = src;
        S.t.aoff[j + 1] = offA[k0 + j + 1] - a_base;
      }
      const int incl = wave_incl_scan_dpp(cnt);
      if (lane == 63) s_scan[wv] = incl;
      __syncthreads();
      int before = carry;
      for (int w = 0; w < wv; ++w) before += s_scan[w];
      if (j < nk) S.t.boff[j + 1] = before + incl;
      int tot = 0;
      for (int w = 0; w < kWaves; ++w) tot += s_scan[w];
      carry += tot;
      __syncthreads();
    }
    if (tid == 0) S.t.boff[0] = S.t.aoff[0] = 0;
    fits = carry <= kBowCapB;  // uniform
  }
  stamp(1, -1);
  if (fits) {
    __syncthreads();
    const int nb = S.t.boff[nk];
    for (int i = tid; i < kBowCapB / 32; i += NT) S.t.taken[i] = 0;
    // the range's A feature indices (phase (1) then needs one dependent global load, not two)
    for (int i = tid; i < na; i += NT) S.t.match[i] = idxA[a_base + i];
    // ---- stage the range's B rows in node order (static filter: KF-KF needs a good MapPoint)
    for (int i = tid; i < nb; i += NT) {
      int lo = 0, hi = nk;  // node j with boff[j] <= i < boff[j+1]
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (S.t.boff[mid] <= i) lo = mid;
        else hi = mid;
      }
      int i2 = idxB[S.t.bsrc[lo] + (i - S.t.boff[lo])];
      bool ok = in_b(i2);
      if (!ok) i2 = 0;
      ok = ok && (!kf_vs_kf || !mpB || mpB[i2] != 0);
      const uint4* d2 = (const uint4*)(descB + (long long)i2 * 32);
      const uint4 v0 = d2[0], v1 = d2[1];
      *(uint4*)&S.t.bdesc[i][0] = v0;
      *(uint4*)&S.t.bdesc[i][4] = v1;
      S.t.bidx[i] = ok ? i2 : -1;
    }
    __syncthreads();
    stamp(2, -1);
    // ---- (1) per A row, its kBowK smallest keys over the node's candidates.
    // A row of a node with nb B rows gets L = 1, 2, 4 or 8 adjacent lanes
    // (nb > 48, 96, 192), each scanning every L-th candidate; the L sorted
    // lists then merge by xor shuffles. Without the split one lane walks all
    // nb candidates and the largest node sets the workgroup's time. Lane
    // slots: nodes ordered by L descending (node order within), each row's L
    // slots contiguous and L-aligned (every block before has a multiple of
    // L slots).
    auto lanes_of = [](int nbn) { return nbn > 192 ? 8 : nbn > 96 ? 4 : nbn > 48 ? 2 : 1; };
    int nslots = 0;
    {
      int base = 0, rank0 = 0;  // slots and nodes of the classes before
      for (int Lc = 8; Lc >= 1; Lc >>= 1) {
        int carry = 0;
        for (int j0 = 0; j0 < nk; j0 += NT) {
          const int j = j0 + tid;
          const bool mine = j < nk && lanes_of(S.t.boff[j + 1] - S.t.boff[j]) == Lc;
          const int sz = mine ? (S.t.aoff[j + 1] - S.t.aoff[j]) * Lc : 0;
          const uint64_t bm = __ballot(mine);
          const int incl = wave_incl_scan_dpp(sz);
          if (lane == 63) s_scan[wv] = incl;
          if (lane == 0) s_hist[wv] = __popcll(bm);
          __syncthreads();
          int before = carry, rb = rank0;
          for (int w = 0; w < wv; ++w) {
            before += s_scan[w];
            rb += s_hist[w];
          }
          if (mine) {
            const int k = rb + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bm, 0u));
            S.t.sstart[k] = base + before + incl - sz;
            S.t.snode[k] = j;
          }
          for (int w = 0; w < kWaves; ++w) {
            carry += s_scan[w];
            rank0 += s_hist[w];
          }
          __syncthreads();
        }
        base += carry;
      }
      nslots = base;
      if (tid == 0) S.t.sstart[nk] = nslots;
    }
    __syncthreads();
    for (int s0 = 0; s0 < nslots; s0 += NT) {  // uniform trip count: the shuffles below see every lane
      const int sl = s0 + tid;
      const bool act = sl < nslots;
      int lo = 0, hi = nk;  // slot-order node k with sstart[k] <= sl < sstart[k+1]
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (S.t.sstart[mid] <= min(sl, nslots - 1)) lo = mid;
        else hi = mid;
      }
      const int j = min(max(S.t.snode[lo], 0), nk - 1);  // (every rank is written; the clamp guards the indexing)
      const int q0 = S.t.boff[j], q1 = S.t.boff[j + 1];
      const int L = lanes_of(q1 - q0), rel = min(sl, nslots - 1) - S.t.sstart[lo];
      const int ia = S.t.aoff[j] + rel / L, sub = rel & (L - 1);
      const int i1 = S.t.match[ia];  // idxA[a_base + ia], staged
      uint32_t t0 = kBowNone, t1 = kBowNone, t2 = kBowNone, t3 = kBowNone;
      uint32_t t4 = kBowNone, t5 = kBowNone, t6 = kBowNone, t7 = kBowNone;
      int nv = -1;
      if (act && in_a(i1) && (!mpA || mpA[i1])) {  // (:191-197)
        nv = 0;
        const uint4* d1 = (const uint4*)(descA + (long long)i1 * 32);
        const uint4 a0 = d1[0], a1 = d1[1];
        auto insert = [&](uint32_t key) {  // into the ascending t0..t7
          uint32_t m;
          m = min(t0, key); key = max(t0, key); t0 = m;
          m = min(t1, key); key = max(t1, key); t1 = m;
          m = min(t2, key); key = max(t2, key); t2 = m;
          m = min(t3, key); key = max(t3, key); t3 = m;
          m = min(t4, key); key = max(t4, key); t4 = m;
          m = min(t5, key); key = max(t5, key); t5 = m;
          m = min(t6, key); key = max(t6, key); t6 = m;
          t7 = min(t7, key);
        };
        // two candidates per step: their LDS reads are in flight together
        int q = q0 + sub;
        for (; q + L < q1; q += 2 * L) {
          const int okA = S.t.bidx[q], okB = S.t.bidx[q + L];
          const uint4 b0 = *(const uint4*)&S.t.bdesc[q][0], b1 = *(const uint4*)&S.t.bdesc[q][4];
          const uint4 c0 = *(const uint4*)&S.t.bdesc[q + L][0], c1 = *(const uint4*)&S.t.bdesc[q + L][4];
          const uint32_t kA = ((uint32_t)hamming256(a0, a1, b0, b1) << 16) | (uint32_t)(q - q0);
          const uint32_t kB = ((uint32_t)hamming256(a0, a1, c0, c1) << 16) | (uint32_t)(q + L - q0);
          if (okA >= 0) insert(kA), ++nv;
          if (okB >= 0) insert(kB), ++nv;
        }
        if (q < q1 && S.t.bidx[q] >= 0) {
          ++nv;
          insert(((uint32_t)hamming256(a0, a1, *(const uint4*)&S.t.bdesc[q][0], *(const uint4*)&S.t.bdesc[q][4]) << 16) |
                 (uint32_t)(q - q0));
        }
      }
      // merge the row's L lists: with the partner's list reversed, the
      // elementwise minima are the 8 smallest of the union as a bitonic
      // sequence, sorted by three half-cleaner stages (both partners end with
      // the same list; keys are unique, so the merge is exact)
      for (int st = 1; st < 8; st <<= 1) {
        if (!__ballot(act && L > st)) break;  // wave-uniform
        const uint32_t u0 = __shfl_xor(t0, st), u1 = __shfl_xor(t1, st), u2 = __shfl_xor(t2, st);
        const uint32_t u3 = __shfl_xor(t3, st), u4 = __shfl_xor(t4, st), u5 = __shfl_xor(t5, st);
        const uint32_t u6 = __shfl_xor(t6, st), u7 = __shfl_xor(t7, st);
        const int unv = __shfl_xor(nv, st);
        if (L > st) {
          uint32_t m[8] = {min(t0, u7), min(t1, u6), min(t2, u5), min(t3, u4),
                           min(t4, u3), min(t5, u2), min(t6, u1), min(t7, u0)};
#pragma unroll
          for (int h = 4; h >= 1; h >>= 1)
#pragma unroll
            for (int i = 0; i < 8; ++i)
              if ((i & h) == 0) {
                const uint32_t x = m[i], y = m[i + h];
                m[i] = min(x, y);
                m[i + h] = max(x, y);
              }
          t0 = m[0]; t1 = m[1]; t2 = m[2]; t3 = m[3]; t4 = m[4]; t5 = m[5]; t6 = m[6]; t7 = m[7];
          nv = (nv < 0 || unv < 0) ? -1 : nv + unv;  // the row's lanes agree on validity
        }
      }
      if (act && sub == 0) {
        S.t.top[ia][0] = make_uint4(t0, t1, t2, t3);
        S.t.top[ia][1] = make_uint4(t4, t5, t6, t7);
        S.t.nv[ia] = nv;
        S.t.rq[ia] = q0 | (q1 << 16);
      }
    }
    __syncthreads();
    stamp(3, -1);
    // ---- (2) the greedy pass as a fixed point (Jacobi rounds). Row i's
    // decision depends only on which of its candidates earlier rows of its
    // node took; every round recomputes all rows in parallel from the previous
    // round's choices (a position counts as taken for row i when a row before
    // i chose it: claim = the first such row). Row 1 of a node is right in
    // round 0 and row i by round i - 1, and a round without changes is the
    // unique fixed point = the sequential result, so the rounds stop there.
    // Rows with a decision changing after max_rounds rounds fall back to the
    // sequential pass below.
    auto decide = [&](int ia, auto&& taken, bool defer = false) -> int {  // staged position, -1, or -2 = deferred rescan
      const int nv = S.t.nv[ia];
      if (nv < 0) return -1;
      const int rq = S.t.rq[ia], q0 = rq & 0xFFFF, q1 = rq >> 16;
      if (q0 == q1) return -1;
      const uint4 tA = S.t.top[ia][0], tB = S.t.top[ia][1];
      const uint32_t keys[kBowK] = {tA.x, tA.y, tA.z, tA.w, tB.x, tB.y, tB.z, tB.w};
      int d1 = 256, d2 = 256, p1 = -1, found = 0;
#pragma unroll
      for (int k = 0; k < kBowK; ++k) {
        const uint32_t key = keys[k];
        if (key == kBowNone || found == 2 || taken(ia, q0 + (int)(key & 0xFFFF))) continue;
        if (found == 0) {
          d1 = (int)(key >> 16);
          p1 = q0 + (int)(key & 0xFFFF);
        } else {
          d2 = (int)(key >> 16);
        }
        ++found;
      }
      if (found < 2 && nv > kBowK) {
        if (defer) return -2;
        // the list ran out under taken rows: rescan the node (strict < of :211-226)
        const int i1 = idxA[a_base + ia];
        const uint4* da = (const uint4*)(descA + (long long)i1 * 32);
        const uint4 a0 = da[0], a1 = da[1];
        d1 = 256;
        d2 = 256;
        p1 = -1;
        for (int q = q0; q < q1; ++q) {
          if (S.t.bidx[q] < 0 || taken(ia, q)) continue;
          const int dist = hamming256(a0, a1, *(const uint4*)&S.t.bdesc[q][0], *(const uint4*)&S.t.bdesc[q][4]);
          if (dist < d1) {
            d2 = d1;
            d1 = dist;
            p1 = q;
          } else if (dist < d2) {
            d2 = dist;
          }
        }
      }
      // d1 = 256 never passes; with d1 < 256 the reference's bestIdx is set
      const bool pass = kf_vs_kf ? (d1 < kThLow) : (d1 <= kThLow);
      return (pass && (float)d1 < __fmul_rn(nnratio, (float)min(d2, 256))) ? p1 : -1;
    };
    const int nb_ = S.t.boff[nk];
    for (int ia = tid; ia < na; ia += NT) S.t.match[ia] = decide(ia, [](int, int) { return false; });
    bool settled = false;
    int rounds = 0;
    for (int round = 0; round < max_rounds && !settled; ++round) {
      ++rounds;
      for (int q = tid; q < nb_; q += NT) S.t.claim[q] = INT_MAX;
      if (tid == 0) s_queue = 0;
      __syncthreads();
      for (int ia = tid; ia < na; ia += NT) {
        const int q = S.t.match[ia];
        if (q >= 0) atomicMin(&S.t.claim[q], ia);
      }
      __syncthreads();
      int changed = 0;
      for (int ia = tid; ia < na; ia += NT) {
        const int m = decide(ia, [&](int row, int q) { return S.t.claim[q] < row; }, true);
        if (m == -2) {
          S.t.rescan[atomicAdd(&s_queue, 1)] = ia;
        } else if (m != S.t.match[ia]) {
          S.t.match[ia] = m;
          changed = 1;
        }
      }
      __syncthreads();
      // rows whose list ran out: a wave per row, lanes over the node's
      // candidates (taken = claimed by an earlier row), two wave minima
      const int nq = s_queue;
      for (int qi = wv; qi < nq; qi += kWaves) {
        const int ia = S.t.rescan[qi];
        const int rq = S.t.rq[ia], q0 = rq & 0xFFFF, q1 = rq >> 16;
        const int i1 = idxA[a_base + ia];
        const uint4* da = (const uint4*)(descA + (long long)i1 * 32);
        const uint4 a0 = da[0], a1 = da[1];
        uint32_t b1k = 0x7FFFFFFFu, b2k = 0x7FFFFFFFu;
        for (int q = q0 + lane; q < q1; q += 64) {
          if (S.t.bidx[q] < 0 || S.t.claim[q] < ia) continue;
          const uint32_t k = ((uint32_t)hamming256(a0, a1, *(const uint4*)&S.t.bdesc[q][0],
                                                   *(const uint4*)&S.t.bdesc[q][4]) << 16) | (uint32_t)(q - q0);
          b2k = min(b2k, max(b1k, k));
          b1k = min(b1k, k);
        }
        const uint32_t m1 = (uint32_t)wave_min((int)b1k);  // keys < 2^25
        const uint32_t m2 = (uint32_t)wave_min((int)(b1k == m1 ? b2k : b1k));
        const int d1 = m1 == 0x7FFFFFFFu ? 256 : (int)(m1 >> 16);
        const int d2 = m2 == 0x7FFFFFFFu ? 256 : (int)(m2 >> 16);
        const bool pass = kf_vs_kf ? (d1 < kThLow) : (d1 <= kThLow);
        const int m = (pass && (float)d1 < __fmul_rn(nnratio, (float)min(d2, 256))) ? q0 + (int)(m1 & 0xFFFF) : -1;
        if (lane == 0 && m != S.t.match[ia]) {
          S.t.match[ia] = m;
          changed = 1;
        }
      }
      settled = !__syncthreads_or(changed);
    }
    if (settled) {
      for (int ia = tid; ia < na; ia += NT) S.t.nv[ia] = S.t.match[ia];
    } else {
      // sequential: a wave per node, A rows in node order. The node's taken
      // set is wave-uniform: four 64-bit masks (positions < 256 in the node;
      // larger nodes use the LDS bits for the rest). Lane k < 8 checks key k
      // of the row's list, a ballot gives the first two untaken keys, and the
      // next row's key is read while the current one is decided. A row whose
      // list ran out (fewer than two untaken keys left while it saw more than
      // kBowK candidates) rescans its node: lanes over the candidates, two
      // wave minima.
      for (int j = wv; j < nk; j += kWaves) {
        const int q0 = S.t.boff[j], q1 = S.t.boff[j + 1];
        const int r0 = S.t.aoff[j], r1 = S.t.aoff[j + 1];
        if (q0 == q1) {  // node absent from B (or empty)
          for (int ia = r0 + lane; ia < r1; ia += 64) S.t.nv[ia] = -1;
          continue;
        }
        uint64_t tk[4] = {0, 0, 0, 0};  // taken node positions 0..255 (uniform)
        auto is_taken = [&](int r) -> bool {  // r: position in the node (per lane)
          if (r < 256) {
            const uint64_t m = r < 128 ? (r < 64 ? tk[0] : tk[1]) : (r < 192 ? tk[2] : tk[3]);
            return (m >> (r & 63)) & 1ull;
          }
          const int q = q0 + r;
          return (S.t.taken[q >> 5] >> (q & 31)) & 1u;
        };
        uint32_t key_n = lane < kBowK ? ((const uint32_t*)S.t.top[r0])[lane] : kBowNone;
        int nv_n = S.t.nv[r0];
        for (int ia = r0; ia < r1; ++ia) {
          const uint32_t key = key_n;
          const int nv = nv_n;  // uniform
          if (ia + 1 < r1) {
            key_n = lane < kBowK ? ((const uint32_t*)S.t.top[ia + 1])[lane] : kBowNone;
            nv_n = S.t.nv[ia + 1];
          }
          int res = -1;
          if (nv >= 0) {
            const bool ok = key != kBowNone && !is_taken((int)(key & 0xFFFF));
            const uint64_t bm = __ballot(ok);
            int d1 = 256, d2 = 256, r1st = -1;
            if (bm) {
              const uint32_t k1 = (uint32_t)__builtin_amdgcn_readlane((int)key, __ffsll((long long)bm) - 1);
              d1 = (int)(k1 >> 16);
              r1st = (int)(k1 & 0xFFFF);
              const uint64_t bm2 = bm & (bm - 1);
              if (bm2) d2 = (int)((uint32_t)__builtin_amdgcn_readlane((int)key, __ffsll((long long)bm2) - 1) >> 16);
            }
            if (__popcll(bm) < 2 && nv > kBowK) {
              // the list ran out under taken rows: rescan the node (strict < of :211-226)
              const int i1 = idxA[a_base + ia];
              const uint4* da = (const uint4*)(descA + (long long)i1 * 32);
              const uint4 a0 = da[0], a1 = da[1];
              uint32_t b1k = 0x7FFFFFFFu, b2k = 0x7FFFFFFFu;  // the lane's two smallest keys
              for (int r = lane; r < q1 - q0; r += 64) {
                if (S.t.bidx[q0 + r] < 0 || is_taken(r)) continue;
                const uint32_t k = ((uint32_t)hamming256(a0, a1, *(const uint4*)&S.t.bdesc[q0 + r][0],
                                                         *(const uint4*)&S.t.bdesc[q0 + r][4]) << 16) | (uint32_t)r;
                b2k = min(b2k, max(b1k, k));
                b1k = min(b1k, k);
              }
              // keys < 2^25: the signed DPP minimum orders them
              const uint32_t m1 = (uint32_t)wave_min((int)b1k);
              const uint32_t m2 = (uint32_t)wave_min((int)(b1k == m1 ? b2k : b1k));
              d1 = m1 == 0x7FFFFFFFu ? 256 : (int)(m1 >> 16);
              d2 = m2 == 0x7FFFFFFFu ? 256 : (int)(m2 >> 16);
              r1st = m1 == 0x7FFFFFFFu ? -1 : (int)(m1 & 0xFFFF);
            }
            // d1 = 256 never passes; with d1 < 256 the reference's bestIdx is set
            const bool pass = kf_vs_kf ? (d1 < kThLow) : (d1 <= kThLow);
            if (pass && (float)d1 < __fmul_rn(nnratio, (float)min(d2, 256))) {
              res = q0 + r1st;
              if (r1st < 256) {
                const uint64_t bit = 1ull << (r1st & 63);
                tk[0] |= r1st < 64 ? bit : 0ull;
                tk[1] |= (r1st >> 6) == 1 ? bit : 0ull;
                tk[2] |= (r1st >> 6) == 2 ? bit : 0ull;
                tk[3] |= (r1st >> 6) == 3 ? bit : 0ull;
              } else if (lane == 0) {
                atomicOr(&S.t.taken[res >> 5], 1u << (res & 31));  // words shared with other waves' nodes
              }
            }
          }
          if (lane == 0) S.t.nv[ia] = res;
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
        }
      }
    }
    __syncthreads();
    stamp(4, -1);
    // ---- the accepted matches: outputs, then count and rotation histogram
    // summed in LDS first (one global atomic per bin per workgroup)
    if (tid < 32) s_hist[tid] = 0;
    __syncthreads();
    for (int ia = tid; ia < na; ia += NT) {
      const int q = S.t.nv[ia];
      if (q >= 0) accept(idxA[a_base + ia], S.t.bidx[q], s_hist);
    }
    __syncthreads();
    if (tid < 32 && s_hist[tid]) atomicAdd(&hist[tid], s_hist[tid]);
    if (dbg) {
      __syncthreads();
      stamp(0, -1);
      stamp(5, nk + 1000 * (settled ? rounds : 99));  // diagnostics: nodes + 1000 x rounds (99: sequential)
      stamp(6, na);
      stamp(7, S.t.boff[nk]);
    }
    return;
  }

  // ---- fallback: a wave per node through a queue, best/second reduced across lanes
  stamp(5, -nk);
  __syncthreads();
  volatile uint32_t* s_taken = S.f.taken;
  for (int i = tid; i < 2048; i += NT) S.f.taken[i] = 0;
  if (tid == 0) s_queue = 0;
  __syncthreads();
  for (;;) {
    int qi = 0;
    if (lane == 0) qi = atomicAdd(&s_queue, 1);
    const int ka = k0 + __builtin_amdgcn_readfirstlane(qi);
    if (ka >= k1) break;
    const int lo = find_b(nodesA[ka]);
    if (lo < 0) continue;
    const int b0 = offB[lo], b1 = offB[lo + 1];
    const int a0i = offA[ka], a1i = offA[ka + 1];
    const int nbn = b1 - b0;
    if (nbn <= kBowMaxB) {
      // the node's B descriptors in registers (lane l holds positions l, l+64,
      // ...), A descriptors staged 64 at a time in LDS and read back as
      // broadcasts: the greedy loop over A waits on no global load
      constexpr int kC = kBowMaxB / 64;
      uint4 q0[kC], q1[kC];
      int bidx[kC];
      bool bok[kC];
#pragma unroll
      for (int c = 0; c < kC; ++c) {
        const int pos = c * 64 + lane;
        bidx[c] = -1;
        bok[c] = false;
        q0[c] = q1[c] = make_uint4(0, 0, 0, 0);
        if (pos < nbn) {
          int i2 = idxB[b0 + pos];
          if (!in_b(i2)) i2 = -1;
          bidx[c] = i2;
          bok[c] = i2 >= 0 && (!kf_vs_kf || !mpB || mpB[i2] != 0);
          if (i2 < 0) i2 = 0;
          const uint4* d2 = (const uint4*)(descB + (long long)i2 * 32);
          q0[c] = d2[0];
          q1[c] = d2[1];
          S.f.bidx[wv][pos] = bidx[c];
        }
      }
      for (int ac = a0i; ac < a1i; ac += 64) {
        const int nan_ = min(64, a1i - ac);
        __builtin_amdgcn_wave_barrier();
        if (lane < nan_) {
          int i1 = idxA[ac + lane];
          const bool in = in_a(i1);
          if (!in) i1 = 0;
          const bool ok = in && (!mpA || mpA[i1]);
          const uint4* d1 = (const uint4*)(descA + (long long)i1 * 32);
          const uint4 v0 = d1[0], v1 = d1[1];
          uint32_t* w = S.f.adesc[wv][lane];
          w[0] = v0.x; w[1] = v0.y; w[2] = v0.z; w[3] = v0.w;
          w[4] = v1.x; w[5] = v1.y; w[6] = v1.z; w[7] = v1.w;
          S.f.aidx[wv][lane] = ok ? i1 : -1;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (int i = 0; i < nan_; ++i) {
          const int idx1 = S.f.aidx[wv][i];
          if (idx1 < 0) continue;  // (:191-197) uniform
          const uint32_t* w = S.f.adesc[wv][i];
          const uint4 a0 = make_uint4(w[0], w[1], w[2], w[3]), a1 = make_uint4(w[4], w[5], w[6], w[7]);
          // per lane the two smallest (distance << 16 | position) keys over its
          // chunks, then the wave's: position order = the node vector's order,
          // so equal distances resolve to the earlier candidate as in :211-226
          uint32_t k1 = 0x7FFFFFFFu, k2 = 0x7FFFFFFFu;
#pragma unroll
          for (int c = 0; c < kC; ++c) {
            if (c * 64 >= nbn) break;  // uniform
            const int i2 = bidx[c];
            const bool valid = i2 >= 0 && bok[c] && !((s_taken[i2 >> 5] >> (i2 & 31)) & 1u);
            if (valid) {
              const uint32_t key = ((uint32_t)hamming256(a0, a1, q0[c], q1[c]) << 16) | (uint32_t)(c * 64 + lane);
              k2 = min(k2, max(k1, key));
              k1 = min(k1, key);
            }
          }
          const uint32_t m1 = (uint32_t)wave_min((int)k1);
          const uint32_t m2 = (uint32_t)wave_min((int)(k1 == m1 ? k2 : k1));
          // merged with the initial best = second = 256 of the reference loop
          const int d1 = m1 == 0x7FFFFFFFu ? 256 : min((int)(m1 >> 16), 256);
          const int d2 = m2 == 0x7FFFFFFFu ? 256 : min((int)(m2 >> 16), 256);
          const bool pass = kf_vs_kf ? (d1 < kThLow) : (d1 <= kThLow);
          if (pass && (float)d1 < __fmul_rn(nnratio, (float)d2)) {
            if (lane == 0) {
              const int i2 = S.f.bidx[wv][m1 & 0xFFFF];
              atomicOr((unsigned*)&s_taken[i2 >> 5], 1u << (i2 & 31));
              accept(idx1, i2, hist);
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
          }
        }
      }
      continue;
    }
    // very large nodes: candidates streamed from global memory 64 at a time
    for (int pa = a0i; pa < a1i; ++pa) {
      const int idx1 = idxA[pa];
      if (!in_a(idx1) || (mpA && !mpA[idx1])) continue;
      const uint4* d1 = (const uint4*)(descA + (long long)idx1 * 32);
      const uint4 a0 = d1[0], a1 = d1[1];
      Top2 acc{256, -1, 256};
      for (int q0 = b0; q0 < b1; q0 += 64) {
        const int q = q0 + lane;
        bool valid = false;
        int dist = 0, idx2 = -1;
        if (q < b1 && in_b(idxB[q])) {
          idx2 = idxB[q];
          const bool taken = (s_taken[idx2 >> 5] >> (idx2 & 31)) & 1u;
          valid = !taken && (!kf_vs_kf || !mpB || mpB[idx2] != 0);
          if (valid) {
            const uint4* d2 = (const uint4*)(descB + (long long)idx2 * 32);
            dist = hamming256(a0, a1, d2[0], d2[1]);
          }
        }
        const Top2 t = wave_top2(valid, dist, idx2);
        if (t.best < acc.best) {
          acc.second = min(acc.best, t.second);
          acc.best = t.best;
          acc.pos = t.pos;
        } else {
          acc.second = min(acc.second, t.best);
        }
      }
      const bool pass = kf_vs_kf ? (acc.best < kThLow) : (acc.best <= kThLow);
      if (pass && (float)acc.best < __fmul_rn(nnratio, (float)acc.second)) {
        if (lane == 0) {
          atomicOr((unsigned*)&s_taken[acc.pos >> 5], 1u << (acc.pos & 31));
          accept(idx1, acc.pos, hist);
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
      }
    }
  }
}

// Rotation consistency (src/ORBmatcher.cc:267-285, ComputeThreeMaxima :1601-1642)
// and the final count, one workgroup per pair: `out` rows from the row
// records (-1 for rows without a match, past the pair's extent, or whose bin
// is not one of the three maxima), then the records and the histogram go back
// to -1 / 0 for the next call.
__global__ __launch_bounds__(256) void search_bow_finalize_kernel(int check_ori, int* __restrict__ out_all,
                                                                  long long out_pitch, int* __restrict__ rec_all,
                                                                  int* __restrict__ hist_all, int* __restrict__ nmatches) {
  __shared__ int s_var[4];
  const int p = blockIdx.x, tid = threadIdx.x;
  int* hist = hist_all + p * 32;
  int count = 0;
  if (tid == 0) {
    count = hist[30];
    int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
    if (check_ori) {
      for (int i = 0; i < kHistoLength; i++) {
        const int s = hist[i];
        if (s > max1) {
          max3 = max2; max2 = max1; max1 = s;
          ind3 = ind2; ind2 = ind1; ind1 = i;
        } else if (s > max2) {
          max3 = max2; max2 = s;
          ind3 = ind2; ind2 = i;
        } else if (s > max3) {
          max3 = s;
          ind3 = i;
        }
      }
      if (max2 < __fmul_rn(0.1f, (float)max1)) {
        ind2 = -1;
        ind3 = -1;
      } else if (max3 < __fmul_rn(0.1f, (float)max1)) {
        ind3 = -1;
      }
    }
    s_var[0] = ind1;
    s_var[1] = ind2;
    s_var[2] = ind3;
    s_var[3] = 0;
  }
  __syncthreads();
  if (tid < 32) hist[tid] = 0;
  const int ind1 = s_var[0], ind2 = s_var[1], ind3 = s_var[2];
  int* out = out_all + p * out_pitch;
  int* rec = rec_all + p * out_pitch;
  int removed = 0;
  for (long long i = tid; i < out_pitch; i += 256) {
    const int v = rec[i];
    int o = -1;
    if (v >= 0) {
      rec[i] = -1;
      const int b = v >> 16;
      if (!check_ori || b == ind1 || b == ind2 || b == ind3) o = v & 0xFFFF;
      else ++removed;
    }
    out[i] = o;
  }
  if (removed) atomicAdd(&s_var[3], removed);
  __syncthreads();
  if (tid == 0) nmatches[p] = count - s_var[3];
}

// rec_scratch / hist_scratch: the row records (all -1) and histograms (all 0)
// between calls when *clean; otherwise their first rec_ints / hist_ints (the
// whole buffers, so that a later call with more pairs or a wider pitch also
// finds them clean) are filled first. *clean is false from the search launch
// until its finalize is queued.
int launch_search_bow(const BowSide& A, const BowSide& B, int pairs, float nnratio, int check_ori, int kf_vs_kf,
                      int* out, long long out_pitch, int* nmatches, int* rec_scratch, size_t rec_ints,
                      int* hist_scratch, size_t hist_ints, bool* clean, int* err, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if ((size_t)pairs * out_pitch > rec_ints || (size_t)pairs * 32 > hist_ints) return ORBX_ECAPACITY;
  if (!*clean && (hipMemsetAsync(rec_scratch, 0xFF, rec_ints * 4, s) != hipSuccess ||
                  hipMemsetAsync(hist_scratch, 0, hist_ints * 4, s) != hipSuccess))
    return ORBX_EDEVICE;
  *clean = false;
  static int* dbg = nullptr;  // diagnostics only: per-workgroup phase cycles (ORBX_BOW_PROF=1)
  static const bool prof = getenv("ORBX_BOW_PROF") && getenv("ORBX_BOW_PROF")[0] == '1';
  const int nwg = pairs * kBowGroups;
  const char* rs = getenv("ORBX_BOW_ROUNDS");  // read per call (tests force the sequential pass with 0)
  const int rounds = rs ? std::max(0, std::min(atoi(rs), 1 << 16)) : kBowRounds;
  if (prof && !dbg) (void)hipMalloc(&dbg, (size_t)65536 * 32);
  if (prof) (void)hipMemsetAsync(dbg, 0, (size_t)nwg * 32, s);
  hipLaunchKernelGGL(search_bow_kernel<kBowThreads>, dim3(nwg), dim3(kBowThreads), 0, s, A, B, nnratio,
                     check_ori, kf_vs_kf, kBowGroups, rounds, out_pitch, rec_scratch, hist_scratch, err,
                     prof ? dbg : nullptr);
  if (prof) {
    std::vector<int> h((size_t)nwg * 8);
    (void)hipStreamSynchronize(s);
    (void)hipMemcpy(h.data(), dbg, h.size() * 4, hipMemcpyDeviceToHost);
    double t[8] = {0}, mx[8] = {0};
    int nfb = 0, nseq = 0, rsum = 0;
    for (int w = 0; w < nwg; ++w) {
      if (h[w * 8 + 5] < 0) ++nfb;
      if (h[w * 8 + 5] >= 0) {  // nodes + 1000 x rounds
        const int rd = h[w * 8 + 5] / 1000;
        nseq += rd == 99;
        rsum += rd == 99 ? 0 : rd;
        h[w * 8 + 5] %= 1000;
      }
      for (int k = 0; k < 8; ++k) t[k] += h[w * 8 + k], mx[k] = std::max(mx[k], (double)h[w * 8 + k]);
    }
    fprintf(stderr, "bow: %d WGs sequential greedy, the others settled in %.1f rounds on average\n", nseq,
            nwg > nseq ? (double)rsum / (nwg - nseq) : 0.0);
    fprintf(stderr, "bow: %d WGs (%d fallback); avg/max cycles at: table %.0f/%.0f staged %.0f/%.0f top %.0f/%.0f greedy %.0f/%.0f end %.0f/%.0f; avg nodes %.1f rows A %.1f B %.1f\n",
            nwg, nfb, t[1] / nwg, mx[1], t[2] / nwg, mx[2], t[3] / nwg, mx[3], t[4] / nwg, mx[4], t[0] / nwg, mx[0], t[5] / nwg, t[6] / nwg, t[7] / nwg);
    // the slowest workgroups: phase ends, nodes, A rows, B rows, and the pair's group index
    std::vector<int> order(nwg);
    for (int w = 0; w < nwg; ++w) order[w] = w;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return h[a * 8] > h[b * 8]; });
    for (int r = 0; r < std::min(nwg, 8); ++r) {
      const int w = order[r];
      fprintf(stderr, "bow slow[%d]: wg %d (pair %d group %d) table %d staged %d top %d greedy %d end %d; nodes %d A %d B %d\n",
              r, w, w / kBowGroups, w % kBowGroups, h[w * 8 + 1], h[w * 8 + 2], h[w * 8 + 3], h[w * 8 + 4], h[w * 8], h[w * 8 + 5],
              h[w * 8 + 6], h[w * 8 + 7]);
    }
  }
  hipLaunchKernelGGL(search_bow_finalize_kernel, dim3(pairs), dim3(256), 0, s, check_ori, out, out_pitch, rec_scratch,
                     hist_scratch, nmatches);
  if (hipGetLastError() != hipSuccess) return ORBX_EDEVICE;
  *clean = true;
  return ORBX_OK;
}

}  // namespace orbx
