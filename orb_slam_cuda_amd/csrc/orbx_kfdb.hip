// orbx_kfdb.hip — the keyframe database on the GPU: BoW scores and the
// loop / relocalisation candidates (KeyFrameDatabase, ORBVocabulary::score).
//
// Reference: KeyFrameDatabase::add / erase / clear (src/KeyFrameDatabase.cc:76-109),
// DetectLoopCandidates (:112-233), DetectRelocalizationCandidates (:235-345)
// and the DBoW2 scorings (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-311).
// The reference keeps an inverted file (word -> list of keyframes) and walks
// the query's words; what it computes per keyframe is the number of shared
// words (mnLoopWords / mnRelocWords) and, above 0.8 of the maximum, the L1
// score. Here every keyframe's BowVector sits in a row of device memory and a
// query is one sorted-set intersection per row.
//
// Device layout (one handle): words[slot][word_pitch] u32 and
// values[slot][word_pitch] f64 in separate arrays (counting reads the words
// only), n[slot] (0 for a dead slot and for an empty BowVector).
//
// Kernels:
//   kfdb_count_kernel   grid (slot groups, queries), 4 waves per workgroup.
//                       The query's words are staged in LDS once per
//                       workgroup with a bucket table over their range
//                       (QIndex); each wave takes one slot at a time, lane i
//                       looks keyframe word i up in LDS, ballot + popcount
//                       give `common`, the first set lane of the first
//                       non-empty ballot the smallest shared word (the row
//                       ascends). One atomic maximum per wave.
//   kfdb_score_kernel   the same walk for the slots with common > minCommon
//                       (the maximum is complete at the kernel boundary). The
//                       terms fabs(vi-wi) - fabs(vi) - fabs(wi) of a 64-word
//                       chunk sit one per lane; they are added one at a time
//                       in lane (= word) order from the ballot mask, so the
//                       double rounds as L1Scoring::score's loop does.
//   kfdb_score_slots_kernel  the same scoring walk over a list of slots.
//   kfdb_add_kernel     rows of orbv_transform_batch's output into their slots.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

#include "orbx_hostutil.h"
#include "orbx_internal.h"

namespace orbx {

constexpr int kDbThreads = 256, kDbWaves = kDbThreads / 64;
constexpr int kDbMaxWords = 8192;  // the cap of orbv_transform

struct DbDev {
  const uint32_t* words;
  const double* values;
  const int* n;
  int slots, pitch;
};

// A query staged in LDS: its n ascending words w[], and over their range
// [qmin, qmax] a table of nb equal buckets, tab[b] = the index of the first
// word in bucket b or later (tab[nb] = n). A lookup reads its bucket's two
// bounds and bisects between them: with nb about n that is one or two words,
// three dependent LDS reads where a bisection of the whole query takes
// log2(n) (11 at 1500 words). Any distribution of words stays correct; a
// skewed one only bisects longer.
struct QIndex {
  const uint32_t* w;
  const int* tab;
  int n, nb;
  uint32_t qmin, qmax;
  unsigned long long mult;  // bucket(x) = ((x - qmin) * mult) >> 32 < nb for x in [qmin, qmax]
};

__device__ __forceinline__ int q_bucket(const QIndex& X, uint32_t w) {
  // (the minimum only matters for words outside [qmin, qmax]: a query that does not ascend)
  return (int)min(((unsigned long long)(w - X.qmin) * X.mult) >> 32, (unsigned long long)(X.nb - 1));
}

// LDS bytes of a staged query of up to `pitch` words, and its table's buckets
__host__ __device__ inline int q_buckets(int pitch) {
  int nb = 64;
  while (nb < pitch && nb < 4096) nb <<= 1;
  return nb;
}
__host__ inline size_t q_lds_bytes(int pitch) { return ((size_t)pitch + q_buckets(pitch) + 1) * 4; }

// workgroup-wide: stage nq words from qw and build the table (s_mem: q_lds_bytes(pitch))
__device__ __forceinline__ QIndex stage_query(uint32_t* s_mem, int pitch, const uint32_t* __restrict__ qw, int nq) {
  uint32_t* s_q = s_mem;
  int* s_tab = (int*)(s_mem + pitch);
  const int tid = threadIdx.x;
  for (int i = tid; i < nq; i += kDbThreads) s_q[i] = qw[i];
  __syncthreads();
  QIndex X;
  X.w = s_q;
  X.tab = s_tab;
  X.n = nq;
  if (nq == 0) {  // uniform over the workgroup; nothing is ever found
    X.nb = 1;
    X.qmin = 1;
    X.qmax = 0;
    X.mult = 0;
    return X;
  }
  int nb = q_buckets(pitch);
  while (nb > 64 && nb > nq) nb >>= 1;  // about one word per bucket
  X.nb = nb;
  X.qmin = s_q[0];
  X.qmax = s_q[nq - 1];
  X.mult = ((unsigned long long)nb << 32) / ((unsigned long long)(X.qmax - X.qmin) + 1ull);
  for (int i = tid; i < nq; i += kDbThreads) {
    const int b = q_bucket(X, s_q[i]), pb = i ? q_bucket(X, s_q[i - 1]) : -1;
    for (int k = pb + 1; k <= b; ++k) s_tab[k] = i;
  }
  for (int k = q_bucket(X, X.qmax) + 1 + tid; k <= nb; k += kDbThreads) s_tab[k] = nq;
  __syncthreads();
  return X;
}

// index of w among the query's words, -1 when absent
__device__ __forceinline__ int find_word(const QIndex& X, uint32_t w) {
  if (w < X.qmin || w > X.qmax) return -1;
  const int b = q_bucket(X, w);
  // (the clamps only matter for a query whose words do not ascend: no index leaves [0, n])
  int lo = min(max(X.tab[b], 0), X.n), hi = min(max(X.tab[b + 1], lo), X.n);
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (X.w[mid] < w) lo = mid + 1; else hi = mid;
  }
  return (lo < X.n && X.w[lo] == w) ? lo : -1;
}

// lane l's double, l uniform over the wave: two scalar lane reads, no LDS permute
__device__ __forceinline__ double readlane_f64(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

// one wave: words shared by the staged query and a keyframe row; *first =
// the smallest of them (0 when there is none)
__device__ __forceinline__ int wave_common(const QIndex& Xq, const uint32_t* __restrict__ kw, int nk,
                                           uint32_t* first) {
  const int lane = threadIdx.x & 63;
  int common = 0;
  uint32_t fw = 0;
  for (int base = 0; base < nk; base += 64) {
    const int i = base + lane;
    const uint32_t w = i < nk ? kw[i] : 0u;
    const bool hit = i < nk && find_word(Xq, w) >= 0;
    const unsigned long long m = __ballot(hit);
    if (m) {
      if (!common) fw = (uint32_t)__builtin_amdgcn_readlane((int)w, __ffsll((long long)m) - 1);
      common += __popcll(m);
    }
  }
  *first = fw;
  return common;
}

// one wave: L1Scoring::score(query, keyframe) (ScoringObject.cpp:23-68). The
// terms are added in ascending word order, one at a time, starting from +0.0;
// every lane carries the same sum.
__device__ __forceinline__ double wave_l1_score(const QIndex& Xq, const double* __restrict__ qv,
                                                const uint32_t* __restrict__ kw, const double* __restrict__ kv,
                                                int nk) {
  const int lane = threadIdx.x & 63;
  double score = 0;
  for (int base = 0; base < nk; base += 64) {
    const int i = base + lane;
    const int j = i < nk ? find_word(Xq, kw[i]) : -1;
    double t = 0.0;
    if (j >= 0) {
      const double vi = qv[j], wi = kv[i];
      t = fabs(vi - wi) - fabs(vi) - fabs(wi);
    }
    unsigned long long m = __ballot(j >= 0);
    while (m) {
      score += readlane_f64(t, __ffsll((long long)m) - 1);
      m &= m - 1;
    }
  }
  score = -score / 2.0;
  return score;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(kDbThreads) void kfdb_count_kernel(DbDev D, const uint32_t* __restrict__ q_words,
                                                                const int* __restrict__ q_n, int q_pitch,
                                                                const int* __restrict__ excl,
                                                                const int* __restrict__ n_excl, int excl_pitch,
                                                                orbdb_hit* __restrict__ hits,
                                                                int* __restrict__ max_common) {
  extern __shared__ uint32_t s_mem[];  // q_lds_bytes(q_pitch)
  const int q = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nq = clampi(q_n[q], 0, q_pitch);
  const QIndex Xq = stage_query(s_mem, q_pitch, q_words + (size_t)q * q_pitch, nq);
  const int ne = excl ? clampi(n_excl[q], 0, excl_pitch) : 0;
  int wmax = 0;
  for (int slot = blockIdx.x * kDbWaves + wave; slot < D.slots; slot += gridDim.x * kDbWaves) {
    const int nk = clampi(D.n[slot], 0, D.pitch);
    int common = 0;
    uint32_t fw = 0;
    if (nk > 0 && nq > 0) {
      bool ex = false;
      for (int e = lane; e < ne; e += 64) ex |= excl[(size_t)q * excl_pitch + e] == slot;
      if (!__any(ex)) common = wave_common(Xq, D.words + (size_t)slot * D.pitch, nk, &fw);
    }
    if (lane == 0) {
      orbdb_hit h;
      h.common = common;
      h.first_word = fw;
      h.score = -1.0;
      hits[(size_t)q * D.slots + slot] = h;
    }
    wmax = max(wmax, common);
  }
  if (lane == 0 && wmax > 0) atomicMax(&max_common[q], wmax);
}

__global__ __launch_bounds__(kDbThreads) void kfdb_score_kernel(DbDev D, const uint32_t* __restrict__ q_words,
                                                                const double* __restrict__ q_values,
                                                                const int* __restrict__ q_n, int q_pitch,
                                                                orbdb_hit* __restrict__ hits,
                                                                const int* __restrict__ max_common) {
  extern __shared__ uint32_t s_mem[];  // q_lds_bytes(q_pitch)
  const int q = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // int minCommonWords = maxCommonWords*0.8f  (src/KeyFrameDatabase.cc:156, :271)
  const int min_common = (int)((float)max_common[q] * 0.8f);
  orbdb_hit* hq = hits + (size_t)q * D.slots;
  // most workgroups have nothing to score: look before staging the query
  int any = 0;
  for (int k = tid;; k += kDbThreads) {
    const long long base = (long long)blockIdx.x * kDbWaves + (long long)k * gridDim.x * kDbWaves;
    if (base >= D.slots) break;
    for (int w = 0; w < kDbWaves; ++w)
      if (base + w < D.slots && hq[base + w].common > min_common) any = 1;
  }
  if (!__syncthreads_or(any)) return;
  const int nq = clampi(q_n[q], 0, q_pitch);
  const QIndex Xq = stage_query(s_mem, q_pitch, q_words + (size_t)q * q_pitch, nq);
  for (int slot = blockIdx.x * kDbWaves + wave; slot < D.slots; slot += gridDim.x * kDbWaves) {
    if (hq[slot].common <= min_common) continue;  // uniform over the wave
    const int nk = clampi(D.n[slot], 0, D.pitch);
    const double s = wave_l1_score(Xq, q_values + (size_t)q * q_pitch, D.words + (size_t)slot * D.pitch,
                                   D.values + (size_t)slot * D.pitch, nk);
    if (lane == 0) hq[slot].score = s;
  }
}

__global__ __launch_bounds__(kDbThreads) void kfdb_score_slots_kernel(DbDev D, const uint32_t* __restrict__ q_words,
                                                                      const double* __restrict__ q_values, int nq,
                                                                      const int* __restrict__ slots, int nslots,
                                                                      double* __restrict__ out) {
  extern __shared__ uint32_t s_mem[];  // q_lds_bytes(max(nq, 1))
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const QIndex Xq = stage_query(s_mem, max(nq, 1), q_words, nq);
  for (int k = blockIdx.x * kDbWaves + wave; k < nslots; k += gridDim.x * kDbWaves) {
    const int slot = slots[k];
    if (slot < 0 || slot >= D.slots) continue;  // checked on the host
    const int nk = clampi(D.n[slot], 0, D.pitch);
    const double s = wave_l1_score(Xq, q_values, D.words + (size_t)slot * D.pitch,
                                   D.values + (size_t)slot * D.pitch, nk);
    if (lane == 0) out[k] = s;
  }
}

// frame f of a BowVector batch (pitch src_pitch) into row slots[f]
__global__ __launch_bounds__(kDbThreads) void kfdb_add_kernel(const uint32_t* __restrict__ src_words,
                                                              const double* __restrict__ src_values,
                                                              const int* __restrict__ src_n, int src_pitch,
                                                              const int* __restrict__ slots, int nslots,
                                                              uint32_t* __restrict__ words,
                                                              double* __restrict__ values, int* __restrict__ n,
                                                              int pitch) {
  const int f = blockIdx.x;
  const int slot = slots[f];
  if (slot < 0 || slot >= nslots) return;
  const int m = clampi(src_n[f], 0, min(src_pitch, pitch));
  for (int i = threadIdx.x; i < m; i += kDbThreads) {
    words[(size_t)slot * pitch + i] = src_words[(size_t)f * src_pitch + i];
    values[(size_t)slot * pitch + i] = src_values[(size_t)f * src_pitch + i];
  }
  if (threadIdx.x == 0) n[slot] = m;
}

}  // namespace orbx

// ======================================================= C ABI (database)
using namespace orbx;

namespace {
thread_local ErrorSlot g_dberr;  // the orbdb_ family's last error
const char* const kScoringNames[6] = {"L1_NORM", "L2_NORM", "CHI_SQUARE", "KL", "BHATTACHARYYA", "DOT_PRODUCT"};

// the walk shared by L1, L2, chi-square, Bhattacharyya and the dot product:
// the reference's lower_bound jumps skip words that add nothing, so a plain
// merge adds the same terms in the same order
template <class Term>
double walk_shared(const uint32_t* w1, const double* v1, int n1, const uint32_t* w2, const double* v2, int n2,
                   Term term) {
  double score = 0;
  int i = 0, j = 0;
  while (i < n1 && j < n2) {
    if (w1[i] == w2[j]) {
      term(score, v1[i], v2[j]);
      ++i;
      ++j;
    } else if (w1[i] < w2[j]) {
      ++i;
    } else {
      ++j;
    }
  }
  return score;
}
}  // namespace

struct orbdb_database {
  int device = 0, max_kf = 0, pitch = 0;
  // device storage
  uint32_t* words = nullptr;
  double* values = nullptr;
  int* n = nullptr;
  // staging of the synchronous entry points: one query, its hits, lists
  uint32_t* q_words = nullptr;  // [kDbMaxWords]
  double* q_values = nullptr;   // [kDbMaxWords]
  int* q_meta = nullptr;        // {n, max_common, n_exclude}
  orbdb_hit* hits = nullptr;    // [max_kf]
  DeviceBuf ilist;              // exclude / slot lists, ints (grows)
  DeviceBuf dout;               // orbdb_score_slots results, doubles (grows)
  PinnedBuf h_slots;            // orbdb_add_batch's slot list [max_kf]
  hipStream_t stream = nullptr;
  WsOrder order;  // the storage's last user
  // host mirror
  std::vector<uint8_t> live;
  std::vector<uint32_t> seq;
  std::set<int> freed;  // dead slots below high_water
  int high_water = 0, nlive = 0;
  uint32_t next_seq = 0;
  // the last orbdb_query of each mode, as orbdb_select_candidates reads it:
  // mnLoopWords / mnRelocWords (0 = not listed), minCommonWords, mLoopScore
  std::vector<int> common[2];
  int min_common[2] = {0, 0};
  bool queried[2] = {false, false};
  std::vector<float> loop_score;
  std::vector<float> reloc_score;  // mRelocScore: survives queries (see the header)
  std::vector<orbdb_hit> h_hits;
};

static int db_reserve_ilist(orbdb_database* db, size_t ints) {
  return db->ilist.reserve(ints * 4) == hipSuccess ? ORBX_OK : g_dberr.fail(ORBX_ENOMEM, "list of %zu entries", ints);
}

static int db_take_slot(orbdb_database* db) {
  int slot;
  if (!db->freed.empty()) {
    slot = *db->freed.begin();
    db->freed.erase(db->freed.begin());
  } else {
    slot = db->high_water++;
  }
  db->live[slot] = 1;
  db->seq[slot] = db->next_seq++;
  db->reloc_score[slot] = 0.0f;
  db->loop_score[slot] = 0.0f;
  db->common[0][slot] = db->common[1][slot] = 0;
  ++db->nlive;
  return slot;
}

static DbDev db_dev(const orbdb_database* db) { return DbDev{db->words, db->values, db->n, db->max_kf, db->pitch}; }

static int db_grid(int slots, int queries) {
  const int per = (slots + kDbWaves - 1) / kDbWaves;
  return std::max(1, std::min(per, std::max(8, 2048 / std::max(1, queries))));
}

// count + score launches of `queries` queries on st (the storage order is the caller's)
static int db_launch_query(orbdb_database* db, const uint32_t* d_qw, const double* d_qv, const int* d_qn, int pitch,
                           int queries, const int* d_excl, const int* d_nexcl, int excl_pitch, orbdb_hit* d_hits,
                           int* d_max, hipStream_t st) {
  HIP_OK(g_dberr, hipMemsetAsync(d_max, 0, (size_t)queries * 4, st));
  const dim3 grid(db_grid(db->max_kf, queries), queries);
  const size_t lds = q_lds_bytes(pitch);
  hipLaunchKernelGGL(kfdb_count_kernel, grid, dim3(kDbThreads), lds, st, db_dev(db), d_qw, d_qn, pitch, d_excl,
                     d_nexcl, excl_pitch, d_hits, d_max);
  HIP_OK(g_dberr, hipGetLastError());
  hipLaunchKernelGGL(kfdb_score_kernel, grid, dim3(kDbThreads), lds, st, db_dev(db), d_qw, d_qv, d_qn, pitch, d_hits,
                     d_max);
  HIP_OK(g_dberr, hipGetLastError());
  return ORBX_OK;
}

// the synchronous entry points' query upload: words, values, n into the staging
static int db_stage_query(orbdb_database* db, const uint32_t* words, const double* values, int n, hipStream_t st) {
  if (n) {
    HIP_OK(g_dberr, hipMemcpyAsync(db->q_words, words, (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIP_OK(g_dberr, hipMemcpyAsync(db->q_values, values, (size_t)n * 8, hipMemcpyHostToDevice, st));
  }
  return ORBX_OK;
}

extern "C" {

const char* orbdb_last_error(void) { return g_dberr.msg.c_str(); }

int orbv_score(int scoring, const uint32_t* w1, const double* v1, int n1, const uint32_t* w2, const double* v2,
               int n2, double* out) {
  if (!out || n1 < 0 || n2 < 0 || (n1 && (!w1 || !v1)) || (n2 && (!w2 || !v2)))
    return g_dberr.fail(ORBX_EINVAL, "bad argument");
  double score = 0;
  switch (scoring) {
    case 0:  // L1Scoring (ScoringObject.cpp:23-68)
      score = walk_shared(w1, v1, n1, w2, v2, n2,
                          [](double& s, double vi, double wi) { s += fabs(vi - wi) - fabs(vi) - fabs(wi); });
      score = -score / 2.0;
      break;
    case 1:  // L2Scoring (:73-120)
      score = walk_shared(w1, v1, n1, w2, v2, n2, [](double& s, double vi, double wi) { s += vi * wi; });
      if (score >= 1)  // rounding errors
        score = 1.0;
      else
        score = 1.0 - sqrt(1.0 - score);
      break;
    case 2:  // ChiSquareScoring (:125-170)
      score = walk_shared(w1, v1, n1, w2, v2, n2, [](double& s, double vi, double wi) {
        if (vi + wi != 0.0) s += vi * wi / (vi + wi);
      });
      score = 2. * score;
      break;
    case 3: {  // KLScoring (:175-221): every word of v1 counts, v2 only where shared
      static const double LOG_EPS = log(DBL_EPSILON);
      int i = 0, j = 0;
      while (i < n1 && j < n2) {
        const double vi = v1[i], wi = v2[j];
        if (w1[i] == w2[j]) {
          if (vi != 0 && wi != 0) score += vi * log(vi / wi);
          ++i;
          ++j;
        } else if (w1[i] < w2[j]) {
          score += vi * (log(vi) - LOG_EPS);
          ++i;
        } else {
          ++j;  // lower_bound(v1's word): the skipped words of v2 add nothing
        }
      }
      for (; i < n1; ++i)
        if (v1[i] != 0) score += v1[i] * (log(v1[i]) - LOG_EPS);
      break;
    }
    case 4:  // BhattacharyyaScoring (:226-266)
      score = walk_shared(w1, v1, n1, w2, v2, n2, [](double& s, double vi, double wi) { s += sqrt(vi * wi); });
      break;
    case 5:  // DotProductScoring (:271-311)
      score = walk_shared(w1, v1, n1, w2, v2, n2, [](double& s, double vi, double wi) { s += vi * wi; });
      break;
    default:
      return g_dberr.fail(ORBX_EINVAL, "unknown scoring %d", scoring);
  }
  *out = score;
  return ORBX_OK;
}

int orbdb_destroy(orbdb_handle db) {
  if (!db) return ORBX_OK;
  (void)hipSetDevice(db->device);
  if (db->order.used) (void)hipEventSynchronize(db->order.ev);
  if (db->stream) (void)hipStreamSynchronize(db->stream);
  for (void* p : {(void*)db->words, (void*)db->values, (void*)db->n, (void*)db->q_words, (void*)db->q_values,
                  (void*)db->q_meta, (void*)db->hits})
    if (p) (void)hipFree(p);
  db->ilist.release();
  db->dout.release();
  db->h_slots.release();
  db->order.release();
  if (db->stream) (void)hipStreamDestroy(db->stream);
  delete db;
  return ORBX_OK;
}

int orbdb_create(int device, int max_keyframes, int word_pitch, int scoring, orbdb_handle* out) {
  if (!out || max_keyframes < 1) return g_dberr.fail(ORBX_EINVAL, "bad argument");
  if (scoring != 0) {
    if (scoring >= 1 && scoring <= 5)
      return g_dberr.fail(ORBX_EINVAL, "scoring %s (%d) is not supported on the device: only L1_NORM (0)",
                    kScoringNames[scoring], scoring);
    return g_dberr.fail(ORBX_EINVAL, "unknown scoring %d", scoring);
  }
  if (word_pitch < 1 || word_pitch > kDbMaxWords)
    return g_dberr.fail(ORBX_EINVAL, "word_pitch %d outside 1..%d", word_pitch, kDbMaxWords);
  if (hipSetDevice(device) != hipSuccess) return g_dberr.fail(ORBX_EDEVICE, "no device %d", device);
  orbdb_database* db = new orbdb_database();
  db->device = device;
  db->max_kf = max_keyframes;
  db->pitch = word_pitch;
  const size_t rows = (size_t)max_keyframes * word_pitch;
  if (hipMalloc(&db->words, rows * 4) != hipSuccess || hipMalloc(&db->values, rows * 8) != hipSuccess ||
      hipMalloc(&db->n, (size_t)max_keyframes * 4) != hipSuccess ||
      hipMalloc(&db->q_words, (size_t)kDbMaxWords * 4) != hipSuccess ||
      hipMalloc(&db->q_values, (size_t)kDbMaxWords * 8) != hipSuccess || hipMalloc(&db->q_meta, 16) != hipSuccess ||
      hipMalloc(&db->hits, (size_t)max_keyframes * sizeof(orbdb_hit)) != hipSuccess ||
      db->h_slots.alloc((size_t)max_keyframes * 4) != hipSuccess) {
    (void)hipGetLastError();
    orbdb_destroy(db);
    return g_dberr.fail(ORBX_ENOMEM, "database allocation failed (%d keyframes x %d words)", max_keyframes, word_pitch);
  }
  if (hipStreamCreateWithFlags(&db->stream, hipStreamNonBlocking) != hipSuccess ||
      hipMemsetAsync(db->n, 0, (size_t)max_keyframes * 4, db->stream) != hipSuccess ||
      hipStreamSynchronize(db->stream) != hipSuccess) {
    orbdb_destroy(db);
    return g_dberr.fail(ORBX_EDEVICE, "database set-up failed");
  }
  db->live.assign(max_keyframes, 0);
  db->seq.assign(max_keyframes, 0);
  db->common[0].assign(max_keyframes, 0);
  db->common[1].assign(max_keyframes, 0);
  db->loop_score.assign(max_keyframes, 0.0f);
  db->reloc_score.assign(max_keyframes, 0.0f);
  db->h_hits.resize(max_keyframes);
  *out = db;
  return ORBX_OK;
}

int orbdb_size(orbdb_handle db, int* live, int* slots_high_water) {
  if (!db) return g_dberr.fail(ORBX_EINVAL, "null handle");
  if (live) *live = db->nlive;
  if (slots_high_water) *slots_high_water = db->high_water;
  return ORBX_OK;
}

int orbdb_clear(orbdb_handle db) {
  if (!db) return g_dberr.fail(ORBX_EINVAL, "null handle");
  HIP_OK(g_dberr, hipSetDevice(db->device));
  hipStream_t st = db->stream;
  if (db->order.before_pending(st)) return g_dberr.fail(ORBX_EDEVICE, "stream order");
  HIP_OK(g_dberr, hipMemsetAsync(db->n, 0, (size_t)db->max_kf * 4, st));
  HIP_OK(g_dberr, hipStreamSynchronize(st));
  std::fill(db->live.begin(), db->live.end(), 0);
  db->freed.clear();
  db->high_water = db->nlive = 0;
  for (int m = 0; m < 2; ++m) {
    std::fill(db->common[m].begin(), db->common[m].end(), 0);
    db->min_common[m] = 0;
    db->queried[m] = false;
  }
  return ORBX_OK;
}

int orbdb_add(orbdb_handle db, const uint32_t* words, const double* values, int n, int* slot) {
  if (!db || !slot || n < 0 || (n && (!words || !values))) return g_dberr.fail(ORBX_EINVAL, "bad argument");
  if (n > db->pitch) return g_dberr.fail(ORBX_ECAPACITY, "BowVector of %d words > word_pitch %d", n, db->pitch);
  if (db->nlive >= db->max_kf) return g_dberr.fail(ORBX_ECAPACITY, "database full (%d keyframes)", db->max_kf);
  if (db->next_seq == UINT32_MAX) return g_dberr.fail(ORBX_ECAPACITY, "add sequence counter exhausted");
  for (int i = 1; i < n; ++i)
    if (words[i] <= words[i - 1]) return g_dberr.fail(ORBX_EINVAL, "words not ascending at %d", i);
  HIP_OK(g_dberr, hipSetDevice(db->device));
  hipStream_t st = db->stream;
  if (db->order.before_pending(st)) return g_dberr.fail(ORBX_EDEVICE, "stream order");
  const int s = db->freed.empty() ? db->high_water : *db->freed.begin();
  if (n) {
    HIP_OK(g_dberr, hipMemcpyAsync(db->words + (size_t)s * db->pitch, words, (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIP_OK(g_dberr, hipMemcpyAsync(db->values + (size_t)s * db->pitch, values, (size_t)n * 8, hipMemcpyHostToDevice, st));
  }
  HIP_OK(g_dberr, hipMemcpyAsync(db->n + s, &n, 4, hipMemcpyHostToDevice, st));
  HIP_OK(g_dberr, hipStreamSynchronize(st));
  *slot = db_take_slot(db);
  return ORBX_OK;
}

int orbdb_add_batch(orbdb_handle db, const uint32_t* d_bow_words, const double* d_bow_values, const int* d_bow_n,
                    int pitch, int frames, int* slots, void* stream) {
  if (!db || !d_bow_words || !d_bow_values || !d_bow_n || !slots || pitch < 1 || frames < 1)
    return g_dberr.fail(ORBX_EINVAL, "bad argument");
  if (frames > db->max_kf - db->nlive)
    return g_dberr.fail(ORBX_ECAPACITY, "database full (%d live + %d > %d keyframes)", db->nlive, frames, db->max_kf);
  if ((uint64_t)db->next_seq + (uint64_t)frames >= UINT32_MAX)
    return g_dberr.fail(ORBX_ECAPACITY, "add sequence counter exhausted");
  HIP_OK(g_dberr, hipSetDevice(db->device));
  hipStream_t st = (hipStream_t)stream;
  // after this wait the storage's previous user, and the pinned slot list's, has finished
  if (db->order.before(st)) return g_dberr.fail(ORBX_EDEVICE, "stream order");
  std::vector<int> hn(frames);
  HIP_OK(g_dberr, hipMemcpyAsync(hn.data(), d_bow_n, (size_t)frames * 4, hipMemcpyDeviceToHost, st));
  HIP_OK(g_dberr, hipStreamSynchronize(st));
  for (int f = 0; f < frames; ++f) {
    if (hn[f] < 0) return g_dberr.fail(ORBX_EINVAL, "frame %d: count %d", f, hn[f]);
    if (hn[f] > db->pitch || hn[f] > pitch)
      return g_dberr.fail(ORBX_ECAPACITY, "frame %d: BowVector of %d words > word_pitch %d", f, hn[f],
                    std::min(db->pitch, pitch));
  }
  if (db_reserve_ilist(db, (size_t)db->max_kf)) return ORBX_ENOMEM;
  for (int f = 0; f < frames; ++f) slots[f] = db->h_slots.as<int>()[f] = db_take_slot(db);
  HIP_OK(g_dberr, hipMemcpyAsync(db->ilist.p, db->h_slots.p, (size_t)frames * 4, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(kfdb_add_kernel, dim3(frames), dim3(kDbThreads), 0, st, d_bow_words, d_bow_values, d_bow_n, pitch,
                     db->ilist.as<int>(), db->max_kf, db->words, db->values, db->n, db->pitch);
  HIP_OK(g_dberr, hipGetLastError());
  if (db->order.after(st)) return g_dberr.fail(ORBX_EDEVICE, "stream order");
  return ORBX_OK;
}

int orbdb_erase(orbdb_handle db, int slot) {
  if (!db) return g_dberr.fail(ORBX_EINVAL, "null handle");
  if (slot < 0 || slot >= db->max_kf || !db->live[slot]) return g_dberr.fail(ORBX_EINVAL, "slot %d is not live", slot);
  HIP_OK(g_dberr, hipSetDevice(db->device));
  hipStream_t st = db->stream;
  if (db->order.before_pending(st)) return g_dberr.fail(ORBX_EDEVICE, "stream order");
  HIP_OK(g_dberr, hipMemsetAsync(db->n + slot, 0, 4, st));
  HIP_OK(g_dberr, hipStreamSynchronize(st));
  db->live[slot] = 0;
  db->freed.insert(slot);
  --db->nlive;
  db->common[0][slot] = db->common[1][slot] = 0;
  return ORBX_OK;
}

int orbdb_query_batch(orbdb_handle db, const uint32_t* d_bow_words, const double* d_bow_values, const int* d_bow_n,
                      int pitch, int queries, const int* d_exclude, const int* d_n_exclude, int exclude_pitch,
                      orbdb_hit* d_hits, int* d_max_common, void* stream) {
  if (!db || !d_bow_words || !d_bow_values || !d_bow_n || !d_hits || !d_max_common || queries < 1 || pitch < 1)
    return g_dberr.fail(ORBX_EINVAL, "bad argument");
  if (pitch > kDbMaxWords) return g_dberr.fail(ORBX_ECAPACITY, "pitch %d > %d words per query", pitch, kDbMaxWords);
  if (queries > 65535) return g_dberr.fail(ORBX_ECAPACITY, "more than 65535 queries per call");
  if (d_exclude && (!d_n_exclude || exclude_pitch < 1)) return g_dberr.fail(ORBX_EINVAL, "exclude list without counts");
  HIP_OK(g_dberr, hipSetDevice(db->device));
  hipStream_t st = (hipStream_t)stream;
  if (db->order.before(st)) return g_dberr.fail(ORBX_EDEVICE, "stream order");
  const int rc = db_launch_query(db, d_bow_words, d_bow_values, d_bow_n, pitch, queries, d_exclude, d_n_exclude,
                                 exclude_pitch, d_hits, d_max_common, st);
  if (rc) return rc;
  if (db->order.after(st)) return g_dberr.fail(ORBX_EDEVICE, "stream order");
  return ORBX_OK;
}

int orbdb_score_slots(orbdb_handle db, const uint32_t* words, const double* values, int n, const int* slots,
                      int nslots, double* out) {
  if (!db || n < 0 || nslots < 0 || (n && (!words || !values)) || (nslots && (!slots || !out)))
    return g_dberr.fail(ORBX_EINVAL, "bad argument");
  if (n > kDbMaxWords) return g_dberr.fail(ORBX_ECAPACITY, "query of %d words > %d", n, kDbMaxWords);
  for (int k = 0; k < nslots; ++k)
    if (slots[k] < 0 || slots[k] >= db->max_kf || !db->live[slots[k]])
      return g_dberr.fail(ORBX_EINVAL, "slot %d is not live", slots[k]);
  if (!nslots) return ORBX_OK;
  HIP_OK(g_dberr, hipSetDevice(db->device));
  hipStream_t st = db->stream;
  if (db->order.before_pending(st)) return g_dberr.fail(ORBX_EDEVICE, "stream order");
  int rc;
  if ((rc = db_reserve_ilist(db, (size_t)nslots))) return rc;
  if (db->dout.reserve((size_t)nslots * 8) != hipSuccess) return g_dberr.fail(ORBX_ENOMEM, "%d scores", nslots);
  if ((rc = db_stage_query(db, words, values, n, st))) return rc;
  HIP_OK(g_dberr, hipMemcpyAsync(db->ilist.p, slots, (size_t)nslots * 4, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(kfdb_score_slots_kernel, dim3(db_grid(nslots, 1)), dim3(kDbThreads), q_lds_bytes(std::max(n, 1)),
                     st, db_dev(db), db->q_words, db->q_values, n, db->ilist.as<int>(), nslots, db->dout.as<double>());
  HIP_OK(g_dberr, hipGetLastError());
  HIP_OK(g_dberr, hipMemcpyAsync(out, db->dout.p, (size_t)nslots * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(g_dberr, hipStreamSynchronize(st));
  return ORBX_OK;
}

int orbdb_query(orbdb_handle db, int mode, const uint32_t* words, const double* values, int n, const int* exclude,
                int n_exclude, float min_score, int* cand_slots, float* cand_scores, int cap, int* ncand,
                int* min_common) {
  if (!db || (mode != ORBDB_LOOP && mode != ORBDB_RELOC) || n < 0 || (n && (!words || !values)) || n_exclude < 0 ||
      (n_exclude && !exclude) || cap < 0 || (cap && (!cand_slots || !cand_scores)) || !ncand)
    return g_dberr.fail(ORBX_EINVAL, "bad argument");
  if (n > kDbMaxWords) return g_dberr.fail(ORBX_ECAPACITY, "query of %d words > %d", n, kDbMaxWords);
  HIP_OK(g_dberr, hipSetDevice(db->device));
  hipStream_t st = db->stream;
  if (db->order.before_pending(st)) return g_dberr.fail(ORBX_EDEVICE, "stream order");
  int rc;
  if (n_exclude && (rc = db_reserve_ilist(db, (size_t)n_exclude))) return rc;
  if ((rc = db_stage_query(db, words, values, n, st))) return rc;
  const int meta[3] = {n, 0, n_exclude};
  HIP_OK(g_dberr, hipMemcpyAsync(db->q_meta, meta, sizeof meta, hipMemcpyHostToDevice, st));
  if (n_exclude) HIP_OK(g_dberr, hipMemcpyAsync(db->ilist.p, exclude, (size_t)n_exclude * 4, hipMemcpyHostToDevice, st));
  const int hw = db->high_water;
  int maxc = 0;
  if (hw > 0) {
    if ((rc = db_launch_query(db, db->q_words, db->q_values, db->q_meta, std::max(n, 1), 1,
                              n_exclude ? db->ilist.as<int>() : nullptr, n_exclude ? db->q_meta + 2 : nullptr,
                              std::max(n_exclude, 1), db->hits, db->q_meta + 1, st)))
      return rc;
    HIP_OK(g_dberr, hipMemcpyAsync(db->h_hits.data(), db->hits, (size_t)hw * sizeof(orbdb_hit), hipMemcpyDeviceToHost, st));
    HIP_OK(g_dberr, hipMemcpyAsync(&maxc, db->q_meta + 1, 4, hipMemcpyDeviceToHost, st));
  }
  HIP_OK(g_dberr, hipStreamSynchronize(st));
  // everything below is the host's: lKFsSharingWords in the reference's order
  // (first encounter walking the query's words upwards, each word's list in
  // insertion order), minCommonWords, lScoreAndMatch
  const int minc = (int)(maxc * 0.8f);
  std::vector<int>& common = db->common[mode];
  std::fill(common.begin(), common.end(), 0);
  std::vector<int> sharing;
  for (int s = 0; s < hw; ++s) {
    if (!db->live[s]) continue;
    common[s] = db->h_hits[s].common;
    if (common[s] > 0) sharing.push_back(s);
  }
  std::sort(sharing.begin(), sharing.end(), [&](int a, int b) {
    const orbdb_hit &x = db->h_hits[a], &y = db->h_hits[b];
    return x.first_word != y.first_word ? x.first_word < y.first_word : db->seq[a] < db->seq[b];
  });
  db->min_common[mode] = minc;
  db->queried[mode] = true;
  int cnt = 0;
  for (int s : sharing) {
    if (common[s] <= minc) continue;
    const float si = (float)db->h_hits[s].score;
    if (mode == ORBDB_LOOP) {
      db->loop_score[s] = si;
      if (!(si >= min_score)) continue;
    } else {
      db->reloc_score[s] = si;
    }
    if (cnt < cap) {
      cand_slots[cnt] = s;
      cand_scores[cnt] = si;
    }
    ++cnt;
  }
  *ncand = cnt;
  if (min_common) *min_common = minc;
  if (cnt > cap) return g_dberr.fail(ORBX_ECAPACITY, "%d candidates > cap %d", cnt, cap);
  return ORBX_OK;
}

int orbdb_select_candidates(orbdb_handle db, int mode, const int* cand_slots, const float* cand_scores, int ncand,
                            const int* neigh, float min_score, int* out_slots, int* nout) {
  if (!db || (mode != ORBDB_LOOP && mode != ORBDB_RELOC) || ncand < 0 || !nout ||
      (ncand && (!cand_slots || !cand_scores || !neigh || !out_slots)))
    return g_dberr.fail(ORBX_EINVAL, "bad argument");
  if (!db->queried[mode]) return g_dberr.fail(ORBX_EINVAL, "no orbdb_query of mode %d on this handle yet", mode);
  for (int i = 0; i < ncand; ++i) {
    if (cand_slots[i] < 0 || cand_slots[i] >= db->max_kf) return g_dberr.fail(ORBX_EINVAL, "candidate slot %d", cand_slots[i]);
    for (int k = 0; k < 10; ++k)
      if (neigh[i * 10 + k] < -1 || neigh[i * 10 + k] >= db->max_kf)
        return g_dberr.fail(ORBX_EINVAL, "neighbour slot %d", neigh[i * 10 + k]);
  }
  const std::vector<int>& common = db->common[mode];
  const int minc = db->min_common[mode];
  const std::vector<float>& kscore = mode == ORBDB_LOOP ? db->loop_score : db->reloc_score;
  // lAccScoreAndMatch (src/KeyFrameDatabase.cc:180-209, :294-323)
  std::vector<float> acc(ncand);
  std::vector<int> best(ncand);
  float bestAccScore = mode == ORBDB_LOOP ? min_score : 0;
  for (int i = 0; i < ncand; ++i) {
    float bestScore = cand_scores[i];
    float accScore = cand_scores[i];
    int pBestKF = cand_slots[i];
    for (int k = 0; k < 10; ++k) {
      const int s2 = neigh[i * 10 + k];
      if (s2 < 0) continue;
      // loop: mnLoopQuery == mnId && mnLoopWords > minCommonWords; reloc: mnRelocQuery == mnId
      const bool counts = mode == ORBDB_LOOP ? (common[s2] > 0 && common[s2] > minc) : common[s2] > 0;
      if (!counts) continue;
      accScore += kscore[s2];
      if (kscore[s2] > bestScore) {
        pBestKF = s2;
        bestScore = kscore[s2];
      }
    }
    acc[i] = accScore;
    best[i] = pBestKF;
    if (accScore > bestAccScore) bestAccScore = accScore;
  }
  const float minScoreToRetain = 0.75f * bestAccScore;
  std::set<int> added;
  int cnt = 0;
  for (int i = 0; i < ncand; ++i)
    if (acc[i] > minScoreToRetain && added.insert(best[i]).second) out_slots[cnt++] = best[i];
  *nout = cnt;
  return ORBX_OK;
}

}  // extern "C"
