// orbx_matcher.hip — the orbm_* C ABI: the matcher handle, the stream order of
// its workspaces, the batch (device-array) entry points and the synchronous
// host-array entry points staged through the handle's arena. The kernels are in
// orbx_top2.hip, orbx_bow.hip, orbx_init.hip, orbx_stereo.hip,
// orbx_project.hip, orbx_project_pose.hip, orbx_frustum.hip,
// orbx_triangulate.hip, orbx_mappoint.hip, orbx_poseopt.hip, orbx_sim3.hip, orbx_optsim3.hip,
// orbx_newpoints.hip and orbx_initializer.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "orbx_hostutil.h"
#include "orbx_initializer.cuh"
#include "orbx_internal.h"
#include "orbx_mappoint.cuh"
#include "orbx_newpoints.cuh"
#include "orbx_optsim3.cuh"
#include "orbx_posemath.cuh"
#include "orbx_poseopt.cuh"
#include "orbx_sim3.cuh"

using namespace orbx;

namespace {
thread_local ErrorSlot g_merr;  // the orbm_ family's last error
}  // namespace

extern "C" const char* orbm_last_error(void) { return g_merr.msg.c_str(); }

struct orbx_matcher {
  int device = 0, max_pairs = 0, max_kps = 0;
  int sortn = 1;
  DeviceBuf init_ws;  // SearchForInitialization: per-pair records, keys (init_ws_bytes_per_pair)
  size_t init_ws_pair = 0;  // bytes per pair
  DeviceBuf host_init_ws;  // orbm_search_for_initialization's own (its pitch is the call's; grows)
  DeviceBuf err;
  DeviceBuf stereo_sad;    // [max_pairs][max_kps] SAD per left keypoint (-1 = none)
  DeviceBuf bow_hist;      // [max_pairs][32] SearchByBoW rotation histogram (+ match count), 0 between calls
  DeviceBuf bow_rec;       // [max_pairs][max_kps] SearchByBoW row records, -1 between calls
  bool bow_clean = false;  // bow_hist / bow_rec hold their between-calls values
  // grown on demand, each after a wait for the workspace's last user (ws)
  DeviceBuf pose_picks;  // pose-projection picks per point (frames x mp_pitch)
  DeviceBuf view_ws;     // SearchLocalPoints: isInFrustum records, then the points in view compacted
  DeviceBuf refresh_ws;  // RefreshMapPoints: class counters and work lists
  DeviceBuf po_ws;       // PoseOptimization: edge records of frame pitches above kPoLdsEdges
  DeviceBuf sim3_ws;     // Sim3Solver: the hypotheses' records, gathered lists of pitches above kSim3LdsCorr
  DeviceBuf sim3_tab;    // Sim3Solver: mRansacMaxIts per count, of the parameters below
  std::vector<int> sim3_tab_host;  // its source (the upload reads it)
  double sim3_prob = 0;
  int sim3_min_inliers = -1, sim3_max_iterations = -1;
  DeviceBuf initz_ws;    // Initializer: headers, gathered lists, hypotheses, flags, cosine keys
  DeviceBuf os3_ws;      // OptimizeSim3: edge pair records and bitmaps of pair pitches above kOs3LdsCorr
  hipStream_t stream = nullptr;
  WsOrder ws;  // stream order of cand / stereo_sad / pose_picks / view_ws / refresh_ws / po_ws / sim3_* / initz_ws / os3_ws / bow_* across caller streams
  // streams of the launches that may set `err` (top-2, SearchByBoW, SearchLocalPoints, RefreshMapPoints, PoseOptimization, Sim3Solver, Initializer, OptimizeSim3)
  StreamMarks errm;
  // staging for the synchronous entry points
  DeviceBuf stage;
  PinnedBuf h_stage;  // orbm_compute_stereo_matches_last
};

// the growth of the two stagings, with the messages their own hipMalloc lines gave
static int stage_reserve(orbx_matcher* m, size_t bytes) {
  const hipError_t e = m->stage.reserve(bytes);
  return e == hipSuccess ? ORBX_OK
                         : g_merr.fail(ORBX_EDEVICE, "hipMalloc(&m->stage, bytes): %s", hipGetErrorString(e));
}
static int host_stage_reserve(orbx_matcher* m, size_t bytes) {
  const hipError_t e = m->h_stage.reserve(bytes);
  return e == hipSuccess ? ORBX_OK
                         : g_merr.fail(ORBX_EDEVICE, "hipHostMalloc(&m->h_stage, bytes, hipHostMallocDefault): %s",
                                       hipGetErrorString(e));
}

// the handle's own stream (status polls and the synchronous entry points), created on first use
static int matcher_stream(orbx_matcher* m, hipStream_t* st) {
  if (!m->stream) HIP_OK(g_merr, hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
  *st = m->stream;
  return ORBX_OK;
}

namespace {
// A typed range of the handle's arena: a device pointer once Stage::reserve has run.
template <class T>
struct Slot {
  void* const* base;
  size_t off;
  operator T*() const { return (T*)((uint8_t*)*base + off); }
};

// One synchronous (host-array) call's use of the handle's arena and stream:
// carve the slots, reserve, upload, run the batch entry on `st`, download,
// finish (the call's one wait). Leaving the scope any other way with work
// enqueued waits for the stream first: the next call on the handle reuses the
// arena, and the caller's arrays must not be in use after the return.
//
// Every slot starts at a multiple of 256 bytes from the arena's base (a
// hipMalloc allocation, aligned at least as much). The kernels need 16: they
// read descriptors as uint4 pairs (orbx_init, orbx_stereo, orbx_projgrid.cuh
// for the two projection kernels, orbx_triangulate, orbx_bow). orbx_kp records
// (28 bytes apart) and the map point, pose and pair records are read field by
// field, everything else is 1- and 4-byte arrays. 256 also keeps two slots
// out of one cache line.
struct Stage {
  orbx_matcher* m;
  hipStream_t st = nullptr;
  size_t used = 0;
  bool pending = false;  // work enqueued on st that finish() has not waited for
  explicit Stage(orbx_matcher* m_) : m(m_) {}
  ~Stage() {
    if (pending) (void)hipStreamSynchronize(st);
  }
  template <class T>
  Slot<T> slot(size_t count) {
    const Slot<T> s{&m->stage.p, used};
    used += (count * sizeof(T) + 255) & ~(size_t)255;
    return s;
  }
  int open() { return matcher_stream(m, &st); }
  int reserve() {
    const int rc = stage_reserve(m, used);
    return rc ? rc : open();
  }
  // one copy per call; an absent array (count 0 or src null) is skipped
  int copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    if (!bytes || !src) return ORBX_OK;
    pending = true;
    HIP_OK(g_merr, hipMemcpyAsync(dst, src, bytes, kind, st));
    return ORBX_OK;
  }
  template <class T>
  int up(Slot<T> dst, const T* src, size_t count) {
    return copy(dst, src, count * sizeof(T), hipMemcpyHostToDevice);
  }
  template <class T>
  int down(T* dst, Slot<T> src, size_t count) {
    return copy(dst, src, count * sizeof(T), hipMemcpyDeviceToHost);
  }
  int finish() {
    pending = false;
    HIP_OK(g_merr, hipStreamSynchronize(st));
    return ORBX_OK;
  }
};
}  // namespace

// minX .. invH of InitParams / ProjParams / PoseParams from the frame's image
// bounds: mfGridElementWidthInv / HeightInv = FRAME_GRID_COLS / (mnMaxX - mnMinX),
// FRAME_GRID_ROWS / (mnMaxY - mnMinY) (src/Frame.cc:154-155)
template <class Params>
static void set_grid_bounds(Params& P, const orbm_grid_bounds& b) {
  P.minX = b.min_x;
  P.maxX = b.max_x;
  P.minY = b.min_y;
  P.maxY = b.max_y;
  P.invW = static_cast<float>(kGridCols) / static_cast<float>(b.max_x - b.min_x);
  P.invH = static_cast<float>(kGridRows) / static_cast<float>(b.max_y - b.min_y);
}

static int search_init_launch(orbx_matcher* m, const orbx_kp* d_kp1, const uint8_t* d_desc1, const int* d_n1,
                              const orbx_kp* d_kp2, const uint8_t* d_desc2, const int* d_n2, int kp_pitch, int pairs,
                              orbm_grid_bounds b, float* d_prev_xy, int window, float nnratio, int check_ori,
                              int* d_matches12, int* d_nmatches, void* stream, int* ws) {
  InitParams P{};
  set_grid_bounds(P, b);  // F2's grid
  P.r = (float)window;
  P.nnratio = nnratio;
  P.check_ori = check_ori;
  P.kp_pitch = kp_pitch;
  if (m->ws.before((hipStream_t)stream)) return g_merr.fail(ORBX_EDEVICE, "stream wait on the workspace failed");
  const int rc = launch_search_init(P, d_kp1, d_desc1, d_n1, d_kp2, d_desc2, d_n2, d_prev_xy, ws, d_matches12,
                                    d_nmatches, pairs, stream);
  if (!rc && m->ws.after((hipStream_t)stream)) return g_merr.fail(ORBX_EDEVICE, "event record failed");
  if (rc == ORBX_ECAPACITY)
    return g_merr.fail(ORBX_ECAPACITY, "kp_pitch %d too large for SearchForInitialization at nnratio %g (<= %d)", kp_pitch,
                 (double)nnratio, search_init_max_pitch(nnratio));
  if (rc) return g_merr.fail(ORBX_EDEVICE, "search_init launch: %s", hipGetErrorString(hipGetLastError()));
  return ORBX_OK;
}

extern "C" {

int orbm_create(int device, int max_pairs, int max_kps, orbm_handle* out) {
  if (!out || max_pairs < 1 || max_kps < 1) return g_merr.fail(ORBX_EINVAL, "bad argument");
  if (max_kps > 65535) return g_merr.fail(ORBX_EINVAL, "max_kps must be <= 65535");
  HIP_OK(g_merr, hipSetDevice(device));
  orbx_matcher* m = new orbx_matcher();
  m->device = device;
  m->max_pairs = max_pairs;
  m->max_kps = max_kps;
  while (m->sortn < max_kps) m->sortn <<= 1;
  m->init_ws_pair = init_ws_bytes_per_pair(max_kps);
  if (m->init_ws.alloc((size_t)max_pairs * m->init_ws_pair) != hipSuccess || m->err.alloc(16) != hipSuccess ||
      m->stereo_sad.alloc((size_t)max_pairs * max_kps * 4) != hipSuccess ||
      m->bow_hist.alloc((size_t)max_pairs * 32 * 4) != hipSuccess ||
      m->bow_rec.alloc((size_t)max_pairs * max_kps * 4) != hipSuccess) {
    orbm_destroy(m);
    return g_merr.fail(ORBX_ENOMEM, "matcher workspace allocation failed");
  }
  (void)hipMemset(m->err.as<int>(), 0, 16);
  *out = m;
  return ORBX_OK;
}

int orbm_destroy(orbm_handle m) {
  if (!m) return ORBX_OK;
  (void)hipSetDevice(m->device);
  if (m->stream) (void)hipStreamSynchronize(m->stream);
  if (m->ws.ev) (void)hipEventSynchronize(m->ws.ev);
  m->ws.release();
  (void)m->errm.wait();
  m->errm.release();
  // the buffers go before the stream, not with the handle after it
  for (DeviceBuf* b : {&m->init_ws, &m->host_init_ws, &m->err, &m->stereo_sad, &m->bow_hist, &m->bow_rec, &m->pose_picks,
                       &m->view_ws, &m->refresh_ws, &m->po_ws, &m->sim3_ws, &m->sim3_tab, &m->initz_ws, &m->os3_ws, &m->stage})
    b->release();
  m->h_stage.release();
  if (m->stream) (void)hipStreamDestroy(m->stream);
  delete m;
  return ORBX_OK;
}

int orbm_get_status(orbm_handle m, int reset, int* status) {
  if (!m || !status) return g_merr.fail(ORBX_EINVAL, "null argument");
  HIP_OK(g_merr, hipSetDevice(m->device));
  // the kernels that set the word ran on caller streams: wait for those
  // launches (their stream marks), not for the device
  if (m->errm.wait()) return g_merr.fail(ORBX_EDEVICE, "status: event wait failed");
  hipStream_t st;
  int rc;
  if ((rc = matcher_stream(m, &st))) return rc;
  int e = 0;
  HIP_OK(g_merr, hipMemcpyAsync(&e, m->err.as<int>(), 4, hipMemcpyDeviceToHost, st));
  HIP_OK(g_merr, hipStreamSynchronize(st));
  if (reset && e) {
    HIP_OK(g_merr, hipMemsetAsync(m->err.as<int>(), 0, 16, st));
    HIP_OK(g_merr, hipStreamSynchronize(st));
  }
  *status = e;
  return ORBX_OK;
}

int orbm_descriptor_distance(const uint8_t* a, const uint8_t* b) {
  int d = 0;
  for (int i = 0; i < 32; ++i) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
  return d;
}

int orbm_hamming_top2(orbm_handle m, const uint8_t* d_A, size_t a_pitch, const int* d_nA, int a_cap,
                      const uint8_t* d_B, size_t b_pitch, const int* d_nB, int pairs, int* d_best_idx, int* d_best,
                      int* d_second, void* stream) {
  if (!m || !d_A || !d_B || !d_nA || !d_nB || pairs < 1) return g_merr.fail(ORBX_EINVAL, "bad argument");
  if ((a_pitch | b_pitch) & 15) return g_merr.fail(ORBX_EINVAL, "pitches must be multiples of 16 bytes");
  HIP_OK(g_merr, hipSetDevice(m->device));
  const int rc = launch_hamming_top2(d_A, a_pitch, d_nA, a_cap, d_B, b_pitch, d_nB, pairs, d_best_idx, d_best,
                                     d_second, m->err.as<int>(), stream);
  if (rc) return g_merr.fail(rc, "launch failed");
  return m->errm.mark((hipStream_t)stream) ? g_merr.fail(ORBX_EDEVICE, "event record failed") : ORBX_OK;
}

int orbm_search_for_initialization_batch(orbm_handle m, const orbx_kp* d_kp1, const uint8_t* d_desc1,
                                         const int* d_n1, const orbx_kp* d_kp2, const uint8_t* d_desc2,
                                         const int* d_n2, int kp_pitch, int pairs, orbm_grid_bounds b,
                                         float* d_prev_xy, int window, float nnratio, int check_ori,
                                         int* d_matches12, int* d_nmatches, void* stream) {
  if (!m || pairs < 1 || pairs > m->max_pairs || kp_pitch < 1 || kp_pitch > m->max_kps)
    return g_merr.fail(ORBX_EINVAL, "pairs/kp_pitch exceed the matcher workspace");
  HIP_OK(g_merr, hipSetDevice(m->device));
  return search_init_launch(m, d_kp1, d_desc1, d_n1, d_kp2, d_desc2, d_n2, kp_pitch, pairs, b, d_prev_xy, window,
                            nnratio, check_ori, d_matches12, d_nmatches, stream, m->init_ws.as<int>());
}

int orbm_search_for_initialization(orbm_handle m, const orbx_kp* kp1, const uint8_t* desc1, int n1,
                                   const orbx_kp* kp2, const uint8_t* desc2, int n2, orbm_grid_bounds bounds,
                                   float* prev_xy, int window, float nnratio, int check_ori, int* matches12,
                                   int* nmatches) {
  if (!m || !nmatches || n1 < 0 || n2 < 0) return g_merr.fail(ORBX_EINVAL, "bad argument");
  if ((n1 && (!kp1 || !desc1 || !prev_xy || !matches12)) || (n2 && (!kp2 || !desc2)))
    return g_merr.fail(ORBX_EINVAL, "null array");
  HIP_OK(g_merr, hipSetDevice(m->device));
  // Only octave-0 keypoints take part (src/ORBmatcher.cc:424-428: level1 > 0 is
  // skipped; GetFeaturesInArea(.., level1, level1) returns octave-0 keypoints of
  // F2, src/Frame.cc:350-352), so both frames are compacted to them in index
  // order before the upload: the kernel's per-keypoint tables then scale with
  // the octave-0 counts, not with the frames' sizes, and every result maps back
  // through the index lists. Other keypoints keep matches12 = -1 and their
  // vbPrevMatched entry.
  std::vector<int> q1, q2;
  q1.reserve(n1);
  q2.reserve(n2);
  for (int i = 0; i < n1; ++i)
    if (kp1[i].octave == 0) q1.push_back(i);
  for (int i = 0; i < n2; ++i)
    if (kp2[i].octave == 0) q2.push_back(i);
  const int c1 = (int)q1.size(), c2 = (int)q2.size();
  for (int i = 0; i < n1; ++i) matches12[i] = -1;
  if (c1 == 0 || c2 == 0) {
    *nmatches = 0;
    return ORBX_OK;
  }
  const int pitch = std::max(c1, c2);
  if (pitch > 65535) return g_merr.fail(ORBX_ECAPACITY, "more than 65535 octave-0 keypoints");
  std::vector<orbx_kp> hk((size_t)c1 + c2);
  std::vector<uint8_t> hd(((size_t)c1 + c2) * 32);
  std::vector<float> hp((size_t)c1 * 2);
  for (int k = 0; k < c1; ++k) {
    hk[k] = kp1[q1[k]];
    memcpy(&hd[(size_t)k * 32], desc1 + (size_t)q1[k] * 32, 32);
    hp[2 * k] = prev_xy[2 * q1[k]];
    hp[2 * k + 1] = prev_xy[2 * q1[k] + 1];
  }
  for (int k = 0; k < c2; ++k) {
    hk[c1 + k] = kp2[q2[k]];
    memcpy(&hd[((size_t)c1 + k) * 32], desc2 + (size_t)q2[k] * 32, 32);
  }
  const int hn[2] = {c1, c2};
  int nm = 0, rc;
  std::vector<int> hm(c1);
  Stage st(m);  // after the host arrays: an error exit waits for the copies that use them
  auto dk1 = st.slot<orbx_kp>(pitch), dk2 = st.slot<orbx_kp>(pitch);
  auto dd1 = st.slot<uint8_t>((size_t)pitch * 32), dd2 = st.slot<uint8_t>((size_t)pitch * 32);
  auto dprev = st.slot<float>((size_t)pitch * 2);
  auto dm = st.slot<int>(pitch);
  auto dn = st.slot<int>(2);  // n1, n2
  auto dnm = st.slot<int>(1);
  if ((rc = st.reserve()) || (rc = st.up(dk1, hk.data(), c1)) || (rc = st.up(dd1, hd.data(), (size_t)c1 * 32)) ||
      (rc = st.up(dprev, hp.data(), (size_t)c1 * 2)) || (rc = st.up(dk2, hk.data() + c1, c2)) ||
      (rc = st.up(dd2, hd.data() + (size_t)c1 * 32, (size_t)c2 * 32)) || (rc = st.up(dn, hn, 2)))
    return rc;
  // the call's own workspace, sized for its pitch (the octave-0 counts)
  const size_t wsb = init_ws_bytes_per_pair(pitch);
  if (wsb > m->host_init_ws.n) {
    if (m->host_init_ws.p) HIP_OK(g_merr, hipStreamSynchronize(st.st));
    if (const hipError_t e = m->host_init_ws.reserve(wsb))
      return g_merr.fail(ORBX_EDEVICE, "hipMalloc(&m->host_init_ws, wsb): %s", hipGetErrorString(e));
  }
  rc = search_init_launch(m, dk1, dd1, dn, dk2, dd2, dn + 1, pitch, 1, bounds, dprev, window, nnratio, check_ori, dm,
                          dnm, st.st, m->host_init_ws.as<int>());
  if (rc || (rc = st.down(&nm, dnm, 1)) || (rc = st.down(hm.data(), dm, c1)) ||
      (rc = st.down(hp.data(), dprev, (size_t)c1 * 2)) || (rc = st.finish()))
    return rc;
  for (int k = 0; k < c1; ++k) {
    const int i1 = q1[k];
    matches12[i1] = hm[k] >= 0 ? q2[hm[k]] : -1;
    prev_xy[2 * i1] = hp[2 * k];  // written by the kernel for matched queries, else the uploaded value
    prev_xy[2 * i1 + 1] = hp[2 * k + 1];
  }
  *nmatches = nm;
  return ORBX_OK;
}

int orbm_search_by_bow(orbm_handle m, const uint8_t* descA, const float* angleA, const uint8_t* mpA, int nA,
                       orbm_feature_vector fvA, const uint8_t* descB, const float* angleB, const uint8_t* mpB,
                       int nB, orbm_feature_vector fvB, float nnratio, int check_ori, int kf_vs_kf, int* out,
                       int* nmatches) {
  if (!m || !nmatches || nA < 0 || nB < 0) return g_merr.fail(ORBX_EINVAL, "bad argument");
  // DBoW2 precondition: each feature sits in at most one node; node ids ascending
  auto check_fv = [&](const orbm_feature_vector& fv, int n) -> bool {
    std::vector<char> seen(std::max(n, 1), 0);
    for (int k = 0; k < fv.n_nodes; ++k) {
      if (k && fv.nodes[k] <= fv.nodes[k - 1]) return false;
      for (int p = fv.off[k]; p < fv.off[k + 1]; ++p) {
        const int i = fv.idx[p];
        if (i < 0 || i >= n || seen[i]) return false;
        seen[i] = 1;
      }
    }
    return true;
  };
  // the row records keep the matched index in 16 bits (bin << 16 | index):
  // B's index in KF-KF mode, A's in KF-Frame mode; B's candidates are 16-bit too
  if (nB > 65536) return g_merr.fail(ORBX_EINVAL, "nB must be <= 65536");
  if (!kf_vs_kf && nA > 65536) return g_merr.fail(ORBX_EINVAL, "nA must be <= 65536 (KF-Frame row records)");
  if (!check_fv(fvA, nA) || !check_fv(fvB, nB))
    return g_merr.fail(ORBX_EINVAL, "FeatureVector must have ascending node ids and disjoint in-range indices");
  HIP_OK(g_merr, hipSetDevice(m->device));
  const int nout = kf_vs_kf ? nA : nB;
  const int ia = fvA.n_nodes ? fvA.off[fvA.n_nodes] : 0, ib = fvB.n_nodes ? fvB.off[fvB.n_nodes] : 0;
  const int pitch = std::max(nout, 1);  // out / records: the launch's pitch
  const int hn[4] = {nA, nB, fvA.n_nodes, fvB.n_nodes};
  int nm = 0, rc;
  Stage st(m);
  auto ddA = st.slot<uint8_t>((size_t)nA * 32), ddB = st.slot<uint8_t>((size_t)nB * 32);  // descriptors
  auto dgA = st.slot<float>(nA), dgB = st.slot<float>(nB);                                // angles
  auto dmA = st.slot<uint8_t>(nA), dmB = st.slot<uint8_t>(nB);                            // MapPoint masks
  auto dnoA = st.slot<uint32_t>(fvA.n_nodes), dnoB = st.slot<uint32_t>(fvB.n_nodes);      // FeatureVector CSR
  auto dofA = st.slot<int>(fvA.n_nodes + 1), dofB = st.slot<int>(fvB.n_nodes + 1);
  auto dixA = st.slot<int>(ia), dixB = st.slot<int>(ib);
  auto dout = st.slot<int>(pitch), drec = st.slot<int>(pitch);
  auto dnm = st.slot<int>(1);
  auto dn = st.slot<int>(4);  // nA, nB, nodes of A, nodes of B
  auto dhist = st.slot<int>(32);
  if ((rc = st.reserve()) || (rc = st.up(ddA, descA, (size_t)nA * 32)) || (rc = st.up(dgA, angleA, nA)) ||
      (rc = st.up(dmA, mpA, nA)) || (rc = st.up(dnoA, fvA.nodes, fvA.n_nodes)) ||
      (rc = st.up(dofA, fvA.off, fvA.n_nodes + 1)) || (rc = st.up(dixA, fvA.idx, ia)) ||
      (rc = st.up(ddB, descB, (size_t)nB * 32)) || (rc = st.up(dgB, angleB, nB)) || (rc = st.up(dmB, mpB, nB)) ||
      (rc = st.up(dnoB, fvB.nodes, fvB.n_nodes)) || (rc = st.up(dofB, fvB.off, fvB.n_nodes + 1)) ||
      (rc = st.up(dixB, fvB.idx, ib)) || (rc = st.up(dn, hn, 4)))
    return rc;
  BowSide A{ddA, dgA, 1, mpA ? (uint8_t*)dmA : nullptr, dn, dnoA, dofA, dixA, dn + 2, 0, 0};
  BowSide B{ddB, dgB, 1, mpB ? (uint8_t*)dmB : nullptr, dn + 1, dnoB, dofB, dixB, dn + 3, 0, 0};
  bool clean = false;  // staging memory: records and histogram filled first
  if ((rc = launch_search_bow(A, B, 1, nnratio, check_ori, kf_vs_kf, dout, pitch, dnm, drec, (size_t)pitch, dhist, 32,
                              &clean, m->err.as<int>(), st.st)))
    return g_merr.fail(rc, "search_bow launch: %s", hipGetErrorString(hipGetLastError()));
  if (m->errm.mark(st.st)) return g_merr.fail(ORBX_EDEVICE, "event record failed");
  if ((rc = st.down(&nm, dnm, 1)) || (rc = st.down(out, dout, nout)) || (rc = st.finish())) return rc;
  *nmatches = nm;
  return ORBX_OK;
}

int orbm_search_by_bow_batch(orbm_handle m, int pairs, int kp_pitch, int node_pitch, const orbx_kp* d_kpA,
                             const uint8_t* d_descA, const int* d_nA, const uint8_t* d_mpA, const uint32_t* d_nodesA,
                             const int* d_offA, const int* d_idxA, const int* d_nnA, const orbx_kp* d_kpB,
                             const uint8_t* d_descB, const int* d_nB, const uint8_t* d_mpB, const uint32_t* d_nodesB,
                             const int* d_offB, const int* d_idxB, const int* d_nnB, float nnratio, int check_ori,
                             int kf_vs_kf, int* d_out, int* d_nmatches, void* stream) {
  if (!m || pairs < 1 || kp_pitch < 1 || node_pitch < 1 || !d_kpA || !d_descA || !d_nA || !d_nodesA || !d_offA ||
      !d_idxA || !d_nnA || !d_kpB || !d_descB || !d_nB || !d_nodesB || !d_offB || !d_idxB || !d_nnB || !d_out ||
      !d_nmatches)
    return g_merr.fail(ORBX_EINVAL, "bad argument");
  if (pairs > m->max_pairs || kp_pitch > m->max_kps)
    return g_merr.fail(ORBX_ECAPACITY, "pairs/kp_pitch above the matcher's max_pairs/max_kps");
  if (kp_pitch > 65536) return g_merr.fail(ORBX_EINVAL, "kp_pitch must be <= 65536");
  HIP_OK(g_merr, hipSetDevice(m->device));
  // angles straight from the orbx_kp records (cv::KeyPoint::angle, float 3 of 7)
  BowSide A{d_descA, (const float*)d_kpA + 3, 7, d_mpA, d_nA, d_nodesA, d_offA, d_idxA, d_nnA, kp_pitch, node_pitch};
  BowSide B{d_descB, (const float*)d_kpB + 3, 7, d_mpB, d_nB, d_nodesB, d_offB, d_idxB, d_nnB, kp_pitch, node_pitch};
  hipStream_t s = (hipStream_t)stream;
  if (m->ws.before(s)) return g_merr.fail(ORBX_EDEVICE, "stream wait on the workspace failed");
  const int rc = launch_search_bow(A, B, pairs, nnratio, check_ori, kf_vs_kf, d_out, kp_pitch, d_nmatches,
                                   m->bow_rec.as<int>(),
                                   (size_t)m->max_pairs * m->max_kps, m->bow_hist.as<int>(), (size_t)m->max_pairs * 32,
                                   &m->bow_clean, m->err.as<int>(), stream);
  if (rc) return g_merr.fail(rc, "search_bow launch: %s", hipGetErrorString(hipGetLastError()));
  if (m->ws.after(s) || m->errm.mark(s)) return g_merr.fail(ORBX_EDEVICE, "event record failed");
  return ORBX_OK;
}

// sync: a synchronous caller that waits for the launch itself: its
// workspaces' earlier users are waited for only if still running, and no
// event is recorded after it (no barrier packets around its kernels)
static int stereo_batch(orbm_handle m, orbx_handle left, int left_frame0, orbx_handle right, int right_frame0,
                        const orbx_kp* d_kpL, const uint8_t* d_descL, const int* d_nL, const orbx_kp* d_kpR,
                        const uint8_t* d_descR, const int* d_nR, int kp_pitch, int pairs, float mb, float mbf,
                        float* d_uRight, float* d_depth, int* d_nkept, void* stream, bool sync) {
  if (!m || !left || !right || !d_kpL || !d_descL || !d_nL || !d_kpR || !d_descR || !d_nR || !d_uRight ||
      !d_depth || !d_nkept || pairs < 1 || kp_pitch < 1)
    return g_merr.fail(ORBX_EINVAL, "bad argument");
  if (pairs > m->max_pairs || kp_pitch > m->max_kps)
    return g_merr.fail(ORBX_ECAPACITY, "pairs/kp_pitch above the matcher's max_pairs/max_kps");
  if (!(mb > 0.f)) return g_merr.fail(ORBX_EINVAL, "baseline mb must be positive");
  HIP_OK(g_merr, hipSetDevice(m->device));
  StereoParams P{};
  int wr[kMaxLevels], hr[kMaxLevels], LR = 0;
  float sr[kMaxLevels], isr[kMaxLevels];
  if (extractor_pyramid(left, left_frame0, pairs, &P.pl, P.lw, P.lh, P.scale, P.inv_scale, &P.L) ||
      extractor_pyramid(right, right_frame0, pairs, &P.pr, wr, hr, sr, isr, &LR))
    return g_merr.fail(ORBX_EINVAL, "stereo pyramid: %s", orbx_last_error());
  if (LR != P.L) return g_merr.fail(ORBX_EINVAL, "left and right extractors have different level counts");
  for (int l = 0; l < P.L; ++l)
    if (wr[l] != P.lw[l] || hr[l] != P.lh[l]) return g_merr.fail(ORBX_EINVAL, "left and right image sizes differ");
  P.nrows = P.lh[0];
  P.kp_pitch = kp_pitch;
  P.mb = mb;
  P.mbf = mbf;
  // ~256 workgroups (one per CU) over the batch, 8 per pair for batches of
  // 32+ pairs; each stages its pair's right keypoints and descriptors in LDS.
  // Few pairs (the stereo Frame's one) take up to 64 per pair: the left
  // keypoints each wave walks through one after another set the latency
  // (one pair: 0.107 ms with 8, 0.085 ms with 64, shim_latency's stereo_parts)
  P.groups = std::max(1, std::min(64, (256 + pairs - 1) / pairs));
  if (const char* e = getenv("ORBX_STEREO_GROUPS")) P.groups = std::max(1, atoi(e));  // tuning experiments
  P.stop = 0;
#ifdef ORBX_DIAG  // diagnostics builds only: stop after a phase, results incomplete
  if (const char* e = getenv("ORBX_STEREO_STOP")) P.stop = atoi(e);
#endif
  // workgroup g takes left keypoints iL = g + groups * m: at most this many
  P.jobs_cap = (kp_pitch + P.groups - 1) / P.groups;
  if (stereo_lds_bytes(P.nrows, kp_pitch, P.jobs_cap) > 156 * 1024)
    return g_merr.fail(ORBX_ECAPACITY, "stereo row table does not fit in LDS (rows %d, kp_pitch %d)", P.nrows, kp_pitch);
  // the SAD scratch is the matcher's, the pyramids the extractors': order
  // this launch after their last users and make their next users wait for it
  hipStream_t s = (hipStream_t)stream;
  WsOrder* wl = extractor_ws(left);
  WsOrder* wr2 = extractor_ws(right);
  if (sync ? (m->ws.before_pending(s) || wl->before_pending(s) || wr2->before_pending(s))
           : (m->ws.before(s) || wl->before(s) || wr2->before(s)))
    return g_merr.fail(ORBX_EDEVICE, "stream wait on the workspaces failed");
  if (launch_stereo(P, d_kpL, d_descL, d_nL, d_kpR, d_descR, d_nR, pairs, d_uRight, d_depth, m->stereo_sad.as<int>(),
                    d_nkept,
                    stream) != ORBX_OK)
    return g_merr.fail(ORBX_EDEVICE, "stereo launch: %s", hipGetErrorString(hipGetLastError()));
  if (!sync && (m->ws.after(s) || wl->after(s) || wr2->after(s))) return g_merr.fail(ORBX_EDEVICE, "event record failed");
  return ORBX_OK;
}

int orbm_compute_stereo_matches_batch(orbm_handle m, orbx_handle left, int left_frame0, orbx_handle right,
                                      int right_frame0, const orbx_kp* d_kpL, const uint8_t* d_descL,
                                      const int* d_nL, const orbx_kp* d_kpR, const uint8_t* d_descR,
                                      const int* d_nR, int kp_pitch, int pairs, float mb, float mbf,
                                      float* d_uRight, float* d_depth, int* d_nkept, void* stream) {
  return stereo_batch(m, left, left_frame0, right, right_frame0, d_kpL, d_descL, d_nL, d_kpR, d_descR, d_nR,
                      kp_pitch, pairs, mb, mbf, d_uRight, d_depth, d_nkept, stream, false);
}

int orbm_compute_stereo_matches(orbm_handle m, orbx_handle left, orbx_handle right, const orbx_kp* kpL,
                                const uint8_t* descL, int nL, const orbx_kp* kpR, const uint8_t* descR, int nR,
                                float mb, float mbf, float* uRight, float* depth, int* nkept) {
  if (!m || !nkept || nL < 0 || nR < 0 || (nL && (!kpL || !descL || !uRight || !depth)) || (nR && (!kpR || !descR)))
    return g_merr.fail(ORBX_EINVAL, "bad argument");
  if (nL > m->max_kps || nR > m->max_kps) return g_merr.fail(ORBX_ECAPACITY, "more keypoints than max_kps");
  if (nR > 65535) return g_merr.fail(ORBX_ECAPACITY, "more than 65535 right keypoints");
  HIP_OK(g_merr, hipSetDevice(m->device));
  const int pitch = std::max(std::max(nL, nR), 1);
  const int hn[2] = {nL, nR};
  int kept = 0, rc;
  Stage st(m);
  auto dkl = st.slot<orbx_kp>(pitch), dkr = st.slot<orbx_kp>(pitch);
  auto ddl = st.slot<uint8_t>((size_t)pitch * 32), ddr = st.slot<uint8_t>((size_t)pitch * 32);
  auto du = st.slot<float>(pitch), dd = st.slot<float>(pitch);
  auto dn = st.slot<int>(2);  // nL, nR
  auto dkept = st.slot<int>(1);
  if ((rc = st.reserve()) || (rc = st.up(dkl, kpL, nL)) || (rc = st.up(ddl, descL, (size_t)nL * 32)) ||
      (rc = st.up(dkr, kpR, nR)) || (rc = st.up(ddr, descR, (size_t)nR * 32)) || (rc = st.up(dn, hn, 2)) ||
      (rc = stereo_batch(m, left, 0, right, 0, dkl, ddl, dn, dkr, ddr, dn + 1, pitch, 1, mb, mbf, du, dd, dkept, st.st,
                         true)) ||
      (rc = st.down(&kept, dkept, 1)) || (rc = st.down(uRight, du, nL)) || (rc = st.down(depth, dd, nL)) ||
      (rc = st.finish()))
    return rc;
  *nkept = kept;
  return ORBX_OK;
}

// The stereo kernels' outputs {kept, -, -, -, uRight[cap], depth[cap]} in one
// block at the head of the arena (cap = the kernels' pitch), so that one copy
// brings them into the matcher's pinned staging.
struct StereoBlock {
  int* kept;
  float *uRight, *depth;  // device
  size_t bytes;
  static int reserve(orbx_matcher* m, int cap, StereoBlock* b) {
    b->bytes = 16 + (size_t)cap * 8;
    int rc;
    if ((rc = stage_reserve(m, b->bytes)) || (rc = host_stage_reserve(m, b->bytes))) return rc;
    b->kept = m->stage.as<int>();
    b->uRight = m->stage.as<float>() + 4;
    b->depth = b->uRight + cap;
    return ORBX_OK;
  }
  // from the pinned copy, the first nL of each array
  static void unpack(const orbx_matcher* m, int cap, int nL, float* uRight, float* depth, int* nkept) {
    const uint8_t* h = m->h_stage.as<const uint8_t>();
    *nkept = ((const int*)h)[0];
    if (nL) {
      memcpy(uRight, h + 16, (size_t)nL * 4);
      memcpy(depth, h + 16 + (size_t)cap * 4, (size_t)nL * 4);
    }
  }
};

// Frame::ComputeStereoMatches right after the stereo constructor's two
// extractions (src/Frame.cc:77-89): the keypoints and descriptors are read
// where the two orbx_extract calls left them on the device, so only mvuRight
// and mvDepth cross the link.
int orbm_compute_stereo_matches_last(orbm_handle m, orbx_handle left, orbx_handle right, float mb, float mbf,
                                     float* uRight, float* depth, int nL, int* nkept) {
  if (!m || !left || !right || !nkept || nL < 0 || (nL && (!uRight || !depth))) return g_merr.fail(ORBX_EINVAL, "bad argument");
  const int* dnL = nullptr;
  const int* dnR = nullptr;
  const orbx_kp *dkl = nullptr, *dkr = nullptr;
  const uint8_t *ddl = nullptr, *ddr = nullptr;
  int capL = 0, capR = 0;
  if (extractor_last_output(left, &dnL, &dkl, &ddl, &capL) || extractor_last_output(right, &dnR, &dkr, &ddr, &capR))
    return g_merr.fail(ORBX_EINVAL, "stereo (last extraction): %s", orbx_last_error());
  if (!dnL || !dnR) {
    // an empty left or right image: no right keypoints to match, every left
    // keypoint keeps uRight = depth = -1 (src/Frame.cc:465-470)
    if (!dnL && nL) return g_merr.fail(ORBX_EINVAL, "nL %d but the left extraction was of an empty image", nL);
    for (int i = 0; i < nL; ++i) uRight[i] = depth[i] = -1.f;
    *nkept = 0;
    return ORBX_OK;
  }
  if (capL != capR) return g_merr.fail(ORBX_EINVAL, "left and right extractors have different capacities");
  if (nL > capL) return g_merr.fail(ORBX_EINVAL, "nL %d above the left extraction's capacity %d", nL, capL);
  HIP_OK(g_merr, hipSetDevice(m->device));
  // the device path sizes its LDS by the extractors' capacity; past the
  // matcher's limits (max_kps, or the stereo kernel's LDS for large
  // nFeatures) the keypoints come to the host and take the host-array path,
  // whose pitch is the actual counts
  auto host_fallback = [&]() -> int {
    int cnt[2] = {0, 0};
    HIP_OK(g_merr, hipMemcpy(&cnt[0], dnL, 4, hipMemcpyDeviceToHost));
    HIP_OK(g_merr, hipMemcpy(&cnt[1], dnR, 4, hipMemcpyDeviceToHost));
    if (nL > cnt[0]) return g_merr.fail(ORBX_EINVAL, "nL %d above the left extraction's count %d", nL, cnt[0]);
    std::vector<orbx_kp> kl(std::max(cnt[0], 1)), kr(std::max(cnt[1], 1));
    std::vector<uint8_t> dl((size_t)std::max(cnt[0], 1) * 32), dr((size_t)std::max(cnt[1], 1) * 32);
    HIP_OK(g_merr, hipMemcpy(kl.data(), dkl, (size_t)cnt[0] * sizeof(orbx_kp), hipMemcpyDeviceToHost));
    HIP_OK(g_merr, hipMemcpy(kr.data(), dkr, (size_t)cnt[1] * sizeof(orbx_kp), hipMemcpyDeviceToHost));
    HIP_OK(g_merr, hipMemcpy(dl.data(), ddl, (size_t)cnt[0] * 32, hipMemcpyDeviceToHost));
    HIP_OK(g_merr, hipMemcpy(dr.data(), ddr, (size_t)cnt[1] * 32, hipMemcpyDeviceToHost));
    return orbm_compute_stereo_matches(m, left, right, kl.data(), dl.data(), nL, kr.data(), dr.data(), cnt[1], mb, mbf,
                                       uRight, depth, nkept);
  };
  if (capL > m->max_kps) return host_fallback();
  StereoBlock blk;
  Stage st(m);
  int rc;
  if ((rc = StereoBlock::reserve(m, capL, &blk)) || (rc = st.open())) return rc;
  rc = stereo_batch(m, left, 0, right, 0, dkl, ddl, dnL, dkr, ddr, dnR, capL, 1, mb, mbf, blk.uRight, blk.depth,
                    blk.kept, st.st, true);
  if (rc == ORBX_ECAPACITY) return host_fallback();  // checked before any launch
  st.pending = true;  // no upload went before: the kernels count as enqueued even where stereo_batch failed
  if (rc || (rc = st.copy(m->h_stage.p, blk.kept, blk.bytes, hipMemcpyDeviceToHost)) || (rc = st.finish())) return rc;
  StereoBlock::unpack(m, capL, nL, uRight, depth, nkept);
  return ORBX_OK;
}

// orbm_stereo_frame's host phases (ORBX_STEREO_PROF=1): left staged, issued,
// right staged, issued, stereo issued, waited, copied out; medians of the
// calls after the first 20 per left handle, printed at exit
struct StereoProf {
  std::mutex mu;
  std::vector<std::pair<const void*, std::vector<double>>> per;  // per left handle: 7 phases per call
  void add(const void* key, const double* st) {
    std::lock_guard<std::mutex> lk(mu);
    size_t i = 0;
    while (i < per.size() && per[i].first != key) ++i;
    if (i == per.size()) per.push_back({key, {}});
    for (int k = 0; k < 7; ++k) per[i].second.push_back(st[k + 1] - st[k]);
  }
  ~StereoProf() {
    const char* names[7] = {"left staged", "issued", "right staged", "issued", "stereo issued", "wait", "copy-out"};
    for (auto& e : per) {
      const size_t n = e.second.size() / 7;
      if (n <= 20) continue;
      fprintf(stderr, "orbm_stereo_frame host phases, median of %zu calls (us):", n - 20);
      for (int k = 0; k < 7; ++k) {
        std::vector<double> v;
        for (size_t c = 20; c < n; ++c) v.push_back(e.second[c * 7 + k]);
        std::nth_element(v.begin(), v.begin() + v.size() / 2, v.end());
        fprintf(stderr, " %s %.1f", names[k], v[v.size() / 2] * 1e6);
      }
      fprintf(stderr, "\n");
    }
  }
};
static StereoProf& stereo_prof() {
  static StereoProf p;
  return p;
}

// The stereo Frame's construction steps (src/Frame.cc:77-89: ExtractORB on
// threadLeft / threadRight, then ComputeStereoMatches :465-639) with one
// device round trip: both extraction chains are issued from the calling
// thread on the two handles' streams (they run concurrently), the stereo
// kernels follow on the right stream once both are done, and their {kept,
// uRight, depth} block comes back (a copy kernel into pinned memory) in the
// same wait as the two extractions' outputs. Results are those of
// orbx_extract x2 + orbm_compute_stereo_matches_last.
int orbm_stereo_frame(orbm_handle m, orbx_handle left, orbx_handle right, const uint8_t* img_left,
                      size_t stride_left, const uint8_t* img_right, size_t stride_right, int w, int h, float mb,
                      float mbf, orbx_kp* kps_left, int cap_left, uint8_t* desc_left, int* n_left,
                      orbx_kp* kps_right, int cap_right, uint8_t* desc_right, int* n_right, float* uRight,
                      float* depth, int* nkept) {
  if (!m || !left || !right || !n_left || !n_right || !nkept || w < 0 || h < 0) return g_merr.fail(ORBX_EINVAL, "bad argument");
  if (left == right) return g_merr.fail(ORBX_EINVAL, "left and right need two extractor handles");
  if (!(mb > 0.f)) return g_merr.fail(ORBX_EINVAL, "baseline mb must be positive");
  *nkept = 0;
  if (w == 0 || h == 0) {
    // empty images: the two calls' own semantics (no outputs, uRight = -1)
    if (orbx_extract(left, img_left, w, h, stride_left, kps_left, cap_left, desc_left, n_left) ||
        orbx_extract(right, img_right, w, h, stride_right, kps_right, cap_right, desc_right, n_right))
      return g_merr.fail(ORBX_EINVAL, "stereo frame: %s", orbx_last_error());
    return orbm_compute_stereo_matches_last(m, left, right, mb, mbf, uRight, depth, *n_left, nkept);
  }
  HIP_OK(g_merr, hipSetDevice(m->device));
  int brc = ORBX_OK, cap = 0;
  auto between = [&](hipStream_t st) -> int {
    const int* dnL = nullptr;
    const int* dnR = nullptr;
    const orbx_kp *dkl = nullptr, *dkr = nullptr;
    const uint8_t *ddl = nullptr, *ddr = nullptr;
    int capR = 0;
    if (extractor_last_output(left, &dnL, &dkl, &ddl, &cap) || extractor_last_output(right, &dnR, &dkr, &ddr, &capR))
      return brc = g_merr.fail(ORBX_EINVAL, "stereo frame: %s", orbx_last_error());
    if (cap != capR) return brc = g_merr.fail(ORBX_EINVAL, "left and right extractors have different capacities");
    // past the matcher's limits: the host-array path after the extractions
    if (cap > m->max_kps) return (brc = ORBX_ECAPACITY), ORBX_OK;
    StereoBlock blk;
    int rc;
    if ((rc = StereoBlock::reserve(m, cap, &blk))) return brc = rc;
    rc = stereo_batch(m, left, 0, right, 0, dkl, ddl, dnL, dkr, ddr, dnR, cap, 1, mb, mbf, blk.uRight, blk.depth,
                      blk.kept, st, true);
    if (rc == ORBX_ECAPACITY) return (brc = ORBX_ECAPACITY), ORBX_OK;  // checked before any launch
    if (rc) return brc = rc;
    if ((rc = copy_to_host_async(m->h_stage.p, blk.kept, blk.bytes, st))) return brc = g_merr.fail(rc, "%s", orbx_last_error());
    return ORBX_OK;
  };
  // ORBX_STEREO_PROF=1 (diagnostics): host phases per call, medians printed at exit
  static const bool prof = getenv("ORBX_STEREO_PROF") && getenv("ORBX_STEREO_PROF")[0] == '1';
  double st[8];
  if (prof) st[0] = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
  int rc = extract_pair(left, right, img_left, stride_left, img_right, stride_right, w, h, between, kps_left, cap_left,
                        desc_left, n_left, kps_right, cap_right, desc_right, n_right, prof ? st + 1 : nullptr);
  if (prof && !rc) stereo_prof().add(left, st);
  if (rc) return brc ? brc : g_merr.fail(rc, "stereo frame: %s", orbx_last_error());
  if (brc == ORBX_ECAPACITY)
    return orbm_compute_stereo_matches_last(m, left, right, mb, mbf, uRight, depth, *n_left, nkept);
  if (brc) return brc;
  const int nL = *n_left;
  const bool no_out = nL && (!uRight || !depth);
  StereoBlock::unpack(m, cap, no_out ? 0 : nL, uRight, depth, nkept);
  return no_out ? g_merr.fail(ORBX_EINVAL, "null uRight/depth") : ORBX_OK;
}

int orbm_search_by_projection_batch(orbm_handle m, const orbx_kp* d_kps, const uint8_t* d_desc, const int* d_n,
                                    int kp_pitch, const float* d_uright, orbm_grid_bounds b, const float* scale,
                                    int nlevels, const uint8_t* d_blocked, const orbm_map_point_proj* d_mps,
                                    const uint8_t* d_mpdesc, const int* d_nmp, int mp_pitch, int frames, float th,
                                    float nnratio, int* d_out, int* d_nmatches, void* stream) {
  if (!m || !d_kps || !d_desc || !d_n || !scale || !d_blocked || !d_mps || !d_mpdesc || !d_nmp || !d_out ||
      !d_nmatches || frames < 1 || kp_pitch < 1 || mp_pitch < 1 || nlevels < 1 || nlevels > kMaxLevels)
    return g_merr.fail(ORBX_EINVAL, "bad argument");
  if (mp_pitch > 8192) return g_merr.fail(ORBX_ECAPACITY, "more than 8192 map points per frame");
  if (!(b.max_x > b.min_x) || !(b.max_y > b.min_y)) return g_merr.fail(ORBX_EINVAL, "empty grid bounds");
  if (proj_lds_bytes(kp_pitch) > 156 * 1024) return g_merr.fail(ORBX_ECAPACITY, "kp_pitch %d too large", kp_pitch);
  HIP_OK(g_merr, hipSetDevice(m->device));
  ProjParams P{};
  set_grid_bounds(P, b);
  for (int l = 0; l < kMaxLevels; ++l) P.scale[l] = scale[std::min(l, nlevels - 1)];
  P.th = th;
  P.nnratio = nnratio;
  P.kp_pitch = kp_pitch;
  P.mp_pitch = mp_pitch;
  P.has_uright = d_uright != nullptr;
  P.max_rounds = 32;
  if (const char* e = getenv("ORBX_PROJ_ROUNDS")) P.max_rounds = atoi(e);  // tests: force the sequential pass
  static long long* prof = nullptr;  // ORBX_PROJ_PROF: phase clocks of frame 0 printed after the call
  const bool do_prof = getenv("ORBX_PROJ_PROF") != nullptr;
  if (do_prof) {
    if (!prof) HIP_OK(g_merr, hipMalloc(&prof, (size_t)frames * 64 * 8));
    HIP_OK(g_merr, hipMemset(prof, 0, (size_t)frames * 64 * 8));
    P.prof = prof;
  }
  if (launch_search_proj(P, d_kps, d_desc, d_n, d_uright, d_blocked, d_mps, d_mpdesc, d_nmp, frames, d_out,
                         d_nmatches, stream))
    return g_merr.fail(ORBX_EDEVICE, "search_proj launch: %s", hipGetErrorString(hipGetLastError()));
  if (do_prof) {
    long long h[64];
    HIP_OK(g_merr, hipStreamSynchronize((hipStream_t)stream));
    HIP_OK(g_merr, hipMemcpy(h, prof, sizeof h, hipMemcpyDeviceToHost));
    fprintf(stderr, "proj prof frame 0:");
    for (int i = 1; i < 42 && h[i]; ++i) fprintf(stderr, " r%d=%lld", i - 1, h[i] - h[0]);
    fprintf(stderr, "\n");
  }
  return ORBX_OK;
}

int orbm_search_by_projection(orbm_handle m, const orbx_kp* kps, const uint8_t* desc, int n, const float* uright,
                              orbm_grid_bounds b, const float* scale, int nlevels, const uint8_t* blocked,
                              const orbm_map_point_proj* mps, const uint8_t* mpdesc, int nmp, float th,
                              float nnratio, int* out, int* nmatches) {
  if (!m || !nmatches || n < 0 || nmp < 0 || (n && (!kps || !desc || !blocked || !out)) ||
      (nmp && (!mps || !mpdesc)))
    return g_merr.fail(ORBX_EINVAL, "bad argument");
  if (nmp > 8192) return g_merr.fail(ORBX_ECAPACITY, "more than 8192 map points");
  HIP_OK(g_merr, hipSetDevice(m->device));
  const int kp = std::max(n, 1), mp = std::max(nmp, 1);
  const int hn[2] = {n, nmp};
  int nm = 0, rc;
  Stage st(m);
  auto dk = st.slot<orbx_kp>(kp);
  auto dd = st.slot<uint8_t>((size_t)kp * 32);
  auto dur = st.slot<float>(kp);
  auto dbl = st.slot<uint8_t>(kp);
  auto dmp = st.slot<orbm_map_point_proj>(mp);
  auto dmd = st.slot<uint8_t>((size_t)mp * 32);
  auto dout = st.slot<int>(kp);
  auto cnt = st.slot<int>(2);  // n, nmp
  auto dnm = st.slot<int>(1);
  if ((rc = st.reserve()) || (rc = st.up(dk, kps, n)) || (rc = st.up(dd, desc, (size_t)n * 32)) ||
      (rc = st.up(dur, uright, n)) || (rc = st.up(dbl, blocked, n)) || (rc = st.up(dmp, mps, nmp)) ||
      (rc = st.up(dmd, mpdesc, (size_t)nmp * 32)) || (rc = st.up(cnt, hn, 2)) ||
      (rc = orbm_search_by_projection_batch(m, dk, dd, cnt, kp, uright ? (float*)dur : nullptr, b, scale, nlevels, dbl,
                                            dmp, dmd, cnt + 1, mp, 1, th, nnratio, dout, dnm, st.st)) ||
      (rc = st.down(&nm, dnm, 1)) || (rc = st.down(out, dout, n)) || (rc = st.finish()))
    return rc;
  *nmatches = nm;
  return ORBX_OK;
}

// ------------------------------- Frame::isInFrustum, Tracking::SearchLocalPoints
static int frustum_params(orbm_grid_bounds b, float scale_factor, int nlevels, float viewing_cos_limit, int mp_pitch,
                          FrustumParams* P) {
  if (nlevels < 1 || nlevels > kMaxLevels) return g_merr.fail(ORBX_EINVAL, "nlevels must be in 1..%d", kMaxLevels);
  if (!(b.max_x > b.min_x) || !(b.max_y > b.min_y)) return g_merr.fail(ORBX_EINVAL, "empty grid bounds");
  *P = FrustumParams{};
  P->minX = b.min_x;
  P->maxX = b.max_x;
  P->minY = b.min_y;
  P->maxY = b.max_y;
  // the thresholds of the thread's last (scale factor, levels) are kept: the
  // shim's Frame::isInFrustum comes here once per point
  struct Thr {
    float sf = 0.f;
    int L = 0;
    float thr[kMaxLevels];
  };
  static thread_local Thr last;
  if (last.L != nlevels || last.sf != scale_factor) {
    last.L = 0;
    const int rc = orbm_predict_scale_thresholds(scale_factor, nlevels, last.thr);
    if (rc) return rc;
    last.sf = scale_factor;
    last.L = nlevels;
  }
  std::memcpy(P->pred_thr, last.thr, sizeof last.thr);
  P->L = nlevels;
  P->cos_limit = viewing_cos_limit;
  P->mp_pitch = mp_pitch;
  return ORBX_OK;
}

int orbm_is_in_frustum(const orbm_pose* pose, orbm_grid_bounds b, float scale_factor, int nlevels,
                       float viewing_cos_limit, const orbm_map_point_world* mps, int nmp, orbm_map_point_proj* out,
                       int* n_in_view) {
  if (!pose || !n_in_view || nmp < 0 || (nmp && (!mps || !out))) return g_merr.fail(ORBX_EINVAL, "bad argument");
  FrustumParams P;
  const int rc = frustum_params(b, scale_factor, nlevels, viewing_cos_limit, std::max(nmp, 1), &P);
  if (rc) return rc;
  int c = 0;
  for (int j = 0; j < nmp; ++j) c += frustum_point(P, *pose, mps[j], &out[j]) ? 1 : 0;
  *n_in_view = c;
  return ORBX_OK;
}

int orbm_is_in_frustum_batch(orbm_handle m, const orbm_pose* d_poses, orbm_grid_bounds b, float scale_factor,
                             int nlevels, float viewing_cos_limit, const orbm_map_point_world* d_mps,
                             const int* d_nmp, int mp_pitch, int frames, orbm_map_point_proj* d_out,
                             int* d_n_in_view, void* stream) {
  if (!m || !d_poses || !d_mps || !d_nmp || !d_out || !d_n_in_view || frames < 1 || mp_pitch < 1)
    return g_merr.fail(ORBX_EINVAL, "bad argument");
  if (mp_pitch > 65536) return g_merr.fail(ORBX_ECAPACITY, "more than 65536 map points per frame");
  FrustumParams P;
  const int rc = frustum_params(b, scale_factor, nlevels, viewing_cos_limit, mp_pitch, &P);
  if (rc) return rc;
  HIP_OK(g_merr, hipSetDevice(m->device));
  HIP_OK(g_merr, hipMemsetAsync(d_n_in_view, 0, (size_t)frames * 4, (hipStream_t)stream));
  if (launch_frustum(P, d_poses, d_mps, d_nmp, frames, d_out, d_n_in_view, stream))
    return g_merr.fail(ORBX_EDEVICE, "frustum launch: %s", hipGetErrorString(hipGetLastError()));
  return ORBX_OK;
}

// status: the compaction reports more than kFrustumMaxView points in view in
// the handle's status word (the batch call); the synchronous call reads the
// count itself instead
static int local_points_batch(orbm_handle m, const orbx_kp* d_kps, const uint8_t* d_desc, const int* d_n, int kp_pitch,
                              const float* d_uright, orbm_grid_bounds b, const float* scale, int nlevels,
                              float scale_factor, const uint8_t* d_blocked, const orbm_pose* d_poses,
                              const orbm_map_point_world* d_mps, const uint8_t* d_mpdesc, const int* d_nmp,
                              int mp_pitch, int frames, float viewing_cos_limit, float th, float nnratio, int* d_out,
                              int* d_nmatches, orbm_map_point_proj* d_proj, int* d_n_in_view, void* stream,
                              bool status) {
  if (!m || !d_kps || !d_desc || !d_n || !scale || !d_blocked || !d_poses || !d_mps || !d_mpdesc || !d_nmp ||
      !d_out || !d_nmatches || !d_n_in_view || frames < 1 || kp_pitch < 1 || mp_pitch < 1)
    return g_merr.fail(ORBX_EINVAL, "bad argument");
  if (mp_pitch > 65536) return g_merr.fail(ORBX_ECAPACITY, "more than 65536 map points per frame");
  if (proj_lds_bytes(kp_pitch) > 156 * 1024) return g_merr.fail(ORBX_ECAPACITY, "kp_pitch %d too large", kp_pitch);
  FrustumParams P;
  int rc = frustum_params(b, scale_factor, nlevels, viewing_cos_limit, mp_pitch, &P);
  if (rc) return rc;
  HIP_OK(g_merr, hipSetDevice(m->device));
  hipStream_t s = (hipStream_t)stream;
  // scratch: the isInFrustum records (when the caller keeps none), then per
  // frame the points in view: records, descriptors, original indices, count
  const int cp = std::min(mp_pitch, kFrustumMaxView);
  auto a256 = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t o_cproj = d_proj ? 0 : a256((size_t)frames * mp_pitch * sizeof(orbm_map_point_proj));
  const size_t o_cdesc = o_cproj + a256((size_t)frames * cp * sizeof(orbm_map_point_proj));
  const size_t o_cmap = o_cdesc + a256((size_t)frames * cp * 32);
  const size_t o_cnmp = o_cmap + a256((size_t)frames * cp * 4);
  const size_t need = o_cnmp + a256((size_t)frames * 4);
  if (m->ws.before(s)) return g_merr.fail(ORBX_EDEVICE, "stream wait on the workspace failed");
  if (m->view_ws.n < need) {
    if (m->ws.ev) HIP_OK(g_merr, hipEventSynchronize(m->ws.ev));
    if (m->view_ws.reserve(need) != hipSuccess) return g_merr.fail(ORBX_ENOMEM, "local points workspace");
  }
  uint8_t* ws = m->view_ws.as<uint8_t>();
  orbm_map_point_proj* proj = d_proj ? d_proj : m->view_ws.as<orbm_map_point_proj>();
  orbm_map_point_proj* c_proj = (orbm_map_point_proj*)(ws + o_cproj);
  uint8_t* c_desc = ws + o_cdesc;
  int* c_map = (int*)(ws + o_cmap);
  int* c_nmp = (int*)(ws + o_cnmp);
  HIP_OK(g_merr, hipMemsetAsync(d_n_in_view, 0, (size_t)frames * 4, s));
  if (launch_frustum(P, d_poses, d_mps, d_nmp, frames, proj, d_n_in_view, stream) ||
      launch_compact_in_view(proj, d_mpdesc, d_nmp, mp_pitch, frames, c_proj, c_desc, c_map, c_nmp, cp,
                             status ? m->err.as<int>() : nullptr, stream))
    return g_merr.fail(ORBX_EDEVICE, "local points launch: %s", hipGetErrorString(hipGetLastError()));
  // a frame with nothing in view (src/Tracking.cc:1268 skips the search) leaves out = -1, nmatches = 0
  if ((rc = orbm_search_by_projection_batch(m, d_kps, d_desc, d_n, kp_pitch, d_uright, b, scale, nlevels, d_blocked,
                                            c_proj, c_desc, c_nmp, cp, frames, th, nnratio, d_out, d_nmatches,
                                            stream)))
    return rc;
  if (launch_remap_out(d_out, d_n, kp_pitch, c_map, cp, frames, stream))
    return g_merr.fail(ORBX_EDEVICE, "local points launch: %s", hipGetErrorString(hipGetLastError()));
  if (m->ws.after(s) || (status && m->errm.mark(s))) return g_merr.fail(ORBX_EDEVICE, "event record failed");
  return ORBX_OK;
}

int orbm_search_local_points_batch(orbm_handle m, const orbx_kp* d_kps, const uint8_t* d_desc, const int* d_n,
                                   int kp_pitch, const float* d_uright, orbm_grid_bounds b, const float* scale,
                                   int nlevels, float scale_factor, const uint8_t* d_blocked,
                                   const orbm_pose* d_poses, const orbm_map_point_world* d_mps,
                                   const uint8_t* d_mpdesc, const int* d_nmp, int mp_pitch, int frames,
                                   float viewing_cos_limit, float th, float nnratio, int* d_out, int* d_nmatches,
                                   orbm_map_point_proj* d_proj, int* d_n_in_view, void* stream) {
  return local_points_batch(m, d_kps, d_desc, d_n, kp_pitch, d_uright, b, scale, nlevels, scale_factor, d_blocked,
                            d_poses, d_mps, d_mpdesc, d_nmp, mp_pitch, frames, viewing_cos_limit, th, nnratio, d_out,
                            d_nmatches, d_proj, d_n_in_view, stream, true);
}

int orbm_search_local_points(orbm_handle m, const orbx_kp* kps, const uint8_t* desc, int n, const float* uright,
                             orbm_grid_bounds b, const float* scale, int nlevels, float scale_factor,
                             const uint8_t* blocked, const orbm_camera* cur, const orbm_map_point_world* mps,
                             const uint8_t* mpdesc, int nmp, float viewing_cos_limit, float th, float nnratio,
                             int* out, int* nmatches, orbm_map_point_proj* proj, int* n_in_view) {
  if (!m || !nmatches || !n_in_view || !cur || !scale || n < 0 || nmp < 0 ||
      (n && (!kps || !desc || !blocked || !out)) || (nmp && (!mps || !mpdesc)))
    return g_merr.fail(ORBX_EINVAL, "bad argument");
  if (nmp > 65536) return g_merr.fail(ORBX_ECAPACITY, "more than 65536 map points");
  orbm_pose pose;
  int rc = orbm_prepare_pose(ORBM_PROJ_KEYFRAME, cur, nullptr, 0, &pose);
  if (rc) return rc;
  HIP_OK(g_merr, hipSetDevice(m->device));
  const int kp = std::max(n, 1), mp = std::max(nmp, 1);
  const int hn[2] = {n, nmp};
  int nm = 0, niv = 0;
  Stage st(m);
  auto dk = st.slot<orbx_kp>(kp);
  auto dd = st.slot<uint8_t>((size_t)kp * 32);
  auto dur = st.slot<float>(kp);
  auto dbl = st.slot<uint8_t>(kp);
  auto dmp = st.slot<orbm_map_point_world>(mp);
  auto dmd = st.slot<uint8_t>((size_t)mp * 32);
  auto dpr = st.slot<orbm_map_point_proj>(mp);
  auto dout = st.slot<int>(kp);
  auto cnt = st.slot<int>(2);  // n, nmp
  auto dnm = st.slot<int>(1);
  auto dniv = st.slot<int>(1);
  auto dpose = st.slot<orbm_pose>(1);
  if ((rc = st.reserve()) || (rc = st.up(dk, kps, n)) || (rc = st.up(dd, desc, (size_t)n * 32)) ||
      (rc = st.up(dur, uright, n)) || (rc = st.up(dbl, blocked, n)) || (rc = st.up(dmp, mps, nmp)) ||
      (rc = st.up(dmd, mpdesc, (size_t)nmp * 32)) || (rc = st.up(cnt, hn, 2)) || (rc = st.up(dpose, &pose, 1)) ||
      (rc = local_points_batch(m, dk, dd, cnt, kp, uright ? (float*)dur : nullptr, b, scale, nlevels, scale_factor,
                               dbl, dpose, dmp, dmd, cnt + 1, mp, 1, viewing_cos_limit, th, nnratio, dout, dnm, dpr,
                               dniv, st.st, false)) ||
      (rc = st.down(&nm, dnm, 1)) || (rc = st.down(&niv, dniv, 1)) || (rc = st.down(out, dout, n)) ||
      (proj && (rc = st.down(proj, dpr, nmp))) || (rc = st.finish()))
    return rc;
  *n_in_view = niv;
  if (niv > kFrustumMaxView)
    return g_merr.fail(ORBX_ECAPACITY, "%d map points in view, more than %d can be searched", niv, kFrustumMaxView);
  *nmatches = nm;
  return ORBX_OK;
}

// ------------- MapPoint::ComputeDistinctiveDescriptors, UpdateNormalAndDepth
int orbm_distinctive_descriptor(const uint8_t* desc, int n, int* best, int* median) {
  if (!best || n < 0 || (n && !desc)) return g_merr.fail(ORBX_EINVAL, "bad argument");
  int best_i = -1, best_med = INT_MAX;
  std::vector<uint32_t> w((size_t)n * 8);
  if (n) memcpy(w.data(), desc, (size_t)n * 32);
  const int at = (n - 1) >> 1;  // vDists[0.5*(N-1)] (src/MapPoint.cc:299)
  for (int i = 0; i < n; ++i) {
    int hist[257] = {0};
    for (int j = 0; j < n; ++j) ++hist[mp_hamming(&w[(size_t)i * 8], &w[(size_t)j * 8])];
    int med = 0;
    for (int seen = hist[0]; seen <= at; seen += hist[med]) ++med;
    if (med < best_med) {  // strictly smaller: the first row wins a tie (:301)
      best_med = med;
      best_i = i;
    }
  }
  *best = best_i;
  if (median) *median = n ? best_med : -1;
  return ORBX_OK;
}

int orbm_update_normal_and_depth(const float* pos, const float* Ow_list, int n, const float* Ow_ref, float ref_scale,
                                 float last_scale, float* normal_out, float* min_distance, float* max_distance) {
  if (!pos || !Ow_ref || !normal_out || !min_distance || !max_distance || n < 0 || (n && !Ow_list))
    return g_merr.fail(ORBX_EINVAL, "bad argument");
  if (n == 0) return ORBX_OK;  // observations.empty() (src/MapPoint.cc:350)
  float sum[3] = {0.f, 0.f, 0.f}, t[3], out[5];
  for (int k = 0; k < n; ++k) {
    mp_normal_term(pos, Ow_list + 3 * (size_t)k, t);
    mp_normal_add(sum, t);
  }
  mp_finish(sum, (unsigned)n, pos, Ow_ref, ref_scale, last_scale, out);
  normal_out[0] = out[0];
  normal_out[1] = out[1];
  normal_out[2] = out[2];
  *min_distance = out[3];
  *max_distance = out[4];
  return ORBX_OK;
}

int orbm_refresh_map_points_batch(orbm_handle m, const orbm_observation* d_obs, const uint32_t* d_obs_off,
                                  const uint32_t* d_point_ids, int points, const orbm_keyframe_ref* d_kfs, int n_kfs,
                                  const uint8_t* d_desc, uint32_t desc_rows, const orbm_point_refkf* d_ref,
                                  const float* scale, int nlevels, orbm_map_point_world* d_mps, uint8_t* d_mpdesc,
                                  int* d_best, int* d_median, void* stream) {
  if (!m || !d_obs || !d_obs_off || !d_kfs || !d_desc || points < 1 || n_kfs < 0)
    return g_merr.fail(ORBX_EINVAL, "bad argument");
  if (!d_mps && !d_mpdesc && !d_best && !d_median) return g_merr.fail(ORBX_EINVAL, "nothing to refresh: no output array");
  if (d_mps && (!d_ref || !scale || nlevels < 1 || nlevels > kMaxLevels))
    return g_merr.fail(ORBX_EINVAL, "records need d_ref and 1..%d scale factors", kMaxLevels);
  if (((uintptr_t)d_desc | (uintptr_t)d_mpdesc) & 15) return g_merr.fail(ORBX_EINVAL, "descriptors must be 16-byte aligned");
  HIP_OK(g_merr, hipSetDevice(m->device));
  hipStream_t s = (hipStream_t)stream;
  if (m->ws.before(s)) return g_merr.fail(ORBX_EDEVICE, "stream wait on the workspace failed");
  const size_t need = refresh_ws_bytes(points);
  if (m->refresh_ws.n < need) {
    if (m->ws.ev) HIP_OK(g_merr, hipEventSynchronize(m->ws.ev));
    if (m->refresh_ws.reserve(need) != hipSuccess) return g_merr.fail(ORBX_ENOMEM, "map point refresh workspace");
  }
  RefreshArgs A{};
  A.obs = d_obs;
  A.off = d_obs_off;
  A.ids = d_point_ids;
  A.points = points;
  A.kfs = d_kfs;
  A.n_kfs = (uint32_t)n_kfs;
  A.desc = d_desc;
  A.desc_rows = desc_rows;
  A.ref = d_mps ? d_ref : nullptr;
  if (d_mps) std::memcpy(A.scale, scale, (size_t)nlevels * sizeof(float));
  A.nlevels = d_mps ? nlevels : 0;
  A.mps = d_mps;
  A.mpdesc = d_mpdesc;
  A.best = d_best;
  A.median = d_median;
  A.err = m->err.as<int>();
  A.counts = m->refresh_ws.as<int>();
  A.lists = (int*)(m->refresh_ws.as<uint8_t>() + 256);
  if (launch_refresh_map_points(A, stream))
    return g_merr.fail(ORBX_EDEVICE, "map point refresh launch: %s", hipGetErrorString(hipGetLastError()));
  if (m->ws.after(s) || m->errm.mark(s)) return g_merr.fail(ORBX_EDEVICE, "event record failed");
  return ORBX_OK;
}

int orbm_refresh_map_points(orbm_handle m, const orbm_observation* obs, const uint32_t* obs_off,
                            const uint32_t* point_ids, int points, const orbm_keyframe_ref* kfs, int n_kfs,
                            const uint8_t* desc, uint32_t desc_rows, const orbm_point_refkf* ref, const float* scale,
                            int nlevels, orbm_map_point_world* mps, uint8_t* mpdesc, int n_mps, int* best,
                            int* median) {
  if (!m || !obs_off || points < 0 || n_kfs < 0 || n_mps < 0) return g_merr.fail(ORBX_EINVAL, "bad argument");
  if (points == 0) return ORBX_OK;
  if (!mps && !mpdesc && !best && !median) return g_merr.fail(ORBX_EINVAL, "nothing to refresh: no output array");
  for (int p = 0; p < points; ++p)
    if (obs_off[p + 1] < obs_off[p]) return g_merr.fail(ORBX_EINVAL, "obs_off descends at point %d", p);
  const size_t nobs = obs_off[points];
  if (nobs && (!obs || !kfs || !desc || !n_kfs || !desc_rows)) return g_merr.fail(ORBX_EINVAL, "null array");
  if (mps || mpdesc) {
    if (!point_ids && n_mps < points) return g_merr.fail(ORBX_EINVAL, "%d points in a table of %d", points, n_mps);
    for (int p = 0; point_ids && p < points; ++p)
      if (point_ids[p] >= (uint32_t)n_mps) return g_merr.fail(ORBX_EINVAL, "point id %u outside the table", point_ids[p]);
  }
  HIP_OK(g_merr, hipSetDevice(m->device));
  const size_t tab = std::max(n_mps, 1), nk = std::max(n_kfs, 1), nr = std::max<size_t>(desc_rows, 1);
  int rc;
  Stage st(m);
  auto dobs = st.slot<orbm_observation>(std::max<size_t>(nobs, 1));
  auto doff = st.slot<uint32_t>((size_t)points + 1);
  auto dids = st.slot<uint32_t>(points);
  auto dkf = st.slot<orbm_keyframe_ref>(nk);
  auto dds = st.slot<uint8_t>(nr * 32);
  auto drf = st.slot<orbm_point_refkf>(points);
  auto dmp = st.slot<orbm_map_point_world>(tab);
  auto dmd = st.slot<uint8_t>(tab * 32);
  auto dbe = st.slot<int>(points);
  auto dme = st.slot<int>(points);
  if ((rc = st.reserve()) || (rc = st.up(dobs, obs, nobs)) || (rc = st.up(doff, obs_off, (size_t)points + 1)) ||
      (rc = st.up(dids, point_ids, points)) || (rc = st.up(dkf, kfs, n_kfs)) ||
      (rc = st.up(dds, desc, (size_t)desc_rows * 32)) || (rc = st.up(drf, ref, points)) ||
      (rc = st.up(dmp, (const orbm_map_point_world*)mps, n_mps)) ||
      (rc = st.up(dmd, (const uint8_t*)mpdesc, (size_t)n_mps * 32)) ||
      (rc = orbm_refresh_map_points_batch(m, dobs, doff, point_ids ? (uint32_t*)dids : nullptr, points, dkf, n_kfs,
                                          dds, desc_rows, ref ? (orbm_point_refkf*)drf : nullptr, scale, nlevels,
                                          mps ? (orbm_map_point_world*)dmp : nullptr,
                                          mpdesc ? (uint8_t*)dmd : nullptr, best ? (int*)dbe : nullptr,
                                          median ? (int*)dme : nullptr, st.st)) ||
      (mps && (rc = st.down(mps, dmp, n_mps))) || (mpdesc && (rc = st.down(mpdesc, dmd, (size_t)n_mps * 32))) ||
      (best && (rc = st.down(best, dbe, points))) || (median && (rc = st.down(median, dme, points))) ||
      (rc = st.finish()))
    return rc;
  return ORBX_OK;
}

// ------------------------------------------- Optimizer::PoseOptimization
namespace {

// the sums of po_run over host edges, edge after edge in keypoint order
struct HostPoCtx {
  std::vector<PoEdge>& E;
  PoCam cam;
  void linearise(const PoPose& est, bool robust, double* acc) {
    for (int k = 0; k < kPoSums; ++k) acc[k] = 0.0;
    for (const PoEdge& e : E)
      if (!(e.tag & kPoOutlier)) po_edge_linearise(cam, est, e, robust, acc);
  }
  double robust_chi2(const PoPose& est, bool robust) {
    double s = 0.0;
    for (const PoEdge& e : E)
      if (!(e.tag & kPoOutlier)) s += po_edge_robust_chi2(cam, est, e, robust);
    return s;
  }
  int classify(const PoPose& est, const PoPose& err_pose) {
    int bad = 0;
    for (PoEdge& e : E) {
      const bool out = po_is_outlier(e, po_edge_chi2(cam, (e.tag & kPoOutlier) ? est : err_pose, e));
      e.tag = out ? (e.tag | kPoOutlier) : (e.tag & ~kPoOutlier);
      bad += out ? 1 : 0;
    }
    return bad;
  }
};

}  // namespace

int orbm_pose_optimization_host(const orbx_kp* kps, int n, const float* uright, int* assign,
                                const orbm_map_point_world* mps, int nmp, const float* inv_sigma2, int nlevels,
                                const orbm_camera* cam, int flags, float* Tcw, orbm_pose* pose, uint8_t* outlier,
                                orbm_poseopt_result* result, int* status) {
  if (n < 0 || nmp < 0 || !cam || !inv_sigma2 || nlevels < 1 || nlevels > kMaxLevels || (n && (!kps || !assign)) ||
      (nmp && !mps))
    return g_merr.fail(ORBX_EINVAL, "bad argument");
  // an edge's tag holds the keypoint index in 16 bits; the index travels beside it here
  std::vector<PoEdge> E;
  std::vector<int> index;
  int st_bits = 0;
  for (int i = 0; i < n; ++i) {
    const int row = assign[i];
    if (row < 0) continue;
    const int octave = kps[i].octave;
    if (row >= nmp || octave < 0 || octave >= nlevels) {
      st_bits |= kStatusPoseOptSkipped;
      continue;
    }
    const float u = uright ? uright[i] : -1.0f;
    PoEdge e;
    for (int k = 0; k < 3; ++k) e.X[k] = mps[row].pos[k];
    e.obs[0] = kps[i].x;
    e.obs[1] = kps[i].y;
    e.obs[2] = u;
    e.w = inv_sigma2[octave];
    e.tag = (u < 0 ? 0u : kPoStereo) | (mps[row].obs_positive ? kPoObs : 0u);
    E.push_back(e);
    index.push_back(i);
  }
  const int ne = (int)E.size();
  PoStats st{0, 0, 0, 0};
  float Tout[12];
  std::memcpy(Tout, cam->Tcw, sizeof Tout);
  if (ne >= 3) {
    HostPoCtx ctx{E, PoCam{(double)cam->fx, (double)cam->fy, (double)cam->cx, (double)cam->cy, (double)cam->mbf}};
    PoPose T0, est;
    po_from_Tcw(cam->Tcw, &T0);
    po_run(ctx, T0, ne, &est, &st);
    po_to_Tcw(est, Tout);
  }
  int with_obs = 0;
  for (int k = 0; k < ne; ++k) {
    const bool out = (E[k].tag & kPoOutlier) != 0;
    if (outlier) outlier[index[k]] = out ? 1 : 0;
    if (out && (flags & ORBM_POSEOPT_DISCARD_OUTLIERS)) assign[index[k]] = -1;
    with_obs += (!out && (E[k].tag & kPoObs)) ? 1 : 0;
  }
  if (Tcw) std::memcpy(Tcw, Tout, sizeof Tout);
  if (pose) pose_from_rt(*cam, Tout, pose);
  if (result) {
    result->ret = ne >= 3 ? ne - st.n_bad : 0;
    result->n_initial = ne;
    result->n_bad = st.n_bad;
    result->n_inliers_with_obs = with_obs;
    result->rounds = st.rounds;
    result->trials = st.trials;
    result->rejected = st.rejected;
    result->reserved = 0;
  }
  if (status) *status = st_bits;
  return ORBX_OK;
}

int orbm_pose_optimization_batch(orbm_handle m, const orbx_kp* d_kps, const int* d_n, int kp_pitch,
                                 const float* d_uright, int* d_assign, const orbm_map_point_world* d_mps,
                                 const int* d_nmp, int mp_pitch, const float* inv_sigma2, int nlevels,
                                 const orbm_camera* d_cams, int frames, int flags, float* d_Tcw, orbm_pose* d_pose,
                                 uint8_t* d_outlier, orbm_poseopt_result* d_result, void* stream) {
  if (!m || !d_kps || !d_n || !d_assign || !d_mps || !d_nmp || !inv_sigma2 || !d_cams || frames < 1 || kp_pitch < 1 ||
      mp_pitch < 1 || nlevels < 1 || nlevels > kMaxLevels)
    return g_merr.fail(ORBX_EINVAL, "bad argument");
  if (kp_pitch > m->max_kps) return g_merr.fail(ORBX_ECAPACITY, "kp_pitch %d above the handle's max_kps %d", kp_pitch, m->max_kps);
  HIP_OK(g_merr, hipSetDevice(m->device));
  hipStream_t s = (hipStream_t)stream;
  const size_t need = poseopt_spill_bytes(kp_pitch, frames);
  if (need) {
    if (m->ws.before(s)) return g_merr.fail(ORBX_EDEVICE, "stream wait on the workspace failed");
    if (m->po_ws.n < need) {
      if (m->ws.ev) HIP_OK(g_merr, hipEventSynchronize(m->ws.ev));
      if (m->po_ws.reserve(need) != hipSuccess) return g_merr.fail(ORBX_ENOMEM, "pose optimisation workspace");
    }
  }
  PoseOptArgs A{};
  A.kps = d_kps;
  A.n = d_n;
  A.kp_pitch = kp_pitch;
  A.uright = d_uright;
  A.assign = d_assign;
  A.mps = d_mps;
  A.nmp = d_nmp;
  A.mp_pitch = mp_pitch;
  A.inv_sigma2 = inv_sigma2;
  A.nlevels = nlevels;
  A.cams = d_cams;
  A.frames = frames;
  A.flags = flags;
  A.Tcw = d_Tcw;
  A.pose = d_pose;
  A.outlier = d_outlier;
  A.result = d_result;
  A.err = m->err.as<int>();
  if (launch_pose_optimization(A, need ? m->po_ws.p : nullptr, stream))
    return g_merr.fail(ORBX_EDEVICE, "pose optimisation launch: %s", hipGetErrorString(hipGetLastError()));
  if ((need && m->ws.after(s)) || m->errm.mark(s)) return g_merr.fail(ORBX_EDEVICE, "event record failed");
  return ORBX_OK;
}

int orbm_pose_optimization(orbm_handle m, const orbx_kp* kps, int n, const float* uright, int* assign,
                           const orbm_map_point_world* mps, int nmp, const float* inv_sigma2, int nlevels,
                           const orbm_camera* cam, int flags, float* Tcw, orbm_pose* pose, uint8_t* outlier,
                           orbm_poseopt_result* result) {
  if (!m || n < 0 || nmp < 0 || !cam || (n && (!kps || !assign)) || (nmp && !mps))
    return g_merr.fail(ORBX_EINVAL, "bad argument");
  if (n > m->max_kps) return g_merr.fail(ORBX_ECAPACITY, "%d keypoints above the handle's max_kps %d", n, m->max_kps);
  HIP_OK(g_merr, hipSetDevice(m->device));
  const size_t kp = std::max(n, 1), np = std::max(nmp, 1);
  int rc;
  Stage st(m);
  auto dk = st.slot<orbx_kp>(kp);
  auto dn = st.slot<int>(2);
  auto du = st.slot<float>(kp);
  auto da = st.slot<int>(kp);
  auto dm = st.slot<orbm_map_point_world>(np);
  auto dc = st.slot<orbm_camera>(1);
  auto dT = st.slot<float>(12);
  auto dp = st.slot<orbm_pose>(1);
  auto dout = st.slot<uint8_t>(kp);
  auto dr = st.slot<orbm_poseopt_result>(1);
  const int counts[2] = {n, nmp};
  // the caller's flags go up too: the bytes of keypoints without a point come back as they were
  if ((rc = st.reserve()) || (rc = st.up(dk, kps, n)) || (rc = st.up(dn, counts, 2)) || (rc = st.up(du, uright, n)) ||
      (rc = st.up(da, (const int*)assign, n)) || (rc = st.up(dm, mps, nmp)) || (rc = st.up(dc, cam, 1)) ||
      (rc = st.up(dout, (const uint8_t*)outlier, n)) ||
      (rc = orbm_pose_optimization_batch(m, dk, dn, (int)kp, uright ? (float*)du : nullptr, da, dm, (int*)dn + 1,
                                         (int)np, inv_sigma2, nlevels, dc, 1, flags, dT, dp,
                                         outlier ? (uint8_t*)dout : nullptr, dr, st.st)) ||
      (Tcw && (rc = st.down(Tcw, dT, 12))) || (pose && (rc = st.down(pose, dp, 1))) ||
      (outlier && (rc = st.down(outlier, dout, n))) || (result && (rc = st.down(result, dr, 1))) ||
      ((flags & ORBM_POSEOPT_DISCARD_OUTLIERS) && (rc = st.down(assign, da, n))) || (rc = st.finish()))
    return rc;
  return ORBX_OK;
}

// ---------------------------------------------------------------- Sim3Solver
namespace {
int sim3_check(const orbx_kp* kps1, int n1, const orbx_kp* kps2, int n2, const orbm_map_point_world* mps1,
               const orbm_map_point_world* mps2, const orbm_camera* cam1, const orbm_camera* cam2, const int* match12,
               const float* level_sigma2, int nlevels, const orbm_sim3_params* P, const uint32_t* rand3) {
  if (n1 < 0 || n2 < 0 || !cam1 || !cam2 || !level_sigma2 || nlevels < 1 || nlevels > kMaxLevels || !P || !rand3 ||
      (n1 && (!kps1 || !mps1 || !match12)) || (n2 && (!kps2 || !mps2)) || P->first_iteration < 0 || P->min_inliers < 0)
    return g_merr.fail(ORBX_EINVAL, "bad argument");
  if (P->max_iterations < 1 || P->max_iterations > kSim3MaxIts)
    return g_merr.fail(ORBX_ECAPACITY, "max_iterations %d outside 1..%d", P->max_iterations, kSim3MaxIts);
  return ORBX_OK;
}
}  // namespace

int orbm_sim3_ransac_host(const orbx_kp* kps1, int n1, const orbx_kp* kps2, int n2, const orbm_map_point_world* mps1,
                          const orbm_map_point_world* mps2, const orbm_camera* cam1, const orbm_camera* cam2,
                          const int* match12, const int* kp_index1, const float* level_sigma2, int nlevels,
                          const orbm_sim3_params* params, const uint32_t* rand3, orbm_sim3_result* result, float* s12,
                          float* R12, float* t12, orbm_pose* pose, uint8_t* inlier, orbm_sim3_hyp* hyp, int* status) {
  int rc;
  if ((rc = sim3_check(kps1, n1, kps2, n2, mps1, mps2, cam1, cam2, match12, level_sigma2, nlevels, params, rand3)))
    return rc;
  return sim3_ransac_host(kps1, n1, kps2, n2, mps1, mps2, cam1, cam2, match12, kp_index1, level_sigma2, nlevels, params,
                          rand3, result, s12, R12, t12, pose, inlier, hyp, status);
}

int orbm_sim3_ransac_batch(orbm_handle m, const orbx_kp* d_kps1, const int* d_n1, const orbx_kp* d_kps2,
                           const int* d_n2, int kp_pitch, const orbm_map_point_world* d_mps1,
                           const orbm_map_point_world* d_mps2, int mp_pitch, const orbm_camera* d_cam1,
                           const orbm_camera* d_cam2, const int* d_match12, const int* d_kp_index1,
                           const float* level_sigma2, int nlevels, const orbm_sim3_params* params,
                           const uint32_t* d_rand3, int pairs, orbm_sim3_result* d_result, float* d_s12, float* d_R12,
                           float* d_t12, orbm_pose* d_pose, uint8_t* d_inlier, orbm_sim3_hyp* d_hyp, void* stream) {
  if (!m || !d_kps1 || !d_n1 || !d_kps2 || !d_n2 || !d_mps1 || !d_mps2 || !d_cam1 || !d_cam2 || !d_match12 ||
      !level_sigma2 || !params || !d_rand3 || pairs < 1 || kp_pitch < 1 || mp_pitch < kp_pitch || nlevels < 1 ||
      nlevels > kMaxLevels || params->first_iteration < 0 || params->min_inliers < 0)
    return g_merr.fail(ORBX_EINVAL, "bad argument");
  if (params->max_iterations < 1 || params->max_iterations > kSim3MaxIts)
    return g_merr.fail(ORBX_ECAPACITY, "max_iterations %d outside 1..%d", params->max_iterations, kSim3MaxIts);
  if (kp_pitch > m->max_kps)
    return g_merr.fail(ORBX_ECAPACITY, "kp_pitch %d above the handle's max_kps %d", kp_pitch, m->max_kps);
  HIP_OK(g_merr, hipSetDevice(m->device));
  hipStream_t s = (hipStream_t)stream;
  size_t hyp_bytes, rec_bytes;
  sim3_ws_bytes(kp_pitch, pairs, params->max_iterations, &hyp_bytes, &rec_bytes);
  const size_t need = hyp_bytes + rec_bytes, tab_n = (size_t)kp_pitch + 1;
  // the workspace and the iteration table are the handle's: after their last user, whatever its stream
  if (m->ws.before(s)) return g_merr.fail(ORBX_EDEVICE, "stream wait on the workspace failed");
  const bool new_tab = m->sim3_tab_host.size() < tab_n || m->sim3_prob != params->probability ||
                       m->sim3_min_inliers != params->min_inliers || m->sim3_max_iterations != params->max_iterations;
  if (m->sim3_ws.n < need || new_tab) {
    // replaced memory and a rewritten host table must not be in use: wait for the last user
    if (m->ws.ev) HIP_OK(g_merr, hipEventSynchronize(m->ws.ev));
    if (m->sim3_ws.reserve(need) != hipSuccess) return g_merr.fail(ORBX_ENOMEM, "Sim3 workspace");
  }
  if (new_tab) {
    // SetRansacParameters with the host's libm, one entry per count the pitch allows
    const size_t n = std::max(tab_n, m->sim3_tab_host.size());
    m->sim3_tab_host.resize(n);
    for (size_t N = 0; N < n; ++N)
      m->sim3_tab_host[N] = sim3_iterations(params->probability, params->min_inliers, params->max_iterations, (int)N);
    m->sim3_prob = params->probability;
    m->sim3_min_inliers = params->min_inliers;
    m->sim3_max_iterations = params->max_iterations;
    if (m->sim3_tab.reserve(n * sizeof(int)) != hipSuccess) return g_merr.fail(ORBX_ENOMEM, "Sim3 iteration table");
    HIP_OK(g_merr, hipMemcpyAsync(m->sim3_tab.p, m->sim3_tab_host.data(), n * sizeof(int), hipMemcpyHostToDevice, s));
  }
  Sim3LaunchArgs A{};
  A.kps1 = d_kps1;
  A.kps2 = d_kps2;
  A.n1 = d_n1;
  A.n2 = d_n2;
  A.kp_pitch = kp_pitch;
  A.mp_pitch = mp_pitch;
  A.mps1 = d_mps1;
  A.mps2 = d_mps2;
  A.cam1 = d_cam1;
  A.cam2 = d_cam2;
  A.match12 = d_match12;
  A.kp_index1 = d_kp_index1;
  A.level_sigma2 = level_sigma2;
  A.nlevels = nlevels;
  A.params = *params;
  A.its_tab = m->sim3_tab.as<int>();
  A.rand3 = d_rand3;
  A.pairs = pairs;
  A.result = d_result;
  A.s12 = d_s12;
  A.R12 = d_R12;
  A.t12 = d_t12;
  A.pose = d_pose;
  A.inlier = d_inlier;
  A.hyp = d_hyp;
  A.err = m->err.as<int>();
  if (launch_sim3_ransac(A, m->sim3_ws.p, stream))
    return g_merr.fail(ORBX_EDEVICE, "Sim3 launch: %s", hipGetErrorString(hipGetLastError()));
  if (m->ws.after(s) || m->errm.mark(s)) return g_merr.fail(ORBX_EDEVICE, "event record failed");
  return ORBX_OK;
}

int orbm_sim3_ransac(orbm_handle m, const orbx_kp* kps1, int n1, const orbx_kp* kps2, int n2,
                     const orbm_map_point_world* mps1, const orbm_map_point_world* mps2, const orbm_camera* cam1,
                     const orbm_camera* cam2, const int* match12, const int* kp_index1, const float* level_sigma2,
                     int nlevels, const orbm_sim3_params* params, const uint32_t* rand3, orbm_sim3_result* result,
                     float* s12, float* R12, float* t12, orbm_pose* pose, uint8_t* inlier, orbm_sim3_hyp* hyp) {
  int rc;
  if (!m) return g_merr.fail(ORBX_EINVAL, "bad argument");
  if ((rc = sim3_check(kps1, n1, kps2, n2, mps1, mps2, cam1, cam2, match12, level_sigma2, nlevels, params, rand3)))
    return rc;
  if (std::max(n1, n2) > m->max_kps)
    return g_merr.fail(ORBX_ECAPACITY, "%d keypoints above the handle's max_kps %d", std::max(n1, n2), m->max_kps);
  HIP_OK(g_merr, hipSetDevice(m->device));
  const size_t kp = std::max(std::max(n1, n2), 1), its = params->max_iterations;
  Stage st(m);
  auto dk1 = st.slot<orbx_kp>(kp);
  auto dk2 = st.slot<orbx_kp>(kp);
  auto dn = st.slot<int>(2);
  auto dm1 = st.slot<orbm_map_point_world>(kp);
  auto dm2 = st.slot<orbm_map_point_world>(kp);
  auto dc = st.slot<orbm_camera>(2);
  auto d12 = st.slot<int>(kp);
  auto dki = st.slot<int>(kp);
  auto drand = st.slot<uint32_t>(3 * its);
  auto dres = st.slot<orbm_sim3_result>(1);
  auto dsrt = st.slot<float>(13);
  auto dpose = st.slot<orbm_pose>(2);
  auto din = st.slot<uint8_t>(kp);
  auto dhyp = st.slot<orbm_sim3_hyp>(its);
  const int counts[2] = {n1, n2};
  const orbm_camera cams[2] = {*cam1, *cam2};
  // s12, R12, t12, pose and hyp go up too: what the call leaves untouched comes back as it was
  float srt[13] = {};
  if (s12) srt[0] = *s12;
  if (R12) std::memcpy(srt + 1, R12, 9 * sizeof(float));
  if (t12) std::memcpy(srt + 10, t12, 3 * sizeof(float));
  if ((rc = st.reserve()) || (rc = st.up(dk1, kps1, n1)) || (rc = st.up(dk2, kps2, n2)) ||
      (rc = st.up(dn, counts, 2)) || (rc = st.up(dm1, mps1, n1)) || (rc = st.up(dm2, mps2, n2)) ||
      (rc = st.up(dc, cams, 2)) || (rc = st.up(d12, match12, n1)) || (rc = st.up(dki, kp_index1, n1)) ||
      (rc = st.up(drand, rand3, 3 * its)) || (rc = st.up(dsrt, (const float*)srt, 13)) ||
      (rc = st.up(dpose, (const orbm_pose*)pose, 2)) || (rc = st.up(dhyp, (const orbm_sim3_hyp*)hyp, its)) ||
      (rc = orbm_sim3_ransac_batch(m, dk1, dn, dk2, (int*)dn + 1, (int)kp, dm1, dm2, (int)kp, dc,
                                   (orbm_camera*)dc + 1, d12, kp_index1 ? (int*)dki : nullptr, level_sigma2, nlevels,
                                   params, drand, 1, dres, dsrt, (float*)dsrt + 1, (float*)dsrt + 10,
                                   pose ? (orbm_pose*)dpose : nullptr, inlier ? (uint8_t*)din : nullptr,
                                   hyp ? (orbm_sim3_hyp*)dhyp : nullptr, st.st)) ||
      (rc = st.down(srt, dsrt, 13)) || (result && (rc = st.down(result, dres, 1))) ||
      (pose && (rc = st.down(pose, dpose, 2))) || (inlier && (rc = st.down(inlier, din, n1))) ||
      (hyp && (rc = st.down(hyp, dhyp, its))) || (rc = st.finish()))
    return rc;
  if (s12) *s12 = srt[0];
  if (R12) std::memcpy(R12, srt + 1, 9 * sizeof(float));
  if (t12) std::memcpy(t12, srt + 10, 3 * sizeof(float));
  return ORBX_OK;
}

// ------------------------------------------------- Optimizer::OptimizeSim3
namespace {
int optsim3_check(const orbx_kp* kps1, int n1, const orbx_kp* kps2, int n2, const orbm_map_point_world* mps1,
                  const orbm_map_point_world* mps2, const orbm_camera* cam1, const orbm_camera* cam2,
                  const int* match12, const int* found12, const int* found21, const float* inv_sigma2, int nlevels,
                  const float* s12, const float* R12, const float* t12, float th2) {
  if (n1 < 0 || n2 < 0 || !cam1 || !cam2 || !inv_sigma2 || nlevels < 1 || nlevels > kMaxLevels || !s12 || !R12 ||
      !t12 || !(th2 >= 0.0f) || (n1 && (!kps1 || !mps1 || !match12)) || (n2 && (!kps2 || !mps2)) ||
      (found12 != nullptr) != (found21 != nullptr))
    return g_merr.fail(ORBX_EINVAL, "bad argument");
  return ORBX_OK;
}
}  // namespace

int orbm_optimize_sim3_host(const orbx_kp* kps1, int n1, const orbx_kp* kps2, int n2, const orbm_map_point_world* mps1,
                            const orbm_map_point_world* mps2, const orbm_camera* cam1, const orbm_camera* cam2,
                            const int* match12, const uint8_t* inlier, const int* found12, const int* found21,
                            const float* inv_sigma2, int nlevels, const float* s12, const float* R12,
                            const float* t12, float th2, int fix_scale, int* match12_out, double* S12, float* Scw,
                            orbm_pose* pose, orbm_optsim3_result* result, double* lin, int* status) {
  int rc;
  if ((rc = optsim3_check(kps1, n1, kps2, n2, mps1, mps2, cam1, cam2, match12, found12, found21, inv_sigma2, nlevels,
                          s12, R12, t12, th2)))
    return rc;
  // found lists of an empty keyframe may be absent: nothing is read from them
  OptSim3Args A{};
  A.kps1 = kps1;
  A.kps2 = kps2;
  A.mps1 = mps1;
  A.mps2 = mps2;
  A.cam1 = cam1;
  A.cam2 = cam2;
  A.match12 = match12;
  A.inlier = inlier;
  A.found12 = found12;
  A.found21 = found21;
  A.inv_sigma2 = inv_sigma2;
  A.nlevels = nlevels;
  A.s12 = s12;
  A.R12 = R12;
  A.t12 = t12;
  A.th2 = th2;
  A.fix_scale = fix_scale;
  A.pairs = 1;
  A.match12_out = match12_out;
  A.S12 = S12;
  A.Scw = Scw;
  A.pose = pose;
  A.result = result;
  A.lin = lin;
  return optimize_sim3_host(A, n1, n2, status);
}

int orbm_optimize_sim3_batch(orbm_handle m, const orbx_kp* d_kps1, const int* d_n1, const orbx_kp* d_kps2,
                             const int* d_n2, int kp_pitch, const orbm_map_point_world* d_mps1,
                             const orbm_map_point_world* d_mps2, int mp_pitch, const orbm_camera* d_cam1,
                             const orbm_camera* d_cam2, const int* d_match12, const uint8_t* d_inlier,
                             const int* d_found12, const int* d_found21, const float* inv_sigma2, int nlevels,
                             const float* d_s12, const float* d_R12, const float* d_t12, float th2, int fix_scale,
                             int pairs, int* d_match12_out, double* d_S12, float* d_Scw, orbm_pose* d_pose,
                             orbm_optsim3_result* d_result, double* d_lin, void* stream) {
  if (!m || !d_kps1 || !d_n1 || !d_kps2 || !d_n2 || !d_mps1 || !d_mps2 || !d_cam1 || !d_cam2 || !d_match12 ||
      !inv_sigma2 || !d_s12 || !d_R12 || !d_t12 || !(th2 >= 0.0f) || pairs < 1 || kp_pitch < 1 ||
      mp_pitch < kp_pitch || nlevels < 1 || nlevels > kMaxLevels || (d_found12 != nullptr) != (d_found21 != nullptr))
    return g_merr.fail(ORBX_EINVAL, "bad argument");
  if (kp_pitch > m->max_kps)
    return g_merr.fail(ORBX_ECAPACITY, "kp_pitch %d above the handle's max_kps %d", kp_pitch, m->max_kps);
  HIP_OK(g_merr, hipSetDevice(m->device));
  hipStream_t s = (hipStream_t)stream;
  const size_t need = optsim3_ws_bytes(kp_pitch, pairs);
  if (need) {
    // the workspace is the handle's: after its last user, whatever its stream
    if (m->ws.before(s)) return g_merr.fail(ORBX_EDEVICE, "stream wait on the workspace failed");
    if (m->os3_ws.n < need) {
      if (m->ws.ev) HIP_OK(g_merr, hipEventSynchronize(m->ws.ev));
      if (m->os3_ws.reserve(need) != hipSuccess) return g_merr.fail(ORBX_ENOMEM, "OptimizeSim3 workspace");
    }
  }
  OptSim3Args A{};
  A.kps1 = d_kps1;
  A.kps2 = d_kps2;
  A.n1 = d_n1;
  A.n2 = d_n2;
  A.kp_pitch = kp_pitch;
  A.mp_pitch = mp_pitch;
  A.mps1 = d_mps1;
  A.mps2 = d_mps2;
  A.cam1 = d_cam1;
  A.cam2 = d_cam2;
  A.match12 = d_match12;
  A.inlier = d_inlier;
  A.found12 = d_found12;
  A.found21 = d_found21;
  A.inv_sigma2 = inv_sigma2;
  A.nlevels = nlevels;
  A.s12 = d_s12;
  A.R12 = d_R12;
  A.t12 = d_t12;
  A.th2 = th2;
  A.fix_scale = fix_scale;
  A.pairs = pairs;
  A.match12_out = d_match12_out;
  A.S12 = d_S12;
  A.Scw = d_Scw;
  A.pose = d_pose;
  A.result = d_result;
  A.lin = d_lin;
  A.err = m->err.as<int>();
  if (launch_optimize_sim3(A, need ? m->os3_ws.p : nullptr, stream))
    return g_merr.fail(ORBX_EDEVICE, "OptimizeSim3 launch: %s", hipGetErrorString(hipGetLastError()));
  if ((need && m->ws.after(s)) || m->errm.mark(s)) return g_merr.fail(ORBX_EDEVICE, "event record failed");
  return ORBX_OK;
}

int orbm_optimize_sim3(orbm_handle m, const orbx_kp* kps1, int n1, const orbx_kp* kps2, int n2,
                       const orbm_map_point_world* mps1, const orbm_map_point_world* mps2, const orbm_camera* cam1,
                       const orbm_camera* cam2, const int* match12, const uint8_t* inlier, const int* found12,
                       const int* found21, const float* inv_sigma2, int nlevels, const float* s12, const float* R12,
                       const float* t12, float th2, int fix_scale, int* match12_out, double* S12, float* Scw,
                       orbm_pose* pose, orbm_optsim3_result* result, double* lin) {
  int rc;
  if (!m) return g_merr.fail(ORBX_EINVAL, "bad argument");
  if ((rc = optsim3_check(kps1, n1, kps2, n2, mps1, mps2, cam1, cam2, match12, found12, found21, inv_sigma2, nlevels,
                          s12, R12, t12, th2)))
    return rc;
  if (std::max(n1, n2) > m->max_kps)
    return g_merr.fail(ORBX_ECAPACITY, "%d keypoints above the handle's max_kps %d", std::max(n1, n2), m->max_kps);
  HIP_OK(g_merr, hipSetDevice(m->device));
  const size_t kp = std::max(std::max(n1, n2), 1);
  Stage st(m);
  auto dk1 = st.slot<orbx_kp>(kp);
  auto dk2 = st.slot<orbx_kp>(kp);
  auto dn = st.slot<int>(2);
  auto dm1 = st.slot<orbm_map_point_world>(kp);
  auto dm2 = st.slot<orbm_map_point_world>(kp);
  auto dc = st.slot<orbm_camera>(2);
  auto d12 = st.slot<int>(kp);
  auto din = st.slot<uint8_t>(kp);
  auto df12 = st.slot<int>(kp);
  auto df21 = st.slot<int>(kp);
  auto dsrt = st.slot<float>(13);
  auto dout = st.slot<int>(kp);
  auto dS = st.slot<double>(8);
  auto dScw = st.slot<float>(12);
  auto dpose = st.slot<orbm_pose>(1);
  auto dres = st.slot<orbm_optsim3_result>(1);
  auto dlin = st.slot<double>(kOs3Sums);
  const int counts[2] = {n1, n2};
  const orbm_camera cams[2] = {*cam1, *cam2};
  float srt[13];
  srt[0] = *s12;
  std::memcpy(srt + 1, R12, 9 * sizeof(float));
  std::memcpy(srt + 10, t12, 3 * sizeof(float));
  if ((rc = st.reserve()) || (rc = st.up(dk1, kps1, n1)) || (rc = st.up(dk2, kps2, n2)) ||
      (rc = st.up(dn, counts, 2)) || (rc = st.up(dm1, mps1, n1)) || (rc = st.up(dm2, mps2, n2)) ||
      (rc = st.up(dc, cams, 2)) || (rc = st.up(d12, match12, n1)) || (rc = st.up(din, inlier, n1)) ||
      (rc = st.up(df12, found12, n1)) || (rc = st.up(df21, found21, n2)) ||
      (rc = st.up(dsrt, (const float*)srt, 13)) ||
      (rc = orbm_optimize_sim3_batch(m, dk1, dn, dk2, (int*)dn + 1, (int)kp, dm1, dm2, (int)kp, dc,
                                     (orbm_camera*)dc + 1, d12, inlier ? (uint8_t*)din : nullptr,
                                     found12 ? (int*)df12 : nullptr, found21 ? (int*)df21 : nullptr, inv_sigma2,
                                     nlevels, dsrt, (float*)dsrt + 1, (float*)dsrt + 10, th2, fix_scale, 1,
                                     match12_out ? (int*)dout : nullptr, dS, dScw, dpose, dres,
                                     lin ? (double*)dlin : nullptr, st.st)) ||
      (match12_out && (rc = st.down(match12_out, dout, n1))) || (S12 && (rc = st.down(S12, dS, 8))) ||
      (Scw && (rc = st.down(Scw, dScw, 12))) || (pose && (rc = st.down(pose, dpose, 1))) ||
      (result && (rc = st.down(result, dres, 1))) || (lin && (rc = st.down(lin, dlin, kOs3Sums))) ||
      (rc = st.finish()))
    return rc;
  return ORBX_OK;
}

// ---------------------------------------------------------------- Initializer
namespace {
int initz_check(const orbx_kp* kps1, int n1, const orbx_kp* kps2, int n2, const int* matches12, const orbm_camera* cam,
                const orbm_init_params* P, const uint32_t* rand8) {
  if (n1 < 0 || n2 < 0 || !cam || !P || !rand8 || (n1 && (!kps1 || !matches12)) || (n2 && !kps2))
    return g_merr.fail(ORBX_EINVAL, "bad argument");
  if (P->max_iterations < 1 || P->max_iterations > kInitzMaxIts)
    return g_merr.fail(ORBX_ECAPACITY, "max_iterations %d outside 1..%d", P->max_iterations, kInitzMaxIts);
  return ORBX_OK;
}
}  // namespace

int orbm_initialize_host(const orbx_kp* kps1, int n1, const orbx_kp* kps2, int n2, const int* matches12,
                         const orbm_camera* cam, const orbm_init_params* params, const uint32_t* rand8,
                         orbm_init_result* result, float* R21, float* t21, float* Tcw, float* p3d,
                         uint8_t* triangulated, int* matches12_out, uint8_t* inlier_h, uint8_t* inlier_f, float* T1,
                         float* T2, float* H21, float* F21, orbm_init_hyp* hyp, orbm_init_rt* rt, int* status) {
  int rc;
  if ((rc = initz_check(kps1, n1, kps2, n2, matches12, cam, params, rand8))) return rc;
  return initialize_host(kps1, n1, kps2, n2, matches12, cam, params, rand8, result, R21, t21, Tcw, p3d, triangulated,
                         matches12_out, inlier_h, inlier_f, T1, T2, H21, F21, hyp, rt, status);
}

int orbm_initialize_batch(orbm_handle m, const orbx_kp* d_kps1, const int* d_n1, const orbx_kp* d_kps2,
                          const int* d_n2, int kp_pitch, const int* d_matches12, const orbm_camera* d_cam,
                          const orbm_init_params* params, const uint32_t* d_rand8, int pairs,
                          orbm_init_result* d_result, float* d_R21, float* d_t21, float* d_Tcw, float* d_p3d,
                          uint8_t* d_triangulated, int* d_matches12_out, uint8_t* d_inlier_h, uint8_t* d_inlier_f,
                          float* d_T1, float* d_T2, float* d_H21, float* d_F21, orbm_init_hyp* d_hyp,
                          orbm_init_rt* d_rt, void* stream) {
  if (!m || !d_kps1 || !d_n1 || !d_kps2 || !d_n2 || !d_matches12 || !d_cam || !params || !d_rand8 || pairs < 1 ||
      kp_pitch < 1)
    return g_merr.fail(ORBX_EINVAL, "bad argument");
  if (params->max_iterations < 1 || params->max_iterations > kInitzMaxIts)
    return g_merr.fail(ORBX_ECAPACITY, "max_iterations %d outside 1..%d", params->max_iterations, kInitzMaxIts);
  if (kp_pitch > m->max_kps)
    return g_merr.fail(ORBX_ECAPACITY, "kp_pitch %d above the handle's max_kps %d", kp_pitch, m->max_kps);
  if (pairs > 65535) return g_merr.fail(ORBX_ECAPACITY, "%d pairs above 65535", pairs);
  HIP_OK(g_merr, hipSetDevice(m->device));
  hipStream_t s = (hipStream_t)stream;
  const size_t need = initializer_ws_bytes(kp_pitch, pairs, params->max_iterations);
  // the workspace is the handle's: after its last user, whatever its stream
  if (m->ws.before(s)) return g_merr.fail(ORBX_EDEVICE, "stream wait on the workspace failed");
  if (m->initz_ws.n < need) {
    // replaced memory must not be in use: wait for the last user
    if (m->ws.ev) HIP_OK(g_merr, hipEventSynchronize(m->ws.ev));
    if (m->initz_ws.reserve(need) != hipSuccess) return g_merr.fail(ORBX_ENOMEM, "Initializer workspace");
  }
  InitzLaunchArgs A{};
  A.kps1 = d_kps1;
  A.kps2 = d_kps2;
  A.n1 = d_n1;
  A.n2 = d_n2;
  A.kp_pitch = kp_pitch;
  A.matches12 = d_matches12;
  A.cam = d_cam;
  A.params = *params;
  A.rand8 = d_rand8;
  A.pairs = pairs;
  A.result = d_result;
  A.R21 = d_R21;
  A.t21 = d_t21;
  A.Tcw = d_Tcw;
  A.p3d = d_p3d;
  A.triangulated = d_triangulated;
  A.matches12_out = d_matches12_out;
  A.inlier_h = d_inlier_h;
  A.inlier_f = d_inlier_f;
  A.T1 = d_T1;
  A.T2 = d_T2;
  A.H21 = d_H21;
  A.F21 = d_F21;
  A.hyp = d_hyp;
  A.rt = d_rt;
  A.err = m->err.as<int>();
  if (launch_initialize(A, m->initz_ws.p, stream))
    return g_merr.fail(ORBX_EDEVICE, "Initializer launch: %s", hipGetErrorString(hipGetLastError()));
  if (m->ws.after(s) || m->errm.mark(s)) return g_merr.fail(ORBX_EDEVICE, "event record failed");
  return ORBX_OK;
}

int orbm_initialize(orbm_handle m, const orbx_kp* kps1, int n1, const orbx_kp* kps2, int n2, const int* matches12,
                    const orbm_camera* cam, const orbm_init_params* params, const uint32_t* rand8,
                    orbm_init_result* result, float* R21, float* t21, float* Tcw, float* p3d, uint8_t* triangulated,
                    int* matches12_out, uint8_t* inlier_h, uint8_t* inlier_f, float* T1, float* T2, float* H21,
                    float* F21, orbm_init_hyp* hyp, orbm_init_rt* rt) {
  int rc;
  if (!m) return g_merr.fail(ORBX_EINVAL, "bad argument");
  if ((rc = initz_check(kps1, n1, kps2, n2, matches12, cam, params, rand8))) return rc;
  if (std::max(n1, n2) > m->max_kps)
    return g_merr.fail(ORBX_ECAPACITY, "%d keypoints above the handle's max_kps %d", std::max(n1, n2), m->max_kps);
  HIP_OK(g_merr, hipSetDevice(m->device));
  const size_t kp = std::max(std::max(n1, n2), 1), its = params->max_iterations;
  Stage st(m);
  auto dk1 = st.slot<orbx_kp>(kp);
  auto dk2 = st.slot<orbx_kp>(kp);
  auto dn = st.slot<int>(2);
  auto d12 = st.slot<int>(kp);
  auto dc = st.slot<orbm_camera>(1);
  auto drand = st.slot<uint32_t>(8 * its);
  auto dres = st.slot<orbm_init_result>(1);
  auto dmat = st.slot<float>(60);  // R21 9, t21 3, Tcw 12, T1 9, T2 9, H21 9, F21 9
  auto dp3 = st.slot<float>(3 * kp);
  auto dtri = st.slot<uint8_t>(kp);
  auto dout = st.slot<int>(kp);
  auto dih = st.slot<uint8_t>(kp);
  auto dif = st.slot<uint8_t>(kp);
  auto dhyp = st.slot<orbm_init_hyp>(2 * its);
  auto drt = st.slot<orbm_init_rt>(8);
  const int counts[2] = {n1, n2};
  // the outputs go up too: what the call leaves untouched comes back as it was
  float mat[60] = {};
  float* const mp[7] = {R21, t21, Tcw, T1, T2, H21, F21};
  const int mo[8] = {0, 9, 12, 24, 33, 42, 51, 60};
  for (int k = 0; k < 7; ++k)
    if (mp[k]) std::memcpy(mat + mo[k], mp[k], (mo[k + 1] - mo[k]) * sizeof(float));
  float* dm = dmat;
  if ((rc = st.reserve())) return rc;
  dm = dmat;
  if ((rc = st.up(dk1, kps1, n1)) || (rc = st.up(dk2, kps2, n2)) || (rc = st.up(dn, counts, 2)) ||
      (rc = st.up(d12, matches12, n1)) || (rc = st.up(dc, cam, 1)) || (rc = st.up(drand, rand8, 8 * its)) ||
      (rc = st.up(dres, (const orbm_init_result*)result, 1)) || (rc = st.up(dmat, (const float*)mat, 60)) ||
      (rc = st.up(dp3, (const float*)p3d, 3 * (size_t)n1)) || (rc = st.up(dtri, (const uint8_t*)triangulated, n1)) ||
      (rc = st.up(dout, (const int*)matches12_out, n1)) || (rc = st.up(dih, (const uint8_t*)inlier_h, n1)) ||
      (rc = st.up(dif, (const uint8_t*)inlier_f, n1)) || (rc = st.up(dhyp, (const orbm_init_hyp*)hyp, 2 * its)) ||
      (rc = st.up(drt, (const orbm_init_rt*)rt, 8)) ||
      (rc = orbm_initialize_batch(m, dk1, dn, dk2, (int*)dn + 1, (int)kp, d12, dc, params, drand, 1, dres, dm, dm + 9,
                                  dm + 12, p3d ? (float*)dp3 : nullptr, triangulated ? (uint8_t*)dtri : nullptr,
                                  matches12_out ? (int*)dout : nullptr, inlier_h ? (uint8_t*)dih : nullptr,
                                  inlier_f ? (uint8_t*)dif : nullptr, dm + 24, dm + 33, dm + 42, dm + 51,
                                  hyp ? (orbm_init_hyp*)dhyp : nullptr, rt ? (orbm_init_rt*)drt : nullptr, st.st)) ||
      (rc = st.down(mat, dmat, 60)) || (result && (rc = st.down(result, dres, 1))) ||
      (p3d && (rc = st.down(p3d, dp3, 3 * (size_t)n1))) || (triangulated && (rc = st.down(triangulated, dtri, n1))) ||
      (matches12_out && (rc = st.down(matches12_out, dout, n1))) || (inlier_h && (rc = st.down(inlier_h, dih, n1))) ||
      (inlier_f && (rc = st.down(inlier_f, dif, n1))) || (hyp && (rc = st.down(hyp, dhyp, 2 * its))) ||
      (rt && (rc = st.down(rt, drt, 8))) || (rc = st.finish()))
    return rc;
  for (int k = 0; k < 7; ++k)
    if (mp[k]) std::memcpy(mp[k], mat + mo[k], (mo[k + 1] - mo[k]) * sizeof(float));
  return ORBX_OK;
}

// ------------------------------------- LocalMapping::CreateNewMapPoints
int orbm_compute_f12(const orbm_camera* cam1, const orbm_camera* cam2, float* F12) {
  if (!cam1 || !cam2 || !F12) return g_merr.fail(ORBX_EINVAL, "bad argument");
  compute_f12_host(*cam1, *cam2, F12);
  return ORBX_OK;
}

int orbm_prepare_new_points(const orbm_camera* cam1, const orbm_camera* cam2, float scale_factor, uint32_t kf1,
                            uint32_t kf2, uint32_t desc_base1, uint32_t desc_base2, int kf2_first,
                            orbm_newpt_pair* out) {
  if (!cam1 || !cam2 || !out) return g_merr.fail(ORBX_EINVAL, "bad argument");
  newpt_prepare(*cam1, *cam2, scale_factor, kf1, kf2, desc_base1, desc_base2, kf2_first, out);
  return ORBX_OK;
}

namespace {
int newpt_check(const orbm_newpt_pair* pair, const orbx_kp* kps1, const float* uright1, const float* depth1, int n1,
                const orbx_kp* kps2, const float* uright2, const float* depth2, int n2, const float* level_sigma2,
                const float* scale_factors, int nlevels, const int* matches12, float* pos, uint8_t* reason) {
  if (!pair || n1 < 0 || n2 < 0 || !level_sigma2 || !scale_factors || nlevels < 1 || nlevels > kMaxLevels)
    return g_merr.fail(ORBX_EINVAL, "bad argument");
  if (n1 && (!kps1 || !uright1 || !depth1 || !matches12 || !pos || !reason))
    return g_merr.fail(ORBX_EINVAL, "null array");
  if (n2 && (!kps2 || !uright2 || !depth2)) return g_merr.fail(ORBX_EINVAL, "null array");
  return ORBX_OK;
}
}  // namespace

int orbm_create_new_map_points_host(const orbm_newpt_pair* pair, const orbx_kp* kps1, const orbx_kp* kps_raw1,
                                    const float* uright1, const float* depth1, int n1, const orbx_kp* kps2,
                                    const orbx_kp* kps_raw2, const float* uright2, const float* depth2, int n2,
                                    const float* level_sigma2, const float* scale_factors, int nlevels,
                                    const int* matches12, float* pos, uint8_t* reason, int* nnew, int* status) {
  int rc;
  if ((rc = newpt_check(pair, kps1, uright1, depth1, n1, kps2, uright2, depth2, n2, level_sigma2, scale_factors,
                        nlevels, matches12, pos, reason)))
    return rc;
  return create_new_map_points_host(*pair, kps1, kps_raw1, uright1, depth1, n1, kps2, kps_raw2, uright2, depth2, n2,
                                    level_sigma2, scale_factors, nlevels, matches12, pos, reason, nnew, status);
}

int orbm_create_new_map_points_batch(orbm_handle m, const orbx_kp* d_kps1, const orbx_kp* d_kps_raw1,
                                     const float* d_uright1, const float* d_depth1, const int* d_n1, int kp_pitch1,
                                     const orbx_kp* d_kps2, const orbx_kp* d_kps_raw2, const float* d_uright2,
                                     const float* d_depth2, const int* d_n2, int kp_pitch2,
                                     const orbm_newpt_pair* d_pairs, const float* level_sigma2,
                                     const float* scale_factors, int nlevels, int pairs, const int* d_matches12,
                                     int out_pitch, int dedup, float* d_pos, uint8_t* d_reason, orbm_new_point* d_new,
                                     int capacity, int* d_nnew, int* d_nnew_pair, const orbm_newpt_emit* emit,
                                     uint8_t* d_has_mp1, uint8_t* d_has_mp2, void* stream) {
  if (!m || !d_kps1 || !d_uright1 || !d_depth1 || !d_n1 || !d_kps2 || !d_uright2 || !d_depth2 || !d_n2 || !d_pairs ||
      !level_sigma2 || !scale_factors || !d_matches12 || !d_pos || !d_reason || !d_nnew || !d_nnew_pair ||
      pairs < 1 || kp_pitch1 < 0 || kp_pitch2 < 1 || out_pitch < 1 || capacity < 0 || nlevels < 1 ||
      nlevels > kMaxLevels)
    return g_merr.fail(ORBX_EINVAL, "bad argument");
  if (emit && (!emit->d_mps || !emit->d_obs || !emit->d_obs_off || !emit->d_point_ids || !emit->d_ref))
    return g_merr.fail(ORBX_EINVAL, "the emit arguments need all five arrays");
  HIP_OK(g_merr, hipSetDevice(m->device));
  hipStream_t s = (hipStream_t)stream;
  NewPtArgs A{};
  A.kps1 = d_kps1;
  A.raw1 = d_kps_raw1;
  A.ur1 = d_uright1;
  A.dp1 = d_depth1;
  A.n1 = d_n1;
  A.kp_pitch1 = kp_pitch1;
  A.kps2 = d_kps2;
  A.raw2 = d_kps_raw2;
  A.ur2 = d_uright2;
  A.dp2 = d_depth2;
  A.n2 = d_n2;
  A.kp_pitch2 = kp_pitch2;
  std::memcpy(A.sigma2, level_sigma2, (size_t)nlevels * sizeof(float));
  std::memcpy(A.scale, scale_factors, (size_t)nlevels * sizeof(float));
  A.nlevels = nlevels;
  A.npairs = pairs;
  A.matches12 = d_matches12;
  A.out_pitch = out_pitch;
  A.dedup = dedup;
  A.pos = d_pos;
  A.reason = d_reason;
  A.out_new = d_new;
  A.capacity = capacity;
  A.nnew = d_nnew;
  A.nnew_pair = d_nnew_pair;
  if (emit) A.emit = *emit;
  A.has_emit = emit ? 1 : 0;
  A.has_mp1 = d_has_mp1;
  A.has_mp2 = d_has_mp2;
  A.err = m->err.as<int>();
  if (const int e = launch_new_points(A, d_pairs, stream))
    return g_merr.fail(ORBX_EDEVICE, "CreateNewMapPoints launch: %s", hipGetErrorString((hipError_t)e));
  if (m->errm.mark(s)) return g_merr.fail(ORBX_EDEVICE, "event record failed");
  return ORBX_OK;
}

int orbm_create_new_map_points(orbm_handle m, const orbm_newpt_pair* pair, const orbx_kp* kps1,
                               const orbx_kp* kps_raw1, const float* uright1, const float* depth1, int n1,
                               const orbx_kp* kps2, const orbx_kp* kps_raw2, const float* uright2,
                               const float* depth2, int n2, const float* level_sigma2, const float* scale_factors,
                               int nlevels, const int* matches12, float* pos, uint8_t* reason, int* nnew) {
  int rc;
  if (!m) return g_merr.fail(ORBX_EINVAL, "bad argument");
  if ((rc = newpt_check(pair, kps1, uright1, depth1, n1, kps2, uright2, depth2, n2, level_sigma2, scale_factors,
                        nlevels, matches12, pos, reason)))
    return rc;
  if (n1 == 0) {
    if (nnew) *nnew = 0;
    return ORBX_OK;
  }
  HIP_OK(g_merr, hipSetDevice(m->device));
  const size_t a = n1, b = std::max(n2, 1);
  Stage st(m);
  auto dk1 = st.slot<orbx_kp>(a);
  auto dr1 = st.slot<orbx_kp>(a);
  auto du1 = st.slot<float>(a);
  auto dd1 = st.slot<float>(a);
  auto dk2 = st.slot<orbx_kp>(b);
  auto dr2 = st.slot<orbx_kp>(b);
  auto du2 = st.slot<float>(b);
  auto dd2 = st.slot<float>(b);
  auto dn = st.slot<int>(4);  // n1, n2, nnew, nnew_pair
  auto dp = st.slot<orbm_newpt_pair>(1);
  auto dm = st.slot<int>(a);
  auto dpos = st.slot<float>(3 * a);
  auto dre = st.slot<uint8_t>(a);
  const int counts[2] = {n1, n2};
  int total = 0;
  if ((rc = st.reserve()) || (rc = st.up(dk1, kps1, n1)) || (rc = st.up(dr1, kps_raw1, n1)) ||
      (rc = st.up(du1, uright1, n1)) || (rc = st.up(dd1, depth1, n1)) || (rc = st.up(dk2, kps2, n2)) ||
      (rc = st.up(dr2, kps_raw2, n2)) || (rc = st.up(du2, uright2, n2)) || (rc = st.up(dd2, depth2, n2)) ||
      (rc = st.up(dn, counts, 2)) || (rc = st.up(dp, pair, 1)) || (rc = st.up(dm, matches12, n1)) ||
      (rc = orbm_create_new_map_points_batch(m, dk1, kps_raw1 ? (orbx_kp*)dr1 : nullptr, du1, dd1, dn, (int)a, dk2,
                                             kps_raw2 ? (orbx_kp*)dr2 : nullptr, du2, dd2, (int*)dn + 1, (int)b, dp,
                                             level_sigma2, scale_factors, nlevels, 1, dm, (int)a, 0, dpos, dre,
                                             nullptr, n1, (int*)dn + 2, (int*)dn + 3, nullptr, nullptr, nullptr,
                                             st.st)) ||
      (rc = st.down(pos, dpos, 3 * a)) || (rc = st.down(reason, dre, a)) ||
      (rc = hipMemcpyAsync(&total, (int*)dn + 2, sizeof(int), hipMemcpyDeviceToHost, st.st) == hipSuccess
                ? ORBX_OK
                : g_merr.fail(ORBX_EDEVICE, "count read-back failed")) ||
      (rc = st.finish()))
    return rc;
  if (nnew) *nnew = total;
  return ORBX_OK;
}

// ---------------------------------------------- pose-projection overloads
namespace {

// R*x + t via gemm's small-matrix path (float dot, double add of t)
void host_rx_t(const float* T, const float* x, float* d) {
  for (int r = 0; r < 3; ++r) {
    const float t = T[4 * r] * x[0] + T[4 * r + 1] * x[1] + T[4 * r + 2] * x[2];
    d[r] = (float)((double)t * 1.0 + (double)T[4 * r + 3] * 1.0);
  }
}
// MapPoint::PredictScale's int level as a predicate of the ratio
int host_predict_direct(float ratio, float logsf, int L) {
  const float q = std::ceil(std::log(ratio) / logsf);  // float overloads (logf)
  int s = (q >= -2147483648.0f && q < 2147483648.0f) ? (int)q : INT_MIN;
  return s < 0 ? 0 : (s >= L ? L - 1 : s);
}

}  // namespace

int orbm_prepare_pose(int mode, const orbm_camera* cam, const float* Tlw, int mono, orbm_pose* out) {
  if (!cam || !out || mode < ORBM_PROJ_LAST_FRAME || mode > ORBM_PROJ_FUSE_SIM3 ||
      (mode == ORBM_PROJ_LAST_FRAME && !Tlw))
    return g_merr.fail(ORBX_EINVAL, "bad argument");
  float Rt[12];
  if (mode == ORBM_PROJ_SIM3 || mode == ORBM_PROJ_FUSE_SIM3) {
    // Rcw = sRcw/scw, tcw = t/scw (orbx_posemath.cuh)
    if (!(rt_from_scw(cam->Tcw, Rt) > 0)) return g_merr.fail(ORBX_EINVAL, "Scw has a zero scale");
  } else {
    for (int k = 0; k < 12; ++k) Rt[k] = cam->Tcw[k];
  }
  orbm_pose p;
  pose_from_rt(*cam, Rt, &p);  // intrinsics, Rt, Ow = -Rcw.t()*tcw, level_mode 0
  if (mode == ORBM_PROJ_LAST_FRAME) {
    // twc = -Rcw.t()*tcw; tlc = Rlw*twc + tlw (src/ORBmatcher.cc:1338-1349)
    float tlc[3];
    host_rx_t(Tlw, p.Ow, tlc);
    const bool bForward = tlc[2] > cam->mb && !mono;
    const bool bBackward = -tlc[2] > cam->mb && !mono;
    p.level_mode = bForward ? 1 : (bBackward ? 2 : 0);
  }
  *out = p;
  return ORBX_OK;
}

int orbm_prepare_sim3_match(const orbm_camera* cam1, const float* T1w, const float* T2w, float s12, const float* R12,
                            const float* t12, orbm_pose* out) {
  if (!cam1 || !T1w || !T2w || !R12 || !t12 || !out || !(s12 != 0.0f)) return g_merr.fail(ORBX_EINVAL, "bad argument");
  // sR12 = s12*R12; sR21 = (1.0/s12)*R12.t(); t21 = -sR21*t12 (src/ORBmatcher.cc:1118-1120), as
  // Sim3Solver's step 8 and its kernel compute them (orbx_sim3.cuh)
  orbm_camera c = *cam1;
  sim3_match_poses(c, T1w, T2w, s12, R12, t12, out);
  return ORBX_OK;
}

int orbm_predict_scale_thresholds(float scale_factor, int nlevels, float* thr) {
  if (!thr || nlevels < 1 || nlevels > kMaxLevels || !(scale_factor > 1.0f))
    return g_merr.fail(ORBX_EINVAL, "bad argument");
  const float logsf = std::log(scale_factor);  // Frame::mfLogScaleFactor (src/Frame.cc:70)
  for (int k = 1; k < nlevels; ++k) {
    // least positive float r with level(r) >= k; level is non-decreasing in r
    uint32_t lo = 0x00000001u, hi = 0x7f7fffffu;  // level(lo) = 0 < k <= level(FLT_MAX)
    auto at = [](uint32_t b) {
      float f;
      std::memcpy(&f, &b, 4);
      return f;
    };
    if (host_predict_direct(at(hi), logsf, nlevels) < k) return g_merr.fail(ORBX_EINVAL, "scale factor too small");
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (host_predict_direct(at(mid), logsf, nlevels) >= k)
        hi = mid;
      else
        lo = mid;
    }
    thr[k - 1] = at(hi);
  }
  for (int k = nlevels; k <= kMaxLevels; ++k) thr[k - 1 < kMaxLevels ? k - 1 : 0] = INFINITY;
  return ORBX_OK;
}

int orbm_predict_scale(float max_distance, float dist, float scale_factor, int nlevels) {
  float thr[kMaxLevels];
  if (orbm_predict_scale_thresholds(scale_factor, nlevels, thr)) return -1;
  const float ratio = max_distance / dist;
  if (std::isinf(ratio)) return 0;
  int l = 0;
  for (int k = 0; k < nlevels - 1; ++k) l += ratio >= thr[k];
  return l;
}

int orbm_search_by_projection_pose_batch(orbm_handle m, int mode, const orbx_kp* d_kps, const uint8_t* d_desc,
                                         const int* d_n, int kp_pitch, const float* d_uright, orbm_grid_bounds b,
                                         const float* scale, int nlevels, float scale_factor,
                                         const uint8_t* d_blocked, const orbm_pose* d_poses,
                                         const orbm_map_point_world* d_mps, const uint8_t* d_mpdesc,
                                         const int* d_nmp, int mp_pitch, int frames, float th, int dist_th,
                                         int check_ori, const float* inv_sigma2, int* d_out, int* d_nmatches,
                                         void* stream) {
  if (!m || !d_kps || !d_desc || !d_n || !scale || !d_blocked || !d_poses || !d_mps || !d_mpdesc || !d_nmp ||
      !d_out || !d_nmatches || frames < 1 || kp_pitch < 1 || mp_pitch < 1 || nlevels < 1 ||
      nlevels > kMaxLevels || mode < ORBM_PROJ_LAST_FRAME || mode > ORBM_PROJ_SIM3_MATCH ||
      (mode == ORBM_PROJ_FUSE && !inv_sigma2))
    return g_merr.fail(ORBX_EINVAL, "bad argument");
  if (!(b.max_x > b.min_x) || !(b.max_y > b.min_y)) return g_merr.fail(ORBX_EINVAL, "empty grid bounds");
  if (pose_lds_bytes(kp_pitch) > 156 * 1024) return g_merr.fail(ORBX_ECAPACITY, "kp_pitch %d too large", kp_pitch);
  HIP_OK(g_merr, hipSetDevice(m->device));
  PoseParams P{};
  P.mode = mode;
  set_grid_bounds(P, b);
  for (int l = 0; l < kMaxLevels; ++l) P.scale[l] = scale[std::min(l, nlevels - 1)];
  if (mode != ORBM_PROJ_LAST_FRAME) {
    int rc = orbm_predict_scale_thresholds(scale_factor, nlevels, P.pred_thr);
    if (rc) return rc;
  }
  P.L = nlevels;
  P.th = th;
  P.dist_th = dist_th;
  P.check_ori = check_ori;
  P.kp_pitch = kp_pitch;
  P.mp_pitch = mp_pitch;
  P.has_uright = d_uright != nullptr && (mode == ORBM_PROJ_LAST_FRAME || mode == ORBM_PROJ_FUSE);
  for (int l = 0; l < kMaxLevels; ++l) P.inv_sigma2[l] = inv_sigma2 ? inv_sigma2[std::min(l, nlevels - 1)] : 0.f;
  P.max_rounds = 32;
  if (const char* e = getenv("ORBX_PROJ_ROUNDS")) P.max_rounds = atoi(e);  // tests: force the sequential pass
  const size_t need = (size_t)frames * mp_pitch * 4;
  if (m->ws.before((hipStream_t)stream)) return g_merr.fail(ORBX_EDEVICE, "stream wait on the workspace failed");
  if (m->pose_picks.n < need) {
    if (m->ws.ev) HIP_OK(g_merr, hipEventSynchronize(m->ws.ev));
    if (m->pose_picks.reserve(need) != hipSuccess) return g_merr.fail(ORBX_ENOMEM, "pose picks workspace");
  }
  if (launch_search_pose(P, d_kps, d_desc, d_n, d_uright, d_blocked, d_poses, d_mps, d_mpdesc, d_nmp, frames,
                         m->pose_picks.as<int>(), d_out, d_nmatches, stream))
    return g_merr.fail(ORBX_EDEVICE, "search_pose launch: %s", hipGetErrorString(hipGetLastError()));
  if (m->ws.after((hipStream_t)stream)) return g_merr.fail(ORBX_EDEVICE, "event record failed");
  return ORBX_OK;
}

namespace {
// One frame through orbm_search_by_projection_pose_batch from host buffers.
int pose_sync(orbm_handle m, int mode, const orbx_kp* kps, const uint8_t* desc, int n, const float* uright,
              orbm_grid_bounds b, const float* scale, int nlevels, float scale_factor, const uint8_t* blocked,
              const orbm_pose& pose, const orbm_map_point_world* mps, const uint8_t* mpdesc, int nmp, float th,
              int dist_th, int check_ori, int* out, int* nmatches, const float* inv_sigma2 = nullptr) {
  const bool pp = mode == ORBM_PROJ_FUSE || mode == ORBM_PROJ_FUSE_SIM3 || mode == ORBM_PROJ_SIM3_MATCH;
  if (!m || !nmatches || n < 0 || nmp < 0 || (n && (!kps || !desc)) || (nmp && (!mps || !mpdesc)) ||
      ((pp ? nmp : n) && !out))
    return g_merr.fail(ORBX_EINVAL, "bad argument");
  HIP_OK(g_merr, hipSetDevice(m->device));
  const int kp = std::max(n, 1), mp = std::max(nmp, 1);
  std::vector<uint8_t> bl(kp, 0);  // a null `blocked` uploads zeros
  if (blocked && n) std::memcpy(bl.data(), blocked, n);
  const int hn[2] = {n, nmp};
  int nm = 0, rc;
  Stage st(m);
  auto dk = st.slot<orbx_kp>(kp);
  auto dd = st.slot<uint8_t>((size_t)kp * 32);
  auto dur = st.slot<float>(kp);
  auto dbl = st.slot<uint8_t>(kp);
  auto dmp = st.slot<orbm_map_point_world>(mp);
  auto dmd = st.slot<uint8_t>((size_t)mp * 32);
  auto dout = st.slot<int>(pp ? mp : kp);
  auto cnt = st.slot<int>(2);  // n, nmp
  auto dnm = st.slot<int>(1);
  auto dpose = st.slot<orbm_pose>(1);
  if ((rc = st.reserve()) || (rc = st.up(dk, kps, n)) || (rc = st.up(dd, desc, (size_t)n * 32)) ||
      (rc = st.up(dur, uright, n)) || (rc = st.up(dbl, bl.data(), kp)) || (rc = st.up(dmp, mps, nmp)) ||
      (rc = st.up(dmd, mpdesc, (size_t)nmp * 32)) || (rc = st.up(cnt, hn, 2)) || (rc = st.up(dpose, &pose, 1)) ||
      (rc = orbm_search_by_projection_pose_batch(m, mode, dk, dd, cnt, kp, uright ? (float*)dur : nullptr, b, scale,
                                                 nlevels, scale_factor, dbl, dpose, dmp, dmd, cnt + 1, mp, 1, th,
                                                 dist_th, check_ori, inv_sigma2, dout, dnm, st.st)) ||
      (rc = st.down(&nm, dnm, 1)) || (rc = st.down(out, dout, pp ? nmp : n)) || (rc = st.finish()))
    return rc;
  *nmatches = nm;
  return ORBX_OK;
}
}  // namespace

int orbm_search_by_projection_last_frame(orbm_handle m, const orbx_kp* kps, const uint8_t* desc, int n,
                                         const float* uright, orbm_grid_bounds b, const float* scale, int nlevels,
                                         const uint8_t* blocked, const orbm_camera* cur, const float* Tlw,
                                         const orbm_map_point_world* mps, const uint8_t* mpdesc, int nmp, float th,
                                         int mono, int check_ori, int* out, int* nmatches) {
  orbm_pose pose;
  int rc = orbm_prepare_pose(ORBM_PROJ_LAST_FRAME, cur, Tlw, mono, &pose);
  if (rc) return rc;
  return pose_sync(m, ORBM_PROJ_LAST_FRAME, kps, desc, n, uright, b, scale, nlevels, 1.2f, blocked, pose, mps,
                   mpdesc, nmp, th, 100 /* TH_HIGH */, check_ori, out, nmatches);
}

int orbm_search_by_projection_keyframe(orbm_handle m, const orbx_kp* kps, const uint8_t* desc, int n,
                                       orbm_grid_bounds b, const float* scale, int nlevels, float scale_factor,
                                       const uint8_t* has_mp, const orbm_camera* cur,
                                       const orbm_map_point_world* mps, const uint8_t* mpdesc, int nmp, float th,
                                       int orb_dist, int check_ori, int* out, int* nmatches) {
  orbm_pose pose;
  int rc = orbm_prepare_pose(ORBM_PROJ_KEYFRAME, cur, nullptr, 0, &pose);
  if (rc) return rc;
  return pose_sync(m, ORBM_PROJ_KEYFRAME, kps, desc, n, nullptr, b, scale, nlevels, scale_factor, has_mp, pose,
                   mps, mpdesc, nmp, th, orb_dist, check_ori, out, nmatches);
}

int orbm_search_by_projection_sim3(orbm_handle m, const orbx_kp* kps, const uint8_t* desc, int n,
                                   orbm_grid_bounds b, const float* scale, int nlevels, float scale_factor,
                                   const orbm_camera* kf, const orbm_map_point_world* mps, const uint8_t* mpdesc,
                                   int nmp, int th, const int* matched, int* out, int* nmatches) {
  orbm_pose pose;
  int rc = orbm_prepare_pose(ORBM_PROJ_SIM3, kf, nullptr, 0, &pose);
  if (rc) return rc;
  std::vector<uint8_t> bl(std::max(n, 1), 0);
  if (matched)
    for (int i = 0; i < n; ++i) bl[i] = matched[i] >= 0;  // vpMatched[idx] set on entry
  return pose_sync(m, ORBM_PROJ_SIM3, kps, desc, n, nullptr, b, scale, nlevels, scale_factor, bl.data(), pose, mps,
                   mpdesc, nmp, (float)th, 50 /* TH_LOW */, 0, out, nmatches);
}

int orbm_fuse(orbm_handle m, const orbx_kp* kps, const uint8_t* desc, int n, const float* uright, orbm_grid_bounds b,
              const float* scale, const float* inv_sigma2, int nlevels, float scale_factor, const orbm_camera* kf,
              const orbm_map_point_world* mps, const uint8_t* mpdesc, int nmp, float th, int* out, int* nfused) {
  if (!inv_sigma2) return g_merr.fail(ORBX_EINVAL, "bad argument");
  orbm_pose pose;
  int rc = orbm_prepare_pose(ORBM_PROJ_FUSE, kf, nullptr, 0, &pose);
  if (rc) return rc;
  return pose_sync(m, ORBM_PROJ_FUSE, kps, desc, n, uright, b, scale, nlevels, scale_factor, nullptr, pose, mps,
                   mpdesc, nmp, th, 50 /* TH_LOW */, 0, out, nfused, inv_sigma2);
}

int orbm_fuse_sim3(orbm_handle m, const orbx_kp* kps, const uint8_t* desc, int n, orbm_grid_bounds b,
                   const float* scale, int nlevels, float scale_factor, const orbm_camera* kf,
                   const orbm_map_point_world* mps, const uint8_t* mpdesc, int nmp, float th, int* out, int* nfused) {
  orbm_pose pose;
  int rc = orbm_prepare_pose(ORBM_PROJ_FUSE_SIM3, kf, nullptr, 0, &pose);
  if (rc) return rc;
  return pose_sync(m, ORBM_PROJ_FUSE_SIM3, kps, desc, n, nullptr, b, scale, nlevels, scale_factor, nullptr, pose,
                   mps, mpdesc, nmp, th, 50 /* TH_LOW */, 0, out, nfused);
}

int orbm_search_by_sim3(orbm_handle m, const orbx_kp* kps1, const uint8_t* desc1, int n1, orbm_grid_bounds b1,
                        const float* T1w, const orbm_map_point_world* mps1, const uint8_t* mpdesc1,
                        const orbx_kp* kps2, const uint8_t* desc2, int n2, orbm_grid_bounds b2, const float* T2w,
                        const orbm_map_point_world* mps2, const uint8_t* mpdesc2, const float* scale, int nlevels,
                        float scale_factor, const orbm_camera* cam1, float s12, const float* R12, const float* t12,
                        float th, int* match12, int* nfound) {
  if (!nfound || n1 < 0 || n2 < 0 || (n1 && !match12)) return g_merr.fail(ORBX_EINVAL, "bad argument");
  orbm_pose pz[2];
  int rc = orbm_prepare_sim3_match(cam1, T1w, T2w, s12, R12, t12, pz);
  if (rc) return rc;
  // direction 1: pKF1's points into pKF2 (vnMatch1); direction 2: pKF2's into pKF1 (vnMatch2)
  std::vector<int> vn1(std::max(n1, 1), -1), vn2(std::max(n2, 1), -1);
  int c1 = 0, c2 = 0;
  if ((rc = pose_sync(m, ORBM_PROJ_SIM3_MATCH, kps2, desc2, n2, nullptr, b2, scale, nlevels, scale_factor, nullptr,
                      pz[0], mps1, mpdesc1, n1, th, 100 /* TH_HIGH */, 0, vn1.data(), &c1)))
    return rc;
  if ((rc = pose_sync(m, ORBM_PROJ_SIM3_MATCH, kps1, desc1, n1, nullptr, b1, scale, nlevels, scale_factor, nullptr,
                      pz[1], mps2, mpdesc2, n2, th, 100 /* TH_HIGH */, 0, vn2.data(), &c2)))
    return rc;
  // Check agreement (:1295-1312)
  int nFound = 0;
  for (int i1 = 0; i1 < n1; i1++) {
    match12[i1] = -1;
    const int idx2 = vn1[i1];
    if (idx2 >= 0 && idx2 < n2 && vn2[idx2] == i1) {
      match12[i1] = idx2;
      nFound++;
    }
  }
  *nfound = nFound;
  return ORBX_OK;
}

int orbm_prepare_triangulation(const float* cw1, const float* T2w, const float* cam2, const float* F12,
                               orbm_tri_pair* out) {
  if (!cw1 || !T2w || !cam2 || !F12 || !out) return g_merr.fail(ORBX_EINVAL, "bad argument");
  // C2 = R2w*Cw + t2w; invz = 1.0f/C2.z; ex = fx*C2.x*invz + cx (src/ORBmatcher.cc:664-670)
  float C2[3];
  host_rx_t(T2w, cw1, C2);
  const float invz = 1.0f / C2[2];
  orbm_tri_pair t{};
  std::memcpy(t.F12, F12, sizeof t.F12);
  t.ex = cam2[0] * C2[0] * invz + cam2[2];
  t.ey = cam2[1] * C2[1] * invz + cam2[3];
  *out = t;
  return ORBX_OK;
}

int orbm_search_for_triangulation_batch(
    orbm_handle m, const orbx_kp* d_kps1, const uint8_t* d_desc1, const float* d_uright1, const uint8_t* d_has_mp1,
    const int* d_n1, const uint32_t* d_nodes1, const int* d_off1, const int* d_idx1, const int* d_nn1, int kp_pitch1,
    int node_pitch1, const orbx_kp* d_kps2, const uint8_t* d_desc2, const float* d_uright2, const uint8_t* d_has_mp2,
    const int* d_n2, const uint32_t* d_nodes2, const int* d_off2, const int* d_idx2, const int* d_nn2, int kp_pitch2,
    int node_pitch2, const orbm_tri_pair* d_pairs, const float* scale2, const float* sigma2, int nlevels, int pairs,
    int only_stereo, int check_ori, int* d_matches12, int out_pitch, int* d_nmatches, void* stream) {
  if (!m || !d_kps1 || !d_desc1 || !d_uright1 || !d_has_mp1 || !d_n1 || !d_nodes1 || !d_off1 || !d_idx1 || !d_nn1 ||
      !d_kps2 || !d_desc2 || !d_uright2 || !d_has_mp2 || !d_n2 || !d_nodes2 || !d_off2 || !d_idx2 || !d_nn2 ||
      !d_pairs || !scale2 || !sigma2 || !d_matches12 || !d_nmatches || pairs < 1 || nlevels < 1 ||
      nlevels > kMaxLevels || kp_pitch1 < 0 || node_pitch1 < 0 || kp_pitch2 < 1 || node_pitch2 < 1 || out_pitch < 1 ||
      ((kp_pitch1 == 0) != (node_pitch1 == 0)))
    return g_merr.fail(ORBX_EINVAL, "bad argument");
  HIP_OK(g_merr, hipSetDevice(m->device));
  TriParams P{};
  for (int l = 0; l < kMaxLevels; ++l) {
    P.scale2[l] = scale2[std::min(l, nlevels - 1)];
    P.sigma2[l] = sigma2[std::min(l, nlevels - 1)];
  }
  P.only_stereo = only_stereo;
  P.check_ori = check_ori;
  P.out_pitch = out_pitch;
  const TriSide A{d_kps1, d_desc1, d_uright1, d_has_mp1, d_n1, d_nodes1, d_off1, d_idx1, d_nn1, kp_pitch1,
                  node_pitch1};
  const TriSide B{d_kps2, d_desc2, d_uright2, d_has_mp2, d_n2, d_nodes2, d_off2, d_idx2, d_nn2, kp_pitch2,
                  node_pitch2};
  if (launch_search_tri(P, A, B, d_pairs, pairs, d_matches12, d_nmatches, stream))
    return g_merr.fail(ORBX_EDEVICE, "search_tri launch: %s", hipGetErrorString(hipGetLastError()));
  return ORBX_OK;
}

int orbm_search_for_triangulation(orbm_handle m, const orbx_kp* kps1, const uint8_t* desc1, const float* uright1,
                                  const uint8_t* has_mp1, int n1, orbm_feature_vector fv1, const orbx_kp* kps2,
                                  const uint8_t* desc2, const float* uright2, const uint8_t* has_mp2, int n2,
                                  orbm_feature_vector fv2, const float* cw1, const float* T2w, const float* cam2,
                                  const float* scale2, const float* sigma2, int nlevels, const float* F12,
                                  int only_stereo, int check_ori, int* matches12, int* nmatches) {
  if (!m || !nmatches || n1 < 0 || n2 < 0 || fv1.n_nodes < 0 || fv2.n_nodes < 0 ||
      (n1 && (!kps1 || !desc1 || !uright1 || !has_mp1 || !matches12)) ||
      (n2 && (!kps2 || !desc2 || !uright2 || !has_mp2)) || (fv1.n_nodes && (!fv1.nodes || !fv1.off)) ||
      (fv2.n_nodes && (!fv2.nodes || !fv2.off)))
    return g_merr.fail(ORBX_EINVAL, "bad argument");
  orbm_tri_pair tp;
  int rc = orbm_prepare_triangulation(cw1, T2w, cam2, F12, &tp);
  if (rc) return rc;
  const int f1 = fv1.n_nodes ? fv1.off[fv1.n_nodes] : 0, f2 = fv2.n_nodes ? fv2.off[fv2.n_nodes] : 0;
  if (f1 > n1 || f2 > n2) return g_merr.fail(ORBX_EINVAL, "feature vector holds more indices than keypoints");
  for (int i = 0; i < f1; ++i)
    if (fv1.idx[i] < 0 || fv1.idx[i] >= n1) return g_merr.fail(ORBX_EINVAL, "feature index out of range");
  for (int i = 0; i < f2; ++i)
    if (fv2.idx[i] < 0 || fv2.idx[i] >= n2) return g_merr.fail(ORBX_EINVAL, "feature index out of range");
  HIP_OK(g_merr, hipSetDevice(m->device));
  const int k1 = std::max(n1, 1), k2 = std::max(n2, 1);
  const int nn1 = std::max(fv1.n_nodes, 1), nn2 = std::max(fv2.n_nodes, 1);
  const int zero = 0;  // an empty FeatureVector's off[0]
  const int cnt[4] = {n1, fv1.n_nodes, n2, fv2.n_nodes};
  int nm = 0;
  Stage st(m);
  auto dk1 = st.slot<orbx_kp>(k1), dk2 = st.slot<orbx_kp>(k2);
  auto dd1 = st.slot<uint8_t>((size_t)k1 * 32), dd2 = st.slot<uint8_t>((size_t)k2 * 32);  // descriptors
  auto du1 = st.slot<float>(k1), du2 = st.slot<float>(k2);                                // uRight
  auto dm1 = st.slot<uint8_t>(k1), dm2 = st.slot<uint8_t>(k2);                            // MapPoint masks
  auto dno1 = st.slot<uint32_t>(nn1), dno2 = st.slot<uint32_t>(nn2);                      // FeatureVector CSR
  auto dof1 = st.slot<int>(nn1 + 1), dof2 = st.slot<int>(nn2 + 1);
  auto dix1 = st.slot<int>(k1), dix2 = st.slot<int>(k2);
  auto c = st.slot<int>(4);  // n1, nodes of 1, n2, nodes of 2
  auto dtp = st.slot<orbm_tri_pair>(1);
  auto dout = st.slot<int>(k1);
  auto dnm = st.slot<int>(1);
  if ((rc = st.reserve()) || (rc = st.up(dk1, kps1, n1)) || (rc = st.up(dd1, desc1, (size_t)n1 * 32)) ||
      (rc = st.up(du1, uright1, n1)) || (rc = st.up(dm1, has_mp1, n1)) || (rc = st.up(dno1, fv1.nodes, fv1.n_nodes)) ||
      (rc = st.up(dof1, fv1.n_nodes ? fv1.off : &zero, fv1.n_nodes + 1)) || (rc = st.up(dix1, fv1.idx, f1)) ||
      (rc = st.up(dk2, kps2, n2)) || (rc = st.up(dd2, desc2, (size_t)n2 * 32)) || (rc = st.up(du2, uright2, n2)) ||
      (rc = st.up(dm2, has_mp2, n2)) || (rc = st.up(dno2, fv2.nodes, fv2.n_nodes)) ||
      (rc = st.up(dof2, fv2.n_nodes ? fv2.off : &zero, fv2.n_nodes + 1)) || (rc = st.up(dix2, fv2.idx, f2)) ||
      (rc = st.up(c, cnt, 4)) || (rc = st.up(dtp, &tp, 1)) ||
      (rc = orbm_search_for_triangulation_batch(m, dk1, dd1, du1, dm1, c, dno1, dof1, dix1, c + 1, k1, nn1, dk2, dd2,
                                                du2, dm2, c + 2, dno2, dof2, dix2, c + 3, k2, nn2, dtp, scale2, sigma2,
                                                nlevels, 1, only_stereo, check_ori, dout, k1, dnm, st.st)) ||
      (rc = st.down(&nm, dnm, 1)) || (rc = st.down(matches12, dout, n1)) || (rc = st.finish()))
    return rc;
  *nmatches = nm;
  return ORBX_OK;
}

}  // extern "C"
