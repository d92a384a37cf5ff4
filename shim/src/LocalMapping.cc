// CreateNewMapPoints over orbm_search_for_triangulation_batch ->
// orbm_create_new_map_points_batch -> orbm_refresh_map_points_batch (see
// include/LocalMapping.h). One descriptor arena serves the search and the
// refresh: the current keyframe's rows first, then every neighbour's at a
// pitch of K rows, so a keypoint's arena row is (slot * K + idx) and the
// search's side 2 reads the same memory at kp_pitch2 = K. The keyframe table
// of the refresh is {current, neighbours...} in the same slots. At most one
// point per keypoint of the current keyframe survives the first-pair rule, so
// N1 rows hold every new point.
#include "LocalMapping.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <stdexcept>
#include <string>

#include "ORBmatcher.h"
#include "orbx_c.h"

namespace ORB_SLAM2 {

namespace {

void check(int rc, bool matcher = true) {
  if (rc != ORBX_OK) throw std::runtime_error(std::string("liborbx: ") + (matcher ? orbm_last_error() : orbx_last_error()));
}

// a device allocation holding a host array's bytes (or zeros)
struct Dev {
  void* p = nullptr;
  size_t bytes = 0;
  explicit Dev(size_t n) : bytes(std::max<size_t>(n, 16)) {
    check(orbx_malloc(&p, bytes), false);
    check(orbx_memset(p, 0, bytes), false);
  }
  template <typename T>
  explicit Dev(const std::vector<T>& v) : Dev(v.size() * sizeof(T)) {
    if (!v.empty()) check(orbx_memcpy_htod(p, v.data(), v.size() * sizeof(T)), false);
  }
  Dev(const Dev&) = delete;
  Dev& operator=(const Dev&) = delete;
  ~Dev() { (void)orbx_free(p); }
  template <typename T> T* as() const { return static_cast<T*>(p); }
  template <typename T>
  void down(std::vector<T>& v) const {
    if (!v.empty()) check(orbx_memcpy_dtoh(v.data(), p, v.size() * sizeof(T)), false);
  }
};

struct StreamGuard {
  void* s = nullptr;
  StreamGuard() { check(orbx_stream_create(&s), false); }
  ~StreamGuard() { (void)orbx_stream_destroy(s); }
};

orbm_camera camera_of(KeyFrame* pKF) {
  orbm_camera c{pKF->fx, pKF->fy, pKF->cx, pKF->cy, pKF->mb, pKF->mbf, {}};
  const cv::Mat T = pKF->GetPose();
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 4; ++k) c.Tcw[4 * r + k] = T.at<float>(r, k);
  return c;
}

// one keyframe's arrays into row `slot` of the per-slot tables (pitch K keypoints, NP nodes)
struct Tables {
  int K, NP;
  std::vector<orbx_kp> kps, raw;
  std::vector<float> ur, dp;
  std::vector<uint8_t> has, desc;
  std::vector<int> n, nn, off, idx;
  std::vector<uint32_t> nodes;
  Tables(int slots, int K_, int NP_)
      : K(K_), NP(NP_), kps((size_t)slots * K_), raw((size_t)slots * K_), ur((size_t)slots * K_, -1.0f),
        dp((size_t)slots * K_, -1.0f), has((size_t)slots * K_, 0), desc((size_t)slots * K_ * 32, 0), n(slots, 0),
        nn(slots, 0), off((size_t)slots * (NP_ + 1), 0), idx((size_t)slots * K_, 0), nodes((size_t)slots * NP_, 0) {}
  void fill(int slot, KeyFrame* pKF) {
    static_assert(sizeof(cv::KeyPoint) == sizeof(orbx_kp), "cv::KeyPoint and orbx_kp share their layout");
    const int N = pKF->N;
    const size_t b = (size_t)slot * K;
    n[slot] = N;
    if (N) {
      std::memcpy(&kps[b], pKF->mvKeysUn.data(), (size_t)N * sizeof(orbx_kp));
      // UnprojectStereo reads the distorted keypoints
      std::memcpy(&raw[b], ((int)pKF->mvKeys.size() == N ? pKF->mvKeys : pKF->mvKeysUn).data(), (size_t)N * sizeof(orbx_kp));
      std::memcpy(&desc[b * 32], pKF->mDescriptors.data, (size_t)N * 32);
    }
    for (int i = 0; i < N; ++i) {
      if (i < (int)pKF->mvuRight.size()) ur[b + i] = pKF->mvuRight[i];
      if (i < (int)pKF->mvDepth.size()) dp[b + i] = pKF->mvDepth[i];
      has[b + i] = pKF->GetMapPoint(i) != nullptr;
    }
    int k = 0, pos = 0;
    int* o = &off[(size_t)slot * (NP + 1)];
    for (const auto& e : pKF->mFeatVec) {  // std::map: ascending node ids
      nodes[(size_t)slot * NP + k] = e.first;
      for (unsigned i : e.second) idx[b + pos++] = (int)i;
      o[++k] = pos;
    }
    nn[slot] = k;
  }
};

}  // namespace

std::vector<NewMapPoint> CreateNewMapPoints(KeyFrame* pKF1, const std::vector<KeyFrame*>& vpNeighKFs, bool bMonocular) {
  std::vector<NewMapPoint> out;
  const orbm_camera cam1 = camera_of(pKF1);
  // Check first that baseline is not too short (:277-286)
  std::vector<KeyFrame*> neigh;
  const cv::Mat Ow1 = pKF1->GetCameraCenter();
  for (KeyFrame* pKF2 : vpNeighKFs) {
    if (!bMonocular) {
      const cv::Mat Ow2 = pKF2->GetCameraCenter();
      double s = 0;
      for (int k = 0; k < 3; ++k) {
        const float d = Ow2.at<float>(k) - Ow1.at<float>(k);
        s += (double)d * d;
      }
      const float baseline = (float)std::sqrt(s);
      if (baseline < pKF2->mb) continue;
    }
    neigh.push_back(pKF2);
  }
  const int P = (int)neigh.size(), N1 = pKF1->N;
  if (!P || !N1) return out;
  int K = N1, NP = std::max<int>((int)pKF1->mFeatVec.size(), 1);
  for (KeyFrame* k : neigh) {
    K = std::max(K, k->N);
    NP = std::max<int>(NP, (int)k->mFeatVec.size());
  }
  Tables T(P + 1, K, NP);  // slot 0: the current keyframe
  T.fill(0, pKF1);
  std::vector<orbm_tri_pair> tri(P);
  std::vector<orbm_newpt_pair> np(P);
  std::vector<orbm_keyframe_ref> kfs(P + 1);
  for (int p = 0; p < P; ++p) {
    KeyFrame* pKF2 = neigh[p];
    T.fill(p + 1, pKF2);
    const orbm_camera cam2 = camera_of(pKF2);
    // pKF2 before the current keyframe in a std::map<KeyFrame*, size_t>: mObservations' order
    const int kf2_first = std::less<KeyFrame*>()(pKF2, pKF1) ? 1 : 0;
    check(orbm_prepare_new_points(&cam1, &cam2, pKF1->mfScaleFactor, 0, (uint32_t)(p + 1), 0, (uint32_t)((p + 1) * K),
                                  kf2_first, &np[p]));
    float F12[9];
    const float k2[4] = {pKF2->fx, pKF2->fy, pKF2->cx, pKF2->cy};
    check(orbm_compute_f12(&cam1, &cam2, F12));
    check(orbm_prepare_triangulation(np[p].Ow1, cam2.Tcw, k2, F12, &tri[p]));
    for (int k = 0; k < 3; ++k) kfs[p + 1].Ow[k] = np[p].Ow2[k];
    kfs[p + 1].bad = 0;
  }
  for (int k = 0; k < 3; ++k) kfs[0].Ow[k] = np[0].Ow1[k];
  kfs[0].bad = 0;

  const Dev dk(T.kps), dr(T.raw), du(T.ur), dd(T.dp), dh(T.has), dn(T.n), dnn(T.nn), dof(T.off), dix(T.idx), dnd(T.nodes),
      arena(T.desc), dtri(tri), dnp(np), dkfs(kfs);
  const int cap = N1, OP = N1;
  const Dev dM((size_t)P * OP * 4), dnm((size_t)P * 4), dpos((size_t)P * OP * 12), dre((size_t)P * OP),
      dnew((size_t)cap * sizeof(orbm_new_point)), dcnt(4), dnpair((size_t)P * 4),
      dmps((size_t)cap * sizeof(orbm_map_point_world)), dmd((size_t)cap * 32), dobs((size_t)cap * 2 * sizeof(orbm_observation)),
      doff((size_t)(cap + 1) * 4), dids((size_t)cap * 4), dref((size_t)cap * sizeof(orbm_point_refkf));
  // side 2 of slot s starts one pitch into every table
  const size_t k1 = (size_t)K;
  const orbm_newpt_emit E{dmps.as<orbm_map_point_world>(), dobs.as<orbm_observation>(), doff.as<uint32_t>(),
                          dids.as<uint32_t>(), dref.as<orbm_point_refkf>(), 0, 0};
  const float* sf = pKF1->mvScaleFactors.data();
  const float* sig = pKF1->mvLevelSigma2.data();
  const int L = (int)pKF1->mvScaleFactors.size();
  orbm_handle m = ORBmatcher::Handle();
  StreamGuard st;
  // ORBmatcher matcher(0.6,false): no orientation check, all keypoints (:248, :301)
  check(orbm_search_for_triangulation_batch(
      m, dk.as<orbx_kp>(), arena.as<uint8_t>(), du.as<float>(), dh.as<uint8_t>(), dn.as<int>(), dnd.as<uint32_t>(),
      dof.as<int>(), dix.as<int>(), dnn.as<int>(), 0, 0, dk.as<orbx_kp>() + k1, arena.as<uint8_t>() + k1 * 32,
      du.as<float>() + k1, dh.as<uint8_t>() + k1, dn.as<int>() + 1, dnd.as<uint32_t>() + NP, dof.as<int>() + NP + 1,
      dix.as<int>() + k1, dnn.as<int>() + 1, K, NP, dtri.as<orbm_tri_pair>(), sf, sig, L, P, 0, 0, dM.as<int>(), OP,
      dnm.as<int>(), st.s));
  check(orbm_create_new_map_points_batch(
      m, dk.as<orbx_kp>(), dr.as<orbx_kp>(), du.as<float>(), dd.as<float>(), dn.as<int>(), 0, dk.as<orbx_kp>() + k1,
      dr.as<orbx_kp>() + k1, du.as<float>() + k1, dd.as<float>() + k1, dn.as<int>() + 1, K, dnp.as<orbm_newpt_pair>(), sig,
      sf, L, P, dM.as<int>(), OP, 1, dpos.as<float>(), dre.as<uint8_t>(), dnew.as<orbm_new_point>(), cap, dcnt.as<int>(),
      dnpair.as<int>(), &E, dh.as<uint8_t>(), dh.as<uint8_t>() + k1, st.s));
  check(orbm_refresh_map_points_batch(m, dobs.as<orbm_observation>(), doff.as<uint32_t>(), dids.as<uint32_t>(), cap,
                                      dkfs.as<orbm_keyframe_ref>(), P + 1, arena.as<uint8_t>(), (uint32_t)((P + 1) * K),
                                      dref.as<orbm_point_refkf>(), sf, L, dmps.as<orbm_map_point_world>(),
                                      dmd.as<uint8_t>(), nullptr, nullptr, st.s));
  check(orbx_stream_synchronize(st.s), false);
  int status = 0;
  check(orbm_get_status(m, 1, &status));  // bit 1024: a stereo keypoint without a depth was rejected, as reported in its reason
  std::vector<int> cnt(1, 0);
  dcnt.down(cnt);
  const int n = cnt[0];
  std::vector<orbm_new_point> rec(n);
  std::vector<orbm_map_point_world> rows(n);
  std::vector<uint8_t> md((size_t)n * 32);
  dnew.down(rec);
  dmps.down(rows);
  dmd.down(md);
  out.reserve(n);
  for (int k = 0; k < n; ++k) {
    NewMapPoint q;
    q.x3D = cv::Mat(3, 1, CV_32F);
    q.normal = cv::Mat(3, 1, CV_32F);
    q.descriptor = cv::Mat(1, 32, CV_8U);
    for (int c = 0; c < 3; ++c) {
      q.x3D.at<float>(c) = rec[k].pos[c];
      q.normal.at<float>(c) = rows[k].normal[c];
    }
    std::memcpy(q.descriptor.data, &md[(size_t)k * 32], 32);
    q.pKF2 = neigh[rec[k].pair];
    q.idx1 = (size_t)rec[k].idx1;
    q.idx2 = (size_t)rec[k].idx2;
    q.kind = rec[k].kind;
    q.minDistance = rows[k].min_distance;
    q.maxDistance = rows[k].max_distance;
    out.push_back(q);
  }
  return out;
}

}  // namespace ORB_SLAM2
