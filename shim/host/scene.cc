// Scene mode of the shim host: rebuilds Frames / KeyFrames / MapPoints from a
// binary scene file (written by tests/shimscene.py), calls ONE ORBmatcher
// method the way the reference's threads call it, and writes the resulting
// pointer state as MapPoint indices for tests/test_shim.py to compare with
// the oracle:
//   op 1 SearchByProjection(F, vpMapPoints, th)           Tracking.cc:1277
//   op 2 SearchByProjection(CurrentFrame, LastFrame, ...)  Tracking.cc:962, 968
//   op 3 SearchByProjection(CurrentFrame, pKF, found, ...) Tracking.cc:1540, 1554
//   op 4 SearchByProjection(pKF, Scw, vpPoints, vpMatched) LoopClosing.cc:414
//   op 5 Fuse(pKF, vpMapPoints, th)                       LocalMapping.cc:525, 550
//   op 6 Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)     LoopClosing.cc:654
//   op 7 SearchBySim3(pKF1, pKF2, vpMatches12, ...)        LoopClosing.cc:362
//   op 8 SearchForTriangulation(pKF1, pKF2, F12, ...)      LocalMapping.cc:301
//   op 9 SearchByBoW(pKF, F, vpMapPointMatches)            Tracking.cc:842, 1465
//   op 10 Tracking::SearchLocalPoints' body                Tracking.cc:1229-1279
//   op 11 Optimizer::PoseOptimization(&CurrentFrame)       Tracking.cc:975, 1020
//   op 12 Sim3Solver(pKF1, pKF2, vpMatches12, fix), SetRansacParameters, iterate(k)...  LoopClosing.cc:313-340
//   op 13 CreateNewMapPoints(pKF, vpNeighKFs, bMonocular): the search, triangulation and refresh of LocalMapping.cc:270-483
//   op 14 Initializer(ReferenceFrame, sigma, iterations), Initialize(CurrentFrame, vMatches12, ...)  Tracking.cc:638-700
//   op 15 Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale)    LoopClosing.cc:365
// --scene-latency: the same scene rebuilt per call, only the method call on
// the host clock (median / p99 over the calls after the warm ones).
// Scene file: records of [u32 name length][name][u32 dtype 0 u8 / 1 i32 /
// 2 f32][u32 count][count elements].
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "Frame.h"
#include "Initializer.h"
#include "KeyFrame.h"
#include "LocalMapping.h"
#include "MapPoint.h"
#include "ORBmatcher.h"
#include "Optimizer.h"
#include "Sim3Solver.h"

using namespace ORB_SLAM2;

namespace {
struct Rec {
  int dtype = 0;
  std::vector<char> bytes;
  template <typename T> const T* p() const { return reinterpret_cast<const T*>(bytes.data()); }
  template <typename T> size_t n() const { return bytes.size() / sizeof(T); }
};

struct Scene {
  std::map<std::string, Rec> r;
  bool has(const std::string& k) const { return r.count(k) != 0; }
  const Rec& at(const std::string& k) const {
    auto it = r.find(k);
    if (it == r.end()) throw std::runtime_error("scene lacks " + k);
    return it->second;
  }
  template <typename T> std::vector<T> vec(const std::string& k) const {
    const Rec& x = at(k);
    return std::vector<T>(x.p<T>(), x.p<T>() + x.n<T>());
  }
  float f(const std::string& k) const { return at(k).p<float>()[0]; }
  int i(const std::string& k) const { return at(k).p<int>()[0]; }
};

Scene load(const std::string& path) {
  Scene s;
  FILE* fp = fopen(path.c_str(), "rb");
  if (!fp) throw std::runtime_error("cannot read " + path);
  for (;;) {
    uint32_t len = 0;
    if (fread(&len, 4, 1, fp) != 1) break;
    std::string name(len, '\0');
    uint32_t dt = 0, cnt = 0;
    if (fread(&name[0], 1, len, fp) != len || fread(&dt, 4, 1, fp) != 1 || fread(&cnt, 4, 1, fp) != 1)
      throw std::runtime_error("truncated scene");
    Rec rec;
    rec.dtype = (int)dt;
    rec.bytes.resize((size_t)cnt * (dt == 0 ? 1 : 4));
    if (!rec.bytes.empty() && fread(rec.bytes.data(), 1, rec.bytes.size(), fp) != rec.bytes.size())
      throw std::runtime_error("truncated scene");
    s.r[name] = std::move(rec);
  }
  fclose(fp);
  return s;
}

// the scene's MapPoints (mp_*), indexed by their row
std::vector<std::unique_ptr<MapPoint>> map_points(const Scene& s) {
  std::vector<std::unique_ptr<MapPoint>> pool;
  if (!s.has("mp_desc")) return pool;
  const int M = (int)(s.at("mp_desc").n<uint8_t>() / 32);
  const auto desc = s.vec<uint8_t>("mp_desc");
  for (int i = 0; i < M; ++i) {
    const bool bad = s.has("mp_bad") && s.at("mp_bad").p<uint8_t>()[i];
    pool.emplace_back(new MapPoint((unsigned long)i, bad));
    MapPoint* p = pool.back().get();
    for (int k = 0; k < 32; ++k) p->mDescriptor.data[k] = desc[(size_t)i * 32 + k];
    if (s.has("mp_pos"))
      for (int k = 0; k < 3; ++k) p->mWorldPos.at<float>(k) = s.at("mp_pos").p<float>()[3 * i + k];
    if (s.has("mp_normal"))
      for (int k = 0; k < 3; ++k) p->mNormalVector.at<float>(k) = s.at("mp_normal").p<float>()[3 * i + k];
    if (s.has("mp_dist")) p->SetScaleDistances(s.at("mp_dist").p<float>()[2 * i], s.at("mp_dist").p<float>()[2 * i + 1]);
    if (s.has("mp_track")) {
      const float* t = s.at("mp_track").p<float>() + 4 * i;
      p->mTrackProjX = t[0];
      p->mTrackProjY = t[1];
      p->mTrackProjXR = t[2];
      p->mTrackViewCos = t[3];
      p->mnTrackScaleLevel = s.at("mp_level").p<int>()[i];
      p->mbTrackInView = s.at("mp_inview").p<uint8_t>()[i] != 0;
    }
  }
  return pool;
}

MapPoint* ptr_of(const std::vector<std::unique_ptr<MapPoint>>& pool, int i) { return i >= 0 ? pool.at(i).get() : nullptr; }
int id_of(const MapPoint* p) { return p ? (int)p->mnId : -1; }

cv::Mat pose4(const Scene& s, const std::string& k) {
  const auto v = s.vec<float>(k);  // 12 (3x4) or 16 (4x4) row-major
  cv::Mat T(4, 4, CV_32F);
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) T.at<float>(r, c) = r < 3 ? v[4 * r + c] : (r == c ? 1.f : 0.f);
  return T;
}

// common fields of side X ("A" or "B"): keypoints, descriptors, uright, scale tables
template <typename F>
void fill_common(const Scene& s, const std::string& X, F& f) {
  const Rec& k = s.at(X + "_kps");
  const int n = (int)(k.bytes.size() / sizeof(cv::KeyPoint));
  f.mvKeys.resize(n);
  if (n) memcpy(f.mvKeys.data(), k.bytes.data(), k.bytes.size());
  f.mvKeysUn = f.mvKeys;
  f.N = n;
  f.mDescriptors.create(std::max(n, 1), 32, CV_8U);
  f.mDescriptors.rows = n;
  if (n) memcpy(f.mDescriptors.data, s.at(X + "_desc").bytes.data(), (size_t)n * 32);
  if (s.has(X + "_uright")) f.mvuRight = s.vec<float>(X + "_uright");
  else f.mvuRight.clear();
  f.mvScaleFactors = s.vec<float>(X + "_scale");
  f.mnScaleLevels = (int)f.mvScaleFactors.size();
  f.mfScaleFactor = s.has(X + "_sf") ? s.f(X + "_sf") : 1.2f;
  f.mfLogScaleFactor = std::log(f.mfScaleFactor);
  if (s.has(X + "_sigma2")) f.mvLevelSigma2 = s.vec<float>(X + "_sigma2");
  if (s.has(X + "_invsigma2")) f.mvInvLevelSigma2 = s.vec<float>(X + "_invsigma2");
}

std::unique_ptr<Frame> frame(const Scene& s, const std::string& X, const std::vector<std::unique_ptr<MapPoint>>& pool) {
  std::unique_ptr<Frame> F(new Frame());
  fill_common(s, X, *F);
  const auto cam = s.vec<float>(X + "_cam");  // fx fy cx cy mb mbf
  Frame::fx = cam[0];
  Frame::fy = cam[1];
  Frame::cx = cam[2];
  Frame::cy = cam[3];
  Frame::invfx = 1.0f / cam[0];
  Frame::invfy = 1.0f / cam[1];
  F->mb = cam[4];
  F->mbf = cam[5];
  const auto b = s.vec<float>(X + "_bounds");
  Frame::mnMinX = b[0];
  Frame::mnMaxX = b[1];
  Frame::mnMinY = b[2];
  Frame::mnMaxY = b[3];
  if (s.has(X + "_T")) F->mTcw = pose4(s, X + "_T");
  F->mvpMapPoints.assign(F->N, nullptr);
  if (s.has(X + "_mps")) {
    const auto m = s.vec<int>(X + "_mps");
    for (int i = 0; i < F->N; ++i) F->mvpMapPoints[i] = ptr_of(pool, m[i]);
  }
  if (s.has(X + "_fv_nodes")) {
    const auto nodes = s.vec<int>(X + "_fv_nodes");
    const auto off = s.vec<int>(X + "_fv_off");
    const auto idx = s.vec<int>(X + "_fv_idx");
    for (size_t j = 0; j < nodes.size(); ++j)
      F->mFeatVec[(unsigned)nodes[j]] = std::vector<unsigned>(idx.begin() + off[j], idx.begin() + off[j + 1]);
  }
  F->mvbOutlier.assign(F->N, false);
  if (s.has(X + "_outlier")) {
    const auto o = s.vec<uint8_t>(X + "_outlier");
    for (int i = 0; i < F->N; ++i) F->mvbOutlier[i] = o[i] != 0;
  }
  return F;
}

std::unique_ptr<KeyFrame> keyframe(const Scene& s, const std::string& X,
                                   const std::vector<std::unique_ptr<MapPoint>>& pool) {
  std::unique_ptr<KeyFrame> K(new KeyFrame());
  fill_common(s, X, *K);
  if (K->mvuRight.empty()) K->mvuRight.assign(K->N, -1.0f);
  if (s.has(X + "_depth")) K->mvDepth = s.vec<float>(X + "_depth");
  else K->mvDepth.assign(K->N, -1.0f);
  const auto cam = s.vec<float>(X + "_cam");
  K->fx = cam[0];
  K->fy = cam[1];
  K->cx = cam[2];
  K->cy = cam[3];
  K->invfx = 1.0f / cam[0];
  K->invfy = 1.0f / cam[1];
  K->mb = cam[4];
  K->mbf = cam[5];
  const auto b = s.vec<float>(X + "_bounds");
  K->mnMinX = (int)b[0];
  K->mnMaxX = (int)b[1];
  K->mnMinY = (int)b[2];
  K->mnMaxY = (int)b[3];
  if (s.has(X + "_T")) K->SetPose(pose4(s, X + "_T"));
  K->mvpMapPoints.assign(K->N, nullptr);
  if (s.has(X + "_mps")) {
    const auto m = s.vec<int>(X + "_mps");
    for (int i = 0; i < K->N; ++i) K->mvpMapPoints[i] = ptr_of(pool, m[i]);
  }
  if (s.has(X + "_fv_nodes")) {
    const auto nodes = s.vec<int>(X + "_fv_nodes");
    const auto off = s.vec<int>(X + "_fv_off");
    const auto idx = s.vec<int>(X + "_fv_idx");
    for (size_t j = 0; j < nodes.size(); ++j)
      K->mFeatVec[(unsigned)nodes[j]] = std::vector<unsigned>(idx.begin() + off[j], idx.begin() + off[j + 1]);
  }
  return K;
}

// observations: the points each keyframe holds (AddObservation, src/KeyFrame.cc
// holds the reverse link), then Observations() as the scene sets it (mp_nobs)
void observe(KeyFrame* K, const Scene& s, const std::vector<std::unique_ptr<MapPoint>>& pool) {
  for (int i = 0; i < K->N; ++i)
    if (K->mvpMapPoints[i]) K->mvpMapPoints[i]->AddObservation(K, i);
}
void set_nobs(const Scene& s, const std::vector<std::unique_ptr<MapPoint>>& pool) {
  if (!s.has("mp_nobs")) return;
  const auto n = s.vec<int>("mp_nobs");
  for (size_t i = 0; i < pool.size(); ++i) pool[i]->nObs = n[i];
}

std::vector<MapPoint*> pointers(const Scene& s, const std::string& k,
                                const std::vector<std::unique_ptr<MapPoint>>& pool) {
  std::vector<MapPoint*> v;
  for (int i : s.vec<int>(k)) v.push_back(ptr_of(pool, i));
  return v;
}

void write_ints(const std::string& path, const std::vector<int>& v) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || (!v.empty() && fwrite(v.data(), 4, v.size(), f) != v.size())) throw std::runtime_error("cannot write " + path);
  fclose(f);
}
}  // namespace

// Tracking::SearchLocalPoints (src/Tracking.cc:1229-1279) on a frame and a
// local map, th given by the scene. one_call = false: the reference's body as
// written, Frame::isInFrustum per point and then SearchByProjection; true: the
// same bookkeeping around one ORBmatcher::SearchLocalPoints call.
// -> [nToMatch, n, F.mvpMapPoints..., per local point: mbTrackInView, mnVisible]
static void search_local_points(const Scene& s, bool one_call, std::vector<int>& res) {
  auto pool = map_points(s);
  auto F = frame(s, "A", pool);
  Frame& mCurrentFrame = *F;
  mCurrentFrame.mnId = 7;
  set_nobs(s, pool);
  std::vector<MapPoint*> mvpLocalMapPoints = pointers(s, "vp", pool);
  if (s.has("mp_seen")) {  // matched earlier in this frame (TrackWithMotionModel / TrackReferenceKeyFrame)
    const auto seen = s.vec<uint8_t>("mp_seen");
    for (size_t i = 0; i < pool.size(); ++i)
      if (seen[i]) pool[i]->mnLastFrameSeen = mCurrentFrame.mnId;
  }
  const float th = s.f("th");
  // Do not search map points already matched
  for (std::vector<MapPoint*>::iterator vit = mCurrentFrame.mvpMapPoints.begin(),
                                       vend = mCurrentFrame.mvpMapPoints.end();
       vit != vend; vit++) {
    MapPoint* pMP = *vit;
    if (pMP) {
      if (pMP->isBad()) {
        *vit = static_cast<MapPoint*>(NULL);
      } else {
        pMP->IncreaseVisible();
        pMP->mnLastFrameSeen = mCurrentFrame.mnId;
        pMP->mbTrackInView = false;
      }
    }
  }
  int nToMatch = 0, n = 0;
  ORBmatcher matcher(s.f("nnratio"));
  if (one_call) {
    n = matcher.SearchLocalPoints(mCurrentFrame, mvpLocalMapPoints, th, &nToMatch, 0.5f);
  } else {
    // Project points in frame and check its visibility
    for (std::vector<MapPoint*>::iterator vit = mvpLocalMapPoints.begin(), vend = mvpLocalMapPoints.end(); vit != vend;
         vit++) {
      MapPoint* pMP = *vit;
      if (pMP->mnLastFrameSeen == mCurrentFrame.mnId) continue;
      if (pMP->isBad()) continue;
      // Project (this fills MapPoint variables for matching)
      if (mCurrentFrame.isInFrustum(pMP, 0.5)) {
        pMP->IncreaseVisible();
        nToMatch++;
      }
    }
    if (nToMatch > 0) n = matcher.SearchByProjection(mCurrentFrame, mvpLocalMapPoints, th);
  }
  res.push_back(nToMatch);
  res.push_back(n);
  for (MapPoint* p : mCurrentFrame.mvpMapPoints) res.push_back(id_of(p));
  for (MapPoint* p : mvpLocalMapPoints) {
    res.push_back(p->mbTrackInView ? 1 : 0);
    res.push_back(p->mnVisible);
  }
}

// One method call on the scene's state (built here), its results as int32
// arrays (see each op) and its host time in *ms (the call alone).
static void run_op(const Scene& s, std::vector<int>& res, double* ms) {
  const int op = s.i("op");
  auto pool = map_points(s);
  ORBmatcher matcher(s.has("nnratio") ? s.f("nnratio") : 0.6f, s.has("check_ori") ? s.i("check_ori") != 0 : true);
  using clk = std::chrono::steady_clock;
  clk::time_point t0;
  auto tic = [&]() { t0 = clk::now(); };
  auto toc = [&]() { *ms = std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
  switch (op) {
    case 1: {  // -> [n, F.mvpMapPoints...]
      auto F = frame(s, "A", pool);
      set_nobs(s, pool);
      const std::vector<MapPoint*> vp = pointers(s, "vp", pool);
      tic();
      const int n = matcher.SearchByProjection(*F, vp, s.f("th"));
      toc();
      res.push_back(n);
      for (MapPoint* p : F->mvpMapPoints) res.push_back(id_of(p));
      break;
    }
    case 2: {  // -> [n, CurrentFrame.mvpMapPoints...]
      auto Last = frame(s, "B", pool);
      auto Cur = frame(s, "A", pool);  // A last: the Frame statics are the current frame's
      set_nobs(s, pool);
      tic();
      const int n = matcher.SearchByProjection(*Cur, *Last, s.f("th"), s.i("mono") != 0);
      toc();
      res.push_back(n);
      for (MapPoint* p : Cur->mvpMapPoints) res.push_back(id_of(p));
      break;
    }
    case 3: {  // -> [n, CurrentFrame.mvpMapPoints...]
      auto K = keyframe(s, "B", pool);
      auto Cur = frame(s, "A", pool);
      set_nobs(s, pool);
      std::set<MapPoint*> found;
      for (MapPoint* p : pointers(s, "already", pool)) found.insert(p);
      tic();
      const int n = matcher.SearchByProjection(*Cur, K.get(), found, s.f("th"), s.i("orb_dist"));
      toc();
      res.push_back(n);
      for (MapPoint* p : Cur->mvpMapPoints) res.push_back(id_of(p));
      break;
    }
    case 4: {  // -> [n, vpMatched...]
      auto K = keyframe(s, "A", pool);
      set_nobs(s, pool);
      std::vector<MapPoint*> matched = pointers(s, "matched", pool);
      const cv::Mat Scw = pose4(s, "Scw");
      const std::vector<MapPoint*> vp = pointers(s, "vp", pool);
      tic();
      const int n = matcher.SearchByProjection(K.get(), Scw, vp, matched, s.i("thi"));
      toc();
      res.push_back(n);
      for (MapPoint* p : matched) res.push_back(id_of(p));
      break;
    }
    case 5: {  // -> [nFused, pKF->mvpMapPoints..., per point: bad, Observations()]
      auto K = keyframe(s, "A", pool);
      observe(K.get(), s, pool);
      set_nobs(s, pool);
      const std::vector<MapPoint*> vp = pointers(s, "vp", pool);
      tic();
      const int n = matcher.Fuse(K.get(), vp, s.f("th"));
      toc();
      res.push_back(n);
      for (MapPoint* p : K->mvpMapPoints) res.push_back(id_of(p));
      for (auto& p : pool) res.push_back(p->isBad() ? 1 : 0);
      for (auto& p : pool) res.push_back(p->Observations());
      break;
    }
    case 6: {  // -> [nFused, pKF->mvpMapPoints..., vpReplacePoint...]
      auto K = keyframe(s, "A", pool);
      observe(K.get(), s, pool);
      set_nobs(s, pool);
      const std::vector<MapPoint*> vp = pointers(s, "vp", pool);
      std::vector<MapPoint*> replace(vp.size(), nullptr);
      const cv::Mat Scw = pose4(s, "Scw");
      tic();
      const int n = matcher.Fuse(K.get(), Scw, vp, s.f("th"), replace);
      toc();
      res.push_back(n);
      for (MapPoint* p : K->mvpMapPoints) res.push_back(id_of(p));
      for (MapPoint* p : replace) res.push_back(id_of(p));
      break;
    }
    case 7: {  // -> [nFound, vpMatches12...]
      auto K1 = keyframe(s, "A", pool);
      auto K2 = keyframe(s, "B", pool);
      observe(K1.get(), s, pool);
      observe(K2.get(), s, pool);
      set_nobs(s, pool);
      std::vector<MapPoint*> m12 = pointers(s, "matched", pool);
      const auto R = s.vec<float>("R12"), t = s.vec<float>("t12");
      cv::Mat R12(3, 3, CV_32F), t12(3, 1, CV_32F);
      for (int k = 0; k < 9; ++k) R12.at<float>(k / 3, k % 3) = R[k];
      for (int k = 0; k < 3; ++k) t12.at<float>(k) = t[k];
      const float s12 = s.f("s12");
      tic();
      const int n = matcher.SearchBySim3(K1.get(), K2.get(), m12, s12, R12, t12, s.f("th"));
      toc();
      res.push_back(n);
      for (MapPoint* p : m12) res.push_back(id_of(p));
      break;
    }
    case 8: {  // -> [n, (idx1, idx2)...]
      auto K1 = keyframe(s, "A", pool);
      auto K2 = keyframe(s, "B", pool);
      const auto Fv = s.vec<float>("F12");
      cv::Mat F12(3, 3, CV_32F);
      for (int k = 0; k < 9; ++k) F12.at<float>(k / 3, k % 3) = Fv[k];
      std::vector<std::pair<size_t, size_t>> pairs;
      tic();
      const int n = matcher.SearchForTriangulation(K1.get(), K2.get(), F12, pairs, s.i("only_stereo") != 0);
      toc();
      res.push_back(n);
      for (auto& pr : pairs) {
        res.push_back((int)pr.first);
        res.push_back((int)pr.second);
      }
      break;
    }
    case 9: {  // -> [n, vpMapPointMatches...]
      auto K = keyframe(s, "B", pool);
      auto F = frame(s, "A", pool);
      std::vector<MapPoint*> matches;
      tic();
      const int n = matcher.SearchByBoW(K.get(), *F, matches);
      toc();
      res.push_back(n);
      for (MapPoint* p : matches) res.push_back(id_of(p));
      break;
    }
    case 10: {  // -> the reference's body, then the one-call body, each as search_local_points writes it
      tic();
      search_local_points(s, false, res);
      search_local_points(s, true, res);
      toc();
      break;
    }
    case 11: {  // -> [return value, mvbOutlier..., mTcw rows 0..2 as the bits of 12 floats]
      auto F = frame(s, "A", pool);
      set_nobs(s, pool);
      tic();
      const int n = Optimizer::PoseOptimization(F.get());
      toc();
      res.push_back(n);
      for (int i = 0; i < F->N; ++i) res.push_back(F->mvbOutlier[i] ? 1 : 0);
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) {
          const float v = F->mTcw.at<float>(r, c);
          int bits;
          memcpy(&bits, &v, 4);
          res.push_back(bits);
        }
      break;
    }
    case 12: {  // per iterate(k) call of the scene's list: [nInliers, bNoMore, T12 returned, then with a T12 its
                // rows 0..2 as the bits of 12 floats and vbInliers...]; at the end the bits of scale, R (9), t (3)
      auto K1 = keyframe(s, "A", pool);
      auto K2 = keyframe(s, "B", pool);
      observe(K1.get(), s, pool);
      observe(K2.get(), s, pool);
      const std::vector<MapPoint*> m12 = pointers(s, "matched", pool);
      auto bits = [](float v) {
        int b;
        memcpy(&b, &v, 4);
        return b;
      };
      srand((unsigned)s.i("seed"));
      tic();
      Sim3Solver solver(K1.get(), K2.get(), m12, s.i("fix_scale") != 0);
      solver.SetRansacParameters((double)s.i("prob_num") / (double)s.i("prob_den"), s.i("min_inliers"),
                                 s.i("max_iterations"));
      for (int k : s.vec<int>("iterate")) {
        bool bNoMore = false;
        std::vector<bool> vbInliers;
        int nInliers = 0;
        const cv::Mat T12 = k < 0 ? solver.find(vbInliers, nInliers) : solver.iterate(k, bNoMore, vbInliers, nInliers);
        res.push_back(nInliers);
        res.push_back(bNoMore ? 1 : 0);
        res.push_back(T12.empty() ? 0 : 1);
        if (!T12.empty()) {
          for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) res.push_back(bits(T12.at<float>(r, c)));
          for (bool b : vbInliers) res.push_back(b ? 1 : 0);
        }
        if (bNoMore) break;
      }
      toc();
      res.push_back(bits(solver.GetEstimatedScale()));
      const cv::Mat R = solver.GetEstimatedRotation(), t = solver.GetEstimatedTranslation();
      for (int k = 0; k < 9; ++k) res.push_back(bits(R.at<float>(k / 3, k % 3)));
      for (int k = 0; k < 3; ++k) res.push_back(bits(t.at<float>(k)));
      break;
    }
    case 15: {  // -> [return value, vpMatches1..., the two words of each of g2oS12's 8 doubles (r, t, s)]
      auto K1 = keyframe(s, "A", pool);
      auto K2 = keyframe(s, "B", pool);
      observe(K1.get(), s, pool);
      observe(K2.get(), s, pool);
      std::vector<MapPoint*> m1 = pointers(s, "matched", pool);
      const auto srt = s.vec<float>("srt");  // s, R (9), t (3): the solver's floats (src/LoopClosing.cc:359-364)
      double R[9], t[3];
      for (int k = 0; k < 9; ++k) R[k] = (double)srt[1 + k];
      for (int k = 0; k < 3; ++k) t[k] = (double)srt[10 + k];
      g2o::Sim3 S = g2o::Sim3::fromMatrix(R, t, (double)srt[0]);
      tic();
      const int n = Optimizer::OptimizeSim3(K1.get(), K2.get(), m1, S, s.f("th2"), s.i("fix_scale") != 0);
      toc();
      res.push_back(n);
      for (MapPoint* p : m1) res.push_back(id_of(p));
      const double v[8] = {S.r[0], S.r[1], S.r[2], S.r[3], S.t[0], S.t[1], S.t[2], S.s};
      for (int k = 0; k < 8; ++k) {
        int w[2];
        memcpy(w, &v[k], 8);
        res.push_back(w[0]);
        res.push_back(w[1]);
      }
      break;
    }
    case 13: {  // -> [n, per new point: neighbour, idx1, idx2, kind, pKF2 precedes pKF1 in std::map order, the bits of
                // x3D (3), normal (3), min / max distance, the descriptor as 8 words]
      auto K1 = keyframe(s, "A", pool);
      std::vector<std::unique_ptr<KeyFrame>> owned;
      std::vector<KeyFrame*> neigh;
      for (int p = 0; p < s.i("neighbours"); ++p) {
        owned.push_back(keyframe(s, "B" + std::to_string(p), pool));
        neigh.push_back(owned.back().get());
      }
      tic();
      const std::vector<NewMapPoint> pts = CreateNewMapPoints(K1.get(), neigh, s.i("mono") != 0);
      toc();
      auto bits = [](float v) {
        int b;
        memcpy(&b, &v, 4);
        return b;
      };
      res.push_back((int)pts.size());
      for (const NewMapPoint& q : pts) {
        int p = 0;
        while (neigh[p] != q.pKF2) ++p;
        res.push_back(p);
        res.push_back((int)q.idx1);
        res.push_back((int)q.idx2);
        res.push_back(q.kind);
        res.push_back(std::less<KeyFrame*>()(q.pKF2, K1.get()) ? 1 : 0);
        for (int k = 0; k < 3; ++k) res.push_back(bits(q.x3D.at<float>(k)));
        for (int k = 0; k < 3; ++k) res.push_back(bits(q.normal.at<float>(k)));
        res.push_back(bits(q.minDistance));
        res.push_back(bits(q.maxDistance));
        for (int k = 0; k < 8; ++k) {
          int w;
          memcpy(&w, q.descriptor.data + 4 * k, 4);
          res.push_back(w);
        }
      }
      break;
    }
    case 14: {  // -> [returned, the result's code, model, n, then with a true return the bits of R21 (9), t21 (3),
                // vbTriangulated per keypoint of frame 1 and the bits of vP3D (3 per keypoint)]
      auto F1 = frame(s, "A", pool);
      auto F2 = frame(s, "B", pool);
      const auto cam = s.vec<float>("A_cam");
      F1->mK = cv::Mat(3, 3, CV_32F);
      for (int k = 0; k < 9; ++k) F1->mK.at<float>(k / 3, k % 3) = k % 4 == 0 ? 1.f : 0.f;
      F1->mK.at<float>(0, 0) = cam[0];
      F1->mK.at<float>(1, 1) = cam[1];
      F1->mK.at<float>(0, 2) = cam[2];
      F1->mK.at<float>(1, 2) = cam[3];
      const std::vector<int> m12 = s.vec<int>("matches12");
      auto bits = [](float v) {
        int b;
        memcpy(&b, &v, 4);
        return b;
      };
      tic();
      Initializer init(*F1, s.f("sigma"), s.i("max_iterations"));
      cv::Mat R21, t21;
      std::vector<cv::Point3f> vP3D;
      std::vector<bool> vbTriangulated;
      const bool ok = init.Initialize(*F2, m12, R21, t21, vP3D, vbTriangulated);
      toc();
      res.push_back(ok ? 1 : 0);
      res.push_back(init.LastResult().code);
      res.push_back(init.LastResult().model);
      res.push_back(init.LastResult().n);
      if (ok) {
        for (int k = 0; k < 9; ++k) res.push_back(bits(R21.at<float>(k / 3, k % 3)));
        for (int k = 0; k < 3; ++k) res.push_back(bits(t21.at<float>(k)));
        for (bool b : vbTriangulated) res.push_back(b ? 1 : 0);
        for (const cv::Point3f& q : vP3D) {
          res.push_back(bits(q.x));
          res.push_back(bits(q.y));
          res.push_back(bits(q.z));
        }
      }
      break;
    }
    default:
      throw std::runtime_error("unknown scene op " + std::to_string(op));
  }
}

// Returns 0 on success; results in OUT as int32 arrays (see each op).
int run_scene(const std::string& in, const std::string& out) {
  const Scene s = load(in);
  std::vector<int> res;
  double ms = 0;
  run_op(s, res, &ms);
  write_ints(out, res);
  return 0;
}

// Per-call host time of the scene's method (the state rebuilt before every
// call, outside the clock): one JSON object on stdout.
int run_scene_latency(const std::string& in, int ncalls, int warm) {
  const Scene s = load(in);
  std::vector<double> t;
  int n = 0;
  for (int i = 0; i < warm + ncalls; ++i) {
    std::vector<int> res;
    double ms = 0;
    run_op(s, res, &ms);
    if (i >= warm) t.push_back(ms);
    n = res.empty() ? 0 : res[0];
  }
  std::sort(t.begin(), t.end());
  const double med = t[t.size() / 2], p99 = t[std::min(t.size() - 1, (size_t)(0.99 * (double)t.size()))];
  printf("{\"op\": %d, \"calls\": %d, \"median_ms\": %.4f, \"p99_ms\": %.4f, \"matches\": %d}\n", s.i("op"), ncalls,
         med, p99, n);
  return 0;
}
