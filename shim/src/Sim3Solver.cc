// Sim3Solver over orbm_sim3_ransac (see include/Sim3Solver.h). The arrays are
// those the matcher calls around it take: mvKeysUn of both keyframes, one
// orbm_map_point_world per keypoint, match12[i1] = the keypoint of pKF2 that
// holds vpMatched12[i1] (GetIndexInKeyFrame, src/Sim3Solver.cc:76), kp_index1 =
// pMP1->GetIndexInKeyFrame(pKF1) (:75). mvLevelSigma2 is pKF1's for both
// keyframes (one extractor configuration serves a map).
#include "Sim3Solver.h"

#include <cstring>
#include <stdexcept>
#include <string>

#include "ORBmatcher.h"

namespace ORB_SLAM2 {

namespace {

std::vector<orbx_kp> keys_of(KeyFrame* pKF) {
  static_assert(sizeof(cv::KeyPoint) == sizeof(orbx_kp), "cv::KeyPoint and orbx_kp share their layout");
  std::vector<orbx_kp> v(pKF->mvKeysUn.size());
  if (!v.empty()) std::memcpy(v.data(), pKF->mvKeysUn.data(), v.size() * sizeof(orbx_kp));
  return v;
}

orbm_map_point_world record_of(MapPoint* pMP) {
  orbm_map_point_world r{};
  if (!pMP) return r;
  const cv::Mat Xw = pMP->GetWorldPos();
  for (int k = 0; k < 3; ++k) r.pos[k] = Xw.at<float>(k);
  r.valid = pMP->isBad() ? 0 : 1;
  return r;
}

orbm_camera camera_of(KeyFrame* pKF) {
  orbm_camera c{pKF->fx, pKF->fy, pKF->cx, pKF->cy, pKF->mb, pKF->mbf, {}};
  const cv::Mat T = pKF->GetPose();
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 4; ++k) c.Tcw[4 * r + k] = T.at<float>(r, k);
  return c;
}

}  // namespace

Sim3Solver::Sim3Solver(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<MapPoint*>& vpMatched12, const bool bFixScale)
    : mbFixScale(bFixScale), mbComputed(false), mnIterations(0), mnBestInliers(0), mnBestIteration(-1) {
  mvKeys1 = keys_of(pKF1);
  mvKeys2 = keys_of(pKF2);
  mN1 = (int)vpMatched12.size();
  const std::vector<MapPoint*> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
  const std::vector<MapPoint*> vpKeyFrameMP2 = pKF2->GetMapPointMatches();
  mvKeys1.resize(mN1);
  mvPoints1.resize(mN1);
  mvPoints2.resize(mvKeys2.size());
  for (size_t i2 = 0; i2 < mvPoints2.size(); ++i2) mvPoints2[i2] = record_of(vpKeyFrameMP2[i2]);
  mvMatch12.assign(mN1, -1);
  mvIndexKF1.resize(mN1);
  for (int i1 = 0; i1 < mN1; i1++) {
    MapPoint* pMP1 = i1 < (int)vpKeyFrameMP1.size() ? vpKeyFrameMP1[i1] : static_cast<MapPoint*>(NULL);
    mvPoints1[i1] = record_of(pMP1);
    mvIndexKF1[i1] = pMP1 ? pMP1->GetIndexInKeyFrame(pKF1) : i1;
    MapPoint* pMP2 = vpMatched12[i1];
    if (!pMP2) continue;
    const int indexKF2 = pMP2->GetIndexInKeyFrame(pKF2);
    if (indexKF2 < 0 || indexKF2 >= (int)mvPoints2.size()) continue;
    mvMatch12[i1] = indexKF2;
    mvPoints2[indexKF2] = record_of(pMP2);
  }
  mvLevelSigma2 = pKF1->mvLevelSigma2;
  mCam1 = camera_of(pKF1);
  mCam2 = camera_of(pKF2);
  std::memset(&mFirst, 0, sizeof mFirst);
  std::memset(&mLast, 0, sizeof mLast);
  std::memset(mPoses, 0, sizeof mPoses);
  SetRansacParameters();
}

void Sim3Solver::SetRansacParameters(double probability, int minInliers, int maxIterations) {
  mRansacProb = probability;
  mRansacMinInliers = minInliers;
  mRansacMaxIts = maxIterations;
  mnIterations = 0;
  mbComputed = false;
}

void Sim3Solver::Run(int first, int best, bool keep_hyp) {
  orbm_sim3_params P{};
  P.probability = mRansacProb;
  P.min_inliers = mRansacMinInliers;
  P.max_iterations = mRansacMaxIts;
  P.fix_scale = mbFixScale ? 1 : 0;
  P.first_iteration = first;
  P.best_inliers = best;
  mvInlier.assign(mN1 > 0 ? mN1 : 1, 0);
  if (keep_hyp) mvHyp.assign(mRansacMaxIts, orbm_sim3_hyp{});
  float s12 = 0.f, R12[9] = {}, t12[3] = {};
  const int rc = orbm_sim3_ransac(ORBmatcher::Handle(), mvKeys1.data(), mN1, mvKeys2.data(), (int)mvKeys2.size(),
                                  mvPoints1.data(), mvPoints2.data(), &mCam1, &mCam2, mvMatch12.data(),
                                  mvIndexKF1.data(), mvLevelSigma2.data(), (int)mvLevelSigma2.size(), &P,
                                  mvRand3.data(), &mLast, &s12, R12, t12, mPoses, mvInlier.data(),
                                  keep_hyp ? mvHyp.data() : nullptr);
  if (rc != ORBX_OK) throw std::runtime_error(std::string("liborbx: ") + orbm_last_error());
}

cv::Mat Sim3Solver::iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
  bNoMore = false;
  vbInliers = std::vector<bool>(mN1, false);
  nInliers = 0;
  if (!mbComputed) {
    // every iteration's three rand() values now, then every hypothesis in one call
    mvRand3.assign(3 * (size_t)mRansacMaxIts, 0u);
    orbm_sim3_rand_fill(mvRand3.data(), mRansacMaxIts);
    mnBestInliers = 0;
    mnBestIteration = -1;
    Run(0, 0, true);
    mFirst = mLast;
    mbComputed = true;
  }
  if (mFirst.max_its == 0) {  // N < mRansacMinInliers
    bNoMore = true;
    return cv::Mat();
  }
  int nCurrentIterations = 0;
  while (mnIterations < mFirst.max_its && nCurrentIterations < nIterations) {
    nCurrentIterations++;
    const int h = mnIterations++;
    const int count = mvHyp[h].count;
    if (count >= mnBestInliers) {
      const int bestBefore = mnBestInliers;
      mnBestInliers = count;
      mnBestIteration = h;
      if (count > mRansacMinInliers) {
        // the flags and T12 of hypothesis h: the first call's when it accepted this one, else a resumed call
        if (!(mLast.ret > 0 && mLast.iterations == h + 1)) Run(h, bestBefore, false);
        nInliers = mLast.ret;
        for (int i = 0; i < mN1; i++)
          if (mvInlier[i]) vbInliers[i] = true;
        cv::Mat T12(4, 4, CV_32F);  // [s*R | t], the second transform of pKF2 -> pKF1
        for (int r = 0; r < 4; ++r)
          for (int k = 0; k < 4; ++k) T12.at<float>(r, k) = r < 3 ? mPoses[1].Rt2[4 * r + k] : (r == k ? 1.f : 0.f);
        return T12;
      }
    }
  }
  if (mnIterations >= mFirst.max_its) bNoMore = true;
  return cv::Mat();
}

cv::Mat Sim3Solver::find(std::vector<bool>& vbInliers12, int& nInliers) {
  bool bFlag;
  return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);
}

cv::Mat Sim3Solver::GetEstimatedRotation() {
  cv::Mat R(3, 3, CV_32F);
  for (int k = 0; k < 9; ++k) R.at<float>(k / 3, k % 3) = mnBestIteration >= 0 ? mvHyp[mnBestIteration].R[k] : 0.f;
  return R;
}

cv::Mat Sim3Solver::GetEstimatedTranslation() {
  cv::Mat t(3, 1, CV_32F);
  for (int k = 0; k < 3; ++k) t.at<float>(k) = mnBestIteration >= 0 ? mvHyp[mnBestIteration].t[k] : 0.f;
  return t;
}

float Sim3Solver::GetEstimatedScale() { return mnBestIteration >= 0 ? mvHyp[mnBestIteration].s : 0.f; }

}  // namespace ORB_SLAM2
