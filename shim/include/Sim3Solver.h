// Sim3Solver over liborbx: the reference's public surface (include/Sim3Solver.h:
// 35-49, src/Sim3Solver.cc) with its signatures. The constructor gathers the
// arrays orbm_sim3_ransac takes; the first iterate() / find() draws the rand()
// values of all mRansacMaxIts iterations (orbm_sim3_rand_fill) and makes one
// device call that computes every hypothesis and keeps their inlier counts;
// later iterate(k) calls replay the reference's bookkeeping from the counts and
// go back to the device only for the flags of a later acceptance.
// The draws therefore come from the same rand() stream as the reference's, but
// all at the first call instead of interleaved with other solvers' draws.
#ifndef ORBX_SHIM_SIM3SOLVER_H
#define ORBX_SHIM_SIM3SOLVER_H
#include <vector>

#include <opencv2/core/core.hpp>

#include "KeyFrame.h"
#include "MapPoint.h"
#include "orbx_c.h"

namespace ORB_SLAM2 {

class Sim3Solver {
 public:
  Sim3Solver(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<MapPoint*>& vpMatched12, const bool bFixScale = true);

  void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300);

  cv::Mat find(std::vector<bool>& vbInliers12, int& nInliers);

  cv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers);

  cv::Mat GetEstimatedRotation();
  cv::Mat GetEstimatedTranslation();
  float GetEstimatedScale();

 protected:
  // one orbm_sim3_ransac call from iteration `first` with mnBestInliers = best
  void Run(int first, int best, bool keep_hyp);

  // the constructor's gather, in the arrays of the C ABI
  std::vector<orbx_kp> mvKeys1, mvKeys2;
  std::vector<orbm_map_point_world> mvPoints1, mvPoints2;
  std::vector<int> mvMatch12, mvIndexKF1;
  std::vector<float> mvLevelSigma2;
  orbm_camera mCam1, mCam2;
  int mN1;
  bool mbFixScale;

  // SetRansacParameters
  double mRansacProb;
  int mRansacMinInliers, mRansacMaxIts;

  // the state iterate() keeps (mnIterations, mnBestInliers, mBest*) and what the device calls left
  bool mbComputed;
  int mnIterations, mnBestInliers, mnBestIteration;
  std::vector<uint32_t> mvRand3;
  std::vector<orbm_sim3_hyp> mvHyp;  // of the first call: every hypothesis
  orbm_sim3_result mFirst, mLast;
  std::vector<uint8_t> mvInlier;
  orbm_pose mPoses[2];
};

}  // namespace ORB_SLAM2
#endif
