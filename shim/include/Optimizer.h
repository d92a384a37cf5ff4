// Optimizer over liborbx: the reference's Optimizer::PoseOptimization
// (include/Optimizer.h:53, src/Optimizer.cc:334-543), the per-frame pose solve
// of Tracking, and Optimizer::OptimizeSim3 (include/Optimizer.h:57,
// src/Optimizer.cc:1190-1385), the refinement of a loop candidate's Sim3, each
// with its signature. The other optimisers (the bundle adjustments and the
// essential graph) stay with g2o in a real build.
#ifndef ORBX_SHIM_OPTIMIZER_H
#define ORBX_SHIM_OPTIMIZER_H
#include <vector>

#include "Frame.h"
#include "KeyFrame.h"
#include "MapPoint.h"
#include "Sim3.h"

namespace ORB_SLAM2 {

class Optimizer {
 public:
  // Reads pFrame's mvKeysUn, mvuRight, mvpMapPoints, mvInvLevelSigma2, the
  // camera and mTcw; writes mvbOutlier where a keypoint holds a MapPoint and
  // calls SetPose. Returns nInitialCorrespondences - nBad. One device round
  // trip (orbm_pose_optimization) on the thread's matcher workspace.
  int static PoseOptimization(Frame* pFrame);

  // Reads both keyframes' mvKeysUn, GetMapPointMatches(), camera and pose,
  // pKF1's mvInvLevelSigma2 (one extractor configuration serves a map) and
  // vpMatches1[i] = the MapPoint of pKF2 matched to keypoint i of pKF1; nulls
  // the entries whose edges either check rejected and writes g2oS12 unless the
  // function returns before its second optimisation (fewer than 10 pairs left).
  // Returns nIn. g2oS12 goes in as the floats it was built from (its matrix, or
  // its quaternion's when it has none). One device round trip
  // (orbm_optimize_sim3) on the thread's matcher workspace.
  static int OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches1, g2o::Sim3& g2oS12,
                          const float th2, const bool bFixScale);
};

}  // namespace ORB_SLAM2
#endif
