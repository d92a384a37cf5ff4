// Optimizer over liborbx: the reference's Optimizer::PoseOptimization
// (include/Optimizer.h:53, src/Optimizer.cc:334-543) with its signature, the
// per-frame pose solve of Tracking. The other optimisers (bundle adjustment,
// the essential graph, Sim3) stay with g2o in a real build.
#ifndef ORBX_SHIM_OPTIMIZER_H
#define ORBX_SHIM_OPTIMIZER_H
#include "Frame.h"
#include "MapPoint.h"

namespace ORB_SLAM2 {

class Optimizer {
 public:
  // Reads pFrame's mvKeysUn, mvuRight, mvpMapPoints, mvInvLevelSigma2, the
  // camera and mTcw; writes mvbOutlier where a keypoint holds a MapPoint and
  // calls SetPose. Returns nInitialCorrespondences - nBad. One device round
  // trip (orbm_pose_optimization) on the thread's matcher workspace.
  int static PoseOptimization(Frame* pFrame);
};

}  // namespace ORB_SLAM2
#endif
