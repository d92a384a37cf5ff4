// The device part of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:237-485)
// as one free function: every neighbour's SearchForTriangulation in one
// batched search, the triangulation of all their matches in one launch chain,
// and ComputeDistinctiveDescriptors / UpdateNormalAndDepth of the new points
// in one refresh, with nothing read back in between. The caller keeps what the
// reference does with a new point on the host:
//
//   for (const NewMapPoint& q : CreateNewMapPoints(mpCurrentKeyFrame, vpNeighKFs, mbMonocular)) {
//     MapPoint* pMP = new MapPoint(q.x3D, mpCurrentKeyFrame, mpMap);
//     pMP->AddObservation(mpCurrentKeyFrame, q.idx1);
//     pMP->AddObservation(q.pKF2, q.idx2);
//     mpCurrentKeyFrame->AddMapPoint(pMP, q.idx1);
//     q.pKF2->AddMapPoint(pMP, q.idx2);
//     // q.descriptor, q.normal, q.minDistance, q.maxDistance are what
//     // ComputeDistinctiveDescriptors() and UpdateNormalAndDepth() would compute
//     mpMap->AddMapPoint(pMP);
//     mlpRecentAddedMapPoints.push_back(pMP);
//   }
//
// The points come in the reference's creation order (neighbour, then idx1); a
// keypoint of the current keyframe gets its point from the first neighbour
// that yields one, as in the reference's sequential loop.
#ifndef ORBX_SHIM_LOCALMAPPING_H
#define ORBX_SHIM_LOCALMAPPING_H

#include <vector>

#include <opencv2/core/core.hpp>

#include "KeyFrame.h"

namespace ORB_SLAM2 {

struct NewMapPoint {
  cv::Mat x3D;       // 3x1 CV_32F
  KeyFrame* pKF2;    // the neighbour
  size_t idx1, idx2; // keypoints of the current keyframe and of pKF2
  int kind;          // ORBM_NEWPT_TRIANGULATED / UNPROJECT1 / UNPROJECT2
  cv::Mat descriptor;  // 1x32 CV_8U
  cv::Mat normal;      // 3x1 CV_32F
  float minDistance, maxDistance;
};

// vpNeighKFs: GetBestCovisibilityKeyFrames(nn). With bMonocular false the
// baseline test of :282-286 (baseline < pKF2->mb) is applied here; the
// monocular test (:287-294) needs ComputeSceneMedianDepth and stays with the
// caller, who passes the neighbours that passed it.
std::vector<NewMapPoint> CreateNewMapPoints(KeyFrame* pCurrentKF, const std::vector<KeyFrame*>& vpNeighKFs,
                                            bool bMonocular);

}  // namespace ORB_SLAM2

#endif
