// Optimizer::PoseOptimization over orbm_pose_optimization: the frame's map
// points become one table of orbm_map_point_world records (position and
// Observations() > 0) in keypoint order, assign[i] the row of keypoint i's
// point, and the call's flags and pose go back into the frame as the
// reference leaves them (src/Optimizer.cc:383, :417, :489-495, :518-525, :540).
#include "Optimizer.h"

#include <stdexcept>
#include <string>

#include "ORBmatcher.h"

namespace ORB_SLAM2 {

int Optimizer::PoseOptimization(Frame* pFrame) {
  const int N = pFrame->N;
  std::vector<int> assign(N, -1);
  std::vector<orbm_map_point_world> mps;
  mps.reserve(N);
  for (int i = 0; i < N; i++) {
    MapPoint* pMP = pFrame->mvpMapPoints[i];
    if (!pMP) continue;
    orbm_map_point_world r{};
    const cv::Mat Xw = pMP->GetWorldPos();
    for (int k = 0; k < 3; ++k) r.pos[k] = Xw.at<float>(k);
    r.valid = 1;
    r.obs_positive = pMP->Observations() > 0;
    assign[i] = (int)mps.size();
    mps.push_back(r);
  }
  orbm_camera cam{Frame::fx, Frame::fy, Frame::cx, Frame::cy, pFrame->mb, pFrame->mbf, {}};
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 4; ++k) cam.Tcw[4 * r + k] = pFrame->mTcw.at<float>(r, k);
  std::vector<uint8_t> outlier(N > 0 ? N : 1, 0);
  for (int i = 0; i < N; i++) outlier[i] = pFrame->mvbOutlier[i] ? 1 : 0;
  float Tcw[12];
  orbm_poseopt_result res{};
  const int rc = orbm_pose_optimization(
      ORBmatcher::Handle(), reinterpret_cast<const orbx_kp*>(pFrame->mvKeysUn.data()), N,
      pFrame->mvuRight.empty() ? nullptr : pFrame->mvuRight.data(), assign.data(), mps.data(), (int)mps.size(),
      pFrame->mvInvLevelSigma2.data(), (int)pFrame->mvInvLevelSigma2.size(), &cam, 0, Tcw, nullptr, outlier.data(),
      &res);
  if (rc != ORBX_OK) throw std::runtime_error(std::string("liborbx: ") + orbm_last_error());
  for (int i = 0; i < N; i++)
    if (assign[i] >= 0) pFrame->mvbOutlier[i] = outlier[i] != 0;
  if (res.n_initial < 3) return 0;  // :456, the pose is not set
  cv::Mat pose(4, 4, CV_32F);
  for (int r = 0; r < 4; ++r)
    for (int k = 0; k < 4; ++k) pose.at<float>(r, k) = r < 3 ? Tcw[4 * r + k] : (r == k ? 1.f : 0.f);
  pFrame->SetPose(pose);
  return res.ret;
}

}  // namespace ORB_SLAM2
