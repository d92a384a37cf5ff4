// Optimizer::PoseOptimization over orbm_pose_optimization: the frame's map
// points become one table of orbm_map_point_world records (position and
// Observations() > 0) in keypoint order, assign[i] the row of keypoint i's
// point, and the call's flags and pose go back into the frame as the
// reference leaves them (src/Optimizer.cc:383, :417, :489-495, :518-525, :540).
//
// Optimizer::OptimizeSim3 over orbm_optimize_sim3: mvKeysUn of both keyframes,
// one orbm_map_point_world per keypoint, match12[i1] = the keypoint of pKF2
// that holds vpMatches1[i1] (GetIndexInKeyFrame, src/Optimizer.cc:1254; an
// entry without one forms no edge and stays as it is). The call's match12_out
// nulls the rejected entries (:1340, :1374).
#include "Optimizer.h"

#include <cstring>
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

namespace {

orbm_map_point_world sim3_record_of(MapPoint* pMP) {
  orbm_map_point_world r{};
  if (!pMP) return r;
  const cv::Mat Xw = pMP->GetWorldPos();
  for (int k = 0; k < 3; ++k) r.pos[k] = Xw.at<float>(k);
  r.valid = pMP->isBad() ? 0 : 1;
  return r;
}

orbm_camera sim3_camera_of(KeyFrame* pKF) {
  orbm_camera c{pKF->fx, pKF->fy, pKF->cx, pKF->cy, pKF->mb, pKF->mbf, {}};
  const cv::Mat T = pKF->GetPose();
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 4; ++k) c.Tcw[4 * r + k] = T.at<float>(r, k);
  return c;
}

}  // namespace

int Optimizer::OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches1, g2o::Sim3& g2oS12,
                            const float th2, const bool bFixScale) {
  static_assert(sizeof(cv::KeyPoint) == sizeof(orbx_kp), "cv::KeyPoint and orbx_kp share their layout");
  const int N = (int)vpMatches1.size(), n2 = (int)pKF2->mvKeysUn.size();
  const std::vector<MapPoint*> vpMapPoints1 = pKF1->GetMapPointMatches();
  const std::vector<MapPoint*> vpMapPoints2 = pKF2->GetMapPointMatches();
  std::vector<orbx_kp> keys1(N > 0 ? N : 1), keys2(n2 > 0 ? n2 : 1);
  for (int i = 0; i < N && i < (int)pKF1->mvKeysUn.size(); ++i) std::memcpy(&keys1[i], &pKF1->mvKeysUn[i], sizeof(orbx_kp));
  if (n2) std::memcpy(keys2.data(), pKF2->mvKeysUn.data(), n2 * sizeof(orbx_kp));
  std::vector<orbm_map_point_world> mps1(N > 0 ? N : 1), mps2(n2 > 0 ? n2 : 1);
  for (int i2 = 0; i2 < n2; ++i2) mps2[i2] = sim3_record_of(vpMapPoints2[i2]);
  std::vector<int> match12(N > 0 ? N : 1, -1), out(N > 0 ? N : 1, -1);
  for (int i = 0; i < N; i++) {
    mps1[i] = sim3_record_of(i < (int)vpMapPoints1.size() ? vpMapPoints1[i] : static_cast<MapPoint*>(NULL));
    MapPoint* pMP2 = vpMatches1[i];
    if (!pMP2) continue;
    const int i2 = pMP2->GetIndexInKeyFrame(pKF2);
    if (i2 < 0 || i2 >= n2) continue;  // :1258, no edge
    match12[i] = i2;
    mps2[i2] = sim3_record_of(pMP2);
  }
  const orbm_camera cam1 = sim3_camera_of(pKF1), cam2 = sim3_camera_of(pKF2);
  double R[9];
  if (g2oS12.has_matrix)
    std::memcpy(R, g2oS12.R0, sizeof R);
  else
    g2oS12.rotationMatrix(R);
  float R12[9], t12[3];
  for (int k = 0; k < 9; ++k) R12[k] = (float)R[k];
  for (int k = 0; k < 3; ++k) t12[k] = (float)g2oS12.t[k];
  const float s12 = (float)g2oS12.s;
  double S12[8];
  orbm_optsim3_result res{};
  const int rc = orbm_optimize_sim3(ORBmatcher::Handle(), keys1.data(), N, keys2.data(), n2, mps1.data(), mps2.data(),
                                    &cam1, &cam2, match12.data(), nullptr, nullptr, nullptr,
                                    pKF1->mvInvLevelSigma2.data(), (int)pKF1->mvInvLevelSigma2.size(), &s12, R12, t12,
                                    th2, bFixScale ? 1 : 0, out.data(), S12, nullptr, nullptr, &res, nullptr);
  if (rc != ORBX_OK) throw std::runtime_error(std::string("liborbx: ") + orbm_last_error());
  for (int i = 0; i < N; i++)
    if (match12[i] >= 0 && out[i] < 0) vpMatches1[i] = static_cast<MapPoint*>(NULL);
  if (res.rounds < 2) return 0;  // :1355, g2oS12 is not written
  g2oS12 = g2o::Sim3(S12, S12 + 4, S12[7]);
  return res.ret;
}

}  // namespace ORB_SLAM2
