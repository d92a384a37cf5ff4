// Frame's statics (src/Frame.cc:31-34 defines them for the reference) and the
// drop-in body of Frame::ComputeStereoMatches (src/Frame.cc:465-639): the
// keypoints, descriptors and pyramids of the two extractors' last calls are
// matched where they lie on the device (orbm_compute_stereo_matches_last),
// which fills mvuRight and mvDepth (-1 where a keypoint has no stereo match);
// and of Frame::isInFrustum (:268-324) over orbm_is_in_frustum.
#include "Frame.h"

#include "MapPoint.h"

#include <stdexcept>
#include <string>

#include "ORBmatcher.h"

namespace ORB_SLAM2 {
float Frame::fx, Frame::fy, Frame::cx, Frame::cy, Frame::invfx, Frame::invfy;
float Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY;

void Frame::ComputeStereoMatches() {
  mvuRight = std::vector<float>(N, -1.0f);
  mvDepth = std::vector<float>(N, -1.0f);
  if (N == 0) return;
  int kept = 0;
  // the stereo constructor calls this right after its two extractions
  // (src/Frame.cc:77-89): the keypoints and descriptors are read where those
  // calls left them on the device, only mvuRight / mvDepth come back
  const int rc = orbm_compute_stereo_matches_last(ORBmatcher::Handle(), mpORBextractorLeft->handle(),
                                                  mpORBextractorRight->handle(), mb, mbf, mvuRight.data(),
                                                  mvDepth.data(), N, &kept);
  if (rc != ORBX_OK) throw std::runtime_error(std::string("liborbx: ") + orbm_last_error());
}

// One point through orbm_is_in_frustum (host arithmetic, no device call):
// the same float / double operations as the reference's cv::Mat expressions,
// so the mTrack* fields are the reference's bit for bit.
bool Frame::isInFrustum(MapPoint* pMP, float viewingCosLimit) {
  pMP->mbTrackInView = false;
  orbm_camera cam{fx, fy, cx, cy, mb, mbf, {}};
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 4; ++k) cam.Tcw[4 * r + k] = mTcw.at<float>(r, k);
  orbm_pose pose;
  orbm_map_point_world rec{};
  const cv::Mat P = pMP->GetWorldPos(), Pn = pMP->GetNormal();
  for (int k = 0; k < 3; ++k) {
    rec.pos[k] = P.at<float>(k);
    rec.normal[k] = Pn.at<float>(k);
  }
  rec.min_distance = pMP->mfMinDistance;
  rec.max_distance = pMP->mfMaxDistance;
  rec.valid = 1;
  orbm_map_point_proj o;
  int n = 0;
  if (orbm_prepare_pose(ORBM_PROJ_KEYFRAME, &cam, nullptr, 0, &pose) != ORBX_OK ||
      orbm_is_in_frustum(&pose, {mnMinX, mnMaxX, mnMinY, mnMaxY}, mfScaleFactor, mnScaleLevels, viewingCosLimit, &rec,
                         1, &o, &n) != ORBX_OK)
    throw std::runtime_error(std::string("liborbx: ") + orbm_last_error());
  if (!o.track_in_view) return false;
  pMP->mbTrackInView = true;
  pMP->mTrackProjX = o.proj_x;
  pMP->mTrackProjXR = o.proj_xr;
  pMP->mTrackProjY = o.proj_y;
  pMP->mnTrackScaleLevel = o.predicted_level;
  pMP->mTrackViewCos = o.view_cos;
  return true;
}

// The stereo constructor's extraction and matching steps (src/Frame.cc:77-89:
// ExtractORB on threadLeft / threadRight, N = mvKeys.size(), then
// ComputeStereoMatches) as one call with one device round trip: both
// extraction chains are issued from this thread and run concurrently on the
// device, the stereo kernel follows them there, and the keypoints,
// descriptors, mvuRight and mvDepth come back together (orbm_stereo_frame).
// Same results as those steps.
void Frame::ExtractStereo(const cv::Mat& imLeft, const cv::Mat& imRight) {
  ORBextractor::ExtractStereo(*mpORBextractorLeft, *mpORBextractorRight, imLeft, imRight, ORBmatcher::Handle(), mb, mbf,
                              mvKeys, mDescriptors, mvKeysRight, mDescriptorsRight, mvuRight, mvDepth);
  N = (int)mvKeys.size();
}
}  // namespace ORB_SLAM2
