// Frame's statics (src/Frame.cc:31-34 defines them for the reference) and the
// drop-in body of Frame::ComputeStereoMatches (src/Frame.cc:465-639): the
// keypoints, descriptors and pyramids of the two extractors' last calls are
// matched where they lie on the device (orbm_compute_stereo_matches_last),
// which fills mvuRight and mvDepth (-1 where a keypoint has no stereo match);
// of Frame::isInFrustum (:268-324) over orbm_is_in_frustum; and of the
// calibrated constructors' tail: UndistortKeyPoints (:403-433),
// ComputeImageBounds (:435-463), ComputeStereoFromRGBD (:642-663) and the
// RGB-D constructor's one-round-trip ExtractRGBD (orbx_rgbd_frame).
#include "Frame.h"

#include "MapPoint.h"

#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>

#include "ORBmatcher.h"

namespace ORB_SLAM2 {
float Frame::fx, Frame::fy, Frame::cx, Frame::cy, Frame::invfx, Frame::invfy;
float Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY;
float Frame::mfGridElementWidthInv, Frame::mfGridElementHeightInv;
bool Frame::mbInitialComputations = true;
float Frame::sDepthMapFactor = 1.0f;

static void extractor_check(int rc) {
  if (rc != ORBX_OK) throw std::runtime_error(std::string("liborbx: ") + orbx_last_error());
}

// Frame::UndistortKeyPoints (src/Frame.cc:403-433): cv::undistortPoints with
// mK as the new camera matrix, on the device (orbx_undistort_keypoints); the
// k1 == 0 copy (:405-409) is the library's.
void Frame::UndistortKeyPoints() {
  mvKeysUn.resize(N);
  const orbx_calib c = calib();
  extractor_check(orbx_undistort_keypoints(&c, reinterpret_cast<const orbx_kp*>(mvKeys.data()), N,
                                           reinterpret_cast<orbx_kp*>(mvKeysUn.data())));
}

// Frame::ComputeImageBounds (src/Frame.cc:435-463), host arithmetic
void Frame::ComputeImageBounds(const cv::Mat& imLeft) {
  const orbx_calib c = calib();
  orbm_grid_bounds b;
  extractor_check(orbx_image_bounds(&c, imLeft.cols, imLeft.rows, &b));
  mnMinX = b.min_x;
  mnMaxX = b.max_x;
  mnMinY = b.min_y;
  mnMaxY = b.max_y;
}

// Frame::ComputeStereoFromRGBD (src/Frame.cc:642-663) from mvKeys / mvKeysUn
// as they stand: the device samples and converts the depth pixel under every
// distorted keypoint (orbx_frame_tail_batch with no distortion, whose depth
// output is read); mvuRight is then the reference's own expression on the
// frame's mvKeysUn.
void Frame::ComputeStereoFromRGBD(const cv::Mat& imDepth) {
  mvuRight = std::vector<float>(N, -1);
  mvDepth = std::vector<float>(N, -1);
  if (N == 0 || imDepth.empty()) return;
  if (imDepth.type() != CV_16U && imDepth.type() != CV_32F)
    throw std::runtime_error("liborbx: the depth image must be CV_16U or CV_32F");
  const size_t es = imDepth.elemSize(), row = (size_t)imDepth.cols * es, img_bytes = row * imDepth.rows;
  const size_t kp_bytes = (size_t)N * sizeof(orbx_kp);
  // one device block: count (16 bytes) | keypoints | their copy | uRight | depth | image
  const size_t o_kp = 16, o_un = o_kp + kp_bytes, o_ur = o_un + kp_bytes, o_dp = o_ur + (size_t)N * 4;
  const size_t o_img = (o_dp + (size_t)N * 4 + 15) & ~(size_t)15;
  void* d = nullptr;
  extractor_check(orbx_malloc(&d, o_img + img_bytes));
  struct Free {
    void* p;
    ~Free() { orbx_free(p); }
  } guard{d};
  uint8_t* b = static_cast<uint8_t*>(d);
  std::vector<uint8_t> packed(img_bytes);
  for (int r = 0; r < imDepth.rows; ++r) memcpy(packed.data() + (size_t)r * row, imDepth.ptr<uint8_t>(r), row);
  extractor_check(orbx_memcpy_htod(b, &N, sizeof N));
  extractor_check(orbx_memcpy_htod(b + o_kp, mvKeys.data(), kp_bytes));
  extractor_check(orbx_memcpy_htod(b + o_img, packed.data(), img_bytes));
  const orbx_calib none{1.f, 1.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  extractor_check(orbx_frame_tail_batch(&none, reinterpret_cast<const orbx_kp*>(b + o_kp),
                                        reinterpret_cast<const int*>(b), N, 1, b + o_img,
                                        imDepth.type() == CV_32F ? ORBX_DEPTH_F32 : ORBX_DEPTH_U16, img_bytes, row,
                                        imDepth.cols, imDepth.rows, sDepthMapFactor, mbf,
                                        reinterpret_cast<orbx_kp*>(b + o_un), reinterpret_cast<float*>(b + o_ur),
                                        reinterpret_cast<float*>(b + o_dp), nullptr));
  extractor_check(orbx_memcpy_dtoh(mvDepth.data(), b + o_dp, (size_t)N * 4));  // after the kernel (null stream)
  for (int i = 0; i < N; i++) {
    const float d_i = mvDepth[i];
    if (d_i > 0) mvuRight[i] = mvKeysUn[i].pt.x - mbf / d_i;
  }
}

// The RGB-D constructor's ExtractORB, N = mvKeys.size(), UndistortKeyPoints
// and ComputeStereoFromRGBD (src/Frame.cc:134-144) as one call with one device
// round trip (orbx_rgbd_frame): the raw depth image is uploaded beside the gray
// image, the tail kernel follows the extraction on the device and everything
// comes back together. An empty imDepth: the monocular constructor's steps.
void Frame::ExtractRGBD(const cv::Mat& imGray, const cv::Mat& imDepth) {
  const orbx_calib c = calib();
  mpORBextractorLeft->ExtractRGBD(imGray, imDepth, c, sDepthMapFactor, mbf, mvKeys, mDescriptors, mvKeysUn, mvuRight,
                                  mvDepth);
  N = (int)mvKeys.size();
}

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
