// The slice of ORB_SLAM2::Frame (include/Frame.h) that the extractor and
// matcher shims read, with the reference's member names: N, mvKeys,
// mvKeysUn, mDescriptors, mBowVec, mFeatVec, mpORBvocabulary, the camera
// (static fx .. invfy, mb, mbf), stereo fields (mvKeysRight,
// mDescriptorsRight, mvuRight, mvDepth), the pose mTcw, mvpMapPoints,
// mvbOutlier, SetPose, the scale tables and the static image bounds mnMinX..mnMaxY
// (Frame.h:110-186). ComputeBoW is src/Frame.cc:394-401; ComputeStereoMatches
// (:465-639), isInFrustum (:268-324), UndistortKeyPoints (:403-433),
// ComputeImageBounds (:435-463) and ComputeStereoFromRGBD (:642-663) are the
// drop-in bodies in shim/src/Frame.cc; the RGB-D and the calibrated monocular
// constructor carry the reference's signatures (mK, mDistCoef, mThDepth,
// mfGridElementWidthInv / HeightInv). A test stand-in; a
// real build uses the reference's Frame with that one body replaced.
#ifndef ORBX_SHIM_FRAME_H
#define ORBX_SHIM_FRAME_H
#include <cmath>
#include <cstdlib>
#include <exception>
#include <thread>
#include <vector>

#include <opencv2/core/core.hpp>

#include "DBoW2.h"
#include "ORBVocabulary.h"
#include "ORBextractor.h"

namespace ORB_SLAM2 {
class MapPoint;

class Frame {
 public:
  Frame() = default;
  // The monocular constructor's extraction step (src/Frame.cc:172-190 ->
  // ExtractORB :246-252); no undistortion (mvKeysUn = mvKeys, zero
  // distortion), bounds from the image (ComputeImageBounds, :640-667).
  Frame(const cv::Mat& imGray, ORBextractor* extractor, ORBVocabulary* voc)
      : mpORBvocabulary(voc), mpORBextractorLeft(extractor) {
    scale_info();
    (*mpORBextractorLeft)(imGray, cv::noArray(), mvKeys, mDescriptors);
    N = (int)mvKeys.size();
    mvKeysUn = mvKeys;
    mvpMapPoints.assign(N, static_cast<MapPoint*>(nullptr));
    mvbOutlier.assign(N, false);
    image_bounds(imGray);
  }
  // The stereo constructor (src/Frame.cc:60-128); bf = baseline x fx, mb =
  // bf / fx. Its extraction and matching steps (:77-89) are the drop-in body
  // ExtractStereo (shim/src/Frame.cc: both extractions and ComputeStereoMatches
  // in one device round trip). ORBX_STEREO_THREADS=1 runs the reference's own
  // structure instead, for comparison: ExtractORB on two std::threads
  // (threadLeft / threadRight), an exception on either rethrown here after
  // both joined, then ComputeStereoMatches().
  Frame(const cv::Mat& imLeft, const cv::Mat& imRight, ORBextractor* extractorLeft, ORBextractor* extractorRight,
        ORBVocabulary* voc, float bf)
      : mpORBvocabulary(voc), mpORBextractorLeft(extractorLeft), mpORBextractorRight(extractorRight), mbf(bf) {
    scale_info();
    mb = mbf / fx;
    const char* th = std::getenv("ORBX_STEREO_THREADS");
    if (th && th[0] == '1') {
      std::exception_ptr errL, errR;
      std::thread threadLeft([&] {
        try {
          (*mpORBextractorLeft)(imLeft, cv::noArray(), mvKeys, mDescriptors);
        } catch (...) {
          errL = std::current_exception();
        }
      });
      std::thread threadRight([&] {
        try {
          (*mpORBextractorRight)(imRight, cv::noArray(), mvKeysRight, mDescriptorsRight);
        } catch (...) {
          errR = std::current_exception();
        }
      });
      threadLeft.join();
      threadRight.join();
      if (errL) std::rethrow_exception(errL);
      if (errR) std::rethrow_exception(errR);
      N = (int)mvKeys.size();
      ComputeStereoMatches();
    } else {
      ExtractStereo(imLeft, imRight);
    }
    mvKeysUn = mvKeys;
    image_bounds(imLeft);
    mvpMapPoints.assign(N, static_cast<MapPoint*>(nullptr));
    mvbOutlier.assign(N, false);
  }
  // Constructor for RGB-D cameras, the reference's signature (src/Frame.cc:118-170).
  // imDepth is what Tracking::GrabImageRGBD hands over: the reference converts
  // it first (src/Tracking.cc:276-277); here it may stay raw (CV_16U or
  // CV_32F) with sDepthMapFactor = Tracking's mDepthMapFactor, and only the
  // sampled pixels are converted, on the device. Extraction, UndistortKeyPoints
  // and ComputeStereoFromRGBD are one device round trip (ExtractRGBD,
  // shim/src/Frame.cc).
  Frame(const cv::Mat &imGray, const cv::Mat &imDepth, const double &timeStamp, ORBextractor* extractor,
        ORBVocabulary* voc, cv::Mat &K, cv::Mat &distCoef, const float &bf, const float &thDepth)
      : mpORBvocabulary(voc), mpORBextractorLeft(extractor), mTimeStamp(timeStamp), mK(K.clone()),
        mDistCoef(distCoef.clone()), mbf(bf), mThDepth(thDepth) {
    scale_info();
    ExtractRGBD(imGray, imDepth);
    finish_calibrated(imGray, K);
  }
  // Constructor for Monocular cameras, the reference's signature (src/Frame.cc:173-227)
  Frame(const cv::Mat &imGray, const double &timeStamp, ORBextractor* extractor, ORBVocabulary* voc, cv::Mat &K,
        cv::Mat &distCoef, const float &bf, const float &thDepth)
      : mpORBvocabulary(voc), mpORBextractorLeft(extractor), mTimeStamp(timeStamp), mK(K.clone()),
        mDistCoef(distCoef.clone()), mbf(bf), mThDepth(thDepth) {
    scale_info();
    ExtractRGBD(imGray, cv::Mat());  // no depth: mvuRight = mvDepth = -1 (:200-201)
    finish_calibrated(imGray, K);
  }
  // Undistort keypoints given OpenCV distortion parameters; a copy when k1 == 0
  // (src/Frame.cc:403-433; shim/src/Frame.cc over orbx_undistort_keypoints)
  void UndistortKeyPoints();
  // Computes image bounds for the undistorted image (:435-463, orbx_image_bounds)
  void ComputeImageBounds(const cv::Mat &imLeft);
  // Associate a "right" coordinate to a keypoint if there is valid depth in the
  // depthmap (:642-663). imDepth raw or converted, as for the RGB-D constructor.
  void ComputeStereoFromRGBD(const cv::Mat &imDepth);
  // The RGB-D constructor's ExtractORB + UndistortKeyPoints +
  // ComputeStereoFromRGBD (:134-144) in one call (orbx_rgbd_frame): mvKeys,
  // mDescriptors, N, mvKeysUn, mvuRight, mvDepth
  void ExtractRGBD(const cv::Mat &imGray, const cv::Mat &imDepth);

  void ComputeBoW() {
    if (mBowVec.empty()) {
      std::vector<cv::Mat> vCurrentDesc;  // Converter::toDescriptorVector
      vCurrentDesc.reserve(mDescriptors.rows);
      for (int j = 0; j < mDescriptors.rows; j++) vCurrentDesc.push_back(mDescriptors.row(j));
      mpORBvocabulary->transform(vCurrentDesc, mBowVec, mFeatVec, 4);
    }
  }
  // Search a match for each keypoint in the left image to a keypoint in the
  // right image (shim/src/Frame.cc, over orbm_compute_stereo_matches)
  void ComputeStereoMatches();
  // The stereo constructor's ExtractORB threads and ComputeStereoMatches
  // (src/Frame.cc:77-89) in one call (shim/src/Frame.cc): mvKeys, mDescriptors,
  // mvKeysRight, mDescriptorsRight, N, mvuRight, mvDepth
  void ExtractStereo(const cv::Mat& imLeft, const cv::Mat& imRight);
  // Check if a MapPoint is in the frustum of the camera and fill the variables
  // of the MapPoint used by the tracking (src/Frame.cc:268-324; shim/src/Frame.cc,
  // over orbm_is_in_frustum on the host). Tracking::SearchLocalPoints' loop over
  // it compiles as written; ORBmatcher::SearchLocalPoints does the loop and the
  // search that follows in one device call.
  bool isInFrustum(MapPoint* pMP, float viewingCosLimit);
  // Set the camera pose (src/Frame.cc:254-258; the stand-in keeps no mRcw / mtcw / mOw to update)
  void SetPose(cv::Mat Tcw) { mTcw = Tcw.clone(); }

  ORBVocabulary* mpORBvocabulary = nullptr;
  ORBextractor* mpORBextractorLeft = nullptr;
  ORBextractor* mpORBextractorRight = nullptr;
  double mTimeStamp = 0.0;
  // Calibration matrix and OpenCV distortion parameters (Frame.h:110-118)
  cv::Mat mK;
  cv::Mat mDistCoef;
  static float fx, fy, cx, cy, invfx, invfy;
  float mbf = 0.f, mb = 0.f;
  // Threshold close/far points (Frame.h:127-129)
  float mThDepth = 0.f;
  static float mfGridElementWidthInv, mfGridElementHeightInv;
  static bool mbInitialComputations;
  // mDepthMapFactor of Tracking (src/Tracking.cc:150-154) for a depth image
  // handed over raw; 1 = imDepth is CV_32F and already converted
  static float sDepthMapFactor;
  int N = 0;
  long unsigned int mnId = 0;
  std::vector<cv::KeyPoint> mvKeys, mvKeysRight, mvKeysUn;
  std::vector<float> mvuRight, mvDepth;
  DBoW2::BowVector mBowVec;
  DBoW2::FeatureVector mFeatVec;
  cv::Mat mDescriptors, mDescriptorsRight;
  std::vector<MapPoint*> mvpMapPoints;
  std::vector<bool> mvbOutlier;
  cv::Mat mTcw;
  int mnScaleLevels = 0;
  float mfScaleFactor = 0.f, mfLogScaleFactor = 0.f;
  std::vector<float> mvScaleFactors, mvInvScaleFactors, mvLevelSigma2, mvInvLevelSigma2;
  static float mnMinX, mnMaxX, mnMinY, mnMaxY;

 private:
  void scale_info() {  // src/Frame.cc:68-74
    mnScaleLevels = mpORBextractorLeft->GetLevels();
    mfScaleFactor = mpORBextractorLeft->GetScaleFactor();
    mfLogScaleFactor = std::log(mfScaleFactor);
    mvScaleFactors = mpORBextractorLeft->GetScaleFactors();
    mvInvScaleFactors = mpORBextractorLeft->GetInverseScaleFactors();
    mvLevelSigma2 = mpORBextractorLeft->GetScaleSigmaSquares();
    mvInvLevelSigma2 = mpORBextractorLeft->GetInverseScaleSigmaSquares();
  }
  // the calibrated constructors after their extraction (src/Frame.cc:137-169)
  void finish_calibrated(const cv::Mat& imGray, const cv::Mat& K) {
    if (mvKeys.empty()) return;
    mvpMapPoints.assign(N, static_cast<MapPoint*>(nullptr));
    mvbOutlier.assign(N, false);
    // This is done only for the first Frame (or after a change in the calibration)
    if (mbInitialComputations) {
      ComputeImageBounds(imGray);
      mfGridElementWidthInv = 64.f / (mnMaxX - mnMinX);   // FRAME_GRID_COLS
      mfGridElementHeightInv = 48.f / (mnMaxY - mnMinY);  // FRAME_GRID_ROWS
      fx = K.at<float>(0, 0);
      fy = K.at<float>(1, 1);
      cx = K.at<float>(0, 2);
      cy = K.at<float>(1, 2);
      invfx = 1.0f / fx;
      invfy = 1.0f / fy;
      mbInitialComputations = false;
    }
    mb = mbf / fx;
  }
  orbx_calib calib() const {
    orbx_calib c{mK.at<float>(0, 0), mK.at<float>(1, 1), mK.at<float>(0, 2), mK.at<float>(1, 2), 0, 0, 0, 0, 0};
    const int nd = mDistCoef.rows * mDistCoef.cols;
    c.k1 = mDistCoef.at<float>(0);
    c.k2 = mDistCoef.at<float>(1);
    c.p1 = mDistCoef.at<float>(2);
    c.p2 = mDistCoef.at<float>(3);
    c.k3 = nd > 4 ? mDistCoef.at<float>(4) : 0.f;
    return c;
  }
  static void image_bounds(const cv::Mat& im) {
    mnMinX = 0.0f;
    mnMaxX = (float)im.cols;
    mnMinY = 0.0f;
    mnMaxY = (float)im.rows;
  }
};
}  // namespace ORB_SLAM2
#endif
