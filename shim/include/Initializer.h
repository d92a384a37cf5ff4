// Initializer over liborbx: the reference's public surface (include/Initializer.h:
// 31-95, src/Initializer.cc:33-121) with its signatures. The constructor keeps
// the reference frame's mK and mvKeysUn; Initialize draws the 8 x iterations
// rand() values of mvSets from the C library's stream (seeded once with 0, as
// DUtils::Random::SeedRandOnce(0) does for the first Initializer of a process)
// and makes one device call (orbm_initialize) that computes both RANSACs, the
// model choice and the reconstruction. Where Initialize returns false R21, t21,
// vP3D and vbTriangulated are left as they were.
#ifndef ORBX_SHIM_INITIALIZER_H
#define ORBX_SHIM_INITIALIZER_H
#include <vector>

#include <opencv2/core/core.hpp>

#include "Frame.h"
#include "orbx_c.h"

namespace ORB_SLAM2 {

// THIS IS THE INITIALIZER FOR MONOCULAR SLAM. NOT USED IN THE STEREO OR RGBD CASE.
class Initializer {
  typedef std::pair<int, int> Match;

 public:
  // Fix the reference frame
  Initializer(const Frame& ReferenceFrame, float sigma = 1.0, int iterations = 200);

  // Computes in parallel a fundamental matrix and a homography
  // Selects a model and tries to recover the motion and the structure from motion
  bool Initialize(const Frame& CurrentFrame, const std::vector<int>& vMatches12, cv::Mat& R21, cv::Mat& t21,
                  std::vector<cv::Point3f>& vP3D, std::vector<bool>& vbTriangulated);

  // what the last Initialize left besides its outputs (not in the reference)
  const orbm_init_result& LastResult() const { return mLast; }

 private:
  // Keypoints from Reference Frame (Frame 1)
  std::vector<cv::KeyPoint> mvKeys1;

  // Calibration
  cv::Mat mK;

  // Standard Deviation and Variance
  float mSigma, mSigma2;

  // Ransac max iterations
  int mMaxIterations;

  orbm_init_result mLast;
};

}  // namespace ORB_SLAM2
#endif
