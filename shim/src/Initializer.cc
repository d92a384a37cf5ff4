// Initializer over orbm_initialize (see include/Initializer.h). The arrays are
// those SearchForInitialization works on: mvKeysUn of both frames and
// vMatches12 = mvIniMatches, the index in the current frame per keypoint of
// the reference frame or -1 (src/Tracking.cc:674-682).
#include "Initializer.h"

#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>

#include "ORBmatcher.h"

namespace ORB_SLAM2 {

namespace {

const orbx_kp* kps(const std::vector<cv::KeyPoint>& v) {
  static_assert(sizeof(cv::KeyPoint) == sizeof(orbx_kp), "cv::KeyPoint and orbx_kp share their layout");
  return reinterpret_cast<const orbx_kp*>(v.data());
}

// DUtils::Random::SeedRandOnce(0) (Thirdparty/DBoW2/DUtils/Random.cpp:36-45)
void SeedRandOnce(int seed) {
  static bool already_seeded = false;
  if (!already_seeded) {
    srand((unsigned)seed);
    already_seeded = true;
  }
}

}  // namespace

Initializer::Initializer(const Frame& ReferenceFrame, float sigma, int iterations) {
  mK = ReferenceFrame.mK.clone();
  mvKeys1 = ReferenceFrame.mvKeysUn;
  mSigma = sigma;
  mSigma2 = sigma * sigma;
  mMaxIterations = iterations;
  std::memset(&mLast, 0, sizeof mLast);
}

bool Initializer::Initialize(const Frame& CurrentFrame, const std::vector<int>& vMatches12, cv::Mat& R21, cv::Mat& t21,
                             std::vector<cv::Point3f>& vP3D, std::vector<bool>& vbTriangulated) {
  const std::vector<cv::KeyPoint>& mvKeys2 = CurrentFrame.mvKeysUn;
  const int n1 = (int)mvKeys1.size(), n2 = (int)mvKeys2.size();
  // mvMatches12 is built from vMatches12's entries (:54): one per keypoint of frame 1, absent ones unmatched
  std::vector<int> m12(n1 > 0 ? n1 : 1, -1);
  for (int i = 0; i < n1 && i < (int)vMatches12.size(); ++i) m12[i] = vMatches12[i];
  orbm_camera cam{};
  cam.fx = mK.at<float>(0, 0);
  cam.fy = mK.at<float>(1, 1);
  cam.cx = mK.at<float>(0, 2);
  cam.cy = mK.at<float>(1, 2);
  orbm_init_params P{mSigma, mMaxIterations, 1.0f, 50};  // :116, :118
  // Generate sets of 8 points for each RANSAC iteration (:78-97): the rand() values now, the draws on the device
  SeedRandOnce(0);
  std::vector<uint32_t> rand8(8 * (size_t)(mMaxIterations > 0 ? mMaxIterations : 1), 0u);
  orbm_initializer_rand_fill(rand8.data(), mMaxIterations);
  float R[9] = {}, t[3] = {};
  std::vector<float> p3d(3 * (size_t)(n1 > 0 ? n1 : 1), 0.f);
  std::vector<uint8_t> tri(n1 > 0 ? n1 : 1, 0);
  const int rc = orbm_initialize(ORBmatcher::Handle(), kps(mvKeys1), n1, kps(mvKeys2), n2, m12.data(), &cam, &P,
                                 rand8.data(), &mLast, R, t, nullptr, p3d.data(), tri.data(), nullptr, nullptr, nullptr,
                                 nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  if (rc != ORBX_OK) throw std::runtime_error(std::string("liborbx: ") + orbm_last_error());
  if (!mLast.ok) return false;
  R21.create(3, 3, CV_32F);
  t21.create(3, 1, CV_32F);
  for (int k = 0; k < 9; ++k) R21.at<float>(k / 3, k % 3) = R[k];
  for (int k = 0; k < 3; ++k) t21.at<float>(k) = t[k];
  vP3D.resize(n1);
  vbTriangulated.assign(n1, false);
  for (int i = 0; i < n1; ++i) {
    vP3D[i] = cv::Point3f(p3d[3 * i], p3d[3 * i + 1], p3d[3 * i + 2]);
    vbTriangulated[i] = tri[i] != 0;
  }
  return true;
}

}  // namespace ORB_SLAM2
