// include/data_structure/KeyFrame.h:64-442 (the members adapter/hipSim3Solver.cc touches).
#pragma once
#include <vector>

#include "opencv2/core/core.hpp"

namespace ORB_SLAM2 {

class MapPoint;

class KeyFrame {
 public:
  cv::Mat GetRotation();
  cv::Mat GetTranslation();
  std::vector<MapPoint *> GetMapPointMatches();
  bool isBad();

  long unsigned int mnId;
  const std::vector<cv::KeyPoint> mvKeysUn;
  const std::vector<float> mvLevelSigma2;
  const std::vector<float> mvInvLevelSigma2;
  const cv::Mat mK;
};

}  // namespace ORB_SLAM2
