// include/data_structure/KeyFrame.h:64-505 (the members adapter/hipLocalMapping.cc touches).
#pragma once
#include <cstddef>
#include <vector>

#include "opencv2/core/core.hpp"

namespace ORB_SLAM2 {

class MapPoint;

class KeyFrame {
 public:
  cv::Mat GetPose();
  cv::Mat GetCameraCenter();
  void AddMapPoint(MapPoint *pMP, const size_t &idx);
  bool isBad();

  long unsigned int mnId;
  const float fx, fy, cx, cy, invfx, invfy;
  const std::vector<cv::KeyPoint> mvKeysUn;
  const std::vector<float> mvuRight;
  const cv::Mat mDescriptors;
  const int mnScaleLevels;
  const std::vector<float> mvScaleFactors;
  const std::vector<float> mvLevelSigma2;
};

}  // namespace ORB_SLAM2
