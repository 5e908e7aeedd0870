// include/data_structure/Frame.h:60-520 (the members adapter/hipPnPsolver.cc touches).
#pragma once
#include <vector>

#include "opencv2/core/core.hpp"

namespace ORB_SLAM2 {

class MapPoint;

class Frame {
 public:
  static float fx;
  static float fy;
  static float cx;
  static float cy;
  std::vector<cv::KeyPoint> mvKeysUn;
  std::vector<MapPoint *> mvpMapPoints;
  std::vector<float> mvLevelSigma2;
};

}  // namespace ORB_SLAM2
