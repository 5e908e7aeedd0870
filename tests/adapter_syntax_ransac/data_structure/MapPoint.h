// include/data_structure/MapPoint.h:53-287 (the members adapter/hipSim3Solver.cc touches).
#pragma once
#include "opencv2/core/core.hpp"

namespace ORB_SLAM2 {

class KeyFrame;

class MapPoint {
 public:
  cv::Mat GetWorldPos();
  int GetIndexInKeyFrame(KeyFrame *pKF);
  bool isBad();

  long unsigned int mnId;
};

}  // namespace ORB_SLAM2
