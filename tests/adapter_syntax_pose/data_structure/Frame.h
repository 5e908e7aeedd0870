// include/data_structure/Frame.h:170-428 (the members PoseOptimization touches).
#pragma once
#include <vector>
#include "opencv2/core/core.hpp"
#include "point_types.h"
namespace ORB_SLAM2 {
class MapPoint;
class Frame {
 public:
  void SetPose(cv::Mat Tcw);
  PointIRTCloud corner_points_sharp_;
  PointIRTCloud surface_points_flat_;
  PointIRTCloud surface_points_flat_normal_;
  static float fx;
  static float fy;
  static float cx;
  static float cy;
  int N;
  std::vector<cv::KeyPoint> mvKeysUn;
  std::vector<float> mvuRight;
  std::vector<MapPoint *> mvpMapPoints;
  std::vector<bool> mvbOutlier;
  cv::Mat mTcw;
  std::vector<float> mvInvLevelSigma2;
};
}  // namespace ORB_SLAM2
