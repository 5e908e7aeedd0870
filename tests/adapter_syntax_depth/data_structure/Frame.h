// include/data_structure/Frame.h:259-262, :307-310, :334-367 (the public members the depth adapter uses).
#pragma once
#include <vector>
#include <opencv2/core/core.hpp>
#include "point_types.h"
namespace ORB_SLAM2 {
class Frame {
 public:
  cv::Mat Depthimg_;
  pcl::PointCloud<pcl::PointXYZI>::Ptr lidar_inputPtr_;
  static float fx;
  static float fy;
  static float cx;
  static float cy;
  int N;
  std::vector<cv::KeyPoint> mvKeys;
  std::vector<cv::KeyPoint> mvKeysUn;
  std::vector<float> mvDepth;
};
}  // namespace ORB_SLAM2
