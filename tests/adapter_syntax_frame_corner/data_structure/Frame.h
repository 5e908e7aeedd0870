// include/data_structure/Frame.h:56-59, :258-278 (the public LiDAR members only, the corner clouds included).
#pragma once
#include <vector>
#include "point_types.h"
#include "lidarconfig.h"
struct ImageIndex {
  int row = 0;
  int col = 0;
};
namespace ORB_SLAM2 {
class Frame {
 public:
  const lidarConfig *lidarconfig_;
  pcl::PointCloud<pcl::PointXYZI>::Ptr lidar_inputPtr_;
  std::vector<ImageIndex> surface_points_less_flat_index_;
  PointIRTCloud corner_points_sharp_;
  PointIRTCloud corner_points_less_sharp_;
  PointIRTCloud surface_points_flat_;
  PointIRTCloud surface_points_less_flat_;
  PointIRTCloud surface_points_flat_normal_;
  PointIRTCloud surface_points_less_flat_normal_;
};
}  // namespace ORB_SLAM2
