// include/backend/Optimizer.h:42-71 with the maintainer's one-line change
// (eSolver gains HIP): the entry adapter/hipOptimizerPose.cc defines.
#pragma once
#include "Frame.h"
#include "lidarconfig.h"
#include "pcl/kdtree/kdtree_flann.h"
#include "point_types.h"

namespace ORB_SLAM2 {

class Optimizer {
 public:
  enum eSolver { CERES = 0, G2O = 1, MYOPT = 2, HIP = 3 };

  int static PoseOptimization(Frame *pFrame, PointICloudPtr local_lidarmap_cloud_ptr,
                              pcl::KdTreeFLANN<PointI>::Ptr kdtree_local_map, const lidarConfig *lidarconfig);
};

}  // namespace ORB_SLAM2
