// include/backend/g2oOptimizer.h:136-137 (the entry the dispatch falls back to).
#pragma once
#include "Frame.h"
#include "lidarconfig.h"
#include "pcl/kdtree/kdtree_flann.h"
#include "point_types.h"

namespace ORB_SLAM2 {

class g2oOptimizer {
 public:
  int static PoseOptimization(Frame *pFrame, PointICloudPtr local_lidarmap_cloud_ptr,
                              pcl::KdTreeFLANN<PointI>::Ptr kdtree_local_map, const lidarConfig *lidarconfig);
};

}  // namespace ORB_SLAM2
