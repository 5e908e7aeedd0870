// PCL 1.x pcl::KdTreeFLANN subset (kdtree/include/pcl/kdtree/kdtree_flann.h) with its Ptr.
#pragma once
#include <memory>
#include <vector>
#include "pcl/point_cloud.h"
namespace pcl {
template <typename PointT>
class KdTreeFLANN {
 public:
  typedef std::shared_ptr<KdTreeFLANN<PointT>> Ptr;
  void setInputCloud(const typename PointCloud<PointT>::ConstPtr &cloud);
  int nearestKSearch(const PointT &point, int k, std::vector<int> &k_indices, std::vector<float> &k_sqr_distances) const;
};
}  // namespace pcl
