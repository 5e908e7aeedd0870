// hipOptimizerLidar.cc — LocalBundleAdjustment pass 3 with corner points
// (g2oOptimizer.cc:978-1107, using_sharp_point): the part of the adapter that
// reads KeyFrame::corner_points_less_sharp_ and
// lidarConfig::corner_optimized_weight. Added to the reference tree as
// src/backend/hipOptimizerLidar.cc next to hipOptimizer.cc.
//
// Up to two searches in one library call (sqlm_set_lidar_from_cloud_sets), in
// the reference's insertion order:
//   flat    (using_flat_point)   surface_points_less_flat_ of the other local
//           KFs as the map, pKF's as the queries with their normals,
//           flat_optimized_weight                      -> EdgeLidarFlatPoint
//   corner  (using_sharp_point)  corner_points_less_sharp_ likewise, no
//           normals, corner_optimized_weight           -> EdgeLidarCornerPoint
// Both use the float Twc the caller computed per keyframe (Converter::toCvMat
// then cv::Mat::inv(), hipOptimizer.cc) and the same distance_sq_threshold.
#include "hipOptimizer.h"

#include <cstdint>
#include <iostream>
#include <vector>

#include "KeyFrame.h"
#include "lidarconfig.h"
#include "sqrtlm.h"

namespace ORB_SLAM2 {

namespace {

void pack(const PointIRTCloud& cloud, std::vector<float>& xyz) {
  for (size_t i = 0; i < cloud.size(); ++i) {
    const PointIRT& p = cloud.points[i];
    xyz.insert(xyz.end(), {p.x, p.y, p.z});
  }
}

// the map of one kind: the clouds of the other local KFs, each in its own sensor frame
struct CloudMap {
  std::vector<int64_t> off{0};
  std::vector<float> xyz;
  void add(const PointIRTCloud& cloud) {
    pack(cloud, xyz);
    off.push_back((int64_t)(xyz.size() / 3));
  }
};

}  // namespace

bool hipOptimizer::LidarCloudSets(sqlm_ctx* ctx, KeyFrame* pKF, const std::vector<KeyFrame*>& map_kfs,
                                  int pose_index, const float* map_Twc, const float* cur_Twc,
                                  const lidarConfig* cfg, long long n_pairs[2]) {
  n_pairs[0] = n_pairs[1] = 0;
  if (!cfg) return true;
  CloudMap flat_map, corner_map;
  std::vector<float> flat_q, flat_n, corner_q;
  for (KeyFrame* k : map_kfs) {
    if (cfg->using_flat_point) flat_map.add(k->surface_points_less_flat_);
    if (cfg->using_sharp_point) corner_map.add(k->corner_points_less_sharp_);
  }
  sqlm_lidar_set sets[2];
  int kind_of[2] = {0, 0}, n_sets = 0;
  auto add_set = [&](int kind, const CloudMap& m, const std::vector<float>& q, const float* normal, double info) {
    if (m.xyz.empty()) return;  // the reference would hand an empty cloud to the kd-tree
    sqlm_lidar_set& s = sets[n_sets];
    s.kind = kind;
    s.n_map_clouds = (int32_t)m.off.size() - 1;
    s.map_off = m.off.data();
    s.map_xyz = m.xyz.data();
    s.map_Twc = map_Twc;
    s.n_query = (int64_t)(q.size() / 3);
    s.query_xyz = q.data();
    s.query_Twc = cur_Twc;
    s.query_normal = normal;
    s.info = info;
    s.dist_sq_threshold = cfg->distance_sq_threshold;
    kind_of[n_sets++] = kind;
  };
  if (cfg->using_flat_point) {  // :1034-1070
    pack(pKF->surface_points_less_flat_, flat_q);
    pack(pKF->surface_points_less_flat_normal_, flat_n);
    add_set(0, flat_map, flat_q, flat_n.data(), cfg->flat_optimized_weight);
  }
  if (cfg->using_sharp_point) {  // :1075-1107
    pack(pKF->corner_points_less_sharp_, corner_q);
    add_set(1, corner_map, corner_q, nullptr, cfg->corner_optimized_weight);
  }
  int64_t got[2] = {0, 0};
  const int s = sqlm_set_lidar_from_cloud_sets(ctx, pose_index, n_sets, sets, got);
  if (s != SQLM_OK) {
    std::cerr << "hipOptimizer: sqlm_set_lidar_from_cloud_sets: " << sqlm_status_string(s) << std::endl;
    return false;
  }
  for (int k = 0; k < n_sets; ++k) n_pairs[kind_of[k]] = got[k];
  return true;
}

}  // namespace ORB_SLAM2
