// hipOptimizer.h — libsqrtlm behind the reference's Optimizer seam.
//
// Drop-in sibling of g2oOptimizer (src/backend/g2oOptimizer.cc) for the
// calls the MI355X backend implements: LocalBundleAdjustment,
// BundleAdjustment, GlobalBundleAdjustemnt, OptimizeEssentialGraph,
// OptimizeSim3 and PoseOptimization (include/backend/Optimizer.h:50-69).
// It is meant to be added to the reference tree as include/backend/hipOptimizer.h
// + src/backend/hipOptimizer.cc and selected in Optimizer.cc's dispatch
// (see INTEGRATION.md §4); it builds against the reference's own headers and
// links libsqrtlm.so. It is not compiled in this repository: the reference's
// dependencies (OpenCV, PCL, Eigen, ROS) are absent here.
//
// Capture: with SQLM_CAPTURE_DIR set, every call also writes its seam inputs
// (and, in capture mode, the g2o backend's write-back) as a sqrtlm_capture.h
// file, replayable on a GPU box with tools/sqlm_replay.
#ifndef HIP_OPTIMIZER_H
#define HIP_OPTIMIZER_H

#include <map>
#include <set>
#include <vector>

#include "Eigen/Core"
#include "LoopClosing.h"
#include "pcl/kdtree/kdtree_flann.h"
#include "point_types.h"

// global, as in the reference (include/utils/lidarconfig.h:7 declares it
// outside namespace ORB_SLAM2; a forward declaration inside the namespace
// would name a different, incomplete type)
struct lidarConfig;
struct sqlm_ctx;

namespace ORB_SLAM2 {

class KeyFrame;
class MapPoint;
class Map;
class Frame;

class hipOptimizer {
 public:
  // g2oOptimizer::LocalBundleAdjustment (g2oOptimizer.cc:704-1191) on the GPU.
  static void LocalBundleAdjustment(KeyFrame* pKF, bool* pbStopFlag, Map* pMap, const lidarConfig* cfg);
  // g2oOptimizer::BundleAdjustment (g2oOptimizer.cc:110-362) on the GPU.
  static void BundleAdjustment(const std::vector<KeyFrame*>& vpKFs, const std::vector<MapPoint*>& vpMP,
                               int nIterations, bool* pbStopFlag, unsigned long nLoopKF, bool bRobust);
  // g2oOptimizer::GlobalBundleAdjustemnt (g2oOptimizer.cc:80-95): every KF and MP of the map.
  static void GlobalBundleAdjustemnt(Map* pMap, int nIterations, bool* pbStopFlag, unsigned long nLoopKF,
                                     bool bRobust);
  // g2oOptimizer::OptimizeEssentialGraph (g2oOptimizer.cc:1212-1534) on the GPU
  // (sqlm_eg_*): same vertices, edges, insertion order and write-back.
  static void OptimizeEssentialGraph(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF,
                                     const LoopClosing::KeyFrameAndPose& NonCorrectedSim3,
                                     const LoopClosing::KeyFrameAndPose& CorrectedSim3,
                                     const std::map<KeyFrame*, std::set<KeyFrame*> >& LoopConnections,
                                     const bool& bFixScale);
  // g2oOptimizer::OptimizeSim3 (g2oOptimizer.cc:1560-1793) on the GPU
  // (sqlm_sim3_optimize, adapter/hipOptimizerSim3.cc): returns the inlier
  // count, updates g2oS12 and clears the rejected entries of vpMatches1.
  static int OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches1,
                          g2o::Sim3& g2oS12, const float th2, const bool bFixScale);
  // g2oOptimizer::PoseOptimization (g2oOptimizer.cc:385-679) on the GPU
  // (sqlm_pose_optimize / sqlm_pose_refine_lidar, adapter/hipOptimizerPose.cc):
  // sets the frame's pose and the counted keypoints' mvbOutlier, returns the
  // inlier count. Tree is never given: the default makes this the reference's
  // signature (g2oOptimizer.h:136-137), and keeps the kd-tree's pointer type a
  // dependent name for translation units that never call it.
  template <typename Tree = pcl::KdTreeFLANN<PointI> >
  static int PoseOptimization(Frame* pFrame, PointICloudPtr local_lidarmap_cloud_ptr,
                              typename Tree::Ptr kdtree_local_map, const lidarConfig* lidarconfig);

  // Capture mode around the g2o backend (Optimizer.cc dispatch): Begin*
  // records the seam inputs, End* the g2o write-back, then the file is written.
  static void BeginCaptureLBA(KeyFrame* pKF);
  static void EndCaptureLBA();
  static void BeginCaptureBA(const std::vector<KeyFrame*>& vpKFs, const std::vector<MapPoint*>& vpMP,
                             int nIterations, bool bRobust);
  static void EndCaptureBA(unsigned long nLoopKF);
  // One-line hook for g2oOptimizer.cc:1062-1070 in capture mode: the LiDAR
  // flat pair the reference's kd-tree found for pass 3.
  static void CaptureLidarFlat(const Eigen::Vector3d& p_cam, const Eigen::Vector3d& p_world,
                               const Eigen::Vector3d& normal, double weight);
  // The same for the corner pair of g2oOptimizer.cc:1097-1103 (EdgeLidarCornerPoint).
  static void CaptureLidarCorner(const Eigen::Vector3d& curr_point, const Eigen::Vector3d& near_point, double weight);
  // LocalBundleAdjustment pass 3 with using_sharp_point (hipOptimizerLidar.cc):
  // the flat set (using_flat_point) and the corner set of pKF against the
  // clouds of map_kfs, one sqlm_set_lidar_from_cloud_sets call. map_Twc
  // [map_kfs.size()][16] and cur_Twc [16] are the float T_wc of the pass-2
  // poses; n_pairs receives {flat, corner}. false: the library failed.
  static bool LidarCloudSets(sqlm_ctx* ctx, KeyFrame* pKF, const std::vector<KeyFrame*>& map_kfs, int pose_index,
                             const float* map_Twc, const float* cur_Twc, const lidarConfig* cfg, long long n_pairs[2]);
  static bool CaptureEnabled();
};

}  // namespace ORB_SLAM2

#endif
