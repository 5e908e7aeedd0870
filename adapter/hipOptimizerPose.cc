// hipOptimizerPose.cc — g2oOptimizer::PoseOptimization (src/backend/g2oOptimizer.cc
// :385-679) behind the reference's Optimizer seam, on libsqrtlm
// (sqlm_pose_optimize, sqlm_pose_refine_lidar), and the
// Optimizer::PoseOptimization dispatch that selects it. Like hipOptimizer.cc it
// builds inside the reference tree only.
//
// The adapter does the reference's filtering: a keypoint becomes an edge
// exactly when the reference adds one for it (:437-480: a map point and
// mvuRight < 0; the stereo branch is empty in this fork, so those keypoints get
// no edge, are not counted and keep their mvbOutlier). Between the two library
// calls the pose goes through SetPose / mTcw, a float round trip, as it does in
// the reference (:556-557, :634); the kd-tree association of the LiDAR stage
// (:560-630) stays on the host.
#include "backend/Optimizer.h"
#include "backend/g2oOptimizer.h"
#include "backend/hipOptimizer.h"

#include <cstdint>
#include <cstdlib>
#include <iostream>
#include <vector>

#include "Frame.h"
#include "MapPoint.h"
#include "lidarconfig.h"
#include "sqrtlm.h"

namespace ORB_SLAM2 {

extern Optimizer::eSolver solver;  // Optimizer.cc:26

namespace {

struct PoseCtxHolder {
  sqlm_ctx* ctx = nullptr;
  ~PoseCtxHolder() {
    if (ctx) sqlm_ctx_destroy(ctx);
  }
};

// The tracking thread's context for this call (hipOptimizer.cc keeps its own).
sqlm_ctx* pose_thread_ctx() {
  thread_local PoseCtxHolder h;
  if (!h.ctx) {
    const char* dev = std::getenv("SQLM_DEVICE");
    const int s = sqlm_ctx_create(dev ? std::atoi(dev) : -1, &h.ctx);
    if (s != SQLM_OK) {
      std::cerr << "hipOptimizer: sqlm_ctx_create failed: " << sqlm_status_string(s) << std::endl;
      h.ctx = nullptr;
    }
  }
  return h.ctx;
}

// pFrame->SetPose(Converter::toCvMat(SE3Quat(q, t))): the float matrix
void set_pose(Frame* pFrame, const double q[4], const double t[3]) {
  float T[16];
  sqlm_pose_to_Tcw_f32(q, t, T);
  cv::Mat pose(4, 4, CV_32F);
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) pose.at<float>(r, c) = T[4 * r + c];
  pFrame->SetPose(pose);
}

// Converter::toSE3Quat(pFrame->mTcw)
void get_pose(Frame* pFrame, double q[4], double t[3]) {
  float T[16];
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) T[4 * r + c] = pFrame->mTcw.at<float>(r, c);
  sqlm_pose_from_Tcw_f32(T, q, t);
}

struct LidarPairs {
  std::vector<uint8_t> kind;
  std::vector<double> pc, pw, n, info;
};

// One cloud of the frame against the local map (:575-630): the point goes to
// the world through the float inverse of the pose (pcl::transformPointCloud
// with the Affine3d built from it), its nearest map point within the distance
// threshold becomes a pair.
void associate(const PointIRTCloud& cloud, const PointIRTCloud* normals, const cv::Mat& Twc,
               const PointICloudPtr& map_cloud, const pcl::KdTreeFLANN<PointI>::Ptr& kdtree, double dist_sq,
               double weight, uint8_t kind, LidarPairs& out) {
  double M[3][4];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) M[r][c] = Twc.at<float>(r, c);
  std::vector<int> ind;
  std::vector<float> sq;
  for (size_t i = 0; i < cloud.size(); ++i) {
    const PointIRT& p = cloud[i];
    PointI w;
    w.x = static_cast<float>(M[0][0] * p.x + M[0][1] * p.y + M[0][2] * p.z + M[0][3]);
    w.y = static_cast<float>(M[1][0] * p.x + M[1][1] * p.y + M[1][2] * p.z + M[1][3]);
    w.z = static_cast<float>(M[2][0] * p.x + M[2][1] * p.y + M[2][2] * p.z + M[2][3]);
    w.intensity = p.intensity;
    kdtree->nearestKSearch(w, 1, ind, sq);
    if (!(sq[0] < dist_sq)) continue;
    const PointI& m = map_cloud->points[ind[0]];
    const double pc[3] = {p.x, p.y, p.z}, pw[3] = {m.x, m.y, m.z};
    double n[3] = {0.0, 0.0, 0.0};
    if (normals) {
      const PointIRT& q = (*normals)[i];
      n[0] = q.x;
      n[1] = q.y;
      n[2] = q.z;
    }
    out.kind.push_back(kind);
    out.pc.insert(out.pc.end(), pc, pc + 3);
    out.pw.insert(out.pw.end(), pw, pw + 3);
    out.n.insert(out.n.end(), n, n + 3);
    out.info.push_back(weight);
  }
}

}  // namespace

template <>
int hipOptimizer::PoseOptimization<pcl::KdTreeFLANN<PointI> >(Frame* pFrame, PointICloudPtr local_lidarmap_cloud_ptr,
                                                              pcl::KdTreeFLANN<PointI>::Ptr kdtree_local_map,
                                                              const lidarConfig* lidarconfig) {
  sqlm_ctx* ctx = pose_thread_ctx();
  if (!ctx) return 0;

  // :416-486: the monocular correspondences
  const int N = pFrame->N;
  std::vector<double> Xw, uv, info;
  std::vector<size_t> vnIndexEdgeMono;
  for (int i = 0; i < N; i++) {
    MapPoint* pMP = pFrame->mvpMapPoints[i];
    if (!pMP) continue;
    if (!(pFrame->mvuRight[i] < 0)) continue;  // the stereo branch is empty
    pFrame->mvbOutlier[i] = false;
    const cv::KeyPoint& kpUn = pFrame->mvKeysUn[i];
    uv.push_back(kpUn.pt.x);
    uv.push_back(kpUn.pt.y);
    info.push_back(pFrame->mvInvLevelSigma2[kpUn.octave]);
    const cv::Mat P = pMP->GetWorldPos();
    for (int c = 0; c < 3; ++c) Xw.push_back(P.at<float>(c));
    vnIndexEdgeMono.push_back(i);
  }
  const int64_t n_obs = (int64_t)vnIndexEdgeMono.size();
  if (n_obs < 3) return 0;  // :490-491

  const double intr[4] = {Frame::fx, Frame::fy, Frame::cx, Frame::cy};
  const int64_t obs_off[2] = {0, n_obs};
  const double th2 = 5.991;
  double q[4], t[3], q_out[4], t_out[3];
  get_pose(pFrame, q, t);
  int32_t n_in = 0;
  std::vector<uint8_t> outlier(n_obs, 0);
  int s = sqlm_pose_optimize(ctx, 1, q, t, intr, obs_off, Xw.data(), uv.data(), info.data(), nullptr, th2, 0.0, q_out,
                             t_out, &n_in, outlier.data(), nullptr);
  if (s != SQLM_OK) {
    std::cerr << "hipOptimizer: sqlm_pose_optimize: " << sqlm_status_string(s) << std::endl;
    return 0;
  }
  set_pose(pFrame, q_out, t_out);  // :556-557

  // :560-641: the LiDAR stage
  if (local_lidarmap_cloud_ptr->size() > 100) {
    const cv::Mat Twc = pFrame->mTcw.inv();  // toCvMat(estimate).inv(): the float matrix SetPose stored
    LidarPairs lp;
    if (lidarconfig->using_flat_point)
      associate(pFrame->surface_points_flat_, &pFrame->surface_points_flat_normal_, Twc, local_lidarmap_cloud_ptr,
                kdtree_local_map, lidarconfig->distance_sq_threshold, lidarconfig->flat_optimized_weight, 0, lp);
    if (lidarconfig->using_sharp_point)
      associate(pFrame->corner_points_sharp_, nullptr, Twc, local_lidarmap_cloud_ptr, kdtree_local_map,
                lidarconfig->distance_sq_threshold, lidarconfig->corner_optimized_weight, 1, lp);
    const int64_t lid_off[2] = {0, (int64_t)lp.kind.size()};
    const uint8_t robust_on = n_obs < 10 ? 1 : 0;  // the round that removes the kernels never ran
    const std::vector<uint8_t> outlier_in = outlier;
    get_pose(pFrame, q, t);  // :634 setEstimate(toSE3Quat(pFrame->mTcw))
    s = sqlm_pose_refine_lidar(ctx, 1, q, t, intr, obs_off, Xw.data(), uv.data(), info.data(), outlier_in.data(),
                               &robust_on, lid_off, lp.kind.data(), lp.pc.data(), lp.pw.data(), lp.n.data(),
                               lp.info.data(), nullptr, th2, 0.0, q_out, t_out, &n_in, outlier.data(), nullptr);
    if (s != SQLM_OK) {
      std::cerr << "hipOptimizer: sqlm_pose_refine_lidar: " << sqlm_status_string(s) << std::endl;
      return 0;
    }
    set_pose(pFrame, q_out, t_out);  // :639-640
  }

  // :648-675: mvbOutlier of the counted keypoints only
  for (int64_t k = 0; k < n_obs; ++k) pFrame->mvbOutlier[vnIndexEdgeMono[k]] = outlier[k] != 0;
  return n_in;
}

int Optimizer::PoseOptimization(Frame* pFrame, PointICloudPtr local_lidarmap_cloud_ptr,
                                pcl::KdTreeFLANN<PointI>::Ptr kdtree_local_map, const lidarConfig* lidarconfig) {
  if (solver == Optimizer::HIP)
    return hipOptimizer::PoseOptimization(pFrame, local_lidarmap_cloud_ptr, kdtree_local_map, lidarconfig);
  // the reference's body (Optimizer.cc:49-65; its Ceres and MyOptimizer branches stay as they are, elided here)
  return g2oOptimizer::PoseOptimization(pFrame, local_lidarmap_cloud_ptr, kdtree_local_map, lidarconfig);
}

}  // namespace ORB_SLAM2
