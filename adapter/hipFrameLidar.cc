// hipFrameLidar.cc — see hipFrameLidar.h. What stays here is what the reference
// does with its own objects: packing the input cloud and lidarConfig into plain
// arrays and filling the frame's clouds. The arithmetic is the library's.
#include "hipFrameLidar.h"

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <iostream>
#include <vector>

#include "hipFrameLidarDetail.h"
#include "sqrtlm.h"

namespace ORB_SLAM2 {

namespace {

struct FrameCtxHolder {
  sqlm_ctx* ctx = nullptr;
  ~FrameCtxHolder() {
    if (ctx) sqlm_ctx_destroy(ctx);
  }
};

}  // namespace

namespace frame_lidar_detail {

// one context per calling thread (Tracking's)
sqlm_ctx* frame_thread_ctx() {
  thread_local FrameCtxHolder h;
  if (!h.ctx) {
    const char* dev = std::getenv("SQLM_DEVICE");
    const int s = sqlm_ctx_create(dev ? std::atoi(dev) : -1, &h.ctx);
    if (s != SQLM_OK) {
      std::cerr << "hipFrameLidar: sqlm_ctx_create failed: " << sqlm_status_string(s) << std::endl;
      h.ctx = nullptr;
    }
  }
  return h.ctx;
}

void FillParams(const lidarConfig& c, sqlm_lidar_feat_params& p) {
  p.row_num = c.row_num_;
  p.col_num = c.col_num_;
  p.num_scan_subregions = c.num_scan_subregions;
  p.num_curvature_regions_flat = c.num_curvature_regions_flat;
  p.num_curvature_regions_corner = c.num_curvature_regions_corner;
  p.max_surf_flat = c.max_surf_flat;
  p.max_surf_less_flat = c.max_surf_less_flat;
  p.using_sharp_point = c.using_sharp_point ? 1 : 0;
  p.surf_curv_th = c.surf_curv_th;
  p.max_sq_dis = c.max_sq_dis;
  p.deg_diff = c.deg_diff;
  // Frame.cc:1042-1045; the fourth range is compared against its lower bound at both ends there
  for (int i = 0; i < SQLM_LF_MAX_ROWS; i++) {
    const int r = i + 1;
    p.ring_enabled[i] = (c.lower_ring_num_x_rot <= r && r <= c.upper_ring_num_x_rot) ||
                        (c.lower_ring_num_y_rot <= r && r <= c.upper_ring_num_y_rot) ||
                        (c.lower_ring_num_z_trans <= r && r <= c.upper_ring_num_z_trans) ||
                        (c.lower_ring_num_z_rot_xy_trans <= r && r <= c.lower_ring_num_z_rot_xy_trans);
  }
}

PointIRT MakePoint(const float* xyz, int row) {
  PointIRT p;
  p.x = xyz[0];
  p.y = xyz[1];
  p.z = xyz[2];
  p.intensity = 0;
  p.ring = (uint16_t)row;
  p.timestamp = 0.1;
  return p;
}

}  // namespace frame_lidar_detail

namespace {

using namespace frame_lidar_detail;

bool Extract(Frame* pF, const double* extrinsic) {
  if (!pF || !pF->lidarconfig_ || !pF->lidar_inputPtr_) return false;
  const lidarConfig& cfg = *pF->lidarconfig_;
  if (cfg.using_sharp_point) return false;
  // removeNaNFromPointCloud in place (:1246-1248): the later stages of the constructor read the same cloud
  std::vector<pcl::PointXYZI>& in = pF->lidar_inputPtr_->points;
  size_t kept = 0;
  for (size_t i = 0; i < in.size(); i++)
    if (std::isfinite(in[i].x) && std::isfinite(in[i].y) && std::isfinite(in[i].z)) in[kept++] = in[i];
  in.resize(kept);
  if (!cfg.using_flat_point) return true;
  sqlm_ctx* ctx = frame_thread_ctx();
  if (!ctx) return false;
  sqlm_lidar_feat_params prm;
  FillParams(cfg, prm);
  const size_t n = in.size(), m = n ? n : 1;
  std::vector<float> xyz(3 * m), fx(3 * m), fn(3 * m), lx(3 * m), ln(3 * m);
  std::vector<int32_t> rc(2 * m);
  for (size_t i = 0; i < n; i++) {
    xyz[3 * i] = in[i].x;
    xyz[3 * i + 1] = in[i].y;
    xyz[3 * i + 2] = in[i].z;
  }
  const int64_t off[2] = {0, (int64_t)n};
  int64_t foff[2] = {0, 0}, loff[2] = {0, 0};
  const int s = sqlm_lidar_features(ctx, 1, off, xyz.data(), &prm, extrinsic, foff, fx.data(), fn.data(), loff,
                                    lx.data(), ln.data(), rc.data());
  if (s != SQLM_OK) {
    std::cerr << "hipFrameLidar: sqlm_lidar_features failed: " << sqlm_status_string(s) << std::endl;
    return false;
  }
  // the flat points are the first max_surf_flat less-flat points of their subregion, in the same order:
  // walk both lists together to give a flat point its row
  size_t f = 0;
  for (int64_t k = 0; k < loff[1]; k++) {
    const int row = rc[2 * k];
    pF->surface_points_less_flat_.push_back(MakePoint(&lx[3 * k], row));
    pF->surface_points_less_flat_normal_.push_back(MakePoint(&ln[3 * k], row));
    ImageIndex idx;
    idx.row = row;
    idx.col = rc[2 * k + 1];
    pF->surface_points_less_flat_index_.push_back(idx);
    if (f < (size_t)foff[1] && fx[3 * f] == lx[3 * k] && fx[3 * f + 1] == lx[3 * k + 1] &&
        fx[3 * f + 2] == lx[3 * k + 2]) {
      pF->surface_points_flat_.push_back(MakePoint(&fx[3 * f], row));
      pF->surface_points_flat_normal_.push_back(MakePoint(&fn[3 * f], row));
      f++;
    }
  }
  for (; f < (size_t)foff[1]; f++) {  // not reached: every flat point is a less-flat point
    pF->surface_points_flat_.push_back(MakePoint(&fx[3 * f], 0));
    pF->surface_points_flat_normal_.push_back(MakePoint(&fn[3 * f], 0));
  }
  return true;
}

}  // namespace

bool hipFrameLidar::ExtractFlatFeatures(Frame* pF) { return Extract(pF, nullptr); }

bool hipFrameLidar::ExtractFlatFeatures(Frame* pF, const Eigen::Matrix<double, 4, 4>& extrinsicMatrix) {
  double ext[16];
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) ext[4 * r + c] = extrinsicMatrix(r, c);
  return Extract(pF, ext);
}

}  // namespace ORB_SLAM2
