// hipFrameLidarCorner.cc — hipFrameLidar::ExtractFeatures (hipFrameLidar.h): the
// flat and the corner branch of Frame::ExtractFeaturePoints on one
// sqlm_lidar_features_all call. What stays here is the packing of the input
// cloud and lidarConfig and the filling of the frame's clouds.
#include <cmath>
#include <cstdint>
#include <iostream>
#include <vector>

#include "hipFrameLidar.h"
#include "hipFrameLidarDetail.h"
#include "sqrtlm.h"

namespace ORB_SLAM2 {

namespace {

using namespace frame_lidar_detail;

void FillCornerParams(const lidarConfig& c, sqlm_lidar_corner_params& p) {
  p.max_corner_sharp = c.max_corner_sharp;
  p.max_corner_less_sharp = c.max_corner_less_sharp;
  p.sharp_curv_th = c.sharp_curv_th;
  p.ground_z_bound = c.ground_z_bound;
  // Frame.cc:862
  for (int i = 0; i < SQLM_LF_MAX_ROWS; i++)
    p.corner_ring_enabled[i] = c.lower_ring_num_sharp_point <= i + 1 && i < c.upper_ring_num_sharp_point;
}

bool ExtractAll(Frame* pF, const double* extrinsic) {
  if (!pF || !pF->lidarconfig_ || !pF->lidar_inputPtr_) return false;
  const lidarConfig& cfg = *pF->lidarconfig_;
  std::vector<pcl::PointXYZI>& in = pF->lidar_inputPtr_->points;
  // the finite points (removeNaNFromPointCloud, :1246-1248); the cloud itself changes only on success
  std::vector<float> xyz;
  xyz.reserve(3 * in.size() + 3);
  for (size_t i = 0; i < in.size(); i++)
    if (std::isfinite(in[i].x) && std::isfinite(in[i].y) && std::isfinite(in[i].z)) {
      xyz.push_back(in[i].x);
      xyz.push_back(in[i].y);
      xyz.push_back(in[i].z);
    }
  const size_t n = xyz.size() / 3, m = n ? n : 1;
  const bool flat = cfg.using_flat_point, corner = cfg.using_sharp_point;
  std::vector<float> fx, fn, lx, ln, sx, cx;
  std::vector<int32_t> rc, clabel, crc;
  int64_t foff[2] = {0, 0}, loff[2] = {0, 0}, soff[2] = {0, 0}, coff[2] = {0, 0};
  if (flat || corner) {
    sqlm_ctx* ctx = frame_thread_ctx();
    if (!ctx) return false;
    sqlm_lidar_feat_params prm;
    sqlm_lidar_corner_params cprm;
    FillParams(cfg, prm);
    FillCornerParams(cfg, cprm);
    xyz.resize(3 * m);
    if (flat) {
      fx.resize(3 * m);
      fn.resize(3 * m);
      lx.resize(3 * m);
      ln.resize(3 * m);
      rc.resize(2 * m);
    }
    if (corner) {
      sx.resize(3 * m);
      cx.resize(3 * m);
      clabel.resize(m);
      crc.resize(2 * m);
    }
    const int64_t off[2] = {0, (int64_t)n};
    const int s = sqlm_lidar_features_all(
        ctx, 1, off, xyz.data(), &prm, corner ? &cprm : nullptr, extrinsic, flat ? foff : nullptr,
        flat ? fx.data() : nullptr, flat ? fn.data() : nullptr, flat ? loff : nullptr, flat ? lx.data() : nullptr,
        flat ? ln.data() : nullptr, flat ? rc.data() : nullptr, corner ? soff : nullptr, corner ? sx.data() : nullptr,
        corner ? coff : nullptr, corner ? cx.data() : nullptr, corner ? clabel.data() : nullptr,
        corner ? crc.data() : nullptr);
    if (s != SQLM_OK) {
      std::cerr << "hipFrameLidar: sqlm_lidar_features_all failed: " << sqlm_status_string(s) << std::endl;
      return false;
    }
  }
  size_t kept = 0;
  for (size_t i = 0; i < in.size(); i++)
    if (std::isfinite(in[i].x) && std::isfinite(in[i].y) && std::isfinite(in[i].z)) in[kept++] = in[i];
  in.resize(kept);
  // the flat members, as ExtractFlatFeatures fills them
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
  // the corner members: a sharp point is one of the first max_corner_sharp less-sharp points of its subregion
  size_t sh = 0;
  for (int64_t k = 0; k < coff[1]; k++) {
    PointIRT p = MakePoint(&cx[3 * k], crc[2 * k]);
    p.intensity = (float)clabel[k];  // :1016
    pF->corner_points_less_sharp_.push_back(p);
    if (sh < (size_t)soff[1] && sx[3 * sh] == cx[3 * k] && sx[3 * sh + 1] == cx[3 * k + 1] &&
        sx[3 * sh + 2] == cx[3 * k + 2]) {
      pF->corner_points_sharp_.push_back(p);
      sh++;
    }
  }
  return true;
}

}  // namespace

bool hipFrameLidar::ExtractFeatures(Frame* pF) { return ExtractAll(pF, nullptr); }

bool hipFrameLidar::ExtractFeatures(Frame* pF, const Eigen::Matrix<double, 4, 4>& extrinsicMatrix) {
  double ext[16];
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) ext[4 * r + c] = extrinsicMatrix(r, c);
  return ExtractAll(pF, ext);
}

}  // namespace ORB_SLAM2
