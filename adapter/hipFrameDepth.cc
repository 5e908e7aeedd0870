// hipFrameDepth.cc — see hipFrameDepth.h. What stays here is what the reference
// does with its own objects: packing the input cloud and the keypoints into
// plain arrays and filling the frame's members. The arithmetic is the library's.
#include "hipFrameDepth.h"

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>

#include "sqrtlm.h"

namespace ORB_SLAM2 {

namespace {

struct DepthCtxHolder {
  sqlm_ctx* ctx = nullptr;
  ~DepthCtxHolder() {
    if (ctx) sqlm_ctx_destroy(ctx);
  }
};

// one context per calling thread (Tracking's)
sqlm_ctx* depth_thread_ctx() {
  thread_local DepthCtxHolder h;
  if (!h.ctx) {
    const char* dev = std::getenv("SQLM_DEVICE");
    const int s = sqlm_ctx_create(dev ? std::atoi(dev) : -1, &h.ctx);
    if (s != SQLM_OK) {
      std::cerr << "hipFrameDepth: sqlm_ctx_create failed: " << sqlm_status_string(s) << std::endl;
      h.ctx = nullptr;
    }
  }
  return h.ctx;
}

bool Associate(Frame* pF, const Eigen::Matrix<double, 3, 4>& K, const Eigen::Matrix<double, 4, 4>& E,
               std::vector<cv::Point3f>* vP3Dc) {
  if (!pF || !pF->lidar_inputPtr_) return false;
  cv::Mat& img = pF->Depthimg_;
  if (img.empty() || img.type() != CV_64F || !img.isContinuous()) return false;
  const size_t m = pF->mvKeys.size();
  if (pF->mvDepth.size() != m || (vP3Dc && pF->mvKeysUn.size() != m)) return false;
  sqlm_ctx* ctx = depth_thread_ctx();
  if (!ctx) return false;
  const std::vector<pcl::PointXYZI>& in = pF->lidar_inputPtr_->points;
  const size_t n = in.size();
  std::vector<float> xyz(3 * n + 1), key(2 * m + 1), key_un(vP3Dc ? 2 * m + 1 : 0), depth(m + 1), pcam(vP3Dc ? 3 * m + 1 : 0);
  std::vector<int32_t> cls(m + 1), uv(2 * m + 1);
  std::vector<double> image((size_t)img.rows * img.cols);
  for (size_t i = 0; i < n; i++) {
    xyz[3 * i] = in[i].x;
    xyz[3 * i + 1] = in[i].y;
    xyz[3 * i + 2] = in[i].z;
  }
  for (size_t i = 0; i < m; i++) {
    key[2 * i] = pF->mvKeys[i].pt.x;
    key[2 * i + 1] = pF->mvKeys[i].pt.y;
    if (vP3Dc) {
      key_un[2 * i] = pF->mvKeysUn[i].pt.x;
      key_un[2 * i + 1] = pF->mvKeysUn[i].pt.y;
    }
  }
  double k[12], e[16];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 4; c++) k[4 * r + c] = K(r, c);
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) e[4 * r + c] = E(r, c);
  const float cam[4] = {Frame::fx, Frame::fy, Frame::cx, Frame::cy};
  const int64_t soff[2] = {0, (int64_t)n}, koff[2] = {0, (int64_t)m};
  int32_t stats[4] = {0, 0, 0, 0};
  const int s = sqlm_lidar_depth(ctx, 1, soff, xyz.data(), koff, key.data(), vP3Dc ? key_un.data() : nullptr, img.rows,
                                 img.cols, k, e, vP3Dc ? cam : nullptr, cls.data(), depth.data(), uv.data(),
                                 vP3Dc ? pcam.data() : nullptr, stats, image.data());
  if (s != SQLM_OK) {
    std::cerr << "hipFrameDepth: sqlm_lidar_depth failed: " << sqlm_status_string(s) << std::endl;
    return false;
  }
  if (!image.empty()) std::memcpy(img.ptr<double>(0), image.data(), image.size() * sizeof(double));
  for (size_t i = 0; i < m; i++) {
    pF->mvKeys[i].class_id = cls[i];
    pF->mvDepth[i] = depth[i];
  }
  if (vP3Dc) {
    vP3Dc->resize(m);
    for (size_t i = 0; i < m; i++) {
      (*vP3Dc)[i].x = pcam[3 * i];
      (*vP3Dc)[i].y = pcam[3 * i + 1];
      (*vP3Dc)[i].z = pcam[3 * i + 2];
    }
  }
  return true;
}

}  // namespace

bool hipFrameDepth::AssociateDepth(Frame* pF, const Eigen::Matrix<double, 3, 4>& intrinsicMatrix,
                                   const Eigen::Matrix<double, 4, 4>& extrinsicMatrix) {
  return Associate(pF, intrinsicMatrix, extrinsicMatrix, nullptr);
}

bool hipFrameDepth::UnprojectAll(Frame* pF, const Eigen::Matrix<double, 3, 4>& intrinsicMatrix,
                                 const Eigen::Matrix<double, 4, 4>& extrinsicMatrix, std::vector<cv::Point3f>& vP3Dc) {
  return Associate(pF, intrinsicMatrix, extrinsicMatrix, &vP3Dc);
}

}  // namespace ORB_SLAM2
