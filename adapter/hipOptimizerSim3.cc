// hipOptimizerSim3.cc — g2oOptimizer::OptimizeSim3 (src/backend/g2oOptimizer.cc
// :1560-1793) behind the reference's Optimizer seam, on libsqrtlm
// (sqlm_sim3_optimize), and the Optimizer::OptimizeSim3 dispatch that selects
// it. Like hipOptimizer.cc it builds inside the reference tree only.
//
// The adapter does the reference's filtering: a correspondence becomes a pair
// exactly when the reference adds both edges for it (:1641-1668), so the
// library's pair count is nCorrespondences. The points go to their cameras in
// the float arithmetic of the reference's cv::Mat expressions.
//
// The HIP branch of the dispatch returns the inlier count, g2oOptimizer's
// contract (LoopClosing.cc:513-516 accepts a candidate on nInliers >= 20). The
// as-shipped facade discards it and returns 0 (Optimizer.cc:100-107), which
// keeps every loop from closing; see INTEGRATION.md.
#include "backend/Optimizer.h"
#include "backend/g2oOptimizer.h"
#include "backend/hipOptimizer.h"

#include <cstdint>
#include <cstdlib>
#include <iostream>
#include <vector>

#include "KeyFrame.h"
#include "MapPoint.h"
#include "Thirdparty/g2o/g2o/types/sim3.h"
#include "sqrtlm.h"

namespace ORB_SLAM2 {

extern Optimizer::eSolver solver;  // Optimizer.cc:26

namespace {

struct Sim3CtxHolder {
  sqlm_ctx* ctx = nullptr;
  ~Sim3CtxHolder() {
    if (ctx) sqlm_ctx_destroy(ctx);
  }
};

// The loop-closing thread's context for this call (hipOptimizer.cc keeps its own).
sqlm_ctx* sim3_thread_ctx() {
  thread_local Sim3CtxHolder h;
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

// R * P + t as the reference's CV_32F cv::Mat expression evaluates it (:1651,
// :1660): the 3x3 by 3x1 product accumulates in double and rounds to float
// (OpenCV's gemm for float matrices), the sum is a float addition.
void to_camera(const cv::Mat& R, const cv::Mat& t, const cv::Mat& Pw, double out[3]) {
  for (int r = 0; r < 3; ++r) {
    double acc = 0.0;
    for (int c = 0; c < 3; ++c) acc += (double)R.at<float>(r, c) * (double)Pw.at<float>(c);
    out[r] = (double)((float)acc + t.at<float>(r));
  }
}

}  // namespace

int hipOptimizer::OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches1,
                               g2o::Sim3& g2oS12, const float th2, const bool bFixScale) {
  sqlm_ctx* ctx = sim3_thread_ctx();
  if (!ctx) return 0;

  const cv::Mat& K1 = pKF1->mK;
  const cv::Mat& K2 = pKF2->mK;
  const double intr1[4] = {K1.at<float>(0, 0), K1.at<float>(1, 1), K1.at<float>(0, 2), K1.at<float>(1, 2)};
  const double intr2[4] = {K2.at<float>(0, 0), K2.at<float>(1, 1), K2.at<float>(0, 2), K2.at<float>(1, 2)};
  const cv::Mat R1w = pKF1->GetRotation();
  const cv::Mat t1w = pKF1->GetTranslation();
  const cv::Mat R2w = pKF2->GetRotation();
  const cv::Mat t2w = pKF2->GetTranslation();

  const int N = (int)vpMatches1.size();
  const std::vector<MapPoint*> vpMapPoints1 = pKF1->GetMapPointMatches();
  std::vector<double> X1c, X2c, obs1, obs2, info1, info2;
  std::vector<size_t> vnIndexEdge;
  for (int i = 0; i < N; i++) {
    if (!vpMatches1[i]) continue;
    MapPoint* pMP1 = vpMapPoints1[i];
    MapPoint* pMP2 = vpMatches1[i];
    const int i2 = pMP2->GetIndexInKeyFrame(pKF2);
    if (!pMP1 || !pMP2) continue;
    if (pMP1->isBad() || pMP2->isBad() || i2 < 0) continue;
    double p[3];
    to_camera(R1w, t1w, pMP1->GetWorldPos(), p);
    X1c.insert(X1c.end(), p, p + 3);
    to_camera(R2w, t2w, pMP2->GetWorldPos(), p);
    X2c.insert(X2c.end(), p, p + 3);
    const cv::KeyPoint& kpUn1 = pKF1->mvKeysUn[i];
    const cv::KeyPoint& kpUn2 = pKF2->mvKeysUn[i2];
    obs1.push_back(kpUn1.pt.x);
    obs1.push_back(kpUn1.pt.y);
    obs2.push_back(kpUn2.pt.x);
    obs2.push_back(kpUn2.pt.y);
    info1.push_back(pKF1->mvInvLevelSigma2[kpUn1.octave]);
    info2.push_back(pKF2->mvInvLevelSigma2[kpUn2.octave]);
    vnIndexEdge.push_back(i);
  }

  const int64_t n_pair = (int64_t)vnIndexEdge.size();
  const int64_t pair_off[2] = {0, n_pair};
  const Eigen::Quaterniond& q = g2oS12.rotation();
  const double S12[8] = {q.x(), q.y(), q.z(), q.w(), g2oS12.translation()[0], g2oS12.translation()[1],
                         g2oS12.translation()[2], g2oS12.scale()};
  const uint8_t fix = bFixScale ? 1 : 0;
  const double th2d = th2;
  double S12_out[8];
  int32_t n_in = 0;
  std::vector<uint8_t> state(n_pair > 0 ? n_pair : 1, 0);
  sqlm_sim3_stats st;
  const int s = sqlm_sim3_optimize(ctx, 1, S12, intr1, intr2, &fix, &th2d, pair_off, X1c.data(), X2c.data(),
                                   obs1.data(), obs2.data(), info1.data(), info2.data(), nullptr, 0.0, S12_out, &n_in,
                                   state.data(), &st);
  if (s != SQLM_OK) {
    std::cerr << "hipOptimizer: sqlm_sim3_optimize: " << sqlm_status_string(s) << std::endl;
    return 0;
  }
  // :1743 and :1781: rejected correspondences leave vpMatches1
  for (int64_t k = 0; k < n_pair; ++k)
    if (state[k]) vpMatches1[vnIndexEdge[k]] = static_cast<MapPoint*>(NULL);
  // fewer than 10 pairs after stage 1 (:1760-1761): g2oS12 stays as it was
  if (st.n_corr - st.n_bad < 10) return 0;
  g2oS12 = g2o::Sim3(Eigen::Quaterniond(S12_out[3], S12_out[0], S12_out[1], S12_out[2]),
                     Eigen::Vector3d(S12_out[4], S12_out[5], S12_out[6]), S12_out[7]);
  return n_in;
}

int Optimizer::OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches1, g2o::Sim3& g2oS12,
                            const float th2, const bool bFixScale) {
  if (solver == Optimizer::HIP) return hipOptimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale);
  // the reference's body (Optimizer.cc:100-107; its Ceres branch stays as it is, elided here)
  g2oOptimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale);
  return 0;
}

}  // namespace ORB_SLAM2
