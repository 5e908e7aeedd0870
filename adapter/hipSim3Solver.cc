// hipSim3Solver.cc — Sim3Solver (src/algorithm/Sim3Solver.cc) behind its own
// public interface, on libsqrtlm (sqlm_sim3_ransac). Like hipOptimizer.cc it
// builds inside the reference tree only.
//
// The constructor packs the pairs exactly as :78-127 keep them; the points go
// to their cameras in the float arithmetic of the reference's cv::Mat
// expression. SetRansacParameters fixes the hypothesis count (mRansacMaxIts,
// :145-203) and draws 3 * mRansacMaxIts indices with DUtils::Random::RandomInt
// in the order iterate() would: the draws of hypothesis h are what the
// reference's h-th loop body would have drawn, provided nothing else draws from
// the same generator in between (LoopClosing advances its candidates five
// iterations at a time, so with several candidates the interleaving differs;
// the distribution does not). The first iterate() makes the one library call
// for all hypotheses; iterate / find / the getters then replay :207-300 from
// the flags.
#include "hipSim3Solver.h"

#include <cstdlib>
#include <iostream>

#include "Thirdparty/DBoW2/DUtils/Random.h"
#include "sqrtlm.h"

namespace ORB_SLAM2 {

namespace {

struct RansacCtxHolder {
  sqlm_ctx* ctx = nullptr;
  ~RansacCtxHolder() {
    if (ctx) sqlm_ctx_destroy(ctx);
  }
};

// The loop-closing thread's context for these calls.
sqlm_ctx* ransac_thread_ctx() {
  thread_local RansacCtxHolder h;
  if (!h.ctx) {
    const char* dev = std::getenv("SQLM_DEVICE");
    const int s = sqlm_ctx_create(dev ? std::atoi(dev) : -1, &h.ctx);
    if (s != SQLM_OK) {
      std::cerr << "hipSim3Solver: sqlm_ctx_create failed: " << sqlm_status_string(s) << std::endl;
      h.ctx = nullptr;
    }
  }
  return h.ctx;
}

// Rcw * X3Dw + tcw as the CV_32F cv::Mat expression evaluates it (:119, :122):
// the product accumulates in double and rounds to float, the sum is a float addition.
void to_camera(const cv::Mat& R, const cv::Mat& t, const cv::Mat& Pw, std::vector<double>& out) {
  for (int r = 0; r < 3; ++r) {
    double acc = 0.0;
    for (int c = 0; c < 3; ++c) acc += (double)R.at<float>(r, c) * (double)Pw.at<float>(c);
    out.push_back((double)((float)acc + t.at<float>(r)));
  }
}

}  // namespace

hipSim3Solver::hipSim3Solver(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<MapPoint*>& vpMatched12,
                             const bool bFixScale)
    : mbFixScale(bFixScale), mbSolved(false), mbFailed(false), mnIterations(0), mnBestInliers(0), mnBest(-1) {
  std::vector<MapPoint*> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
  mN1 = (int)vpMatched12.size();
  const cv::Mat Rcw1 = pKF1->GetRotation();
  const cv::Mat tcw1 = pKF1->GetTranslation();
  const cv::Mat Rcw2 = pKF2->GetRotation();
  const cv::Mat tcw2 = pKF2->GetTranslation();
  for (int i1 = 0; i1 < mN1; i1++) {
    if (!vpMatched12[i1]) continue;
    MapPoint* pMP1 = vpKeyFrameMP1[i1];
    MapPoint* pMP2 = vpMatched12[i1];
    if (!pMP1) continue;
    if (pMP1->isBad() || pMP2->isBad()) continue;
    const int indexKF1 = pMP1->GetIndexInKeyFrame(pKF1);
    const int indexKF2 = pMP2->GetIndexInKeyFrame(pKF2);
    if (indexKF1 < 0 || indexKF2 < 0) continue;
    const cv::KeyPoint& kp1 = pKF1->mvKeysUn[indexKF1];
    const cv::KeyPoint& kp2 = pKF2->mvKeysUn[indexKF2];
    const float sigmaSquare1 = pKF1->mvLevelSigma2[kp1.octave];
    const float sigmaSquare2 = pKF2->mvLevelSigma2[kp2.octave];
    // mvnMaxError1/2 are std::vector<size_t> (Sim3Solver.h:158-159): the double is truncated when stored
    mvnMaxError1.push_back((int32_t)(size_t)(9.210 * sigmaSquare1));
    mvnMaxError2.push_back((int32_t)(size_t)(9.210 * sigmaSquare2));
    mvnIndices1.push_back((size_t)i1);
    to_camera(Rcw1, tcw1, pMP1->GetWorldPos(), mvX3Dc1);
    to_camera(Rcw2, tcw2, pMP2->GetWorldPos(), mvX3Dc2);
  }
  const cv::Mat& K1 = pKF1->mK;
  const cv::Mat& K2 = pKF2->mK;
  const double k1[4] = {K1.at<float>(0, 0), K1.at<float>(1, 1), K1.at<float>(0, 2), K1.at<float>(1, 2)};
  const double k2[4] = {K2.at<float>(0, 0), K2.at<float>(1, 1), K2.at<float>(0, 2), K2.at<float>(1, 2)};
  for (int k = 0; k < 4; ++k) {
    mIntr1[k] = k1[k];
    mIntr2[k] = k2[k];
  }
  N = (int)mvnIndices1.size();
  SetRansacParameters();
}

void hipSim3Solver::SetRansacParameters(double probability, int minInliers, int maxIterations) {
  mRansacProb = probability;
  mRansacMinInliers = minInliers;
  // 0 when N < minInliers: iterate() then reports bNoMore at once (:214-218)
  mRansacMaxIts = sqlm_sim3_ransac_max_its(N, probability, minInliers, maxIterations);
  if (N < 3) mRansacMaxIts = 0;  // the reference would index out of range; nothing to fit
  mvDraws.resize(3 * (size_t)mRansacMaxIts);
  for (int h = 0; h < mRansacMaxIts; ++h)
    for (int i = 0; i < 3; ++i) mvDraws[3 * (size_t)h + i] = DUtils::Random::RandomInt(0, N - 1 - i);  // :243
  mnIterations = 0;
  mnBestInliers = 0;
  mnBest = -1;
  mbSolved = false;
  mbFailed = false;
}

bool hipSim3Solver::SolveBatch(const std::vector<hipSim3Solver*>& vpSolvers) {
  const int P = (int)vpSolvers.size();
  if (P == 0) return true;
  sqlm_ctx* ctx = ransac_thread_ctx();
  std::vector<double> intr1, intr2, X1c, X2c;
  std::vector<uint8_t> fix;
  std::vector<int32_t> minIn, e1, e2, draws;
  std::vector<int64_t> pairOff(1, 0), hypOff(1, 0);
  for (int k = 0; k < P; ++k) {
    const hipSim3Solver& s = *vpSolvers[k];
    intr1.insert(intr1.end(), s.mIntr1, s.mIntr1 + 4);
    intr2.insert(intr2.end(), s.mIntr2, s.mIntr2 + 4);
    fix.push_back(s.mbFixScale ? 1 : 0);
    minIn.push_back(s.mRansacMinInliers);
    X1c.insert(X1c.end(), s.mvX3Dc1.begin(), s.mvX3Dc1.end());
    X2c.insert(X2c.end(), s.mvX3Dc2.begin(), s.mvX3Dc2.end());
    e1.insert(e1.end(), s.mvnMaxError1.begin(), s.mvnMaxError1.end());
    e2.insert(e2.end(), s.mvnMaxError2.begin(), s.mvnMaxError2.end());
    draws.insert(draws.end(), s.mvDraws.begin(), s.mvDraws.end());
    pairOff.push_back(pairOff.back() + s.N);
    hypOff.push_back(hypOff.back() + s.mRansacMaxIts);
  }
  const size_t H = (size_t)hypOff.back();
  std::vector<int32_t> nIn(H + 1), first(P), best(P);
  std::vector<uint8_t> flags(H + 1);
  std::vector<float> R12(9 * H + 1), t12(3 * H + 1), s12(H + 1);
  X1c.push_back(0.0);  // never empty: data() stays a valid pointer for an empty batch
  X2c.push_back(0.0);
  e1.push_back(0);
  e2.push_back(0);
  draws.push_back(0);
  int st = ctx ? sqlm_sim3_ransac(ctx, P, intr1.data(), intr2.data(), fix.data(), minIn.data(), pairOff.data(),
                                  X1c.data(), X2c.data(), e1.data(), e2.data(), hypOff.data(), draws.data(),
                                  nIn.data(), flags.data(), R12.data(), t12.data(), s12.data(), first.data(),
                                  best.data())
               : SQLM_ERR_NO_DEVICE;
  if (st != SQLM_OK) std::cerr << "hipSim3Solver: sqlm_sim3_ransac: " << sqlm_status_string(st) << std::endl;
  for (int k = 0; k < P; ++k) {
    hipSim3Solver& s = *vpSolvers[k];
    s.mbSolved = true;
    s.mbFailed = st != SQLM_OK;
    if (s.mbFailed) continue;
    const size_t h0 = (size_t)hypOff[k], n = (size_t)s.mRansacMaxIts;
    s.mvnInliers.assign(nIn.begin() + h0, nIn.begin() + h0 + n);
    s.mvFlags.assign(flags.begin() + h0, flags.begin() + h0 + n);
    s.mvR12.assign(R12.begin() + 9 * h0, R12.begin() + 9 * (h0 + n));
    s.mvt12.assign(t12.begin() + 3 * h0, t12.begin() + 3 * (h0 + n));
    s.mvs12.assign(s12.begin() + h0, s12.begin() + h0 + n);
    s.mvReturnMasks.clear();
    s.mvReturnSlot.assign(n, -1);
    for (size_t h = 0; h < n; ++h) {
      if (!(s.mvFlags[h] & 2)) continue;
      std::vector<uint8_t> mask((size_t)s.N);
      if (sqlm_sim3_ransac_get_inliers(ctx, k, (int)h, mask.data()) != SQLM_OK) s.mbFailed = true;
      s.mvReturnSlot[h] = (int)s.mvReturnMasks.size();
      s.mvReturnMasks.push_back(mask);
    }
  }
  return st == SQLM_OK;
}

cv::Mat hipSim3Solver::T12(int h) const {
  // mT12i = [s R | t] (:440-447); s * R is one float product per element
  cv::Mat T(4, 4, CV_32F);
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) T.at<float>(i, j) = i == j ? 1.f : 0.f;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j)
      T.at<float>(i, j) = (float)((double)mvs12[h] * (double)mvR12[9 * (size_t)h + 3 * i + j]);
    T.at<float>(i, 3) = mvt12[3 * (size_t)h + i];
  }
  return T;
}

cv::Mat hipSim3Solver::iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
  bNoMore = false;
  vbInliers = std::vector<bool>(mN1, false);
  nInliers = 0;
  if (N < mRansacMinInliers) {
    bNoMore = true;
    return cv::Mat();
  }
  if (!mbSolved) SolveBatch(std::vector<hipSim3Solver*>(1, this));
  if (mbFailed) {
    bNoMore = true;
    return cv::Mat();
  }
  int nCurrentIterations = 0;
  while (mnIterations < mRansacMaxIts && nCurrentIterations < nIterations) {
    nCurrentIterations++;
    const int h = mnIterations++;
    if (mvFlags[h] & 1) {  // mnInliersi >= mnBestInliers (:265)
      mnBestInliers = mvnInliers[h];
      mnBest = h;
      if (mvFlags[h] & 2) {  // mnInliersi > mRansacMinInliers (:274)
        nInliers = mvnInliers[h];
        const std::vector<uint8_t>& mask = mvReturnMasks[mvReturnSlot[h]];
        for (int i = 0; i < N; i++)
          if (mask[i]) vbInliers[mvnIndices1[i]] = true;
        return T12(h);
      }
    }
  }
  if (mnIterations >= mRansacMaxIts) bNoMore = true;  // :288-289
  return cv::Mat();
}

cv::Mat hipSim3Solver::find(std::vector<bool>& vbInliers12, int& nInliers) {
  bool bFlag;
  return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);
}

cv::Mat hipSim3Solver::GetEstimatedRotation() {
  if (mnBest < 0) return cv::Mat();
  cv::Mat R(3, 3, CV_32F);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R.at<float>(i, j) = mvR12[9 * (size_t)mnBest + 3 * i + j];
  return R;
}

cv::Mat hipSim3Solver::GetEstimatedTranslation() {
  if (mnBest < 0) return cv::Mat();
  cv::Mat t(3, 1, CV_32F);  // O1 - s R O2 is a 3x1 matrix (:434)
  for (int i = 0; i < 3; ++i) t.at<float>(i) = mvt12[3 * (size_t)mnBest + i];
  return t;
}

float hipSim3Solver::GetEstimatedScale() { return mnBest < 0 ? 1.f : mvs12[mnBest]; }

}  // namespace ORB_SLAM2
