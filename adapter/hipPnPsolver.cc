// hipPnPsolver.cc — PnPsolver (src/algorithm/PnPsolver.cc) behind its own
// public interface, on libsqrtlm (sqlm_pnp_ransac). Like hipOptimizer.cc it
// builds inside the reference tree only.
//
// The constructor keeps what :131-153 keep. SetRansacParameters fixes
// mRansacMinInliers and mRansacMaxIts (:178-227), stores mvMaxError as the
// float product of :226 and draws 4 * max(mRansacMaxIts, 5) indices with
// DUtils::Random::RandomInt in the order iterate() would: the first iterate(5)
// runs max(mRansacMaxIts, 5) hypotheses unless it returns early, because the
// loop condition of :273 is an "or". The first iterate() makes the one library
// call; iterate and find then replay :247-370 from the flags. A call after an
// early return can run past the evaluated hypotheses: the solver then draws
// max(nIterations, 5) more and resubmits the problem with all draws so far; the
// library call is stateless and deterministic, so the prefix reproduces.
#include "hipPnPsolver.h"

#include <cstdlib>
#include <iostream>

#include "Thirdparty/DBoW2/DUtils/Random.h"
#include "sqrtlm.h"

namespace ORB_SLAM2 {

namespace {

struct PnpCtxHolder {
  sqlm_ctx* ctx = nullptr;
  ~PnpCtxHolder() {
    if (ctx) sqlm_ctx_destroy(ctx);
  }
};

// The tracking thread's context for these calls.
sqlm_ctx* pnp_thread_ctx() {
  thread_local PnpCtxHolder h;
  if (!h.ctx) {
    const char* dev = std::getenv("SQLM_DEVICE");
    const int s = sqlm_ctx_create(dev ? std::atoi(dev) : -1, &h.ctx);
    if (s != SQLM_OK) {
      std::cerr << "hipPnPsolver: sqlm_ctx_create failed: " << sqlm_status_string(s) << std::endl;
      h.ctx = nullptr;
    }
  }
  return h.ctx;
}

}  // namespace

hipPnPsolver::hipPnPsolver(const Frame& F, const std::vector<MapPoint*>& vpMapPointMatches)
    : N(0), mnMatches(vpMapPointMatches.size()), mRansacMinInliers(0), mRansacMaxIts(0), mbSolved(false),
      mbFailed(false), mnIterations(0), mnBestInliers(0), mnBest(-1) {
  for (size_t i = 0, iend = vpMapPointMatches.size(); i < iend; i++) {
    MapPoint* pMP = vpMapPointMatches[i];
    if (!pMP) continue;
    if (pMP->isBad()) continue;
    const cv::KeyPoint& kp = F.mvKeysUn[i];
    mvP2D.push_back(kp.pt.x);
    mvP2D.push_back(kp.pt.y);
    mvSigma2.push_back(F.mvLevelSigma2[kp.octave]);
    cv::Mat Pos = pMP->GetWorldPos();
    for (int k = 0; k < 3; ++k) mvP3Dw.push_back(Pos.at<float>(k));
    mvKeyPointIndices.push_back(i);
  }
  mIntr[0] = F.fx;
  mIntr[1] = F.fy;
  mIntr[2] = F.cx;
  mIntr[3] = F.cy;
  N = (int)mvKeyPointIndices.size();
  SetRansacParameters();
}

void hipPnPsolver::Draw(int n) {
  for (int h = 0; h < n; ++h)
    for (int i = 0; i < 4; ++i) mvDraws.push_back(DUtils::Random::RandomInt(0, N - 1 - i));  // :286
  mbSolved = false;
}

void hipPnPsolver::SetRansacParameters(double probability, int minInliers, int maxIterations, int minSet,
                                       float epsilon, float th2) {
  // 0 when N < mRansacMinInliers: iterate() then reports bNoMore at once (:257-261)
  mRansacMaxIts = sqlm_pnp_ransac_max_its(N, probability, minInliers, maxIterations, minSet, epsilon,
                                          &mRansacMinInliers);
  if (N < 4) mRansacMaxIts = 0;  // the reference would index out of range; nothing to fit
  mvMaxError.resize(mvSigma2.size());
  for (size_t i = 0; i < mvSigma2.size(); i++) mvMaxError[i] = mvSigma2[i] * th2;  // :226, a float product
  mvDraws.clear();
  if (mRansacMaxIts > 0) Draw(mRansacMaxIts > 5 ? mRansacMaxIts : 5);
  mnIterations = 0;
  mnBestInliers = 0;
  mnBest = -1;
  mbSolved = false;
  mbFailed = false;
}

bool hipPnPsolver::SolveBatch(const std::vector<hipPnPsolver*>& vpSolvers) {
  std::vector<hipPnPsolver*> vp;  // a solver without hypotheses takes no part (N < mRansacMinInliers)
  for (size_t k = 0; k < vpSolvers.size(); ++k)
    if (vpSolvers[k] && vpSolvers[k]->Evaluated() > 0) vp.push_back(vpSolvers[k]);
  const int P = (int)vp.size();
  if (P == 0) return true;
  sqlm_ctx* ctx = pnp_thread_ctx();
  std::vector<double> intr;
  std::vector<int32_t> minIn, draws;
  std::vector<float> Xw, uv, maxErr;
  std::vector<int64_t> pairOff(1, 0), hypOff(1, 0);
  for (int k = 0; k < P; ++k) {
    const hipPnPsolver& s = *vp[k];
    intr.insert(intr.end(), s.mIntr, s.mIntr + 4);
    minIn.push_back(s.mRansacMinInliers);
    Xw.insert(Xw.end(), s.mvP3Dw.begin(), s.mvP3Dw.end());
    uv.insert(uv.end(), s.mvP2D.begin(), s.mvP2D.end());
    maxErr.insert(maxErr.end(), s.mvMaxError.begin(), s.mvMaxError.end());
    draws.insert(draws.end(), s.mvDraws.begin(), s.mvDraws.end());
    pairOff.push_back(pairOff.back() + s.N);
    hypOff.push_back(hypOff.back() + s.Evaluated());
  }
  const size_t H = (size_t)hypOff.back();
  std::vector<int32_t> nIn(H), first(P), best(P), nRefined(P);
  std::vector<uint8_t> flags(H);
  std::vector<double> R(9 * H), t(3 * H);
  std::vector<float> Tcw(16 * (size_t)P);
  int st = ctx ? sqlm_pnp_ransac(ctx, P, intr.data(), minIn.data(), pairOff.data(), Xw.data(), uv.data(),
                                 maxErr.data(), hypOff.data(), draws.data(), nIn.data(), flags.data(), R.data(),
                                 t.data(), first.data(), best.data(), Tcw.data(), nRefined.data())
               : SQLM_ERR_NO_DEVICE;
  if (st != SQLM_OK) std::cerr << "hipPnPsolver: sqlm_pnp_ransac: " << sqlm_status_string(st) << std::endl;
  for (int k = 0; k < P; ++k) {
    hipPnPsolver& s = *vp[k];
    s.mbSolved = true;
    s.mbFailed = st != SQLM_OK;
    if (s.mbFailed) continue;
    const size_t h0 = (size_t)hypOff[k], n = (size_t)s.Evaluated();
    s.mvnInliers.assign(nIn.begin() + h0, nIn.begin() + h0 + n);
    s.mvFlags.assign(flags.begin() + h0, flags.begin() + h0 + n);
    s.mvR.assign(R.begin() + 9 * h0, R.begin() + 9 * (h0 + n));
    s.mvt.assign(t.begin() + 3 * h0, t.begin() + 3 * (h0 + n));
    s.mvRefined.clear();
    for (size_t h = 0; h < n; ++h) {
      if (!(s.mvFlags[h] & 2)) continue;
      Refined r;
      r.hyp = (int)h;
      r.mask.assign((size_t)s.N, 0);
      r.bestMask.assign((size_t)s.N, 0);
      double Rr[9], tr[3];
      int32_t cnt = 0;
      if (sqlm_pnp_ransac_get_inliers(ctx, k, (int)h, r.bestMask.data()) != SQLM_OK ||
          sqlm_pnp_ransac_get_refined(ctx, k, (int)h, Rr, tr, r.mask.data(), &cnt, nullptr, nullptr, nullptr, nullptr,
                                      nullptr) != SQLM_OK)
        s.mbFailed = true;
      r.nInliers = cnt;
      for (int i = 0; i < 16; ++i) r.Tcw[i] = (i % 5 == 0) ? 1.f : 0.f;
      for (int i = 0; i < 3; ++i) {  // Rcw.convertTo(CV_32F) (:415-421)
        for (int j = 0; j < 3; ++j) r.Tcw[4 * i + j] = (float)Rr[3 * i + j];
        r.Tcw[4 * i + 3] = (float)tr[i];
      }
      s.mvRefined.push_back(r);
    }
  }
  return st == SQLM_OK;
}

cv::Mat hipPnPsolver::Result(const float* Tcw, const std::vector<uint8_t>& mask, std::vector<bool>& vbInliers) const {
  vbInliers = std::vector<bool>(mnMatches, false);
  for (int i = 0; i < N; i++)
    if (mask[i]) vbInliers[mvKeyPointIndices[i]] = true;
  cv::Mat T(4, 4, CV_32F);
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) T.at<float>(i, j) = Tcw[4 * i + j];
  return T;
}

cv::Mat hipPnPsolver::iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
  bNoMore = false;
  vbInliers.clear();
  nInliers = 0;
  if (N < mRansacMinInliers || mRansacMaxIts == 0) {
    bNoMore = true;
    return cv::Mat();
  }
  int nCurrentIterations = 0;
  while (mnIterations < mRansacMaxIts || nCurrentIterations < nIterations) {  // :273, an "or"
    nCurrentIterations++;
    const int h = mnIterations++;
    if (h >= Evaluated()) Draw(nIterations > 5 ? nIterations : 5);  // past the evaluated ones: resubmit with more
    if (!mbSolved) SolveBatch(std::vector<hipPnPsolver*>(1, this));
    if (mbFailed) {
      bNoMore = true;
      return cv::Mat();
    }
    if (mvFlags[h] & 1) {  // mnInliersi >= mRansacMinInliers (:308)
      if (mvFlags[h] & 2) {  // mnInliersi > mnBestInliers (:312)
        mnBestInliers = mvnInliers[h];
        for (size_t r = 0; r < mvRefined.size(); ++r)
          if (mvRefined[r].hyp == h) mnBest = (int)r;
      }
      if (mvFlags[h] & 4) {  // Refine() of the best mask found more than mRansacMinInliers (:327, :412)
        const Refined& r = mvRefined[mnBest];
        nInliers = r.nInliers;
        return Result(r.Tcw, r.mask, vbInliers);
      }
    }
  }
  if (mnIterations >= mRansacMaxIts) {  // :349-366
    bNoMore = true;
    if (mnBestInliers >= mRansacMinInliers && mnBest >= 0) {
      const Refined& r = mvRefined[mnBest];
      nInliers = mnBestInliers;
      float Tcw[16];  // mBestTcw: mRi, mti of the best hypothesis converted to float (:317-323)
      for (int i = 0; i < 16; ++i) Tcw[i] = (i % 5 == 0) ? 1.f : 0.f;
      for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) Tcw[4 * i + j] = (float)mvR[9 * (size_t)r.hyp + 3 * i + j];
        Tcw[4 * i + 3] = (float)mvt[3 * (size_t)r.hyp + i];
      }
      return Result(Tcw, r.bestMask, vbInliers);
    }
  }
  return cv::Mat();
}

cv::Mat hipPnPsolver::find(std::vector<bool>& vbInliers, int& nInliers) {
  bool bFlag;
  return iterate(mRansacMaxIts, bFlag, vbInliers, nInliers);
}

}  // namespace ORB_SLAM2
