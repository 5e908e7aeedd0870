// hipPnPsolver.h — the reference's PnPsolver (include/algorithm/PnPsolver.h)
// on libsqrtlm: the same public interface, so Tracking.cc:2390 changes by one
// type name (`new hipPnPsolver(mCurrentFrame, vvpMapPointMatches[i])`). The
// RANSAC hypotheses are evaluated by one sqlm_pnp_ransac call, made by the
// first iterate() (or by SolveBatch for several candidates at once); iterate
// and find replay PnPsolver.cc:247-370 from its per-hypothesis flags. Like
// hipOptimizer.cc it builds inside the reference tree only.
#ifndef HIPPNPSOLVER_H
#define HIPPNPSOLVER_H

#include <cstddef>
#include <cstdint>
#include <vector>

#include <opencv2/core/core.hpp>

#include "Frame.h"
#include "MapPoint.h"

namespace ORB_SLAM2 {

class hipPnPsolver {
 public:
  hipPnPsolver(const Frame& F, const std::vector<MapPoint*>& vpMapPointMatches);

  void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4,
                           float epsilon = 0.4, float th2 = 5.991);

  cv::Mat find(std::vector<bool>& vbInliers, int& nInliers);

  cv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers);

  // Evaluates the hypotheses of several solvers (Relocalization's candidates)
  // in one library call; their later iterate() calls are served from it. False
  // if the library call failed (the solvers then report bNoMore).
  static bool SolveBatch(const std::vector<hipPnPsolver*>& vpSolvers);

 protected:
  struct Refined {  // Refine() of the mask of a record-breaking hypothesis
    int hyp;
    float Tcw[16];
    int nInliers;
    std::vector<uint8_t> mask;      // mvbRefinedInliers
    std::vector<uint8_t> bestMask;  // mvbBestInliers: the hypothesis's own mask
  };

  // what the constructor keeps (PnPsolver.cc:131-153)
  std::vector<float> mvP2D, mvP3Dw, mvSigma2, mvMaxError;  // [N][2], [N][3], [N], [N]
  std::vector<size_t> mvKeyPointIndices;
  double mIntr[4];  // fu fv uc vc
  int N;
  size_t mnMatches;  // vpMapPointMatches.size()

  // RANSAC parameters and the draws of every hypothesis so far
  int mRansacMinInliers;
  int mRansacMaxIts;
  std::vector<int32_t> mvDraws;  // [n][4] DUtils::Random::RandomInt values

  // results of the library call
  bool mbSolved, mbFailed;
  std::vector<int32_t> mvnInliers;
  std::vector<uint8_t> mvFlags;  // bit 0 qualifies, bit 1 new best, bit 2 returns
  std::vector<double> mvR, mvt;  // [n][9], [n][3]
  std::vector<Refined> mvRefined;  // the record-breaking hypotheses, in order

  // replay state
  int mnIterations;
  int mnBestInliers;
  int mnBest;  // index into mvRefined of the record held as best, -1 none

  int Evaluated() const { return (int)(mvDraws.size() / 4); }
  void Draw(int n);
  cv::Mat Result(const float* Tcw, const std::vector<uint8_t>& mask, std::vector<bool>& vbInliers) const;
};

}  // namespace ORB_SLAM2

#endif  // HIPPNPSOLVER_H
