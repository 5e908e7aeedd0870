// hipSim3Solver.h — the reference's Sim3Solver (include/algorithm/Sim3Solver.h)
// on libsqrtlm: the same public interface, so LoopClosing.cc:433 changes by one
// type name (`new hipSim3Solver(mpCurrentKF, pKF, vvpMapPointMatches[i],
// mbFixScale)`). All RANSAC hypotheses are evaluated by one sqlm_sim3_ransac
// call, made by the first iterate() (or by SolveBatch for several candidates at
// once); iterate / find / the getters replay Sim3Solver.cc:207-300 from its
// per-hypothesis flags. Like hipOptimizer.cc it builds inside the reference
// tree only.
#ifndef HIPSIM3SOLVER_H
#define HIPSIM3SOLVER_H

#include <cstddef>
#include <cstdint>
#include <vector>

#include <opencv2/core/core.hpp>

#include "KeyFrame.h"
#include "MapPoint.h"

namespace ORB_SLAM2 {

class hipSim3Solver {
 public:
  hipSim3Solver(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<MapPoint*>& vpMatched12, const bool bFixScale = true);

  void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300);

  cv::Mat find(std::vector<bool>& vbInliers12, int& nInliers);

  cv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers);

  cv::Mat GetEstimatedRotation();
  cv::Mat GetEstimatedTranslation();
  float GetEstimatedScale();

  // Evaluates the hypotheses of several solvers (LoopClosing's candidates) in
  // one library call; their later iterate() calls are served from it. False if
  // the library call failed (the solvers then report bNoMore).
  static bool SolveBatch(const std::vector<hipSim3Solver*>& vpSolvers);

 protected:
  // the pairs the constructor keeps (Sim3Solver.cc:78-127)
  std::vector<double> mvX3Dc1, mvX3Dc2;        // [N][3] float values
  std::vector<int32_t> mvnMaxError1, mvnMaxError2;  // as stored: size_t in the reference, truncated
  std::vector<size_t> mvnIndices1;
  double mIntr1[4], mIntr2[4];
  int N;
  int mN1;
  bool mbFixScale;

  // RANSAC parameters and the draws of every hypothesis
  double mRansacProb;
  int mRansacMinInliers;
  int mRansacMaxIts;
  std::vector<int32_t> mvDraws;                // [mRansacMaxIts][3] DUtils::Random::RandomInt values

  // results of the library call
  bool mbSolved, mbFailed;
  std::vector<int32_t> mvnInliers;             // [mRansacMaxIts]
  std::vector<uint8_t> mvFlags;                // bit 0 updates the best, bit 1 returns
  std::vector<float> mvR12, mvt12, mvs12;
  std::vector<std::vector<uint8_t> > mvReturnMasks;  // mvbInliersi of the returning hypotheses, in order
  std::vector<int> mvReturnSlot;               // hypothesis -> index into mvReturnMasks or -1

  // replay state
  int mnIterations;
  int mnBestInliers;
  int mnBest;                                  // hypothesis held in mBest*, -1 none

  cv::Mat T12(int h) const;
};

}  // namespace ORB_SLAM2

#endif  // HIPSIM3SOLVER_H
