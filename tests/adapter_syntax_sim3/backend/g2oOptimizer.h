// include/backend/g2oOptimizer.h:189-190 (the entry the dispatch falls back to).
#pragma once
#include <vector>

#include "KeyFrame.h"
#include "MapPoint.h"
#include "Thirdparty/g2o/g2o/types/sim3.h"

namespace ORB_SLAM2 {

class g2oOptimizer {
 public:
  static int OptimizeSim3(KeyFrame *pKF1, KeyFrame *pKF2, std::vector<MapPoint *> &vpMatches1, g2o::Sim3 &g2oS12,
                          const float th2, const bool bFixScale);
};

}  // namespace ORB_SLAM2
