// include/backend/Optimizer.h:42-71 with the maintainer's one-line change
// (eSolver gains HIP): the entry adapter/hipOptimizerSim3.cc defines.
#pragma once
#include <vector>

#include "KeyFrame.h"
#include "MapPoint.h"
#include "Thirdparty/g2o/g2o/types/sim3.h"

namespace ORB_SLAM2 {

class Optimizer {
 public:
  enum eSolver { CERES = 0, G2O = 1, MYOPT = 2, HIP = 3 };

  // if bFixScale is true, optimize SE3 (stereo,rgbd), Sim3 otherwise (mono)
  static int OptimizeSim3(KeyFrame *pKF1, KeyFrame *pKF2, std::vector<MapPoint *> &vpMatches1, g2o::Sim3 &g2oS12,
                          const float th2, const bool bFixScale);
};

}  // namespace ORB_SLAM2
