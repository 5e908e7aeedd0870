// Thirdparty/DBoW2/DUtils/Random.h:24-120 (the member adapter/hipSim3Solver.cc touches).
#pragma once

namespace DUtils {

class Random {
 public:
  static int RandomInt(int min, int max);
};

}  // namespace DUtils
