// Thirdparty/DBoW2/DUtils/Random.h:24-120 (the member adapter/hipPnPsolver.cc touches).
#pragma once

namespace DUtils {

class Random {
 public:
  static int RandomInt(int min, int max);
};

}  // namespace DUtils
