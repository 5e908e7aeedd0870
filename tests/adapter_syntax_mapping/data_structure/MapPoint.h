// include/data_structure/MapPoint.h:53-340 (the members adapter/hipLocalMapping.cc touches) and the two
// setters INTEGRATION.md 4 asks the integrator to add.
#pragma once
#include <cstddef>
#include <map>

#include "opencv2/core/core.hpp"

namespace ORB_SLAM2 {

class KeyFrame;
class Map;

class MapPoint {
 public:
  MapPoint(const cv::Mat &Pos, KeyFrame *pRefKF, Map *pMap);
  cv::Mat GetWorldPos();
  KeyFrame *GetReferenceKeyFrame();
  std::map<KeyFrame *, size_t> GetObservations();
  void AddObservation(KeyFrame *pKF, size_t idx);
  bool isBad();
  // the additions
  void SetDescriptor(const cv::Mat &descriptor);
  void SetNormalAndDepth(const cv::Mat &normal, float minDistance, float maxDistance);
};

}  // namespace ORB_SLAM2
