// include/data_structure/Map.h:40-120 (the member adapter/hipLocalMapping.cc touches).
#pragma once

namespace ORB_SLAM2 {

class MapPoint;

class Map {
 public:
  void AddMapPoint(MapPoint *pMP);
};

}  // namespace ORB_SLAM2
