// include/data_structure/Map.h: adapter/hipOptimizerSim3.cc uses no member of
// Map; this stand-in only keeps LoopClosing.h's include on the overlay's
// KeyFrame.h / MapPoint.h.
#pragma once
#include "KeyFrame.h"
#include "MapPoint.h"

namespace ORB_SLAM2 {

class Map;

}  // namespace ORB_SLAM2
