// hipLocalMapping.h — the two map-point steps of the reference's LocalMapping
// thread (src/backend/LocalMapping.cc) on libsqrtlm:
//
//  TriangulateMatches replaces the match loop of CreateNewMapPoints (:436-624):
//  one sqlm_triangulate_pairs call for the pair, then `new MapPoint`,
//  AddObservation, AddMapPoint in match order, as the reference does.
//
//  UpdateMapPoints replaces the per-point calls of
//  MapPoint::ComputeDistinctiveDescriptors and UpdateNormalAndDepth in
//  ProcessNewKeyFrame (:230-241), in the "Update points" loop of
//  SearchInNeighbors (:763-777) and for the new points of CreateNewMapPoints
//  (:639-642): one sqlm_map_points_update call for all of them.
//
// The write-back needs two setters in MapPoint.h:
//   void SetDescriptor(const cv::Mat& descriptor);
//   void SetNormalAndDepth(const cv::Mat& normal, float minDistance, float maxDistance);
// Like hipOptimizer.cc it builds inside the reference tree only.
#ifndef HIPLOCALMAPPING_H
#define HIPLOCALMAPPING_H

#include <cstddef>
#include <utility>
#include <vector>

#include "KeyFrame.h"
#include "Map.h"
#include "MapPoint.h"

namespace ORB_SLAM2 {

class hipLocalMapping {
 public:
  // The match loop for (pKF1 = mpCurrentKeyFrame, pKF2). ratioFactor = 1.5f *
  // pKF1->mfScaleFactor. The created points are appended to vpNewMapPoints in
  // match order, with their observations added and inserted into both
  // keyframes and the map; the caller refreshes them (UpdateMapPoints) and
  // pushes them to mlpRecentAddedMapPoints. Returns their number (nnew's
  // share), or -1 if the library call failed (nothing is created then).
  static int TriangulateMatches(KeyFrame* pKF1, KeyFrame* pKF2,
                                const std::vector<std::pair<size_t, size_t> >& vMatchedIndices, float ratioFactor,
                                Map* pMap, std::vector<MapPoint*>& vpNewMapPoints);

  // ComputeDistinctiveDescriptors + UpdateNormalAndDepth of every point that
  // is not NULL and not bad. False if the library call failed (no point is
  // changed then).
  static bool UpdateMapPoints(const std::vector<MapPoint*>& vpMapPoints);
};

}  // namespace ORB_SLAM2

#endif  // HIPLOCALMAPPING_H
