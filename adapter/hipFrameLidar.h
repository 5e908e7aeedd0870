// hipFrameLidar.h — the LiDAR thread of the reference's Frame constructor
// (Frame::lidarProcess, src/data_structure/Frame.cc:1243) on libsqrtlm, for the
// configuration cfg/lidar_slam.yaml ships: flat points on, corner points off.
//
//  ExtractFlatFeatures replaces the call of lidarProcess (:286, :458): NaN
//  removal, CalculateRingAndTime, PointToImage and ExtractFeaturePoints become
//  one sqlm_lidar_features call, and the five flat-point members of the frame
//  are filled in the reference's push order. Like lidarProcess it leaves the
//  clouds in the sensor frame; the constructor's transformPointCloud calls
//  (:461-466) stay as they are. The overload with an extrinsic applies that
//  transform in the same call (to the normal clouds as points too, as :465-466
//  do); a caller that uses it drops those lines.
//
// Call it from the constructor's own thread in place of starting `loopthread`:
// the library context is kept per calling thread, and a thread started per
// frame would create one per frame. The range image, the scans and the corner
// members are not filled: the LiDAR depth image (:290-402) reads
// lidar_inputPtr_ alone, which is left NaN-free as lidarProcess leaves it.
// Intensity is not carried into the feature clouds (0), the ring is the row,
// the timestamp 0.1 as CalculateRingAndTime sets it. Like hipOptimizer.cc it
// builds inside the reference tree only.
#ifndef HIPFRAMELIDAR_H
#define HIPFRAMELIDAR_H

#include <Eigen/Core>

#include "Frame.h"

namespace ORB_SLAM2 {

class hipFrameLidar {
 public:
  // False, leaving the frame untouched, when using_sharp_point is set (the
  // corner branch is not built) or the library call failed; the caller then
  // runs lidarProcess. With using_flat_point off the members are left empty.
  static bool ExtractFlatFeatures(Frame* pF);
  static bool ExtractFlatFeatures(Frame* pF, const Eigen::Matrix<double, 4, 4>& extrinsicMatrix);

  // Both branches of ExtractFeaturePoints in one sqlm_lidar_features_all call
  // (hipFrameLidarCorner.cc), for either value of using_sharp_point: the flat
  // members as ExtractFlatFeatures fills them (when using_flat_point) and, with
  // using_sharp_point, corner_points_sharp_ and corner_points_less_sharp_, the
  // latter with the segment label as intensity (Frame.cc:1016). False, with the
  // frame untouched (the input cloud included), when the library call failed;
  // the caller then runs lidarProcess. less_sharp_ and feature_state are not
  // filled.
  static bool ExtractFeatures(Frame* pF);
  static bool ExtractFeatures(Frame* pF, const Eigen::Matrix<double, 4, 4>& extrinsicMatrix);
};

}  // namespace ORB_SLAM2

#endif  // HIPFRAMELIDAR_H
