// hipFrameDepth.h — the LiDAR depth image and the keypoint depth association of
// the reference's Frame constructor (src/data_structure/Frame.cc:290-313 and
// :336-402) on libsqrtlm: the step that makes a frame a fusion frame.
//
//  AssociateDepth replaces the projection loop (:292-313) and the patch loop
//  (:336-402) with one sqlm_lidar_depth call. The constructor keeps :290 (the
//  allocation of Depthimg_, rows x cols of CV_64F, which gives the call its
//  image size), ExtractORB, UndistortKeyPoints and the two assignments of
//  :333-334; AssociateDepth is called after them, because it writes
//  mvKeys[i].class_id and mvDepth[i] and UndistortKeyPoints copies mvKeys into
//  mvKeysUn. It fills Depthimg_, mvKeys[i].class_id and mvDepth. mvKeysUn[i]
//  keeps the class_id UndistortKeyPoints copied, as in the reference, whose
//  loop writes mvKeys alone.
//
//  UnprojectAll does the same and also returns, for every keypoint, the point
//  Frame::UnprojectStereo (:1710-1723) forms in the camera frame before its
//  world transform (zeros where mvDepth is not positive); mRwc * x3Dc + mOw
//  stays with the caller.
//
// Differences from the reference (include/sqrtlm.h has the definition): a patch
// cell outside the image is empty where the reference reads out of bounds (its
// extractor keeps keypoints 16 px inside, so it does not happen there), and a
// point with a non-finite coordinate is dropped. Call it from the constructor's
// own thread: the library context is kept per calling thread. Like
// hipFrameLidar.cc it builds inside the reference tree only.
#ifndef HIPFRAMEDEPTH_H
#define HIPFRAMEDEPTH_H

#include <Eigen/Core>
#include <opencv2/core/core.hpp>
#include <vector>

#include "Frame.h"

namespace ORB_SLAM2 {

class hipFrameDepth {
 public:
  // False, leaving the frame untouched, when Depthimg_ is not an allocated
  // continuous CV_64F image, mvDepth / mvKeysUn do not match mvKeys, or the
  // library call failed; the caller then runs the reference's loops.
  static bool AssociateDepth(Frame* pF, const Eigen::Matrix<double, 3, 4>& intrinsicMatrix,
                             const Eigen::Matrix<double, 4, 4>& extrinsicMatrix);
  static bool UnprojectAll(Frame* pF, const Eigen::Matrix<double, 3, 4>& intrinsicMatrix,
                           const Eigen::Matrix<double, 4, 4>& extrinsicMatrix, std::vector<cv::Point3f>& vP3Dc);
};

}  // namespace ORB_SLAM2

#endif  // HIPFRAMEDEPTH_H
