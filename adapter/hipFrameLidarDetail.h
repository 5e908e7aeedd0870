// hipFrameLidarDetail.h — what hipFrameLidar.cc and hipFrameLidarCorner.cc
// share: the per-thread library context, lidarConfig as sqlm_lidar_feat_params
// and the feature point the frame's clouds hold. Defined in hipFrameLidar.cc.
#ifndef HIPFRAMELIDARDETAIL_H
#define HIPFRAMELIDARDETAIL_H

#include "Frame.h"
#include "sqrtlm.h"

namespace ORB_SLAM2 {
namespace frame_lidar_detail {

sqlm_ctx* frame_thread_ctx();
void FillParams(const lidarConfig& c, sqlm_lidar_feat_params& p);
PointIRT MakePoint(const float* xyz, int row);

}  // namespace frame_lidar_detail
}  // namespace ORB_SLAM2

#endif  // HIPFRAMELIDARDETAIL_H
