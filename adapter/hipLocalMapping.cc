// hipLocalMapping.cc — see hipLocalMapping.h. What stays here is what the
// reference does with its own objects: reading KeyFrame / MapPoint fields into
// plain arrays, the order of the observations (the (mnId, idx) sort of
// MapPoint.cc:404-429 for the descriptors, the std::map order of :556 for the
// normal), and the map edits in match order. The arithmetic is the library's.
#include "hipLocalMapping.h"

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <iostream>
#include <map>

#include "sqrtlm.h"
#include "sqrtlm_orb.h"

namespace ORB_SLAM2 {

namespace {

struct MappingCtxHolder {
  sqlm_ctx* ctx = nullptr;
  ~MappingCtxHolder() {
    if (ctx) sqlm_ctx_destroy(ctx);
  }
};

// one context per calling thread (LocalMapping's, LoopClosing's, Tracking's)
sqlm_ctx* mapping_thread_ctx() {
  thread_local MappingCtxHolder h;
  if (!h.ctx) {
    const char* dev = std::getenv("SQLM_DEVICE");
    const int s = sqlm_ctx_create(dev ? std::atoi(dev) : -1, &h.ctx);
    if (s != SQLM_OK) {
      std::cerr << "hipLocalMapping: sqlm_ctx_create failed: " << sqlm_status_string(s) << std::endl;
      h.ctx = nullptr;
    }
  }
  return h.ctx;
}

struct FrameArrays {
  std::vector<sqlm_keypoint> kps;
};

void FillFrame(KeyFrame* pKF, FrameArrays& a, sqlm_tri_frame& f) {
  const size_t n = pKF->mvKeysUn.size();
  a.kps.resize(n);
  for (size_t i = 0; i < n; i++) {
    const cv::KeyPoint& kp = pKF->mvKeysUn[i];
    sqlm_keypoint& k = a.kps[i];
    k.x = kp.pt.x;
    k.y = kp.pt.y;
    k.size = kp.size;
    k.angle = kp.angle;
    k.response = kp.response;
    k.octave = kp.octave;
  }
  f.kps = a.kps.data();
  f.uright = pKF->mvuRight.size() == n ? pKF->mvuRight.data() : nullptr;
  f.scale_factors = pKF->mvScaleFactors.data();
  f.level_sigma2 = pKF->mvLevelSigma2.data();
  f.n = (int32_t)n;
  f.n_levels = (int32_t)std::min(pKF->mvScaleFactors.size(), pKF->mvLevelSigma2.size());
  const cv::Mat Tcw = pKF->GetPose();
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 4; c++) f.Tcw[4 * r + c] = Tcw.at<float>(r, c);
  f.fx = pKF->fx;
  f.fy = pKF->fy;
  f.cx = pKF->cx;
  f.cy = pKF->cy;
  f.invfx = pKF->invfx;
  f.invfy = pKF->invfy;
}

void Center(KeyFrame* pKF, float* out) {
  const cv::Mat Ow = pKF->GetCameraCenter();
  for (int i = 0; i < 3; i++) out[i] = Ow.at<float>(i);
}

struct Obs {
  KeyFrame* pKF;
  size_t idx;
};

}  // namespace

int hipLocalMapping::TriangulateMatches(KeyFrame* pKF1, KeyFrame* pKF2,
                                        const std::vector<std::pair<size_t, size_t> >& vMatchedIndices,
                                        float ratioFactor, Map* pMap, std::vector<MapPoint*>& vpNewMapPoints) {
  const size_t nmatches = vMatchedIndices.size();
  if (nmatches == 0) return 0;
  sqlm_ctx* ctx = mapping_thread_ctx();
  if (!ctx) return -1;
  FrameArrays a1, a2;
  sqlm_tri_pair pair;
  FillFrame(pKF1, a1, pair.kf1);
  FillFrame(pKF2, a2, pair.kf2);
  pair.ratio_factor = ratioFactor;
  pair.pad = 0;
  const int64_t off[2] = {0, (int64_t)nmatches};
  std::vector<int32_t> matches(2 * nmatches);
  for (size_t i = 0; i < nmatches; i++) {
    matches[2 * i] = (int32_t)vMatchedIndices[i].first;
    matches[2 * i + 1] = (int32_t)vMatchedIndices[i].second;
  }
  std::vector<float> x3d(3 * nmatches);
  std::vector<uint8_t> reason(nmatches);
  int32_t nnew = 0;
  const int s = sqlm_triangulate_pairs(ctx, 1, &pair, off, matches.data(), x3d.data(), reason.data(), &nnew);
  if (s != SQLM_OK) {
    std::cerr << "hipLocalMapping: sqlm_triangulate_pairs failed: " << sqlm_status_string(s) << std::endl;
    return -1;
  }
  // :626-636 in match order
  for (size_t i = 0; i < nmatches; i++) {
    if (reason[i] != 0) continue;
    cv::Mat x3D(3, 1, CV_32F);
    for (int k = 0; k < 3; k++) x3D.at<float>(k) = x3d[3 * i + k];
    MapPoint* pMP = new MapPoint(x3D, pKF1, pMap);
    pMP->AddObservation(pKF1, vMatchedIndices[i].first);
    pMP->AddObservation(pKF2, vMatchedIndices[i].second);
    pKF1->AddMapPoint(pMP, vMatchedIndices[i].first);
    pKF2->AddMapPoint(pMP, vMatchedIndices[i].second);
    pMap->AddMapPoint(pMP);
    vpNewMapPoints.push_back(pMP);
  }
  return nnew;
}

bool hipLocalMapping::UpdateMapPoints(const std::vector<MapPoint*>& vpMapPoints) {
  // per point: the descriptor list (sorted by (mnId, idx), bad keyframes
  // dropped) and the centre list (std::map order, every keyframe)
  std::vector<MapPoint*> pts;
  std::vector<std::vector<Obs> > dObs;
  std::vector<int64_t> dOff(1, 0), cOff(1, 0);
  std::vector<uint8_t> desc;
  std::vector<float> center, pos, ref, levelScale, maxScale;
  bool sameCounts = true;
  for (size_t ip = 0; ip < vpMapPoints.size(); ip++) {
    MapPoint* pMP = vpMapPoints[ip];
    if (!pMP || pMP->isBad()) continue;
    std::map<KeyFrame*, size_t> observations = pMP->GetObservations();
    if (observations.empty()) continue;
    KeyFrame* pRefKF = pMP->GetReferenceKeyFrame();
    std::vector<Obs> sorted;
    for (std::map<KeyFrame*, size_t>::iterator mit = observations.begin(); mit != observations.end(); mit++) {
      float c[3];
      Center(mit->first, c);
      center.insert(center.end(), c, c + 3);
      const Obs o = {mit->first, mit->second};
      sorted.push_back(o);
    }
    std::stable_sort(sorted.begin(), sorted.end(), [](const Obs& a, const Obs& b) {
      if (a.pKF->mnId != b.pKF->mnId) return a.pKF->mnId < b.pKF->mnId;
      return a.idx < b.idx;
    });
    std::vector<Obs> kept;
    for (size_t i = 0; i < sorted.size(); i++) {
      if (sorted[i].pKF->isBad()) continue;
      kept.push_back(sorted[i]);
      for (int b = 0; b < 32; b++) desc.push_back(sorted[i].pKF->mDescriptors.at<unsigned char>((int)sorted[i].idx, b));
    }
    if (kept.size() != observations.size()) sameCounts = false;
    dOff.push_back(dOff.back() + (int64_t)kept.size());
    cOff.push_back(cOff.back() + (int64_t)observations.size());
    dObs.push_back(kept);
    const cv::Mat Pos = pMP->GetWorldPos();
    float rc[3];
    Center(pRefKF, rc);
    for (int k = 0; k < 3; k++) {
      pos.push_back(Pos.at<float>(k));
      ref.push_back(rc[k]);
    }
    const int level = pRefKF->mvKeysUn[observations[pRefKF]].octave;  // :567, a missing entry reads index 0
    levelScale.push_back(pRefKF->mvScaleFactors[level]);
    maxScale.push_back(pRefKF->mvScaleFactors[pRefKF->mnScaleLevels - 1]);
    pts.push_back(pMP);
  }
  const int n = (int)pts.size();
  if (n == 0) return true;
  sqlm_ctx* ctx = mapping_thread_ctx();
  if (!ctx) return false;
  std::vector<int32_t> bestIdx(n), bestMedian(n);
  std::vector<float> normal(3 * (size_t)n), maxDist(n), minDist(n);
  int s;
  if (sameCounts) {
    s = sqlm_map_points_update(ctx, n, cOff.data(), desc.data(), center.data(), pos.data(), ref.data(),
                               levelScale.data(), maxScale.data(), bestIdx.data(), bestMedian.data(), normal.data(),
                               maxDist.data(), minDist.data());
  } else {
    // a bad keyframe is still among some point's observations: the two lists differ in length, each half alone
    s = sqlm_map_points_update(ctx, n, dOff.data(), desc.data(), nullptr, nullptr, nullptr, nullptr, nullptr,
                               bestIdx.data(), bestMedian.data(), nullptr, nullptr, nullptr);
    if (s == SQLM_OK)
      s = sqlm_map_points_update(ctx, n, cOff.data(), nullptr, center.data(), pos.data(), ref.data(),
                                 levelScale.data(), maxScale.data(), nullptr, nullptr, normal.data(), maxDist.data(),
                                 minDist.data());
  }
  if (s != SQLM_OK) {
    std::cerr << "hipLocalMapping: sqlm_map_points_update failed: " << sqlm_status_string(s) << std::endl;
    return false;
  }
  for (int j = 0; j < n; j++) {
    if (bestIdx[j] >= 0) {  // no descriptor left (every keyframe bad): mDescriptor stays (:431)
      const Obs& o = dObs[j][bestIdx[j]];
      pts[j]->SetDescriptor(o.pKF->mDescriptors.row((int)o.idx).clone());
    }
    cv::Mat nv(3, 1, CV_32F);
    for (int k = 0; k < 3; k++) nv.at<float>(k) = normal[3 * (size_t)j + k];
    pts[j]->SetNormalAndDepth(nv, minDist[j], maxDist[j]);
  }
  return true;
}

}  // namespace ORB_SLAM2
