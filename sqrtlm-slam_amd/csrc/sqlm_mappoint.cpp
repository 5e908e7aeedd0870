// sqlm_mappoint.cpp — host side of LocalMapping's map-point steps
// (sqlm_triangulate_pairs, sqlm_map_points_update and their host-only twins):
// argument checks before the device is touched, the gather of every match's
// keypoints and table entries, one staged upload / launch / read-back per call
// on the context's stream (kernels: sqlm_mappoint.hip). Built with
// -ffp-contract=off like the kernels: the twins run the same text,
// mappoint_dev.h, on the CPU.
#include <cstring>
#include <limits>
#include <new>
#include <vector>

#include "../../include/sqrtlm_orb.h"
#include "mappoint_dev.h"
#include "sqlm_ctx.h"
#include "sqlm_staging.h"

#pragma clang fp contract(off)

namespace sqlm {

// the staging buffers of a context's calls and what the last refresh launched
struct MapPointSolver {
  Staged in, out;
  int32_t n_lds = 0, n_global = 0, n_launch = 0;
};

void mappoint_destroy(MapPointSolver *s) { delete s; }

namespace {

int mappoint_solver(sqlm_ctx *c) {
  if (hipSetDevice(c->device) != hipSuccess) return SQLM_ERR_HIP;
  if (!c->mappoint && !(c->mappoint = new (std::nothrow) MapPointSolver)) return SQLM_ERR_OOM;
  return SQLM_OK;
}

bool csr_ok(const int64_t *off, int n) {
  if (!off || off[0] != 0) return false;
  for (int j = 0; j < n; ++j)
    if (off[j + 1] < off[j]) return false;
  return true;
}

bool frame_ok(const sqlm_tri_frame &f) {
  return f.n >= 0 && f.n_levels >= 0 && (f.n == 0 || f.kps) && (f.n_levels == 0 || (f.scale_factors && f.level_sigma2));
}

// The checks of sqlm_triangulate_pairs and the gather: pairs [n_pair] as the
// kernel reads them and one TriMatch per match, written through `pair_out` /
// `match_out` (each may be null: the checks alone).
int tri_gather(int n_pair, const sqlm_tri_pair *pairs, const int64_t *match_off, const int32_t *matches,
               const float *x3d, const uint8_t *reason, const int32_t *n_new, TriPair *pair_out, TriMatch *match_out) {
  if (n_pair < 0 || !csr_ok(match_off, n_pair)) return SQLM_ERR_INVALID_ARG;
  if (n_pair > 0 && (!pairs || !n_new)) return SQLM_ERR_INVALID_ARG;
  const int64_t n_match = match_off[n_pair];
  if (n_match > 0 && (!matches || !x3d || !reason)) return SQLM_ERR_INVALID_ARG;
  if (n_match > std::numeric_limits<int32_t>::max() / 4) return SQLM_ERR_INVALID_ARG;
  bool stereo = false;
  for (int p = 0; p < n_pair; ++p) {
    const sqlm_tri_frame &f1 = pairs[p].kf1, &f2 = pairs[p].kf2;
    if (!frame_ok(f1) || !frame_ok(f2)) return SQLM_ERR_INVALID_ARG;
    for (int64_t i = match_off[p]; i < match_off[p + 1]; ++i) {
      const int32_t i1 = matches[2 * i], i2 = matches[2 * i + 1];
      if (i1 < 0 || i1 >= f1.n || i2 < 0 || i2 >= f2.n) return SQLM_ERR_INVALID_ARG;
      const sqlm_keypoint &k1 = f1.kps[i1], &k2 = f2.kps[i2];
      if (k1.octave < 0 || k1.octave >= f1.n_levels || k2.octave < 0 || k2.octave >= f2.n_levels)
        return SQLM_ERR_INVALID_ARG;
      if ((f1.uright && f1.uright[i1] >= 0) || (f2.uright && f2.uright[i2] >= 0)) stereo = true;
      if (match_out) {
        TriMatch &m = match_out[i];
        m.x1 = k1.x;
        m.y1 = k1.y;
        m.x2 = k2.x;
        m.y2 = k2.y;
        m.sig1 = f1.level_sigma2[k1.octave];
        m.sig2 = f2.level_sigma2[k2.octave];
        m.sf1 = f1.scale_factors[k1.octave];
        m.sf2 = f2.scale_factors[k2.octave];
      }
    }
    if (pair_out) {
      TriPair &P = pair_out[p];
      std::memcpy(P.T1, f1.Tcw, sizeof(P.T1));
      std::memcpy(P.T2, f2.Tcw, sizeof(P.T2));
      const float c1[6] = {f1.fx, f1.fy, f1.cx, f1.cy, f1.invfx, f1.invfy};
      const float c2[6] = {f2.fx, f2.fy, f2.cx, f2.cy, f2.invfx, f2.invfy};
      std::memcpy(P.cam1, c1, sizeof(c1));
      std::memcpy(P.cam2, c2, sizeof(c2));
      P.ratio_factor = pairs[p].ratio_factor;
      P.pad = 0;
      tri_pair_finish(P);
    }
  }
  return stereo ? SQLM_ERR_UNSUPPORTED : SQLM_OK;
}

void tri_count(int n_pair, const int64_t *match_off, const uint8_t *reason, int32_t *n_new) {
  for (int p = 0; p < n_pair; ++p) {
    int32_t n = 0;
    for (int64_t i = match_off[p]; i < match_off[p + 1]; ++i) n += reason[i] == kTriCreated;
    n_new[p] = n;
  }
}

int mp_args_ok(int n_pt, const int64_t *obs_off, const uint8_t *obs_desc, const float *obs_center, const float *pos,
               const float *ref_center, const float *level_scale, const float *max_scale, const int32_t *best_idx,
               const int32_t *best_median, const float *normal, const float *max_dist, const float *min_dist) {
  if (n_pt < 0 || !csr_ok(obs_off, n_pt)) return SQLM_ERR_INVALID_ARG;
  for (int j = 0; j < n_pt; ++j)
    if (obs_off[j + 1] - obs_off[j] > std::numeric_limits<int32_t>::max() / 8) return SQLM_ERR_INVALID_ARG;
  if (n_pt > 0 && obs_desc && (!best_idx || !best_median)) return SQLM_ERR_INVALID_ARG;
  if (n_pt > 0 && obs_center && (!pos || !ref_center || !level_scale || !max_scale || !normal || !max_dist || !min_dist))
    return SQLM_ERR_INVALID_ARG;
  return SQLM_OK;
}

}  // namespace

}  // namespace sqlm

using namespace sqlm;

extern "C" {

int sqlm_triangulate_info(int32_t out[4]) {
  if (!out) return SQLM_ERR_INVALID_ARG;
  out[0] = kTriSweeps;
  out[1] = kTriBlock;
  out[2] = 64;
  out[3] = 0;
  return SQLM_OK;
}

int sqlm_triangulate_pairs_host(int n_pair, const sqlm_tri_pair *pairs, const int64_t *match_off,
                                const int32_t *matches, int sweeps, float *x3d, uint8_t *reason, int32_t *n_new) {
  if (sweeps < 0) return SQLM_ERR_INVALID_ARG;
  if (int r = tri_gather(n_pair, pairs, match_off, matches, x3d, reason, n_new, nullptr, nullptr)) return r;
  const int64_t n_match = match_off[n_pair];
  std::vector<TriPair> P((size_t)n_pair);
  std::vector<TriMatch> M((size_t)n_match);
  (void)tri_gather(n_pair, pairs, match_off, matches, x3d, reason, n_new, P.data(), M.data());
  const int sw = sweeps ? sweeps : kTriSweeps;
  for (int p = 0; p < n_pair; ++p)
    for (int64_t i = match_off[p]; i < match_off[p + 1]; ++i) reason[i] = tri_match(P[p], M[i], sw, x3d + 3 * i);
  tri_count(n_pair, match_off, reason, n_new);
  return SQLM_OK;
}

int sqlm_triangulate_pairs(sqlm_ctx *c, int n_pair, const sqlm_tri_pair *pairs, const int64_t *match_off,
                           const int32_t *matches, float *x3d, uint8_t *reason, int32_t *n_new) {
  if (!c) return SQLM_ERR_INVALID_ARG;
  if (int r = tri_gather(n_pair, pairs, match_off, matches, x3d, reason, n_new, nullptr, nullptr)) return r;
  const int64_t n_match = match_off[n_pair];
  if (n_match == 0) {
    for (int p = 0; p < n_pair; ++p) n_new[p] = 0;
    return SQLM_OK;
  }
  if (int r = mappoint_solver(c)) return r;
  MapPointSolver *s = c->mappoint;
  const size_t np = (size_t)n_pair, nm = (size_t)n_match;
  Arena in, out;
  const size_t i_pair = in.take(np * sizeof(TriPair)), i_first = in.take((np + 1) * sizeof(int64_t)),
               i_match = in.take(nm * sizeof(TriMatch));
  const size_t o_x = out.take(3 * nm * sizeof(float)), o_r = out.take(nm);
  if (int r = s->in.grow(in.off)) return r;
  if (int r = s->out.grow(out.off)) return r;
  char *h = s->in.host;
  (void)tri_gather(n_pair, pairs, match_off, matches, x3d, reason, n_new, at<TriPair>(h, i_pair),
                   at<TriMatch>(h, i_match));
  std::memcpy(h + i_first, match_off, (np + 1) * sizeof(int64_t));
  SQLM_HIP_OK(hipMemcpyAsync(s->in.dev, s->in.host, in.off, hipMemcpyHostToDevice, c->stream));
  SQLM_HIP_OK(hipMemsetAsync(s->out.dev, 0, out.off, c->stream));
  TriDev d;
  d.pair = at<const TriPair>(s->in.dev, i_pair);
  d.first = at<const int64_t>(s->in.dev, i_first);
  d.match = at<const TriMatch>(s->in.dev, i_match);
  d.n_pair = n_pair;
  d.n_match = n_match;
  d.x3d = at<float>(s->out.dev, o_x);
  d.reason = at<uint8_t>(s->out.dev, o_r);
  launch_triangulate(d, c->stream);
  SQLM_HIP_OK(hipGetLastError());
  SQLM_HIP_OK(hipMemcpyAsync(s->out.host, s->out.dev, out.off, hipMemcpyDeviceToHost, c->stream));
  SQLM_HIP_OK(hipStreamSynchronize(c->stream));
  std::memcpy(x3d, s->out.host + o_x, 3 * nm * sizeof(float));
  std::memcpy(reason, s->out.host + o_r, nm);
  tri_count(n_pair, match_off, reason, n_new);
  return SQLM_OK;
}

int sqlm_map_points_update_host(int n_pt, const int64_t *obs_off, const uint8_t *obs_desc, const float *obs_center,
                                const float *pos, const float *ref_center, const float *level_scale,
                                const float *max_scale, int32_t *best_idx, int32_t *best_median, float *normal,
                                float *max_dist, float *min_dist) {
  if (int r = mp_args_ok(n_pt, obs_off, obs_desc, obs_center, pos, ref_center, level_scale, max_scale, best_idx,
                         best_median, normal, max_dist, min_dist))
    return r;
  std::vector<uint32_t> D;
  for (int j = 0; j < n_pt; ++j) {
    const int64_t o0 = obs_off[j], n = obs_off[j + 1] - o0;
    if (obs_desc) {
      D.resize((size_t)(8 * n));
      if (n) std::memcpy(D.data(), obs_desc + 32 * o0, (size_t)(32 * n));
      int bm = std::numeric_limits<int32_t>::max(), bi = -1;
      for (int i = 0; i < (int)n; ++i) {
        const int med = mp_row_median(D.data() + 8 * (size_t)i, D.data(), (int)n);
        if (med < bm) {
          bm = med;
          bi = i;
        }
      }
      best_idx[j] = bi;
      best_median[j] = bm;
    }
    if (obs_center)
      mp_normal_depth(pos + 3 * (size_t)j, obs_center + 3 * o0, n, ref_center + 3 * (size_t)j, level_scale[j],
                      max_scale[j], normal + 3 * (size_t)j, max_dist + j, min_dist + j);
  }
  return SQLM_OK;
}

int sqlm_map_points_update(sqlm_ctx *c, int n_pt, const int64_t *obs_off, const uint8_t *obs_desc,
                           const float *obs_center, const float *pos, const float *ref_center,
                           const float *level_scale, const float *max_scale, int32_t *best_idx,
                           int32_t *best_median, float *normal, float *max_dist, float *min_dist) {
  if (!c) return SQLM_ERR_INVALID_ARG;
  if (int r = mp_args_ok(n_pt, obs_off, obs_desc, obs_center, pos, ref_center, level_scale, max_scale, best_idx,
                         best_median, normal, max_dist, min_dist))
    return r;
  if (c->mappoint) c->mappoint->n_lds = c->mappoint->n_global = c->mappoint->n_launch = 0;
  if (n_pt == 0 || (!obs_desc && !obs_center)) return SQLM_OK;
  if (int r = mappoint_solver(c)) return r;
  MapPointSolver *s = c->mappoint;
  s->n_lds = s->n_global = s->n_launch = 0;
  const size_t np = (size_t)n_pt, no = (size_t)obs_off[n_pt];
  Arena in, out;
  const size_t i_off = in.take((np + 1) * sizeof(int64_t)), i_desc = in.take(obs_desc ? 32 * no : 0),
               i_cen = in.take(obs_center ? 3 * no * sizeof(float) : 0),
               i_pos = in.take(obs_center ? 3 * np * sizeof(float) : 0),
               i_ref = in.take(obs_center ? 3 * np * sizeof(float) : 0),
               i_ls = in.take(obs_center ? np * sizeof(float) : 0), i_ms = in.take(obs_center ? np * sizeof(float) : 0);
  const size_t o_bi = out.take(np * sizeof(int32_t)), o_bm = out.take(np * sizeof(int32_t)),
               o_n = out.take(3 * np * sizeof(float)), o_mx = out.take(np * sizeof(float)),
               o_mn = out.take(np * sizeof(float));
  if (int r = s->in.grow(in.off)) return r;
  if (int r = s->out.grow(out.off)) return r;
  char *h = s->in.host;
  std::memcpy(h + i_off, obs_off, (np + 1) * sizeof(int64_t));
  if (obs_desc && no) std::memcpy(h + i_desc, obs_desc, 32 * no);
  if (obs_center) {
    if (no) std::memcpy(h + i_cen, obs_center, 3 * no * sizeof(float));
    std::memcpy(h + i_pos, pos, 3 * np * sizeof(float));
    std::memcpy(h + i_ref, ref_center, 3 * np * sizeof(float));
    std::memcpy(h + i_ls, level_scale, np * sizeof(float));
    std::memcpy(h + i_ms, max_scale, np * sizeof(float));
  }
  SQLM_HIP_OK(hipMemcpyAsync(s->in.dev, s->in.host, in.off, hipMemcpyHostToDevice, c->stream));
  SQLM_HIP_OK(hipMemsetAsync(s->out.dev, 0, out.off, c->stream));
  char *di = s->in.dev, *dout = s->out.dev;
  MpDev d;
  d.n_pt = n_pt;
  d.obs_off = at<const int64_t>(di, i_off);
  d.desc = at<const uint32_t>(di, i_desc);
  d.center = at<const float>(di, i_cen);
  d.pos = at<const float>(di, i_pos);
  d.ref_center = at<const float>(di, i_ref);
  d.level_scale = at<const float>(di, i_ls);
  d.max_scale = at<const float>(di, i_ms);
  d.best_idx = at<int32_t>(dout, o_bi);
  d.best_median = at<int32_t>(dout, o_bm);
  d.normal = at<float>(dout, o_n);
  d.max_dist = at<float>(dout, o_mx);
  d.min_dist = at<float>(dout, o_mn);
  if (obs_desc) {
    for (int j = 0; j < n_pt; ++j) ++(obs_off[j + 1] - obs_off[j] <= kMpLdsMax ? s->n_lds : s->n_global);
    launch_mp_descriptor(d, c->stream);
    SQLM_HIP_OK(hipGetLastError());
    ++s->n_launch;
  }
  if (obs_center) {
    launch_mp_normal(d, c->stream);
    SQLM_HIP_OK(hipGetLastError());
    ++s->n_launch;
  }
  SQLM_HIP_OK(hipMemcpyAsync(s->out.host, s->out.dev, out.off, hipMemcpyDeviceToHost, c->stream));
  SQLM_HIP_OK(hipStreamSynchronize(c->stream));
  if (obs_desc) {
    std::memcpy(best_idx, s->out.host + o_bi, np * sizeof(int32_t));
    std::memcpy(best_median, s->out.host + o_bm, np * sizeof(int32_t));
  }
  if (obs_center) {
    std::memcpy(normal, s->out.host + o_n, 3 * np * sizeof(float));
    std::memcpy(max_dist, s->out.host + o_mx, np * sizeof(float));
    std::memcpy(min_dist, s->out.host + o_mn, np * sizeof(float));
  }
  return SQLM_OK;
}

int sqlm_map_points_update_info(const sqlm_ctx *c, int32_t out[4]) {
  if (!out) return SQLM_ERR_INVALID_ARG;
  out[0] = kMpLdsMax;
  out[1] = c && c->mappoint ? c->mappoint->n_lds : 0;
  out[2] = c && c->mappoint ? c->mappoint->n_global : 0;
  out[3] = c && c->mappoint ? c->mappoint->n_launch : 0;
  return SQLM_OK;
}

}  // extern "C"
