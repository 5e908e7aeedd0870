// sqlm_api.cpp — the C ABI (include/sqrtlm.h, include/sqrtlm_orb.h): argument
// checks and forwarding. The setup is sqlm_prepare.cpp (planner: sqlm_plan.cpp),
// the host LM driver sqlm_lm.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/sqrtlm.h"
#include "../../include/sqrtlm_orb.h"
#include "se3_dev.h"
#include "sqlm_ctx.h"

using namespace sqlm;

namespace {

const char *kTimerNames[SQLM_NKERNEL_TIMERS] = {"k_linearize", "k_camera_pass", "k_damp", "k_rcs_tile",
                                                "k_solve", "k_pose_update", "k_landmark_update", "reduce+sync",
                                                "k_rcs_reduce"};

void depth_positive_host(const sqlm_ctx *c, std::vector<uint8_t> &out) {
  out.resize(c->n_obs);
  for (int64_t e = 0; e < c->n_obs; ++e) {
    const int p = c->obs_pose[e];
    double o[3];
    q_rotate(&c->pose_q[4 * p], &c->pt[3 * c->obs_pt[e]], o);
    out[e] = (o[2] + c->pose_t[3 * p + 2]) > 0.0;
  }
}

inline double edge_chi2(const sqlm_ctx *c, int64_t e) {
  const double e0 = c->obs_err[2 * e], e1 = c->obs_err[2 * e + 1], w = c->obs_info[e];
  if (c->has_stereo && c->obs_ur[e] >= 0.0) {  // BaseEdge::chi2 of the 3-D stereo error
    const double e2 = c->obs_err3[e];
    return e0 * (w * e0) + e1 * (w * e1) + e2 * (w * e2);
  }
  return e0 * (w * e0) + e1 * (w * e1);
}

// LBA outlier threshold: chi2(0.95), 2 DoF for mono edges (g2oOptimizer.cc:956,
// 1123). The reference's LBA adds no stereo edges (:914-916); 7.815 (3 DoF) is
// the ORB-SLAM2 value for them.
inline double tag_threshold(const sqlm_ctx *c, int64_t e) {
  return (c->has_stereo && c->obs_ur[e] >= 0.0) ? 7.815 : 5.991;
}

}  // namespace

// ====================================================================== ABI

extern "C" {

const char *sqlm_version(void) { return "sqrtlm-mi355x 0.1.0 (gfx950)"; }

const char *sqlm_status_string(int s) {
  switch (s) {
    case SQLM_OK: return "ok";
    case SQLM_ERR_INVALID_ARG: return "invalid argument";
    case SQLM_ERR_HIP: return "HIP runtime error";
    case SQLM_ERR_NOT_SPD: return "system not positive definite";
    case SQLM_ERR_OOM: return "out of device memory";
    case SQLM_ERR_ABORTED: return "aborted by stop flag";
    case SQLM_ERR_NO_DEVICE: return "no HIP device";
    case SQLM_ERR_STATE: return "call order / state error";
    case SQLM_ERR_UNSUPPORTED: return "problem shape not supported by this build";
    case SQLM_ERR_COMM: return "RCCL communicator error";
    default: return "unknown";
  }
}

int sqlm_ctx_create(int device_id, sqlm_ctx **out) {
  if (!out) return SQLM_ERR_INVALID_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return SQLM_ERR_NO_DEVICE;
  int dev = device_id;
  if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return SQLM_ERR_HIP;
  if (dev >= n) return SQLM_ERR_INVALID_ARG;
  if (hipSetDevice(dev) != hipSuccess) return SQLM_ERR_HIP;
  sqlm_ctx *c = new (std::nothrow) sqlm_ctx();
  if (!c) return SQLM_ERR_OOM;
  c->device = dev;
  if (hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c->n_cu <= 0)
    c->n_cu = 256;
  c->htrace = std::getenv("SQLM_HOST_TRACE") != nullptr;
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return SQLM_ERR_HIP; }
  if (hipHostMalloc((void **)&c->h_scalars, sizeof(double) * kNScalars) != hipSuccess) {
    (void)hipStreamDestroy(c->stream);
    delete c;
    return SQLM_ERR_HIP;
  }
  // the mailbox is an optimisation: without it the trial scalars are copied
  if (hipHostMalloc((void **)&c->mbox, sizeof(double) * kNScalars, hipHostMallocMapped | hipHostMallocCoherent) ==
      hipSuccess) {
    std::memset(c->mbox, 0, sizeof(double) * kNScalars);
    if (hipHostGetDevicePointer((void **)&c->mbox_dev, c->mbox, 0) != hipSuccess) {
      (void)hipHostFree(c->mbox);
      c->mbox = c->mbox_dev = nullptr;
    }
  } else {
    c->mbox = nullptr;
  }
  // timing-only events: no system-scope fence, which would flush caches and
  // leave a ~10 us bubble between the kernels they separate
  for (auto &e : c->ev) (void)hipEventCreateWithFlags(&e, hipEventDisableSystemFence);
  for (auto &pr : c->ev_cam)
    for (auto &e : pr) (void)hipEventCreateWithFlags(&e, hipEventDisableSystemFence);
  // The side stream (the speculative camera pass of large problems, beside the
  // next trial's RCS tiles) at the lowest priority: the tiles keep the CUs and
  // the pass fills their tails (config 4 727.7-728.7 -> 729.6-734.6 it/s,
  // interleaved, profiles/r04/ab_side_prio.log).
  auto side_stream = [](hipStream_t *s) {
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess)
      return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
    return hipStreamCreateWithPriority(s, hipStreamNonBlocking, least);
  };
  // the two extra RCS-tile class streams at normal priority (lowest / highest
  // measured within noise, profiles/r04/ab_tile_prio.log)
  auto tile_stream = [](hipStream_t *s, int) { return hipStreamCreateWithFlags(s, hipStreamNonBlocking); };
  if (side_stream(&c->side) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming | hipEventDisableSystemFence) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming | hipEventDisableSystemFence) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_spec_fork, hipEventDisableTiming | hipEventDisableSystemFence) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_spec_join, hipEventDisableTiming | hipEventDisableSystemFence) != hipSuccess ||
      tile_stream(&c->tiles.s[0], 0) != hipSuccess || tile_stream(&c->tiles.s[1], 1) != hipSuccess ||
      hipEventCreateWithFlags(&c->tiles.fork, hipEventDisableTiming | hipEventDisableSystemFence) != hipSuccess ||
      hipEventCreateWithFlags(&c->tiles.join[0], hipEventDisableTiming | hipEventDisableSystemFence) != hipSuccess ||
      hipEventCreateWithFlags(&c->tiles.join[1], hipEventDisableTiming | hipEventDisableSystemFence) != hipSuccess) {
    sqlm_ctx_destroy(c);
    return SQLM_ERR_HIP;
  }
  *out = c;
  return SQLM_OK;
}

int sqlm_ctx_destroy(sqlm_ctx *c) {
  if (!c) return SQLM_ERR_INVALID_ARG;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  comm_destroy(c->comm);
  if (c->eg) eg_destroy(c->eg);
  if (c->sim3) sim3_destroy(c->sim3);
  if (c->ransac) ransac_destroy(c->ransac);
  if (c->pnp) pnp_destroy(c->pnp);
  if (c->pose) pose_destroy(c->pose);
  if (c->lidar) lidar_destroy(c->lidar);
  if (c->orb) orb_destroy(c->orb);
  if (c->bow) bow_destroy(c->bow);
  if (c->mappoint) mappoint_destroy(c->mappoint);
  if (c->lidar_feat) lidar_feat_destroy(c->lidar_feat);
  if (c->lidar_depth) lidar_depth_destroy(c->lidar_depth);
  for (auto &b : c->bufs)
    if (b.p) (void)hipFree(b.p);
  for (auto &b : c->pins) free_pinned(b);
  for (auto &e : c->ev)
    if (e) (void)hipEventDestroy(e);
  if (c->h_scalars) (void)hipHostFree(c->h_scalars);
  if (c->mbox) (void)hipHostFree(c->mbox);
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  if (c->ev_join) (void)hipEventDestroy(c->ev_join);
  if (c->ev_spec_fork) (void)hipEventDestroy(c->ev_spec_fork);
  if (c->ev_spec_join) (void)hipEventDestroy(c->ev_spec_join);
  for (hipStream_t &x : c->tiles.s)
    if (x) (void)hipStreamDestroy(x);
  for (hipEvent_t x : {c->tiles.fork, c->tiles.join[0], c->tiles.join[1]})
    if (x) (void)hipEventDestroy(x);
  for (auto &pr : c->ev_cam)
    for (auto &e : pr)
      if (e) (void)hipEventDestroy(e);
  if (c->side) (void)hipStreamDestroy(c->side);
  (void)hipStreamDestroy(c->stream);
  delete c;
  return SQLM_OK;
}

int sqlm_set_problem(sqlm_ctx *c, int n_pose, const double *pose_q, const double *pose_t,
                     const uint8_t *pose_fixed, const double *intr, int n_pt, const double *pt, int64_t n_obs,
                     const int32_t *obs_pose, const int32_t *obs_pt, const double *obs_uv, const double *obs_info,
                     const double *obs_delta, const uint8_t *obs_level) {
  if (!c || n_pose < 0 || n_pt < 0 || n_obs < 0) return SQLM_ERR_INVALID_ARG;
  if ((n_pose && (!pose_q || !pose_t || !pose_fixed || !intr)) || (n_pt && !pt) ||
      (n_obs && (!obs_pose || !obs_pt || !obs_uv || !obs_info)))
    return SQLM_ERR_INVALID_ARG;
  {
    const int nth = host_threads(n_obs);
    std::vector<uint8_t> bad(nth, 0);
    run_threads(nth, [&](int t) {
      for (int64_t e = n_obs * t / nth; e < n_obs * (t + 1) / nth; ++e)
        if (obs_pose[e] < 0 || obs_pose[e] >= n_pose || obs_pt[e] < 0 || obs_pt[e] >= n_pt) { bad[t] = 1; break; }
    });
    for (uint8_t b : bad)
      if (b) return SQLM_ERR_INVALID_ARG;
  }
  c->n_pose = n_pose;
  c->n_pt = n_pt;
  c->n_obs = n_obs;
  c->pose_q.assign(pose_q, pose_q + 4 * (size_t)n_pose);
  c->pose_t.assign(pose_t, pose_t + 3 * (size_t)n_pose);
  c->pose_fixed.assign(pose_fixed, pose_fixed + n_pose);
  c->intr.assign(intr, intr + 4 * (size_t)n_pose);
  par_assign(c->pt, pt, 3 * (size_t)n_pt);
  par_assign(c->obs_pose, obs_pose, (size_t)n_obs);
  par_assign(c->obs_pt, obs_pt, (size_t)n_obs);
  par_assign(c->obs_uv, obs_uv, 2 * (size_t)n_obs);
  par_assign(c->obs_info, obs_info, (size_t)n_obs);
  par_assign(c->obs_delta, obs_delta, (size_t)n_obs);  // null: no robust kernel (zeros)
  par_assign(c->obs_level, obs_level, (size_t)n_obs);  // null: level 0
  c->err_pending = false;  // sized and zeroed when first read (ensure_host_errors)
  c->err_zero = true;
  c->opt_done = false;
  c->has_stereo = false;
  c->obs_ur.clear(); c->pose_bf.clear(); c->obs_err3.clear();
  c->n_lid = 0;
  c->lid_pose.clear(); c->lid_pc.clear(); c->lid_pw.clear(); c->lid_n.clear(); c->lid_info.clear();
  c->lid_level.clear(); c->lid_kind.clear(); c->lid_err.clear();
  c->has_problem = true;
  c->prepared = false;  // the CR layout of the previous problem no longer applies
  return SQLM_OK;
}

int sqlm_set_stereo(sqlm_ctx *c, const double *obs_ur, const double *pose_bf) {
  if (!c || !c->has_problem) return SQLM_ERR_STATE;
  c->prepared = false;  // a setter changes what prepare() plans
  if (int s = fetch_errors(c)) return s;  // the last call's errors, in the layout they were computed in
  c->has_stereo = false;
  c->obs_ur.clear(); c->pose_bf.clear(); c->obs_err3.clear();
  if (!obs_ur) return SQLM_OK;  // back to all-mono
  if (!pose_bf && c->n_pose) return SQLM_ERR_INVALID_ARG;
  bool any = false;
  for (int64_t e = 0; e < c->n_obs; ++e) {
    if (!std::isfinite(obs_ur[e])) return SQLM_ERR_INVALID_ARG;
    any |= obs_ur[e] >= 0.0;
  }
  if (!any) return SQLM_OK;
  c->obs_ur.assign(obs_ur, obs_ur + c->n_obs);
  c->pose_bf.assign(pose_bf, pose_bf + c->n_pose);
  c->obs_err3.assign(c->n_obs, 0.0);
  c->has_stereo = true;
  return SQLM_OK;
}

int sqlm_set_lidar(sqlm_ctx *c, int64_t n, const int32_t *pose, const double *p_cam, const double *p_world,
                   const double *normal, const double *info) {
  if (!c || !c->has_problem || n < 0) return SQLM_ERR_INVALID_ARG;
  c->prepared = false;  // a setter changes what prepare() plans
  if (n && (!pose || !p_cam || !p_world || !normal || !info)) return SQLM_ERR_INVALID_ARG;
  for (int64_t e = 0; e < n; ++e)
    if (pose[e] < 0 || pose[e] >= c->n_pose) return SQLM_ERR_INVALID_ARG;
  if (int s = fetch_errors(c)) return s;  // the last call's errors, in the layout they were computed in
  c->n_lid = n;
  c->lid_pose.assign(pose, pose + n);
  c->lid_pc.assign(p_cam, p_cam + 3 * n);
  c->lid_pw.assign(p_world, p_world + 3 * n);
  c->lid_n.assign(normal, normal + 3 * n);
  c->lid_info.assign(info, info + n);
  c->lid_level.assign(n, 0);
  c->lid_kind.assign(n, 0);
  c->lid_err.assign(n, 0.0);
  c->opt_done = false;
  return SQLM_OK;
}

int sqlm_set_edge_level(sqlm_ctx *c, const uint8_t *level) {
  if (!c || !c->has_problem || (!level && c->n_obs)) return SQLM_ERR_INVALID_ARG;
  c->prepared = false;  // a setter changes what prepare() plans
  c->obs_level.assign(level, level + c->n_obs);
  return SQLM_OK;
}

int sqlm_set_lidar_level(sqlm_ctx *c, const uint8_t *level) {
  if (!c || !c->has_problem || (!level && c->n_lid)) return SQLM_ERR_INVALID_ARG;
  c->prepared = false;  // a setter changes what prepare() plans
  c->lid_level.assign(level, level + c->n_lid);
  return SQLM_OK;
}

int sqlm_set_lidar_kind(sqlm_ctx *c, const uint8_t *kind) {
  if (!c) return SQLM_ERR_INVALID_ARG;
  if (!c->has_problem) return SQLM_ERR_STATE;
  for (int64_t e = 0; kind && e < c->n_lid; ++e)
    if (kind[e] > 1) return SQLM_ERR_INVALID_ARG;
  c->prepared = false;  // a setter changes what prepare() plans
  if (kind) c->lid_kind.assign(kind, kind + c->n_lid);
  else c->lid_kind.assign((size_t)c->n_lid, 0);
  return SQLM_OK;
}

int sqlm_set_robust(sqlm_ctx *c, const double *delta) {
  if (!c || !c->has_problem) return SQLM_ERR_INVALID_ARG;
  c->prepared = false;  // a setter changes what prepare() plans
  if (delta) c->obs_delta.assign(delta, delta + c->n_obs);
  else c->obs_delta.assign(c->n_obs, 0.0);
  return SQLM_OK;
}

int sqlm_optimize(sqlm_ctx *c, int level, int iterations, double user_lambda, const volatile uint8_t *stop,
                  sqlm_stats *st, int *n_iter) {
  if (!c || iterations < 0) return SQLM_ERR_INVALID_ARG;
  if (hipSetDevice(c->device) != hipSuccess) return SQLM_ERR_HIP;
  return optimize_impl(c, level, iterations, user_lambda, stop, st, n_iter);
}

int sqlm_local_ba(sqlm_ctx *c, const volatile uint8_t *stop, uint8_t *outlier, sqlm_stats st[3], int *ran) {
  if (!c || !c->has_problem) return SQLM_ERR_STATE;
  if (hipSetDevice(c->device) != hipSuccess) return SQLM_ERR_HIP;
  sqlm_stats tmp[3];
  if (!st) st = tmp;
  std::memset(st, 0, 3 * sizeof(sqlm_stats));
  if (ran) *ran = 0;
  if (stopped(stop)) return SQLM_OK;  // g2oOptimizer.cc:923-928
  for (auto &l : c->lid_level) l = 255;  // LiDAR edges only exist in pass 3
  int n = 0, s = optimize_impl(c, 0, 5, 0.0, stop, &st[0], &n);
  if (s) return s;
  if ((s = fetch_errors(c))) return s;
  ensure_host_errors(c);
  if (!stopped(stop)) {  // :952-975
    std::vector<uint8_t> dp;
    depth_positive_host(c, dp);
    for (int64_t e = 0; e < c->n_obs; ++e) {
      if (edge_chi2(c, e) > tag_threshold(c, e) || !dp[e]) c->obs_level[e] = 1;
      c->obs_delta[e] = 0.0;
    }
    s = optimize_impl(c, 0, 10, 0.0, stop, &st[1], &n);
    if (s) return s;
  }
  for (auto &l : c->lid_level) l = 0;  // :1113-1114
  s = optimize_impl(c, 0, 20, 0.0, stop, &st[2], &n);
  if (s) return s;
  if (outlier) {  // :1119-1136
    std::vector<uint8_t> dp;
    depth_positive_host(c, dp);
    if ((s = fetch_errors(c))) return s;
    ensure_host_errors(c);
    for (int64_t e = 0; e < c->n_obs; ++e) outlier[e] = (edge_chi2(c, e) > tag_threshold(c, e) || !dp[e]);
  }
  if (ran) *ran = 1;
  return SQLM_OK;
}

int sqlm_eg_set_problem(sqlm_ctx *c, int n_kf, const double *Siw, const uint8_t *fixed, int fix_scale, int64_t n_edge,
                        const int32_t *ei, const int32_t *ej, const double *Sji, const double *info) {
  if (!c) return SQLM_ERR_INVALID_ARG;
  if (hipSetDevice(c->device) != hipSuccess) return SQLM_ERR_HIP;
  if (!c->eg && !(c->eg = eg_create(c->stream))) return SQLM_ERR_OOM;
  return eg_set_problem(c->eg, n_kf, Siw, fixed, fix_scale, n_edge, ei, ej, Sji, info);
}

int sqlm_eg_optimize(sqlm_ctx *c, int iterations, double user_lambda, const volatile uint8_t *stop, sqlm_stats *st,
                     int *n_iter) {
  if (!c || !c->eg) return SQLM_ERR_STATE;
  if (hipSetDevice(c->device) != hipSuccess) return SQLM_ERR_HIP;
  return eg_optimize(c->eg, iterations, user_lambda, stop, st, n_iter);
}

int sqlm_eg_get_poses(sqlm_ctx *c, double *Siw) {
  if (!c || !c->eg) return SQLM_ERR_STATE;
  return eg_get_poses(c->eg, Siw);
}

int sqlm_eg_get_edge_chi2(sqlm_ctx *c, double *chi2) {
  if (!c || !c->eg) return SQLM_ERR_STATE;
  return eg_get_edge_chi2(c->eg, chi2);
}

int sqlm_eg_get_jacobians(sqlm_ctx *c, double *J) {
  if (!c || !c->eg) return SQLM_ERR_STATE;
  if (hipSetDevice(c->device) != hipSuccess) return SQLM_ERR_HIP;
  return eg_get_jacobians(c->eg, J);
}

int sqlm_eg_get_last_step(sqlm_ctx *c, double *b, double *dx) {
  if (!c || !b || !dx) return SQLM_ERR_INVALID_ARG;
  if (!c->eg) return SQLM_ERR_STATE;
  return eg_get_last_step(c->eg, b, dx);
}

int sqlm_eg_get_exec_info(sqlm_ctx *c, int out[8]) {
  if (!c || !out) return SQLM_ERR_INVALID_ARG;
  if (!c->eg) return SQLM_ERR_STATE;
  return eg_get_exec_info(c->eg, out);
}

int sqlm_sim3_optimize(sqlm_ctx *c, int n_prob, const double *S12, const double *intr1, const double *intr2,
                       const uint8_t *fix_scale, const double *th2, const int64_t *pair_off, const double *X1c,
                       const double *X2c, const double *obs1, const double *obs2, const double *info1,
                       const double *info2, const int32_t iters[3], double user_lambda, double *S12_out,
                       int32_t *n_inliers, uint8_t *pair_state, sqlm_sim3_stats *stats) {
  if (!c || n_prob < 0 || !pair_off) return SQLM_ERR_INVALID_ARG;
  if (iters && (iters[0] < 0 || iters[1] < 0 || iters[2] < 0)) return SQLM_ERR_INVALID_ARG;
  if (n_prob > 0 && (!S12 || !intr1 || !intr2 || !fix_scale || !th2 || !S12_out || !n_inliers))
    return SQLM_ERR_INVALID_ARG;
  for (int k = 0; k < n_prob; ++k)
    if (pair_off[k + 1] < pair_off[k] || pair_off[k + 1] - pair_off[k] > INT32_MAX) return SQLM_ERR_INVALID_ARG;
  if (pair_off[0] < 0) return SQLM_ERR_INVALID_ARG;
  if (pair_off[n_prob] > pair_off[0] && (!X1c || !X2c || !obs1 || !obs2 || !info1 || !info2 || !pair_state))
    return SQLM_ERR_INVALID_ARG;
  if (hipSetDevice(c->device) != hipSuccess) return SQLM_ERR_HIP;
  if (!c->sim3 && !(c->sim3 = sim3_create(c->stream))) return SQLM_ERR_OOM;
  Sim3Args a;
  a.n_prob = n_prob;
  a.S12 = S12; a.intr1 = intr1; a.intr2 = intr2; a.fix_scale = fix_scale; a.th2 = th2; a.pair_off = pair_off;
  a.X1c = X1c; a.X2c = X2c; a.obs1 = obs1; a.obs2 = obs2; a.info1 = info1; a.info2 = info2;
  a.iters = iters; a.user_lambda = user_lambda;
  a.S12_out = S12_out; a.n_inliers = n_inliers; a.pair_state = pair_state; a.stats = stats;
  return sim3_optimize(c->sim3, a);
}

int sqlm_sim3_get_pair_chi2(sqlm_ctx *c, double *chi2) {
  if (!c || !chi2) return SQLM_ERR_INVALID_ARG;
  if (!c->sim3) return SQLM_ERR_STATE;
  return sim3_get_pair_chi2(c->sim3, chi2);
}

int sqlm_sim3_get_linearization(sqlm_ctx *c, double *e, double *J) {
  if (!c || (!e && !J)) return SQLM_ERR_INVALID_ARG;
  if (!c->sim3) return SQLM_ERR_STATE;
  return sim3_get_linearization(c->sim3, e, J);
}

int sqlm_sim3_get_last_step(sqlm_ctx *c, int prob, double *H, double *b, double *dx) {
  if (!c || !H || !b || !dx) return SQLM_ERR_INVALID_ARG;
  if (!c->sim3) return SQLM_ERR_STATE;
  return sim3_get_last_step(c->sim3, prob, H, b, dx);
}

int sqlm_sim3_ransac(sqlm_ctx *c, int n_prob, const double *intr1, const double *intr2, const uint8_t *fix_scale,
                     const int32_t *min_inliers, const int64_t *pair_off, const double *X1c, const double *X2c,
                     const int32_t *max_err1, const int32_t *max_err2, const int64_t *hyp_off, const int32_t *draws,
                     int32_t *n_inliers, uint8_t *flags, float *R12, float *t12, float *s12, int32_t *first_return,
                     int32_t *best) {
  if (!c) return SQLM_ERR_INVALID_ARG;
  RansacArgs a;
  a.n_prob = n_prob;
  a.intr1 = intr1; a.intr2 = intr2; a.fix_scale = fix_scale; a.min_inliers = min_inliers; a.pair_off = pair_off;
  a.X1c = X1c; a.X2c = X2c; a.max_err1 = max_err1; a.max_err2 = max_err2; a.hyp_off = hyp_off; a.draws = draws;
  a.n_inliers = n_inliers; a.flags = flags; a.R12 = R12; a.t12 = t12; a.s12 = s12;
  a.first_return = first_return; a.best = best;
  if (int r = ransac_args_ok(a)) return r;
  if (hipSetDevice(c->device) != hipSuccess) return SQLM_ERR_HIP;
  if (!c->ransac && !(c->ransac = ransac_create(c->stream))) return SQLM_ERR_OOM;
  return ransac_run(c->ransac, a);
}

int sqlm_sim3_ransac_get_inliers(sqlm_ctx *c, int prob, int hyp, uint8_t *mask) {
  if (!c || !mask) return SQLM_ERR_INVALID_ARG;
  if (!c->ransac) return SQLM_ERR_STATE;
  return ransac_get_inliers(c->ransac, prob, hyp, mask);
}

int sqlm_sim3_ransac_get_hypothesis(sqlm_ctx *c, int prob, int hyp, int32_t idx[3], float T12[16], float T21[16]) {
  if (!c || (!idx && !T12 && !T21)) return SQLM_ERR_INVALID_ARG;
  if (!c->ransac) return SQLM_ERR_STATE;
  return ransac_get_hypothesis(c->ransac, prob, hyp, idx, T12, T21);
}

int sqlm_sim3_ransac_max_its(int64_t n_pair, double probability, int min_inliers, int max_iterations) {
  return ransac_max_its(n_pair, probability, min_inliers, max_iterations);
}

int sqlm_sim3_ransac_scan(int64_t n_hyp, const int32_t *counts, int min_inliers, uint8_t *flags,
                          int64_t *first_return, int64_t *best) {
  if (n_hyp < 0 || (n_hyp > 0 && (!counts || !flags))) return SQLM_ERR_INVALID_ARG;
  ransac_scan(n_hyp, counts, min_inliers, flags, first_return, best);
  return SQLM_OK;
}

int sqlm_sim3_ransac_hypothesis_host(int n_pair, const double intr1[4], const double intr2[4], int fix_scale,
                                     const double *X1c, const double *X2c, const int32_t *max_err1,
                                     const int32_t *max_err2, const int32_t draws[3], int32_t idx[3], float R12[9],
                                     float t12[3], float *s12, float T12[16], float T21[16], uint8_t *mask,
                                     int32_t *n_inliers) {
  if (!intr1 || !intr2 || !X1c || !X2c || !max_err1 || !max_err2 || !draws || !idx || !R12 || !t12 || !s12 || !T12 ||
      !T21 || !mask || !n_inliers)
    return SQLM_ERR_INVALID_ARG;
  float h[34];  // RansacHyp: R 9, t 3, s, sR 9, sRinv 9, tinv 3
  if (int r = ransac_hypothesis_host(n_pair, intr1, intr2, fix_scale, X1c, X2c, max_err1, max_err2, draws, idx, h,
                                     mask, n_inliers))
    return r;
  std::memcpy(R12, h, 9 * sizeof(float));
  std::memcpy(t12, h + 9, 3 * sizeof(float));
  *s12 = h[12];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      T12[4 * i + j] = i == 3 ? (j == 3 ? 1.f : 0.f) : (j == 3 ? h[9 + i] : h[13 + 3 * i + j]);
      T21[4 * i + j] = i == 3 ? (j == 3 ? 1.f : 0.f) : (j == 3 ? h[31 + i] : h[22 + 3 * i + j]);
    }
  return SQLM_OK;
}

namespace {

// the diagnostics of a PnP solve (kPnpDiag doubles) into the ABI's separate arrays
void pnp_split_diag(const double *d, double *ut, double *eig, double *betas, double *rep, int32_t *chosen) {
  if (ut) std::memcpy(ut, d, 144 * sizeof(double));
  if (eig) std::memcpy(eig, d + 144, 12 * sizeof(double));
  if (betas) std::memcpy(betas, d + 156, 12 * sizeof(double));
  if (rep) std::memcpy(rep, d + 168, 3 * sizeof(double));
  if (chosen) *chosen = (int32_t)d[171];
}

}  // namespace

int sqlm_pnp_ransac(sqlm_ctx *c, int n_prob, const double *intr, const int32_t *min_inliers, const int64_t *pair_off,
                    const float *Xw, const float *uv, const float *max_err, const int64_t *hyp_off,
                    const int32_t *draws, int32_t *n_inliers, uint8_t *flags, double *R, double *t,
                    int32_t *first_return, int32_t *best, float *Tcw, int32_t *n_refined) {
  if (!c) return SQLM_ERR_INVALID_ARG;
  PnpArgs a;
  a.n_prob = n_prob;
  a.intr = intr; a.min_inliers = min_inliers; a.pair_off = pair_off; a.Xw = Xw; a.uv = uv; a.max_err = max_err;
  a.hyp_off = hyp_off; a.draws = draws; a.n_inliers = n_inliers; a.flags = flags; a.R = R; a.t = t;
  a.first_return = first_return; a.best = best; a.Tcw = Tcw; a.n_refined = n_refined;
  if (int r = pnp_args_ok(a)) return r;
  if (hipSetDevice(c->device) != hipSuccess) return SQLM_ERR_HIP;
  if (!c->pnp && !(c->pnp = pnp_create(c->stream))) return SQLM_ERR_OOM;
  return pnp_run(c->pnp, a);
}

int sqlm_pnp_ransac_get_inliers(sqlm_ctx *c, int prob, int hyp, uint8_t *mask) {
  if (!c || !mask) return SQLM_ERR_INVALID_ARG;
  if (!c->pnp) return SQLM_ERR_STATE;
  return pnp_get_inliers(c->pnp, prob, hyp, mask);
}

int sqlm_pnp_ransac_get_refined(sqlm_ctx *c, int prob, int hyp, double R[9], double t[3], uint8_t *mask,
                                int32_t *n_inliers, double ut[144], double eig[12], double betas[12],
                                double rep_err[3], int32_t *chosen) {
  if (!c) return SQLM_ERR_INVALID_ARG;
  if (!c->pnp) return SQLM_ERR_STATE;
  double d[kPnpDiag];
  if (int r = pnp_get_refined(c->pnp, prob, hyp, R, t, mask, n_inliers, d)) return r;
  pnp_split_diag(d, ut, eig, betas, rep_err, chosen);
  return SQLM_OK;
}

int sqlm_pnp_ransac_get_hypothesis(sqlm_ctx *c, int prob, int hyp, int32_t idx[4], double ut[144], double eig[12],
                                   double betas[12], double rep_err[3], int32_t *chosen) {
  if (!c) return SQLM_ERR_INVALID_ARG;
  if (!c->pnp) return SQLM_ERR_STATE;
  const bool want = ut || eig || betas || rep_err || chosen;
  if (want && hipSetDevice(c->device) != hipSuccess) return SQLM_ERR_HIP;
  double d[kPnpDiag];
  if (int r = pnp_get_hypothesis(c->pnp, prob, hyp, idx, want ? d : nullptr)) return r;
  if (want) pnp_split_diag(d, ut, eig, betas, rep_err, chosen);
  return SQLM_OK;
}

int sqlm_pnp_ransac_max_its(int64_t n_pair, double probability, int min_inliers, int max_iterations, int min_set,
                            float epsilon, int *min_inliers_out) {
  if (n_pair < 0 || n_pair > INT32_MAX) return 0;
  return pnp_max_its(n_pair, probability, min_inliers, max_iterations, min_set, epsilon, min_inliers_out);
}

int sqlm_pnp_ransac_scan(int64_t n_hyp, const int32_t *counts, const int32_t *refined, int64_t n_refined,
                         int min_inliers, uint8_t *flags, int64_t *first_return, int64_t *best, int64_t *n_record) {
  if (n_hyp < 0 || n_refined < 0 || (n_hyp > 0 && !counts)) return SQLM_ERR_INVALID_ARG;
  pnp_scan(n_hyp, counts, refined, n_refined, min_inliers, flags, first_return, best, n_record);
  return SQLM_OK;
}

int sqlm_pnp_ransac_hypothesis_host(int n_pair, const double intr[4], const float *Xw, const float *uv,
                                    const float *max_err, const int32_t draws[4], const int32_t sweeps[3],
                                    int32_t idx[4], double R[9], double t[3], uint8_t *mask, int32_t *n_inliers,
                                    double ut[144], double eig[12], double betas[12], double rep_err[3],
                                    int32_t *chosen) {
  if (!intr || !Xw || !uv || !max_err || !draws || !idx || !R || !t || !mask || !n_inliers)
    return SQLM_ERR_INVALID_ARG;
  double d[kPnpDiag];
  if (int r = pnp_hypothesis_host(n_pair, intr, Xw, uv, max_err, draws, sweeps, idx, R, t, mask, n_inliers, d))
    return r;
  pnp_split_diag(d, ut, eig, betas, rep_err, chosen);
  return SQLM_OK;
}

int sqlm_pnp_ransac_refine_host(int n_pair, const double intr[4], const float *Xw, const float *uv,
                                const float *max_err, const uint8_t *in_mask, const int32_t sweeps[3], double R[9],
                                double t[3], uint8_t *mask, int32_t *n_inliers, double ut[144], double eig[12],
                                double betas[12], double rep_err[3], int32_t *chosen) {
  if (!intr || !Xw || !uv || !max_err || !in_mask || !R || !t || !mask || !n_inliers) return SQLM_ERR_INVALID_ARG;
  double d[kPnpDiag];
  if (int r = pnp_refine_host(n_pair, intr, Xw, uv, max_err, in_mask, sweeps, R, t, mask, n_inliers, d)) return r;
  pnp_split_diag(d, ut, eig, betas, rep_err, chosen);
  return SQLM_OK;
}

namespace {

// the argument checks sqlm_pose_optimize and sqlm_pose_refine_lidar share
int pose_args_ok(const sqlm_ctx *c, const PoseArgs &a) {
  if (!c || a.n_prob < 0 || !a.obs_off) return 0;
  if (!(a.th2 > 0.0) || !(a.user_lambda >= 0.0)) return 0;
  for (int k = 0; k < 5; ++k)
    if (a.iters[k] < 0) return 0;
  if (a.refine && (!a.lid_off || a.iters[4] < 1)) return 0;
  if (a.n_prob > 0 && (!a.pose_q || !a.pose_t || !a.intr || !a.pose_q_out || !a.pose_t_out || !a.n_inliers)) return 0;
  if (a.n_prob > 0 && a.refine && !a.robust_on) return 0;
  if (a.obs_off[0] < 0 || (a.refine && a.lid_off[0] < 0)) return 0;
  for (int k = 0; k < a.n_prob; ++k) {
    if (a.obs_off[k + 1] < a.obs_off[k] || a.obs_off[k + 1] - a.obs_off[k] > INT32_MAX) return 0;
    if (a.refine && (a.lid_off[k + 1] < a.lid_off[k] || a.lid_off[k + 1] - a.lid_off[k] > INT32_MAX)) return 0;
  }
  if (a.obs_off[a.n_prob] > a.obs_off[0] && (!a.Xw || !a.uv || !a.info || !a.outlier || (a.refine && !a.outlier_in)))
    return 0;
  if (a.refine && a.lid_off[a.n_prob] > a.lid_off[0] && (!a.lid_kind || !a.lid_pc || !a.lid_pw || !a.lid_n || !a.lid_info))
    return 0;
  return 1;
}

int pose_call(sqlm_ctx *c, const PoseArgs &a) {
  if (!pose_args_ok(c, a)) return SQLM_ERR_INVALID_ARG;
  if (hipSetDevice(c->device) != hipSuccess) return SQLM_ERR_HIP;
  if (!c->pose && !(c->pose = pose_create(c->stream))) return SQLM_ERR_OOM;
  return pose_run(c->pose, a);
}

}  // namespace

int sqlm_pose_optimize(sqlm_ctx *c, int n_prob, const double *pose_q, const double *pose_t, const double *intr,
                       const int64_t *obs_off, const double *Xw, const double *uv, const double *info,
                       const int32_t iters[4], double th2, double user_lambda, double *pose_q_out, double *pose_t_out,
                       int32_t *n_inliers, uint8_t *outlier, sqlm_pose_stats *stats) {
  PoseArgs a;
  a.n_prob = n_prob;
  a.pose_q = pose_q; a.pose_t = pose_t; a.intr = intr; a.obs_off = obs_off;
  a.Xw = Xw; a.uv = uv; a.info = info;
  if (iters)
    for (int k = 0; k < 4; ++k) a.iters[k] = iters[k];
  a.th2 = th2; a.user_lambda = user_lambda;
  a.pose_q_out = pose_q_out; a.pose_t_out = pose_t_out; a.n_inliers = n_inliers; a.outlier = outlier; a.stats = stats;
  return pose_call(c, a);
}

int sqlm_pose_refine_lidar(sqlm_ctx *c, int n_prob, const double *pose_q, const double *pose_t, const double *intr,
                           const int64_t *obs_off, const double *Xw, const double *uv, const double *info,
                           const uint8_t *outlier_in, const uint8_t *robust_on, const int64_t *lid_off,
                           const uint8_t *lid_kind, const double *lid_pc, const double *lid_pw, const double *lid_n,
                           const double *lid_info, const int32_t *iters, double th2, double user_lambda,
                           double *pose_q_out, double *pose_t_out, int32_t *n_inliers, uint8_t *outlier,
                           sqlm_pose_stats *stats) {
  PoseArgs a;
  a.n_prob = n_prob;
  a.refine = 1;
  a.pose_q = pose_q; a.pose_t = pose_t; a.intr = intr; a.obs_off = obs_off;
  a.Xw = Xw; a.uv = uv; a.info = info;
  a.outlier_in = outlier_in; a.robust_on = robust_on;
  a.lid_off = lid_off; a.lid_kind = lid_kind; a.lid_pc = lid_pc; a.lid_pw = lid_pw; a.lid_n = lid_n;
  a.lid_info = lid_info;
  if (iters) a.iters[4] = iters[0];
  a.th2 = th2; a.user_lambda = user_lambda;
  a.pose_q_out = pose_q_out; a.pose_t_out = pose_t_out; a.n_inliers = n_inliers; a.outlier = outlier; a.stats = stats;
  return pose_call(c, a);
}

int sqlm_pose_get_edge_chi2(sqlm_ctx *c, double *chi2) {
  if (!c || !chi2) return SQLM_ERR_INVALID_ARG;
  if (!c->pose) return SQLM_ERR_STATE;
  return pose_get_edge_chi2(c->pose, chi2);
}

int sqlm_pose_get_linearization(sqlm_ctx *c, double *e, double *J, double *lid_e, double *lid_J) {
  if (!c || (!e && !J && !lid_e && !lid_J)) return SQLM_ERR_INVALID_ARG;
  if (!c->pose) return SQLM_ERR_STATE;
  return pose_get_linearization(c->pose, e, J, lid_e, lid_J);
}

int sqlm_pose_get_last_step(sqlm_ctx *c, int prob, double *H, double *b, double *dx) {
  if (!c || !H || !b || !dx) return SQLM_ERR_INVALID_ARG;
  if (!c->pose) return SQLM_ERR_STATE;
  return pose_get_last_step(c->pose, prob, H, b, dx);
}

namespace {

void lidar_pack(LidarArgs &a, int n_map_clouds, const int64_t *map_off, const float *map_xyz, const float *map_Twc,
                int64_t n_query, const float *query_xyz, const float *query_Twc, double thr) {
  a.n_map_clouds = n_map_clouds; a.map_off = map_off; a.map_xyz = map_xyz; a.map_Twc = map_Twc;
  a.n_query = n_query; a.query_xyz = query_xyz; a.query_Twc = query_Twc; a.thr = thr;
}

int lidar_call(sqlm_ctx *c, const LidarArgs &a) {
  if (hipSetDevice(c->device) != hipSuccess) return SQLM_ERR_HIP;
  if (!c->lidar && !(c->lidar = lidar_create(c->stream, c->n_cu))) return SQLM_ERR_OOM;
  return lidar_run(c->lidar, a);
}

}  // namespace

int sqlm_lidar_associate(sqlm_ctx *c, int n_map_clouds, const int64_t *map_off, const float *map_xyz,
                         const float *map_Twc, int64_t n_query, const float *query_xyz, const float *query_Twc,
                         double dist_sq_threshold, int32_t *nn_index, float *nn_sq_dist, float *nn_xyz,
                         uint8_t *accepted, int64_t *n_pairs) {
  if (!c) return SQLM_ERR_INVALID_ARG;
  LidarArgs a;
  lidar_pack(a, n_map_clouds, map_off, map_xyz, map_Twc, n_query, query_xyz, query_Twc, dist_sq_threshold);
  a.nn_index = nn_index; a.nn_sq_dist = nn_sq_dist; a.nn_xyz = nn_xyz; a.accepted = accepted; a.n_pairs = n_pairs;
  if (!lidar_args_ok(a)) return SQLM_ERR_INVALID_ARG;
  return lidar_call(c, a);
}

int sqlm_set_lidar_from_clouds(sqlm_ctx *c, int32_t pose_index, int n_map_clouds, const int64_t *map_off,
                               const float *map_xyz, const float *map_Twc, int64_t n_query, const float *query_xyz,
                               const float *query_Twc, const float *query_normal, double info,
                               double dist_sq_threshold, int64_t *n_pairs) {
  if (!c) return SQLM_ERR_INVALID_ARG;
  if (!c->has_problem) return SQLM_ERR_STATE;
  if (pose_index < 0 || pose_index >= c->n_pose || c->pose_fixed[pose_index]) return SQLM_ERR_INVALID_ARG;
  LidarArgs a;
  lidar_pack(a, n_map_clouds, map_off, map_xyz, map_Twc, n_query, query_xyz, query_Twc, dist_sq_threshold);
  if (!lidar_args_ok(a) || (n_query > 0 && !query_normal)) return SQLM_ERR_INVALID_ARG;
  if (int s = lidar_call(c, a)) return s;
  // the accepted pairs in query order (g2oOptimizer.cc:1045-1070): p_cam the
  // query in its sensor frame, p_world the transformed float map point
  const int64_t n = lidar_n_pairs(c->lidar);
  std::vector<int32_t> pose((size_t)n, pose_index);
  std::vector<double> pc(3 * (size_t)n), pw(3 * (size_t)n), nm(3 * (size_t)n), w((size_t)n, info);
  const int32_t *pq = n ? lidar_pair_query(c->lidar) : nullptr;
  const float *xyz = n ? lidar_nn_xyz(c->lidar) : nullptr;
  for (int64_t k = 0; k < n; ++k) {
    const int64_t i = pq[k];
    for (int j = 0; j < 3; ++j) {
      pc[3 * k + j] = (double)query_xyz[3 * i + j];
      pw[3 * k + j] = (double)xyz[3 * i + j];
      nm[3 * k + j] = (double)query_normal[3 * i + j];
    }
  }
  if (n_pairs) *n_pairs = n;
  return sqlm_set_lidar(c, n, pose.data(), pc.data(), pw.data(), nm.data(), w.data());
}

int sqlm_set_lidar_from_cloud_sets(sqlm_ctx *c, int32_t pose_index, int n_sets, const sqlm_lidar_set *sets,
                                   int64_t *n_pairs) {
  if (!c) return SQLM_ERR_INVALID_ARG;
  if (!c->has_problem) return SQLM_ERR_STATE;
  if (pose_index < 0 || pose_index >= c->n_pose || c->pose_fixed[pose_index]) return SQLM_ERR_INVALID_ARG;
  if (n_sets < 0 || (n_sets && !sets)) return SQLM_ERR_INVALID_ARG;
  std::vector<LidarArgs> args((size_t)n_sets);
  for (int k = 0; k < n_sets; ++k) {  // every set is checked before the first one reaches the device
    const sqlm_lidar_set &s = sets[k];
    if (s.kind < 0 || s.kind > 1) return SQLM_ERR_INVALID_ARG;
    lidar_pack(args[k], s.n_map_clouds, s.map_off, s.map_xyz, s.map_Twc, s.n_query, s.query_xyz, s.query_Twc,
               s.dist_sq_threshold);
    if (!lidar_args_ok(args[k]) || (s.kind == 0 && s.n_query > 0 && !s.query_normal)) return SQLM_ERR_INVALID_ARG;
  }
  // set by set, the accepted pairs in query order: the reference inserts the
  // flat edges (g2oOptimizer.cc:1034-1070), then the corner edges (:1075-1107)
  std::vector<int32_t> pose;
  std::vector<double> pc, pw, nm, w;
  std::vector<uint8_t> kind;
  for (int k = 0; k < n_sets; ++k) {
    const sqlm_lidar_set &s = sets[k];
    const LidarArgs &a = args[k];
    if (n_pairs) n_pairs[k] = 0;
    // an empty map or no query: no edge, no launch (a lone set goes the way of sqlm_set_lidar_from_clouds)
    if (n_sets > 1 && (a.n_query == 0 || a.map_off[a.n_map_clouds] == a.map_off[0])) continue;
    if (int r = lidar_call(c, a)) return r;
    const int64_t n = lidar_n_pairs(c->lidar);
    const int32_t *pq = n ? lidar_pair_query(c->lidar) : nullptr;
    const float *xyz = n ? lidar_nn_xyz(c->lidar) : nullptr;
    for (int64_t j = 0; j < n; ++j) {
      const int64_t i = pq[j];
      for (int x = 0; x < 3; ++x) {
        pc.push_back((double)s.query_xyz[3 * i + x]);
        pw.push_back((double)xyz[3 * i + x]);
        nm.push_back(s.query_normal ? (double)s.query_normal[3 * i + x] : 0.0);
      }
    }
    pose.insert(pose.end(), (size_t)n, pose_index);
    w.insert(w.end(), (size_t)n, s.info);
    kind.insert(kind.end(), (size_t)n, (uint8_t)s.kind);
    if (n_pairs) n_pairs[k] = n;
  }
  if (int r = sqlm_set_lidar(c, (int64_t)pose.size(), pose.data(), pc.data(), pw.data(), nm.data(), w.data())) return r;
  return sqlm_set_lidar_kind(c, kind.data());
}

int sqlm_lidar_get_exec_info(sqlm_ctx *c, int out[8]) {
  if (!c || !out) return SQLM_ERR_INVALID_ARG;
  if (!c->lidar) return SQLM_ERR_STATE;
  return lidar_get_exec_info(c->lidar, out);
}

int sqlm_global_ba(sqlm_ctx *c, int iterations, const volatile uint8_t *stop, sqlm_stats *st, int *n_iter) {
  return sqlm_optimize(c, 0, iterations, 0.0, stop, st, n_iter);
}

int sqlm_get_poses(sqlm_ctx *c, double *q, double *t) {
  if (!c || !c->has_problem) return SQLM_ERR_STATE;
  if (q) std::memcpy(q, c->pose_q.data(), sizeof(double) * c->pose_q.size());
  if (t) std::memcpy(t, c->pose_t.data(), sizeof(double) * c->pose_t.size());
  return SQLM_OK;
}

int sqlm_get_points(sqlm_ctx *c, double *pt) {
  if (!c || !c->has_problem) return SQLM_ERR_STATE;
  if (pt) std::memcpy(pt, c->pt.data(), sizeof(double) * c->pt.size());
  return SQLM_OK;
}

int sqlm_get_edge_chi2(sqlm_ctx *c, double *chi2) {
  if (!c || !c->has_problem) return SQLM_ERR_STATE;
  if (!chi2 && c->n_obs) return SQLM_ERR_INVALID_ARG;
  if (hipSetDevice(c->device) != hipSuccess) return SQLM_ERR_HIP;
  if (int s = fetch_errors(c)) return s;
  ensure_host_errors(c);
  for (int64_t e = 0; e < c->n_obs; ++e) chi2[e] = edge_chi2(c, e);
  return SQLM_OK;
}

int sqlm_get_lidar_error(sqlm_ctx *c, double *err) {
  if (!c || !err) return SQLM_ERR_INVALID_ARG;
  if (!c->has_problem || !c->opt_done) return SQLM_ERR_STATE;
  if (hipSetDevice(c->device) != hipSuccess) return SQLM_ERR_HIP;
  if (int s = fetch_errors(c)) return s;
  if (c->n_lid) std::memcpy(err, c->lid_err.data(), (size_t)c->n_lid * sizeof(double));
  return SQLM_OK;
}

int sqlm_get_edge_depth_positive(sqlm_ctx *c, uint8_t *pos) {
  if (!c || !c->has_problem) return SQLM_ERR_STATE;
  if (!pos && c->n_obs) return SQLM_ERR_INVALID_ARG;
  std::vector<uint8_t> dp;
  depth_positive_host(c, dp);
  if (c->n_obs) std::memcpy(pos, dp.data(), c->n_obs);
  return SQLM_OK;
}

int sqlm_get_rcs_layout(sqlm_ctx *c, int out[8]) {
  if (!c || !out) return SQLM_ERR_INVALID_ARG;
  if (!c->has_problem || !c->prepared) return SQLM_ERR_STATE;
  const CRPlan &pl = c->plan.cr;
  const int nP = c->d.nP;
  out[0] = nP == 0 ? 0 : !pl.enabled ? 3 : pl.R ? 2 : 1;
  out[1] = pl.B;
  out[2] = pl.p;
  out[3] = pl.n;
  out[4] = pl.nbc;
  out[5] = pl.R;
  out[6] = nP;
  out[7] = pl.init_cnt;
  return SQLM_OK;
}

int sqlm_get_exec_info(sqlm_ctx *c, int out[8]) {
  if (!c || !out) return SQLM_ERR_INVALID_ARG;
  if (!c->has_problem || !c->prepared) return SQLM_ERR_STATE;
  const CRPlan &pl = c->plan.cr;
  for (int k = 0; k < 8; ++k) out[k] = 0;
  out[0] = c->d.obs_f32 ? 1 : 0;
  out[1] = c->d.nP == 0 ? 0 : !pl.enabled ? 4 : pl.R ? 3 : 1;
  const DevProblem &d = c->d;
  out[2] = d.nP == 0 ? kTileKernelNone : !c->use_tiles ? kTileKernelRows : rcs_tile_kernel(d);
  if (c->use_tiles && d.n_tiles > 0)
    for (int nt = 0; nt <= kTileNtMax; ++nt)
      if (d.tile_cls_cnt[nt] > 0) out[3] |= 1 << nt;
  out[4] = d.n_long_s;
  out[5] = d.n_long_g;
  out[6] = d.tile_dups;
  out[7] = d.tile_maxk;
  return SQLM_OK;
}

int sqlm_get_last_step(sqlm_ctx *c, double *g, double *dx) {
  if (!c || !g || !dx) return SQLM_ERR_INVALID_ARG;
  if (!c->has_problem || !c->prepared || !c->step_valid) return SQLM_ERR_STATE;
  const size_t n = 6 * (size_t)c->d.nP;
  if (n == 0) return SQLM_OK;
  if (hipSetDevice(c->device) != hipSuccess) return SQLM_ERR_HIP;
  // g: rcs_put_g / k_rcs; dx: the dense solve's copy, or on a CR layout the
  // pose update's copy of the CR / border solution. Nothing after the trial
  // (speculative camera pass, finish) writes either.
  // Sharded: rank 0's g is k_gather_add's sum over the ranks (the last writer
  // of d.g; the solves only read it), a rank >= 1's g its own share as it was
  // sent (rows outside the rank's range keep what rcs_put_g / k_rcs put there).
  // dx is the solves' copy on rank 0 (the CR solve gathers into d.dx there:
  // the pose update does not read the CR solution on a sharded run) and the
  // broadcast's elsewhere; the flag rides in slot 6 nP, past what is copied.
  SQLM_HIP_OK(hipMemcpyAsync(g, c->d.g, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  SQLM_HIP_OK(hipMemcpyAsync(dx, c->d.dx, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  SQLM_HIP_OK(hipStreamSynchronize(c->stream));
  return SQLM_OK;
}

int sqlm_get_edge_level(sqlm_ctx *c, uint8_t *level) {
  if (!c || !c->has_problem) return SQLM_ERR_STATE;
  if (!level && c->n_obs) return SQLM_ERR_INVALID_ARG;
  if (c->n_obs) std::memcpy(level, c->obs_level.data(), c->n_obs);
  return SQLM_OK;
}

void sqlm_pose_from_Tcw_f32(const float T[16], double q[4], double t[3]) {
  double R[9];
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 3; ++k) R[r * 3 + k] = (double)T[r * 4 + k];
  q_from_mat(R, q);
  q_normalize_rot(q);
  for (int r = 0; r < 3; ++r) t[r] = (double)T[r * 4 + 3];
}

void sqlm_pose_to_Tcw_f32(const double q[4], const double t[3], float T[16]) {
  double R[9];
  q_to_mat(q, R);
  for (int r = 0; r < 3; ++r) {
    for (int k = 0; k < 3; ++k) T[r * 4 + k] = (float)R[r * 3 + k];
    T[r * 4 + 3] = (float)t[r];
  }
  T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
}

int sqlm_ctx_set_host_comm(sqlm_ctx *c, int rank, int nranks, sqlm_allreduce_fn fn, void *user) {
  if (!c || nranks < 1 || rank < 0 || rank >= nranks || (nranks > 1 && !fn)) return SQLM_ERR_INVALID_ARG;
  return comm_init_host(c->comm, rank, nranks, fn, user);
}

int sqlm_ctx_set_host_p2p(sqlm_ctx *c, sqlm_p2p_fn fn, void *user) {
  if (!c || !fn) return SQLM_ERR_INVALID_ARG;
  c->comm.host_p2p = fn;
  c->comm.host_p2p_user = user;
  return SQLM_OK;
}

int sqlm_comm_id_size(void) { return comm_id_size(); }
int sqlm_comm_get_unique_id(char *id) { return comm_get_unique_id(id); }
int sqlm_ctx_set_comm(sqlm_ctx *c, const char *id, int rank, int nranks) {
  if (!c || !id || rank < 0 || nranks < 1 || rank >= nranks) return SQLM_ERR_INVALID_ARG;
  if (hipSetDevice(c->device) != hipSuccess) return SQLM_ERR_HIP;
  return comm_init(c->comm, id, rank, nranks);
}

int sqlm_ctx_comm_info(const sqlm_ctx *c, int *transport, int *rank, int *nranks) {
  if (!c || !transport || !rank || !nranks) return SQLM_ERR_INVALID_ARG;
  return comm_info(c->comm, transport, rank, nranks);
}

int sqlm_ctx_set_comm_selfloop(sqlm_ctx *c, const char *id) {
  if (!c || !id) return SQLM_ERR_INVALID_ARG;
  if (hipSetDevice(c->device) != hipSuccess) return SQLM_ERR_HIP;
  return comm_init_selfloop(c->comm, id) ? SQLM_ERR_COMM : SQLM_OK;
}

int sqlm_comm_selftest(int device, const char *id, int64_t n, double *max_err) {
  if (!id || n <= 0 || !max_err) return SQLM_ERR_INVALID_ARG;
  if (hipSetDevice(device) != hipSuccess) return SQLM_ERR_HIP;
  Comm cm;
  if (comm_init_selfloop(cm, id)) return SQLM_ERR_COMM;
  hipStream_t st = nullptr;
  double *a = nullptr, *b = nullptr;
  int32_t *ia = nullptr;
  uint8_t *ua = nullptr;
  int r = SQLM_OK;
  std::vector<double> ha(n), hb(n);
  std::vector<int32_t> hi(n);
  std::vector<uint8_t> hu(n);
  for (int64_t i = 0; i < n; ++i) {
    ha[i] = 0.5 * (double)i - 3.25;
    hi[i] = (int32_t)(7 * i - 11);
    hu[i] = (uint8_t)(i * 13);
  }
  double err = 0.0;
  auto upd = [&](double v) { err = std::max(err, std::fabs(v)); };
  if (hipStreamCreate(&st) != hipSuccess || hipMalloc(&a, n * 8) != hipSuccess || hipMalloc(&b, n * 8) != hipSuccess ||
      hipMalloc(&ia, n * 4) != hipSuccess || hipMalloc(&ua, n) != hipSuccess) {
    r = SQLM_ERR_HIP;
  } else if (hipMemcpyAsync(a, ha.data(), n * 8, hipMemcpyHostToDevice, st) != hipSuccess ||
             hipMemsetAsync(b, 0, n * 8, st) != hipSuccess ||
             hipMemcpyAsync(ia, hi.data(), n * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
             hipMemcpyAsync(ua, hu.data(), n, hipMemcpyHostToDevice, st) != hipSuccess) {
    r = SQLM_ERR_HIP;
  } else {
    // grouped send to self + receive from self (the rank-0 gather's RCCL group)
    std::vector<P2POp> ops{P2POp{0, true, a, n, SQLM_DT_F64}, P2POp{0, false, b, n, SQLM_DT_F64}};
    if (comm_group_p2p(cm, ops, st)) r = SQLM_ERR_COMM;
    if (!r && comm_bcast_dev(cm, b, n, SQLM_DT_F64, 0, st)) r = SQLM_ERR_COMM;
    if (!r && comm_allreduce_dev(cm, a, n, SQLM_DT_F64, SQLM_OP_SUM, st)) r = SQLM_ERR_COMM;
    if (!r && comm_allreduce_dev(cm, a, n, SQLM_DT_F64, SQLM_OP_MAX, st)) r = SQLM_ERR_COMM;
    if (!r && comm_allreduce_dev(cm, ia, n, SQLM_DT_I32, SQLM_OP_SUM, st)) r = SQLM_ERR_COMM;
    if (!r && comm_allreduce_dev(cm, ua, n, SQLM_DT_U8, SQLM_OP_MAX, st)) r = SQLM_ERR_COMM;
    double hs = 2.5;  // host-buffer all-reduce (setup-time exchanges)
    if (!r && comm_allreduce_host(cm, &hs, 1, SQLM_DT_F64, SQLM_OP_SUM, st)) r = SQLM_ERR_COMM;
    if (!r) upd(hs - 2.5);
    std::vector<double> ra(n), rb(n);
    std::vector<int32_t> ri(n);
    std::vector<uint8_t> ru(n);
    if (!r && (hipMemcpyAsync(ra.data(), a, n * 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
               hipMemcpyAsync(rb.data(), b, n * 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
               hipMemcpyAsync(ri.data(), ia, n * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
               hipMemcpyAsync(ru.data(), ua, n, hipMemcpyDeviceToHost, st) != hipSuccess ||
               hipStreamSynchronize(st) != hipSuccess))
      r = SQLM_ERR_HIP;
    if (!r)
      for (int64_t i = 0; i < n; ++i) {
        upd(ra[i] - ha[i]);
        upd(rb[i] - ha[i]);
        upd((double)(ri[i] - hi[i]));
        upd((double)ru[i] - (double)hu[i]);
      }
  }
  if (st) (void)hipStreamSynchronize(st);
  (void)hipFree(a);
  (void)hipFree(b);
  (void)hipFree(ia);
  (void)hipFree(ua);
  if (st) (void)hipStreamDestroy(st);
  comm_destroy(cm);
  *max_err = err;
  return r;
}

int sqlm_bench_iterations(sqlm_ctx *c, int warmup, int n, double *ms_per_iter, double *kernel_ms, sqlm_stats *st) {
  if (!c || !c->has_problem || n <= 0 || warmup < 0) return SQLM_ERR_INVALID_ARG;
  if (hipSetDevice(c->device) != hipSuccess) return SQLM_ERR_HIP;
  // warmup from the initial state, then reset and time n iterations
  const auto q0 = c->pose_q, t0 = c->pose_t, p0 = c->pt;
  int s = prepare(c, 0);
  if (s) return s;
  if (warmup > 0) {
    s = run_lm(c, warmup, 0.0, nullptr, nullptr, nullptr, true);
    if (s) return s;
    c->pose_q = q0; c->pose_t = t0; c->pt = p0;
    s = prepare(c, 0);
    if (s) return s;
  }
  SQLM_HIP_OK(hipStreamSynchronize(c->stream));
  s = comm_barrier(c->comm, c->stream);
  if (s) return s;
  c->timing = kernel_ms != nullptr;
  std::fill(c->kernel_ms_acc, c->kernel_ms_acc + SQLM_NKERNEL_TIMERS, 0.0);
  c->kernel_ms_n = 0;
  Timer t;
  s = run_lm(c, n, 0.0, nullptr, st, nullptr, true);
  SQLM_HIP_OK(hipStreamSynchronize(c->stream));
  const double ms = t.ms();
  c->timing = false;
  if (s) return s;
  if (ms_per_iter) *ms_per_iter = ms / n;
  if (kernel_ms) {
    for (int i = 0; i < SQLM_NKERNEL_TIMERS; ++i)
      kernel_ms[i] = c->kernel_ms_n ? c->kernel_ms_acc[i] / c->kernel_ms_n : 0.0;
  }
  return finish(c);
}

#ifdef SQLM_TILE_PROF
// Diagnostic build only: 64 tiles x 8 phase cycle sums of k_rcs_tile.
int sqlm_debug_tile_profile(long long *out) { return sqlm::tile_profile_read(out); }
#endif

int sqlm_debug_cr_levels(int out[3]) {
  if (!out) return SQLM_ERR_INVALID_ARG;
  sqlm::cr_last_levels(out);
  return SQLM_OK;
}

const char *sqlm_kernel_timer_name(int i) {
  return (i >= 0 && i < SQLM_NKERNEL_TIMERS) ? kTimerNames[i] : "";
}

// ---- ORB front end (include/sqrtlm_orb.h) ----
static int orb_engine(sqlm_ctx *c) {
  if (!c) return SQLM_ERR_INVALID_ARG;
  if (hipSetDevice(c->device) != hipSuccess) return SQLM_ERR_HIP;
  if (!c->orb && !(c->orb = orb_create(c->stream))) return SQLM_ERR_OOM;
  return SQLM_OK;
}

int sqlm_orb_extract(sqlm_ctx *c, const sqlm_orb_params *p, const uint8_t *image, int w, int h, int stride,
                     sqlm_keypoint *kps, uint8_t *desc, int cap, int *n_out) {
  if (int r = orb_engine(c)) return r;
  return orb_extract(c->orb, p, image, w, h, stride, kps, desc, cap, n_out);
}

int sqlm_orb_get_level(sqlm_ctx *c, int level, uint8_t *out, int cap, int *lw, int *lh) {
  if (!c || !c->orb) return SQLM_ERR_STATE;
  if (hipSetDevice(c->device) != hipSuccess) return SQLM_ERR_HIP;
  return orb_get_level(c->orb, level, out, cap, lw, lh);
}

int sqlm_orb_match_bf(sqlm_ctx *c, const uint8_t *query, int nq, const uint8_t *train, int nt, int32_t *best_idx,
                      int32_t *best_dist, int32_t *second_dist) {
  if (int r = orb_engine(c)) return r;
  return orb_match_bf(c->orb, query, nq, train, nt, best_idx, best_dist, second_dist);
}

int sqlm_orb_search_for_init(sqlm_ctx *c, const sqlm_keypoint *k1, const uint8_t *d1, int n1, const sqlm_keypoint *k2,
                             const uint8_t *d2, int n2, const sqlm_frame_bounds *f2, float *prev, int32_t *m12,
                             int window, float nnratio, int check_ori, int *n_matches) {
  if (int r = orb_engine(c)) return r;
  return orb_search_for_init(c->orb, k1, d1, n1, k2, d2, n2, f2, prev, m12, window, nnratio, check_ori, n_matches);
}

int sqlm_orb_search_by_projection_local(sqlm_ctx *c, sqlm_orb_frame *F, const sqlm_track_point *mps,
                                        const uint8_t *mp_desc, int n_mp, float th, float nnratio, int *n_matches) {
  if (int r = orb_engine(c)) return r;
  return orb_search_by_projection_local(c->orb, F, mps, mp_desc, n_mp, th, nnratio, n_matches);
}

int sqlm_orb_search_by_projection_last(sqlm_ctx *c, sqlm_orb_frame *F, const float *Tcw, const float *Tlw,
                                       const sqlm_last_point *lp, const uint8_t *ldesc, int n_last, float th,
                                       int mono, int check_ori, int *n_matches) {
  if (int r = orb_engine(c)) return r;
  return orb_search_by_projection_last(c->orb, F, Tcw, Tlw, lp, ldesc, n_last, th, mono, check_ori, n_matches);
}

int sqlm_orb_search_by_projection_sim3(sqlm_ctx *c, sqlm_orb_frame *F, const float *Scw, const sqlm_map_point *mps,
                                       const uint8_t *mp_desc, int n, int th, int *n_matches) {
  if (int r = orb_engine(c)) return r;
  return orb_search_by_projection_sim3(c->orb, F, Scw, mps, mp_desc, n, th, n_matches);
}

int sqlm_orb_fuse(sqlm_ctx *c, const sqlm_orb_frame *F, const float *T, int sim3, const sqlm_map_point *mps,
                  const uint8_t *mp_desc, int n, float th, int32_t *fuse_idx, int *n_fused) {
  if (int r = orb_engine(c)) return r;
  return orb_fuse(c->orb, F, T, sim3, mps, mp_desc, n, th, fuse_idx, n_fused);
}

int sqlm_orb_search_by_projection_kf(sqlm_ctx *c, sqlm_orb_frame *F, const float *Tcw, const sqlm_map_point *mps,
                                     const uint8_t *mp_desc, const float *kf_angle, int n, float th, int orb_dist,
                                     int check_ori, int *n_matches) {
  if (int r = orb_engine(c)) return r;
  return orb_search_by_projection_kf(c->orb, F, Tcw, mps, mp_desc, kf_angle, n, th, orb_dist, check_ori, n_matches);
}

int sqlm_orb_search_by_sim3(sqlm_ctx *c, const sqlm_orb_frame *K1, const sqlm_orb_frame *K2, const float *T1w,
                            const float *T2w, const sqlm_map_point *mp1, const uint8_t *md1, const sqlm_map_point *mp2,
                            const uint8_t *md2, float s12, const float *R12, const float *t12, float th,
                            int32_t *matches12, int *n_found) {
  if (int r = orb_engine(c)) return r;
  return orb_search_by_sim3(c->orb, K1, K2, T1w, T2w, mp1, md1, mp2, md2, s12, R12, t12, th, matches12, n_found);
}

int sqlm_orb_search_by_bow_kf_frame(sqlm_ctx *c, const sqlm_bow_frame *KF, const sqlm_bow_frame *F, float nnratio,
                                    int check_ori, int32_t *matches, int *n_matches) {
  if (int r = orb_engine(c)) return r;
  return orb_search_by_bow_kf_frame(c->orb, KF, F, nnratio, check_ori, matches, n_matches);
}

int sqlm_orb_search_by_bow_kf_kf(sqlm_ctx *c, const sqlm_bow_frame *K1, const sqlm_bow_frame *K2, float nnratio,
                                 int check_ori, int32_t *matches12, int *n_matches) {
  if (int r = orb_engine(c)) return r;
  return orb_search_by_bow_kf_kf(c->orb, K1, K2, nnratio, check_ori, matches12, n_matches);
}

int sqlm_orb_search_for_triangulation(sqlm_ctx *c, const sqlm_bow_frame *K1, const sqlm_bow_frame *K2,
                                      const float *C1, const float *T2w, const float *cam2,
                                      const float *scale_factors2, int n_levels2, const float *F12, int only_stereo,
                                      int check_ori, int32_t *m12, int *n_matches) {
  if (int r = orb_engine(c)) return r;
  return orb_search_for_triangulation(c->orb, K1, K2, C1, T2w, cam2, scale_factors2, n_levels2, F12, only_stereo,
                                      check_ori, m12, n_matches);
}

int sqlm_orb_bench_extract(sqlm_ctx *c, const sqlm_orb_params *p, const uint8_t *image, int w, int h, int stride,
                           int reps, double *ms_per_frame, double *stage_ms) {
  if (int r = orb_engine(c)) return r;
  return orb_bench_extract(c->orb, p, image, w, h, stride, reps, ms_per_frame, stage_ms);
}

}  // extern "C"
