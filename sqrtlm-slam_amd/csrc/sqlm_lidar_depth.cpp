// sqlm_lidar_depth.cpp — host side of sqlm_lidar_depth: argument and limit
// checks before the device is touched, one staged upload, the launches
// (sqlm_lidar_depth.hip), the read-back of the packed outputs and, when the
// caller asks for it, of the depth image; the read-back of the intermediate
// state for tests; and sqlm_lidar_depth_host, the host twin: the reference's
// loops run sequentially over the same text (lidar_depth_dev.h) compiled for
// the CPU. Built with -ffp-contract=off like the kernels.
#include <algorithm>
#include <cstring>
#include <limits>
#include <new>
#include <vector>

#include "lidar_depth_dev.h"
#include "sqlm_ctx.h"
#include "sqlm_staging.h"

#pragma clang fp contract(off)

namespace sqlm {

struct LidarDepthSolver {
  Staged in, work, out;
  LdDev d;              // the last call's device pointers
  bool have = false;    // a call has completed
  int32_t launches = 0;
};

void lidar_depth_destroy(LidarDepthSolver *s) { delete s; }

namespace {

int ld_solver(sqlm_ctx *c) {
  if (hipSetDevice(c->device) != hipSuccess) return SQLM_ERR_HIP;
  if (!c->lidar_depth && !(c->lidar_depth = new (std::nothrow) LidarDepthSolver)) return SQLM_ERR_OOM;
  return SQLM_OK;
}

int32_t ld_sat(int64_t v) { return (int32_t)std::min<int64_t>(v, std::numeric_limits<int32_t>::max()); }

}  // namespace

}  // namespace sqlm

using namespace sqlm;

extern "C" {

int sqlm_lidar_depth_host(int n_frame, const int64_t *sweep_off, const float *xyz, const int64_t *key_off,
                          const float *key_xy, const float *key_un_xy, int rows, int cols, const double *intrinsic,
                          const double *extrinsic, const float *cam, int32_t *class_id, float *depth,
                          int32_t *nearest_uv, float *xyz_cam, int32_t *stats, double *depth_image, int32_t *pixel,
                          int32_t *winner) {
  LdCfg cfg;
  if (int r = ld_check(n_frame, sweep_off, xyz, key_off, key_xy, key_un_xy, rows, cols, intrinsic, extrinsic, cam,
                       class_id, depth, nearest_uv, xyz_cam, stats, &cfg))
    return r;
  const size_t per = (size_t)rows * cols;
  std::vector<int32_t> win;
  std::vector<double> img;
  try {
    if (!winner) win.resize(per);
    if (!depth_image) img.resize(per);
  } catch (const std::bad_alloc &) {
    return SQLM_ERR_OOM;
  }
  for (int f = 0; f < n_frame; ++f) {
    const int64_t o = sweep_off[f], k = key_off[f];
    ld_host_frame(cfg, (int32_t)(sweep_off[f + 1] - o), xyz + 3 * o, key_off[f + 1] - k, key_xy + 2 * k,
                  cfg.has_un ? key_un_xy + 2 * k : nullptr, class_id + k, depth + k, nearest_uv + 2 * k,
                  cfg.has_un ? xyz_cam + 3 * k : nullptr, stats + 4 * f, pixel ? pixel + o : nullptr,
                  winner ? winner + f * per : win.data(), depth_image ? depth_image + f * per : img.data());
  }
  return SQLM_OK;
}

int sqlm_lidar_depth(sqlm_ctx *c, int n_frame, const int64_t *sweep_off, const float *xyz, const int64_t *key_off,
                     const float *key_xy, const float *key_un_xy, int rows, int cols, const double *intrinsic,
                     const double *extrinsic, const float *cam, int32_t *class_id, float *depth, int32_t *nearest_uv,
                     float *xyz_cam, int32_t *stats, double *depth_image) {
  if (!c) return SQLM_ERR_INVALID_ARG;
  LdCfg cfg;
  if (int r = ld_check(n_frame, sweep_off, xyz, key_off, key_xy, key_un_xy, rows, cols, intrinsic, extrinsic, cam,
                       class_id, depth, nearest_uv, xyz_cam, stats, &cfg))
    return r;
  if (int r = ld_solver(c)) return r;
  LidarDepthSolver *s = c->lidar_depth;
  s->have = false;
  s->launches = 0;
  const int64_t n = sweep_off[n_frame], m = key_off[n_frame];
  const size_t np = (size_t)n, nk = (size_t)m, nf = (size_t)n_frame, cells = nf * rows * cols;
  LdDev &d = s->d;
  d = LdDev();
  d.c = cfg;
  d.n_frame = n_frame;
  d.n = n;
  d.m = m;
  d.cells = (int64_t)cells;
  if (n == 0 && m == 0) {  // nothing reaches the device: every image is zeros
    if (nf) std::memset(stats, 0, nf * 4 * sizeof(int32_t));
    if (depth_image && cells) std::memset(depth_image, 0, cells * sizeof(double));
    s->have = true;
    return SQLM_OK;
  }
  Arena in, work, out;
  const size_t i_soff = in.take((nf + 1) * 8), i_koff = in.take((nf + 1) * 8), i_xyz = in.take(np * 12),
               i_key = in.take(nk * 8), i_un = in.take(cfg.has_un ? nk * 8 : 0);
  const size_t w_winner = work.take(cells * 4);  // zeroed
  const size_t w_zero = work.off;
  const size_t w_pixel = work.take(np * 4), w_image = work.take(cells * 8);
  const size_t o_stats = out.take(nf * 16);  // zeroed
  const size_t o_zero = out.off;
  const size_t o_cls = out.take(nk * 4), o_depth = out.take(nk * 4), o_uv = out.take(nk * 8),
               o_cam = out.take(cfg.has_un ? nk * 12 : 0);
  if (int r = s->in.grow(in.off)) return r;
  if (int r = s->work.grow(work.off, false)) return r;
  if (int r = s->out.grow(out.off)) return r;
  char *ih = s->in.host;
  std::memcpy(ih + i_soff, sweep_off, (nf + 1) * 8);
  std::memcpy(ih + i_koff, key_off, (nf + 1) * 8);
  if (np) std::memcpy(ih + i_xyz, xyz, np * 12);
  if (nk) std::memcpy(ih + i_key, key_xy, nk * 8);
  if (nk && cfg.has_un) std::memcpy(ih + i_un, key_un_xy, nk * 8);
  SQLM_HIP_OK(hipMemcpyAsync(s->in.dev, s->in.host, in.off, hipMemcpyHostToDevice, c->stream));
  SQLM_HIP_OK(hipMemsetAsync(s->work.dev, 0, w_zero, c->stream));
  SQLM_HIP_OK(hipMemsetAsync(s->out.dev, 0, o_zero, c->stream));
  char *wd = s->work.dev, *od = s->out.dev, *id = s->in.dev;
  d.sweep_off = at<const int64_t>(id, i_soff);
  d.key_off = at<const int64_t>(id, i_koff);
  d.xyz = at<const float>(id, i_xyz);
  d.key_xy = at<const float>(id, i_key);
  d.key_un_xy = at<const float>(id, i_un);
  d.winner = at<int32_t>(wd, w_winner);
  d.pixel = at<int32_t>(wd, w_pixel);
  d.image = at<double>(wd, w_image);
  d.stats = at<int32_t>(od, o_stats);
  d.class_id = at<int32_t>(od, o_cls);
  d.depth = at<float>(od, o_depth);
  d.nearest_uv = at<int32_t>(od, o_uv);
  d.xyz_cam = at<float>(od, o_cam);
  s->launches = launch_lidar_depth(d, c->stream);
  SQLM_HIP_OK(hipGetLastError());
  SQLM_HIP_OK(hipMemcpyAsync(s->out.host, s->out.dev, out.off, hipMemcpyDeviceToHost, c->stream));
  if (depth_image)
    SQLM_HIP_OK(hipMemcpyAsync(depth_image, d.image, cells * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  SQLM_HIP_OK(hipStreamSynchronize(c->stream));
  const char *oh = s->out.host;
  const int32_t *st = reinterpret_cast<const int32_t *>(oh + o_stats);
  for (size_t f = 0; f < nf; ++f) {
    const int32_t s0 = st[4 * f];
    if (s0 < 0 || s0 > rows) return SQLM_ERR_HIP;  // never: the key is rows - v of a row of the image
    stats[4 * f] = s0 ? rows - s0 : 0;
    stats[4 * f + 1] = st[4 * f + 1];
    stats[4 * f + 2] = st[4 * f + 2];
    stats[4 * f + 3] = st[4 * f + 3];
  }
  if (nk) {
    std::memcpy(class_id, oh + o_cls, nk * 4);
    std::memcpy(depth, oh + o_depth, nk * 4);
    std::memcpy(nearest_uv, oh + o_uv, nk * 8);
    if (cfg.has_un) std::memcpy(xyz_cam, oh + o_cam, nk * 12);
  }
  s->have = true;
  return SQLM_OK;
}

int sqlm_lidar_depth_get_state(sqlm_ctx *c, int32_t *pixel, int32_t *winner, double *depth_image) {
  if (!c) return SQLM_ERR_INVALID_ARG;
  LidarDepthSolver *s = c->lidar_depth;
  if (!s || !s->have) return SQLM_ERR_STATE;
  const LdDev &d = s->d;
  const size_t cells = (size_t)d.cells, np = (size_t)d.n;
  if (s->launches == 0) {  // the last call reached no device: no point, every pixel unwritten
    if (winner && cells) std::memset(winner, 0, cells * 4);
    if (depth_image && cells) std::memset(depth_image, 0, cells * 8);
    return SQLM_OK;
  }
  if (hipSetDevice(c->device) != hipSuccess) return SQLM_ERR_HIP;
  SQLM_HIP_OK(hipStreamSynchronize(c->stream));
  if (pixel && np) SQLM_HIP_OK(hipMemcpy(pixel, d.pixel, np * 4, hipMemcpyDeviceToHost));
  if (winner && cells) SQLM_HIP_OK(hipMemcpy(winner, d.winner, cells * 4, hipMemcpyDeviceToHost));
  if (depth_image && cells) SQLM_HIP_OK(hipMemcpy(depth_image, d.image, cells * 8, hipMemcpyDeviceToHost));
  return SQLM_OK;
}

int sqlm_lidar_depth_info(const sqlm_ctx *c, int32_t out[8]) {
  if (!out) return SQLM_ERR_INVALID_ARG;
  const LidarDepthSolver *s = c ? c->lidar_depth : nullptr;
  out[0] = SQLM_LD_MAX_DIM;
  out[1] = SQLM_LD_MAX_CELLS;
  out[2] = s ? s->launches : 0;
  out[3] = SQLM_LD_HALF_W;
  out[4] = SQLM_LD_HALF_H;
  out[5] = kLdLanes;
  out[6] = s && s->have ? ld_sat(s->d.n) : 0;
  out[7] = s && s->have ? ld_sat(s->d.m) : 0;
  return SQLM_OK;
}

}  // extern "C"
