// sqlm_lidar_feat.cpp — host side of sqlm_lidar_features and of
// sqlm_lidar_features_all (the flat branch and the corner branch on one range
// image; corner kernels: sqlm_lidar_corner.hip): argument and limit
// checks before the device is touched, one staged upload, the launches
// (sqlm_lidar_feat.hip), the read-back of the packed outputs; the read-back of
// the intermediate state for tests; and sqlm_lidar_features_host, the host
// twin: the reference's loops run sequentially over the same text
// (lidar_feat_dev.h, lidar_corner_dev.h) compiled for the CPU. Built with
// -ffp-contract=off like the kernels.
#include <algorithm>
#include <cstring>
#include <limits>
#include <new>
#include <vector>

#include "lidar_feat_host.h"
#include "sqlm_ctx.h"
#include "sqlm_staging.h"

#pragma clang fp contract(off)

namespace sqlm {

struct LidarFeatSolver {
  Staged in, work, out;
  LfDev d;              // the last call's device pointers
  bool have = false;    // a call has completed
  int32_t launches = 0, stats[4] = {0, 0, 0, 0};
  LcDev lc;                  // the corner stage of the last sqlm_lidar_features_all
  bool have_corner = false;  // that call ran one
  int32_t cstats[5] = {0, 0, 0, 0, 0};
  int64_t n_less_sharp = 0, n_sharp = 0;
};

void lidar_feat_destroy(LidarFeatSolver *s) { delete s; }

namespace {

int lf_solver(sqlm_ctx *c) {
  if (hipSetDevice(c->device) != hipSuccess) return SQLM_ERR_HIP;
  if (!c->lidar_feat && !(c->lidar_feat = new (std::nothrow) LidarFeatSolver)) return SQLM_ERR_OOM;
  return SQLM_OK;
}

// The device side of both branches: `p` has passed lf_check (and `lc`, when
// not null, lc_check); do_flat = the flat outputs exist.
int lf_run(sqlm_ctx *c, int n_sweep, const int64_t *sweep_off, const float *xyz, const LfParams &p,
           const double *extrinsic, bool do_flat, int64_t *flat_off, float *flat_xyz, float *flat_normal,
           int64_t *less_off, float *less_xyz, float *less_normal, int32_t *less_row_col, const LcParams *lc,
           const LcOut &co) {
  if (int r = lf_solver(c)) return r;
  LidarFeatSolver *s = c->lidar_feat;
  s->have = false;
  s->have_corner = false;
  s->launches = 0;
  s->n_less_sharp = s->n_sharp = 0;
  std::memset(s->stats, 0, sizeof(s->stats));
  std::memset(s->cstats, 0, sizeof(s->cstats));
  const int64_t n = sweep_off[n_sweep];
  const size_t np = (size_t)n, ns = (size_t)n_sweep, n_rows = ns * p.row_num, cells = n_rows * p.col_num,
               regions = n_rows * p.n_sub;
  LfDev &d = s->d;
  d = LfDev();
  d.p = p;
  d.n_sweep = n_sweep;
  d.n_rows = (int32_t)n_rows;
  d.n = n;
  s->lc = LcDev();
  if (n == 0) {
    for (int k = 0; k <= n_sweep; ++k) {
      if (do_flat) flat_off[k] = less_off[k] = 0;
      if (lc) co.sharp_off[k] = co.less_off[k] = 0;
    }
    s->lc.f = d;
    if (lc) s->lc.p = *lc;
    s->have = true;
    s->have_corner = lc != nullptr;
    return SQLM_OK;
  }
  d.has_ext = extrinsic ? 1 : 0;
  if (extrinsic) std::memcpy(d.ext, extrinsic, sizeof(d.ext));
  Arena in, ones, zeros, out;
  const size_t i_off = in.take((ns + 1) * sizeof(int64_t)), i_xyz = in.take(3 * np * sizeof(float));
  // work, first part: set to all ones (no index / unoccupied / -1)
  const size_t w_first = ones.take(ns * 4), w_half = ones.take(ns * 4), w_last = ones.take(ns * 4),
               w_key = ones.take(cells * 8), w_cfirst = ones.take(cells * 4), w_image = ones.take(cells * 4),
               w_sorted = ones.take(cells * 4);
  // second part: zeroed
  const size_t z_ring = zeros.take(np * 4), z_azi = zeros.take(np * 4), z_scan_n = zeros.take(n_rows * 4),
               z_src = zeros.take(cells * 4), z_col = zeros.take(cells * 4), z_xyz = zeros.take(cells * 12),
               z_curv = zeros.take(cells * 4), z_normal = zeros.take(cells * 12), z_mask = zeros.take(cells),
               z_reason = zeros.take(cells), z_nbr = zeros.take(cells * 4), z_ord = zeros.take(cells * 4),
               z_cnt = zeros.take(regions * 4), z_rl = zeros.take(regions * 8), z_rf = zeros.take(regions * 8);
  // the corner stage's work: its sorted order in the first part, the rest zeroed
  size_t c_sorted = 0, c_state = 0, c_edge = 0, c_mask = 0, c_reason = 0, c_curv = 0, c_cand = 0, c_cand_n = 0,
         c_queue = 0, c_ord = 0, c_label = 0, c_cnt = 0, c_rl = 0, c_rs = 0;
  if (lc) {
    c_sorted = ones.take(cells * 4);
    c_state = zeros.take(cells * 4);
    c_edge = zeros.take(cells);
    c_mask = zeros.take(cells);
    c_reason = zeros.take(cells);
    c_curv = zeros.take(cells * 4);
    c_cand = zeros.take(cells * 4);
    c_cand_n = zeros.take(regions * 4);
    c_queue = zeros.take(cells * 4);
    c_ord = zeros.take(cells * 4);
    c_label = zeros.take(cells * 4);
    c_cnt = zeros.take(regions * 4);
    c_rl = zeros.take(regions * 8);
    c_rs = zeros.take(regions * 8);
  }
  // out: the small part first, read back before the clouds
  const size_t o_foff = out.take((ns + 1) * 8), o_loff = out.take((ns + 1) * 8), o_stats = out.take(16);
  size_t o_csoff = 0, o_cloff = 0, o_cstats = 0;
  if (lc) {
    o_csoff = out.take((ns + 1) * 8);
    o_cloff = out.take((ns + 1) * 8);
    o_cstats = out.take(sizeof(s->cstats));
  }
  const size_t o_small = out.off;
  const size_t o_fx = out.take(np * 12), o_fn = out.take(np * 12), o_lx = out.take(np * 12), o_ln = out.take(np * 12),
               o_rc = out.take(np * 8);
  size_t o_csx = 0, o_clx = 0, o_clab = 0, o_crc = 0;
  if (lc) {
    o_csx = out.take(np * 12);
    o_clx = out.take(np * 12);
    o_clab = out.take(np * 4);
    o_crc = out.take(np * 8);
  }
  if (int r = s->in.grow(in.off)) return r;
  if (int r = s->work.grow(ones.off + zeros.off, false)) return r;
  if (int r = s->out.grow(out.off)) return r;
  std::memcpy(s->in.host + i_off, sweep_off, (ns + 1) * sizeof(int64_t));
  std::memcpy(s->in.host + i_xyz, xyz, 3 * np * sizeof(float));
  SQLM_HIP_OK(hipMemcpyAsync(s->in.dev, s->in.host, in.off, hipMemcpyHostToDevice, c->stream));
  SQLM_HIP_OK(hipMemsetAsync(s->work.dev, 0xff, ones.off, c->stream));
  SQLM_HIP_OK(hipMemsetAsync(s->work.dev + ones.off, 0, zeros.off, c->stream));
  SQLM_HIP_OK(hipMemsetAsync(s->out.dev, 0, o_small, c->stream));
  char *w1 = s->work.dev, *w0 = s->work.dev + ones.off, *od = s->out.dev;
  d.sweep_off = at<const int64_t>(s->in.dev, i_off);
  d.xyz = at<const float>(s->in.dev, i_xyz);
  d.sweep_first = at<uint32_t>(w1, w_first);
  d.sweep_half = at<uint32_t>(w1, w_half);
  d.sweep_last = at<int32_t>(w1, w_last);
  d.cell_key = at<unsigned long long>(w1, w_key);
  d.cell_first = at<uint32_t>(w1, w_cfirst);
  d.image_index = at<int32_t>(w1, w_image);
  d.sorted = at<int32_t>(w1, w_sorted);
  d.ring = at<int32_t>(w0, z_ring);
  d.azi = at<float>(w0, z_azi);
  d.scan_n = at<int32_t>(w0, z_scan_n);
  d.scan_src = at<int32_t>(w0, z_src);
  d.scan_col = at<int32_t>(w0, z_col);
  d.scan_xyz = at<float>(w0, z_xyz);
  d.curv = at<float>(w0, z_curv);
  d.normal = at<float>(w0, z_normal);
  d.mask = at<uint8_t>(w0, z_mask);
  d.reason = at<uint8_t>(w0, z_reason);
  d.nbr = at<int32_t>(w0, z_nbr);
  d.ord = at<int32_t>(w0, z_ord);
  d.region_cnt = at<int32_t>(w0, z_cnt);
  d.region_less = at<int64_t>(w0, z_rl);
  d.region_flat = at<int64_t>(w0, z_rf);
  d.flat_off = at<int64_t>(od, o_foff);
  d.less_off = at<int64_t>(od, o_loff);
  d.stats = at<int32_t>(od, o_stats);
  d.flat_xyz = at<float>(od, o_fx);
  d.flat_normal = at<float>(od, o_fn);
  d.less_xyz = at<float>(od, o_lx);
  d.less_normal = at<float>(od, o_ln);
  d.less_rc = at<int32_t>(od, o_rc);
  s->launches = launch_lidar_feat_image(d, c->stream);
  if (do_flat) s->launches += launch_lidar_feat_flat(d, c->stream);
  LcDev &e = s->lc;
  e.f = d;
  if (lc) {
    e.p = *lc;
    e.sorted = at<int32_t>(w1, c_sorted);
    e.state = at<int32_t>(w0, c_state);
    e.edge = at<uint8_t>(w0, c_edge);
    e.mask = at<uint8_t>(w0, c_mask);
    e.reason = at<uint8_t>(w0, c_reason);
    e.curv = at<float>(w0, c_curv);
    e.cand = at<int32_t>(w0, c_cand);
    e.cand_n = at<int32_t>(w0, c_cand_n);
    e.queue = at<int32_t>(w0, c_queue);
    e.ord = at<int32_t>(w0, c_ord);
    e.label = at<int32_t>(w0, c_label);
    e.region_cnt = at<int32_t>(w0, c_cnt);
    e.region_less = at<int64_t>(w0, c_rl);
    e.region_sharp = at<int64_t>(w0, c_rs);
    e.sharp_off = at<int64_t>(od, o_csoff);
    e.less_off = at<int64_t>(od, o_cloff);
    e.stats = at<int32_t>(od, o_cstats);
    e.sharp_xyz = at<float>(od, o_csx);
    e.less_xyz = at<float>(od, o_clx);
    e.less_label = at<int32_t>(od, o_clab);
    e.less_rc = at<int32_t>(od, o_crc);
    s->launches += launch_lidar_corner(e, c->stream);
  }
  SQLM_HIP_OK(hipGetLastError());
  SQLM_HIP_OK(hipMemcpyAsync(s->out.host, s->out.dev, o_small, hipMemcpyDeviceToHost, c->stream));
  SQLM_HIP_OK(hipStreamSynchronize(c->stream));
  char *oh = s->out.host;
  int64_t kf = 0, kl = 0, ks = 0, kc = 0;
  if (do_flat) {
    std::memcpy(flat_off, oh + o_foff, (ns + 1) * 8);
    std::memcpy(less_off, oh + o_loff, (ns + 1) * 8);
    std::memcpy(s->stats, oh + o_stats, 16);
    kf = flat_off[n_sweep];
    kl = less_off[n_sweep];
  }
  if (lc) {
    std::memcpy(co.sharp_off, oh + o_csoff, (ns + 1) * 8);
    std::memcpy(co.less_off, oh + o_cloff, (ns + 1) * 8);
    std::memcpy(s->cstats, oh + o_cstats, sizeof(s->cstats));
    ks = co.sharp_off[n_sweep];
    kc = co.less_off[n_sweep];
  }
  if (kf < 0 || kl < 0 || kf > n || kl > n) return SQLM_ERR_HIP;  // never: a scan point is picked once
  if (ks < 0 || kc < 0 || ks > n || kc > n) return SQLM_ERR_HIP;
  if (ks) SQLM_HIP_OK(hipMemcpyAsync(oh + o_csx, od + o_csx, (size_t)ks * 12, hipMemcpyDeviceToHost, c->stream));
  if (kc) {
    SQLM_HIP_OK(hipMemcpyAsync(oh + o_clx, od + o_clx, (size_t)kc * 12, hipMemcpyDeviceToHost, c->stream));
    SQLM_HIP_OK(hipMemcpyAsync(oh + o_clab, od + o_clab, (size_t)kc * 4, hipMemcpyDeviceToHost, c->stream));
    SQLM_HIP_OK(hipMemcpyAsync(oh + o_crc, od + o_crc, (size_t)kc * 8, hipMemcpyDeviceToHost, c->stream));
  }
  if (kf) {
    SQLM_HIP_OK(hipMemcpyAsync(oh + o_fx, od + o_fx, (size_t)kf * 12, hipMemcpyDeviceToHost, c->stream));
    SQLM_HIP_OK(hipMemcpyAsync(oh + o_fn, od + o_fn, (size_t)kf * 12, hipMemcpyDeviceToHost, c->stream));
  }
  if (kl) {
    SQLM_HIP_OK(hipMemcpyAsync(oh + o_lx, od + o_lx, (size_t)kl * 12, hipMemcpyDeviceToHost, c->stream));
    SQLM_HIP_OK(hipMemcpyAsync(oh + o_ln, od + o_ln, (size_t)kl * 12, hipMemcpyDeviceToHost, c->stream));
    SQLM_HIP_OK(hipMemcpyAsync(oh + o_rc, od + o_rc, (size_t)kl * 8, hipMemcpyDeviceToHost, c->stream));
  }
  SQLM_HIP_OK(hipStreamSynchronize(c->stream));
  if (kf) {
    std::memcpy(flat_xyz, oh + o_fx, (size_t)kf * 12);
    std::memcpy(flat_normal, oh + o_fn, (size_t)kf * 12);
  }
  if (kl) {
    std::memcpy(less_xyz, oh + o_lx, (size_t)kl * 12);
    std::memcpy(less_normal, oh + o_ln, (size_t)kl * 12);
    std::memcpy(less_row_col, oh + o_rc, (size_t)kl * 8);
  }
  if (ks) std::memcpy(co.sharp_xyz, oh + o_csx, (size_t)ks * 12);
  if (kc) {
    std::memcpy(co.less_xyz, oh + o_clx, (size_t)kc * 12);
    std::memcpy(co.less_label, oh + o_clab, (size_t)kc * 4);
    std::memcpy(co.less_rc, oh + o_crc, (size_t)kc * 8);
  }
  s->n_sharp = ks;
  s->n_less_sharp = kc;
  s->have = true;
  s->have_corner = lc != nullptr;
  return SQLM_OK;
}

}  // namespace

}  // namespace sqlm

using namespace sqlm;

extern "C" {

int sqlm_lidar_features_host(int n_sweep, const int64_t *sweep_off, const float *xyz,
                             const sqlm_lidar_feat_params *params, const double *extrinsic, int64_t *flat_off,
                             float *flat_xyz, float *flat_normal, int64_t *less_off, float *less_xyz,
                             float *less_normal, int32_t *less_row_col, sqlm_lidar_feat_state *state) {
  LfParams p;
  const void *outs[7] = {flat_off, less_off, flat_xyz, flat_normal, less_xyz, less_normal, less_row_col};
  if (int r = lf_check(n_sweep, sweep_off, xyz, params, outs, 7, &p)) return r;
  return lf_host(n_sweep, sweep_off, xyz, p, extrinsic, true, flat_off, flat_xyz, flat_normal, less_off, less_xyz,
                 less_normal, less_row_col, state, nullptr, LcOut(), nullptr);
}

int sqlm_lidar_features(sqlm_ctx *c, int n_sweep, const int64_t *sweep_off, const float *xyz,
                        const sqlm_lidar_feat_params *params, const double *extrinsic, int64_t *flat_off,
                        float *flat_xyz, float *flat_normal, int64_t *less_off, float *less_xyz, float *less_normal,
                        int32_t *less_row_col) {
  if (!c) return SQLM_ERR_INVALID_ARG;
  LfParams p;
  const void *outs[7] = {flat_off, less_off, flat_xyz, flat_normal, less_xyz, less_normal, less_row_col};
  if (int r = lf_check(n_sweep, sweep_off, xyz, params, outs, 7, &p)) return r;
  return lf_run(c, n_sweep, sweep_off, xyz, p, extrinsic, true, flat_off, flat_xyz, flat_normal, less_off, less_xyz,
                less_normal, less_row_col, nullptr, LcOut());
}

// The checks sqlm_lidar_features_all and its host twin share
static int lf_check_all(int n_sweep, const int64_t *sweep_off, const float *xyz, const sqlm_lidar_feat_params *params,
                        const sqlm_lidar_corner_params *corner, const void *const *fouts, const LcOut &co, LfParams *p,
                        LcParams *q, bool *do_flat) {
  *do_flat = false;
  for (int k = 0; k < 7; ++k) *do_flat = *do_flat || fouts[k];
  if (int r = lf_check(n_sweep, sweep_off, xyz, params, fouts, *do_flat ? 7 : 0, p, true)) return r;
  if (corner) {
    const void *couts[6] = {co.sharp_off, co.sharp_xyz, co.less_off, co.less_xyz, co.less_label, co.less_rc};
    if (int r = lc_check(sweep_off[n_sweep], params, corner, couts, 6, q)) return r;
  }
  return SQLM_OK;
}

int sqlm_lidar_features_all_host(int n_sweep, const int64_t *sweep_off, const float *xyz,
                                 const sqlm_lidar_feat_params *params, const sqlm_lidar_corner_params *corner,
                                 const double *extrinsic, int64_t *flat_off, float *flat_xyz, float *flat_normal,
                                 int64_t *less_off, float *less_xyz, float *less_normal, int32_t *less_row_col,
                                 int64_t *sharp_off, float *sharp_xyz, int64_t *less_sharp_off, float *less_sharp_xyz,
                                 int32_t *less_sharp_label, int32_t *less_sharp_row_col,
                                 sqlm_lidar_feat_state *flat_state, sqlm_lidar_corner_state *corner_state) {
  LfParams p;
  LcParams q;
  bool do_flat;
  const void *outs[7] = {flat_off, less_off, flat_xyz, flat_normal, less_xyz, less_normal, less_row_col};
  const LcOut co{sharp_off, less_sharp_off, sharp_xyz, less_sharp_xyz, less_sharp_label, less_sharp_row_col};
  if (int r = lf_check_all(n_sweep, sweep_off, xyz, params, corner, outs, co, &p, &q, &do_flat)) return r;
  return lf_host(n_sweep, sweep_off, xyz, p, extrinsic, do_flat, flat_off, flat_xyz, flat_normal, less_off, less_xyz,
                 less_normal, less_row_col, flat_state, corner ? &q : nullptr, co, corner ? corner_state : nullptr);
}

int sqlm_lidar_features_all(sqlm_ctx *c, int n_sweep, const int64_t *sweep_off, const float *xyz,
                            const sqlm_lidar_feat_params *params, const sqlm_lidar_corner_params *corner,
                            const double *extrinsic, int64_t *flat_off, float *flat_xyz, float *flat_normal,
                            int64_t *less_off, float *less_xyz, float *less_normal, int32_t *less_row_col,
                            int64_t *sharp_off, float *sharp_xyz, int64_t *less_sharp_off, float *less_sharp_xyz,
                            int32_t *less_sharp_label, int32_t *less_sharp_row_col) {
  if (!c) return SQLM_ERR_INVALID_ARG;
  LfParams p;
  LcParams q;
  bool do_flat;
  const void *outs[7] = {flat_off, less_off, flat_xyz, flat_normal, less_xyz, less_normal, less_row_col};
  const LcOut co{sharp_off, less_sharp_off, sharp_xyz, less_sharp_xyz, less_sharp_label, less_sharp_row_col};
  if (int r = lf_check_all(n_sweep, sweep_off, xyz, params, corner, outs, co, &p, &q, &do_flat)) return r;
  return lf_run(c, n_sweep, sweep_off, xyz, p, extrinsic, do_flat, flat_off, flat_xyz, flat_normal, less_off, less_xyz,
                less_normal, less_row_col, corner ? &q : nullptr, co);
}

int sqlm_lidar_features_all_get_state(sqlm_ctx *c, sqlm_lidar_feat_state *flat_state,
                                      sqlm_lidar_corner_state *cs) {
  if (!c) return SQLM_ERR_INVALID_ARG;
  LidarFeatSolver *s = c->lidar_feat;
  if (!s || !s->have) return SQLM_ERR_STATE;
  if (cs && !s->have_corner) return SQLM_ERR_STATE;
  if (flat_state)
    if (int r = sqlm_lidar_features_get_state(c, flat_state)) return r;
  if (!cs) return SQLM_OK;
  LcDev &e = s->lc;
  const LfDev &d = e.f;
  const size_t cells = (size_t)d.n_rows * d.p.col_num;
  std::vector<int32_t> scan_n((size_t)d.n_rows, 0), cstate(cells, -3), sorted(cells, -1);
  std::vector<uint8_t> mask(cells, 0), reason(cells, 0), edge(cells, 0);
  std::vector<float> curv(cells, 0.f), angle;
  if (cs->angle) angle.assign(cells * kLcOffsets, lc_quiet_nan());
  if (d.n > 0) {
    if (hipSetDevice(c->device) != hipSuccess) return SQLM_ERR_HIP;
    SQLM_HIP_OK(hipStreamSynchronize(c->stream));
    SQLM_HIP_OK(hipMemcpy(scan_n.data(), d.scan_n, (size_t)d.n_rows * 4, hipMemcpyDeviceToHost));
    SQLM_HIP_OK(hipMemcpy(cstate.data(), e.state, cells * 4, hipMemcpyDeviceToHost));
    SQLM_HIP_OK(hipMemcpy(sorted.data(), e.sorted, cells * 4, hipMemcpyDeviceToHost));
    SQLM_HIP_OK(hipMemcpy(mask.data(), e.mask, cells, hipMemcpyDeviceToHost));
    SQLM_HIP_OK(hipMemcpy(reason.data(), e.reason, cells, hipMemcpyDeviceToHost));
    SQLM_HIP_OK(hipMemcpy(edge.data(), e.edge, cells, hipMemcpyDeviceToHost));
    SQLM_HIP_OK(hipMemcpy(curv.data(), e.curv, cells * 4, hipMemcpyDeviceToHost));
    for (int q = 0; q < d.n_rows; ++q)
      if (scan_n[q] < 0 || scan_n[q] > d.p.col_num) return SQLM_ERR_HIP;
    if (cs->angle) {  // the edge kernel once more, this time storing its angles
      float *dev = nullptr;
      if (hipMalloc((void **)&dev, angle.size() * sizeof(float)) != hipSuccess) return SQLM_ERR_OOM;
      LcDev a = e;
      a.angle = dev;
      launch_lidar_corner_angles(a, c->stream);
      hipError_t err = hipGetLastError();
      if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
      if (err == hipSuccess) err = hipMemcpy(angle.data(), dev, angle.size() * sizeof(float), hipMemcpyDeviceToHost);
      (void)hipFree(dev);
      if (err != hipSuccess) return SQLM_ERR_HIP;
    }
  }
  lc_pack_state(d.p, d.n_rows, scan_n.data(), cstate.data(), mask.data(), curv.data(), sorted.data(), reason.data(),
                edge.data(), angle.empty() ? nullptr : angle.data(), cs);
  return SQLM_OK;
}

int sqlm_lidar_features_all_info(const sqlm_ctx *c, int32_t out[8]) {
  if (!out) return SQLM_ERR_INVALID_ARG;
  const LidarFeatSolver *s = c ? c->lidar_feat : nullptr;
  out[0] = s ? s->launches : 0;
  for (int k = 0; k < 5; ++k) out[1 + k] = s ? s->cstats[k] : 0;
  out[6] = s ? (int32_t)s->n_less_sharp : 0;
  out[7] = s ? (int32_t)s->n_sharp : 0;
  return SQLM_OK;
}

int sqlm_lidar_corner_trig_probe(int64_t n, int which, const double *x, double *out) {
  if (n < 0 || which < 0 || which > 2 || (n > 0 && (!x || !out))) return SQLM_ERR_INVALID_ARG;
  for (int64_t i = 0; i < n; ++i) out[i] = which == 0 ? sqlm_acos(x[i]) : (which == 1 ? sqlm_sin(x[i]) : sqlm_cos(x[i]));
  return SQLM_OK;
}

int sqlm_lidar_corner_angle_probe(int64_t n, const float *p1, const float *p2, float *out) {
  if (n < 0 || (n > 0 && (!p1 || !p2 || !out))) return SQLM_ERR_INVALID_ARG;
  for (int64_t i = 0; i < n; ++i) out[i] = lc_angle(p1 + 3 * i, p2 + 3 * i);
  return SQLM_OK;
}

int sqlm_lidar_features_get_state(sqlm_ctx *c, sqlm_lidar_feat_state *st) {
  if (!c || !st) return SQLM_ERR_INVALID_ARG;
  LidarFeatSolver *s = c->lidar_feat;
  if (!s || !s->have) return SQLM_ERR_STATE;
  const LfDev &d = s->d;
  const size_t cells = (size_t)d.n_rows * d.p.col_num, np = (size_t)d.n;
  std::vector<int32_t> ring(np, -1), scan_n((size_t)d.n_rows, 0), scan_src(cells, 0), scan_col(cells, 0),
      image_index(cells, -1), nbr(cells, 0), sorted(cells, -1);
  std::vector<uint8_t> mask(cells, 0), reason(cells, 0);
  std::vector<float> curv(cells, 0.f);
  if (d.n > 0) {
    if (hipSetDevice(c->device) != hipSuccess) return SQLM_ERR_HIP;
    SQLM_HIP_OK(hipStreamSynchronize(c->stream));
    SQLM_HIP_OK(hipMemcpy(ring.data(), d.ring, np * 4, hipMemcpyDeviceToHost));
    SQLM_HIP_OK(hipMemcpy(scan_n.data(), d.scan_n, (size_t)d.n_rows * 4, hipMemcpyDeviceToHost));
    SQLM_HIP_OK(hipMemcpy(scan_src.data(), d.scan_src, cells * 4, hipMemcpyDeviceToHost));
    SQLM_HIP_OK(hipMemcpy(scan_col.data(), d.scan_col, cells * 4, hipMemcpyDeviceToHost));
    SQLM_HIP_OK(hipMemcpy(image_index.data(), d.image_index, cells * 4, hipMemcpyDeviceToHost));
    SQLM_HIP_OK(hipMemcpy(nbr.data(), d.nbr, cells * 4, hipMemcpyDeviceToHost));
    SQLM_HIP_OK(hipMemcpy(sorted.data(), d.sorted, cells * 4, hipMemcpyDeviceToHost));
    SQLM_HIP_OK(hipMemcpy(mask.data(), d.mask, cells, hipMemcpyDeviceToHost));
    SQLM_HIP_OK(hipMemcpy(reason.data(), d.reason, cells, hipMemcpyDeviceToHost));
    SQLM_HIP_OK(hipMemcpy(curv.data(), d.curv, cells * 4, hipMemcpyDeviceToHost));
    for (int q = 0; q < d.n_rows; ++q)
      if (scan_n[q] < 0 || scan_n[q] > d.p.col_num) return SQLM_ERR_HIP;
  }
  LfStrided a{scan_n.data(), scan_src.data(), scan_col.data(), image_index.data(), nbr.data(),
              sorted.data(), mask.data(),     reason.data(),   curv.data()};
  lf_pack_state(d.p, d.n_rows, d.n, ring.data(), a, st);
  return SQLM_OK;
}

int sqlm_lidar_features_info(const sqlm_ctx *c, int32_t out[8]) {
  if (!out) return SQLM_ERR_INVALID_ARG;
  const LidarFeatSolver *s = c ? c->lidar_feat : nullptr;
  out[0] = SQLM_LF_MAX_ROWS;
  out[1] = SQLM_LF_MAX_COLS;
  out[2] = s ? s->launches : 0;
  out[3] = s ? s->stats[0] : 0;
  out[4] = s ? s->stats[1] : 0;
  out[5] = s ? s->stats[2] : 0;
  out[6] = s ? s->stats[3] : 0;
  out[7] = SQLM_LF_MAX_HALF_WIDTH;
  return SQLM_OK;
}

int sqlm_lidar_feat_trig_probe(int64_t n, const double *y, const double *x, double *out) {
  if (n < 0 || (n > 0 && (!y || !out))) return SQLM_ERR_INVALID_ARG;
  for (int64_t i = 0; i < n; ++i) out[i] = x ? sqlm_atan2(y[i], x[i]) : sqlm_atan(y[i]);
  return SQLM_OK;
}

}  // extern "C"
