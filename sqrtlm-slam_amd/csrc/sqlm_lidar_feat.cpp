// sqlm_lidar_feat.cpp — host side of sqlm_lidar_features: argument and limit
// checks before the device is touched, one staged upload, the launches
// (sqlm_lidar_feat.hip), the read-back of the packed outputs; the read-back of
// the intermediate state for tests; and sqlm_lidar_features_host, the host
// twin: the reference's loops run sequentially over the same text
// (lidar_feat_dev.h) compiled for the CPU. Built with -ffp-contract=off like
// the kernels.
#include <algorithm>
#include <cstring>
#include <limits>
#include <new>
#include <vector>

#include "lidar_feat_dev.h"
#include "sqlm_ctx.h"
#include "sqlm_staging.h"

#pragma clang fp contract(off)

namespace sqlm {

struct LidarFeatSolver {
  Staged in, work, out;
  LfDev d;              // the last call's device pointers
  bool have = false;    // a call has completed
  int32_t launches = 0, stats[4] = {0, 0, 0, 0};
};

void lidar_feat_destroy(LidarFeatSolver *s) { delete s; }

namespace {

// The checks every entry point shares; fills `p` when they pass.
int lf_check(int n_sweep, const int64_t *sweep_off, const float *xyz, const sqlm_lidar_feat_params *prm,
             const void *const *outs, int n_outs, LfParams *p) {
  if (n_sweep < 0 || !sweep_off || !prm || sweep_off[0] != 0) return SQLM_ERR_INVALID_ARG;
  for (int s = 0; s < n_sweep; ++s) {
    if (sweep_off[s + 1] < sweep_off[s]) return SQLM_ERR_INVALID_ARG;
    if (sweep_off[s + 1] - sweep_off[s] >= (int64_t)std::numeric_limits<int32_t>::max()) return SQLM_ERR_INVALID_ARG;
  }
  const int64_t n = sweep_off[n_sweep];
  if (!outs[0] || !outs[1]) return SQLM_ERR_INVALID_ARG;  // the offset arrays
  if (n > 0) {
    if (!xyz) return SQLM_ERR_INVALID_ARG;
    for (int k = 2; k < n_outs; ++k)
      if (!outs[k]) return SQLM_ERR_INVALID_ARG;
  }
  if (prm->num_scan_subregions < 1 || prm->num_curvature_regions_flat < 1 || prm->num_curvature_regions_corner < 0 ||
      prm->max_surf_flat < 0 || prm->max_surf_less_flat < 0 || !(prm->deg_diff > 0.0) || prm->row_num < 1 ||
      prm->col_num < 1)
    return SQLM_ERR_INVALID_ARG;
  if (prm->using_sharp_point != 0) return SQLM_ERR_UNSUPPORTED;
  if (prm->row_num > SQLM_LF_MAX_ROWS || prm->col_num > SQLM_LF_MAX_COLS) return SQLM_ERR_UNSUPPORTED;
  const double hw = 0.01 / (prm->deg_diff / 180.0 * kLfPi) + 0.5;
  if (!(hw + 1.0 < (double)(kLfMaxHalf + 1))) return SQLM_ERR_UNSUPPORTED;
  if ((int64_t)n_sweep * prm->row_num * prm->num_scan_subregions >= (1ll << 30)) return SQLM_ERR_INVALID_ARG;
  if (prm->num_curvature_regions_flat > SQLM_LF_MAX_COLS || prm->num_curvature_regions_corner > SQLM_LF_MAX_COLS)
    return SQLM_ERR_INVALID_ARG;
  p->row_num = prm->row_num;
  p->col_num = prm->col_num;
  p->n_sub = prm->num_scan_subregions;
  p->ncr = prm->num_curvature_regions_flat;
  p->min_scan = 2 * std::max(prm->num_curvature_regions_flat, prm->num_curvature_regions_corner) + 1;
  p->max_flat = prm->max_surf_flat;
  p->max_less = prm->max_surf_less_flat;
  p->curv_th = prm->surf_curv_th;
  p->max_sq_dis = prm->max_sq_dis;
  p->deg_diff = prm->deg_diff;
  std::memcpy(p->ring_enabled, prm->ring_enabled, sizeof(p->ring_enabled));
  return SQLM_OK;
}

// The per-scan-point arrays as both sides hold them: [n_rows][col_num]
struct LfStrided {
  const int32_t *scan_n, *scan_src, *scan_col, *image_index, *nbr, *sorted;
  const uint8_t *mask, *reason;
  const float *curv;
};

void lf_pack_state(const LfParams &p, int n_rows, int64_t n, const int32_t *ring, const LfStrided &a,
                   sqlm_lidar_feat_state *st) {
  if (st->ring && n) std::memcpy(st->ring, ring, (size_t)n * sizeof(int32_t));
  if (st->image_index && n_rows)
    std::memcpy(st->image_index, a.image_index, (size_t)n_rows * p.col_num * sizeof(int32_t));
  int64_t off = 0;
  for (int q = 0; q < n_rows; ++q) {
    if (st->scan_off) st->scan_off[q] = off;
    const int m = a.scan_n[q];
    const size_t b = (size_t)q * p.col_num;
    if (st->scan_src) std::copy(a.scan_src + b, a.scan_src + b + m, st->scan_src + off);
    if (st->scan_col) std::copy(a.scan_col + b, a.scan_col + b + m, st->scan_col + off);
    if (st->mask) std::copy(a.mask + b, a.mask + b + m, st->mask + off);
    if (st->curvature) std::copy(a.curv + b, a.curv + b + m, st->curvature + off);
    if (st->neighbours) std::copy(a.nbr + b, a.nbr + b + m, st->neighbours + off);
    if (st->sorted) std::copy(a.sorted + b, a.sorted + b + m, st->sorted + off);
    if (st->reason) std::copy(a.reason + b, a.reason + b + m, st->reason + off);
    off += m;
  }
  if (st->scan_off) st->scan_off[n_rows] = off;
}

void lf_put_host(const double *ext, const float *p, float *out) {
  if (ext)
    lf_transform(ext, p, out);
  else
    std::memcpy(out, p, 3 * sizeof(float));
}

int lf_solver(sqlm_ctx *c) {
  if (hipSetDevice(c->device) != hipSuccess) return SQLM_ERR_HIP;
  if (!c->lidar_feat && !(c->lidar_feat = new (std::nothrow) LidarFeatSolver)) return SQLM_ERR_OOM;
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
  const int64_t n = sweep_off[n_sweep];
  const int rows = p.row_num, cols = p.col_num, n_rows = n_sweep * rows;
  const size_t cells = (size_t)n_rows * cols;
  std::vector<int32_t> ring((size_t)n, -1), scan_n((size_t)n_rows, 0), scan_src(cells, 0), scan_col(cells, 0),
      image_index(cells, -1), nbr(cells, 0), sorted(cells, -1);
  std::vector<uint8_t> mask(cells, 0), reason(cells, 0);
  std::vector<float> curv(cells, 0.f), scan_xyz(3 * cells, 0.f), azi;
  std::vector<unsigned long long> cell_key, keys;
  std::vector<uint32_t> cell_first;
  int64_t n_flat = 0, n_less = 0;
  for (int s = 0; s < n_sweep; ++s) {
    flat_off[s] = n_flat;
    less_off[s] = n_less;
    const int64_t o = sweep_off[s];
    const int32_t ns = (int32_t)(sweep_off[s + 1] - o);
    const float *P = xyz + 3 * o;
    azi.assign((size_t)ns, 0.f);
    int32_t first = -1, last = -1;
    for (int32_t i = 0; i < ns; ++i) {
      const float x = P[3 * i], y = P[3 * i + 1], z = P[3 * i + 2];
      if (!(lf_finite(x) && lf_finite(y) && lf_finite(z))) continue;
      const int rg = lf_ring(x, y, z);
      ring[(size_t)(o + i)] = rg;
      if (rg < 0) continue;
      azi[i] = -lf_atan2f(y, x);
      if (first < 0) first = i;
      last = i;
    }
    if (first < 0) continue;
    float start, end;
    lf_oris(azi[first], azi[last], &start, &end);
    const size_t sbase = (size_t)s * rows * cols;
    cell_key.assign((size_t)rows * cols, ~0ull);
    cell_first.assign((size_t)rows * cols, kLfNoIndex);
    bool half = false;  // PointToImage's loop, state and all
    for (int32_t i = 0; i < ns; ++i) {
      const int rg = ring[(size_t)(o + i)];
      if (rg < 0) continue;
      float a;
      if (!half) {
        a = lf_unpassed(azi[i], start);
        if (lf_turns_half(a, start)) half = true;
      } else {
        a = lf_passed(azi[i], end);
      }
      const int col = lf_col(a, start, cols);
      if (col < 0 || rg >= rows) continue;
      const size_t cell = (size_t)rg * cols + col;
      const unsigned long long key = ((unsigned long long)lf_bits(lf_dist(P + 3 * i)) << 32) | (uint32_t)i;
      if (key < cell_key[cell]) cell_key[cell] = key;
      if ((uint32_t)i < cell_first[cell]) cell_first[cell] = (uint32_t)i;
    }
    for (int r = 0; r < rows; ++r) {
      const size_t base = sbase + (size_t)r * cols;
      keys.clear();
      for (int c = 0; c < cols; ++c) {
        const uint32_t f = cell_first[(size_t)r * cols + c];
        if (f != kLfNoIndex) keys.push_back(((unsigned long long)f << 12) | (unsigned)c);
      }
      std::sort(keys.begin(), keys.end());
      const int m = (int)keys.size();
      scan_n[(size_t)s * rows + r] = m;
      for (int q = 0; q < m; ++q) {
        const int c = (int)(keys[q] & 4095u);
        const uint32_t occ = (uint32_t)(cell_key[(size_t)r * cols + c] & 0xffffffffull);
        scan_src[base + q] = (int32_t)occ;
        scan_col[base + q] = c;
        std::memcpy(&scan_xyz[3 * (base + q)], P + 3 * (size_t)occ, 3 * sizeof(float));
        image_index[base + c] = q;
      }
      if (!p.ring_enabled[r] || m <= p.min_scan) continue;
      const float *scan = &scan_xyz[3 * base];
      for (int i = p.ncr; i + p.ncr < m; ++i) {
        const int rule = lf_mask_rule(scan, i);
        if (rule == 1)
          std::fill_n(&mask[base + i - p.ncr], p.ncr + 1, (uint8_t)1);
        else if (rule == 2)
          std::fill_n(&mask[base + i + 1], p.ncr, (uint8_t)1);
      }
    }
    LfView v;
    v.image_index = &image_index[sbase];
    v.scan_xyz = &scan_xyz[3 * sbase];
    v.scan_col = &scan_col[sbase];
    v.row_num = rows;
    v.col_num = cols;
    for (int r = 0; r < rows; ++r) {
      const size_t base = sbase + (size_t)r * cols;
      const int m = scan_n[(size_t)s * rows + r];
      if (!p.ring_enabled[r] || m <= p.min_scan) continue;
      const float *scan = &scan_xyz[3 * base];
      for (int j = 0; j < p.n_sub; ++j) {
        int64_t sp, ep;
        lf_region(m, p.ncr, p.n_sub, j, &sp, &ep);
        if (ep <= sp) continue;
        const int size = (int)(ep - sp + 1);
        keys.resize((size_t)size);
        for (int k = 0; k < size; ++k) {
          const int i = (int)sp + k;
          int nb;
          const float cv = lf_curvature(scan, i, m, p.ncr, &nb);
          curv[base + i] = cv;
          nbr[base + i] = nb;
          keys[k] = ((unsigned long long)lf_bits(cv) << 32) | (unsigned)i;
        }
        std::sort(keys.begin(), keys.end());
        int picked = 0, k = 0;
        for (; k < size; ++k) {  // :1070-1233, the break included
          const int idx = (int)(keys[k] & 0xffffffffull);
          sorted[base + sp + k] = idx;
          if (mask[base + idx]) {
            reason[base + idx] = SQLM_LF_MASKED;
            continue;
          }
          if (!((double)curv[base + idx] < p.curv_th)) {
            reason[base + idx] = SQLM_LF_CURVATURE;
            continue;
          }
          float nrm[3];
          const int code = lf_candidate(v, p, r, idx, nrm);
          reason[base + idx] = (uint8_t)code;
          if (code != SQLM_LF_PICKED) continue;
          if (picked < p.max_less) {
            lf_put_host(extrinsic, scan + 3 * idx, less_xyz + 3 * n_less);
            lf_put_host(extrinsic, nrm, less_normal + 3 * n_less);
            less_row_col[2 * n_less] = r;
            less_row_col[2 * n_less + 1] = scan_col[base + idx];
            ++n_less;
            if (picked < p.max_flat) {
              lf_put_host(extrinsic, scan + 3 * idx, flat_xyz + 3 * n_flat);
              lf_put_host(extrinsic, nrm, flat_normal + 3 * n_flat);
              ++n_flat;
            }
            ++picked;
          } else {
            reason[base + idx] = SQLM_LF_OVER_CAP;
          }
          if (picked >= p.max_less) {
            ++k;
            break;
          }
        }
        for (; k < size; ++k) {
          const int idx = (int)(keys[k] & 0xffffffffull);
          sorted[base + sp + k] = idx;
          reason[base + idx] = SQLM_LF_OVER_CAP;
        }
      }
    }
  }
  flat_off[n_sweep] = n_flat;
  less_off[n_sweep] = n_less;
  if (state) {
    LfStrided a{scan_n.data(), scan_src.data(), scan_col.data(), image_index.data(), nbr.data(),
                sorted.data(), mask.data(),     reason.data(),   curv.data()};
    lf_pack_state(p, n_rows, n, ring.data(), a, state);
  }
  return SQLM_OK;
}

int sqlm_lidar_features(sqlm_ctx *c, int n_sweep, const int64_t *sweep_off, const float *xyz,
                        const sqlm_lidar_feat_params *params, const double *extrinsic, int64_t *flat_off,
                        float *flat_xyz, float *flat_normal, int64_t *less_off, float *less_xyz, float *less_normal,
                        int32_t *less_row_col) {
  if (!c) return SQLM_ERR_INVALID_ARG;
  LfParams p;
  const void *outs[7] = {flat_off, less_off, flat_xyz, flat_normal, less_xyz, less_normal, less_row_col};
  if (int r = lf_check(n_sweep, sweep_off, xyz, params, outs, 7, &p)) return r;
  if (int r = lf_solver(c)) return r;
  LidarFeatSolver *s = c->lidar_feat;
  s->have = false;
  s->launches = 0;
  std::memset(s->stats, 0, sizeof(s->stats));
  const int64_t n = sweep_off[n_sweep];
  const size_t np = (size_t)n, ns = (size_t)n_sweep, n_rows = ns * p.row_num, cells = n_rows * p.col_num,
               regions = n_rows * p.n_sub;
  LfDev &d = s->d;
  d = LfDev();
  d.p = p;
  d.n_sweep = n_sweep;
  d.n_rows = (int32_t)n_rows;
  d.n = n;
  if (n == 0) {
    for (int k = 0; k <= n_sweep; ++k) flat_off[k] = less_off[k] = 0;
    s->have = true;
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
  // out: the small part first, read back before the clouds
  const size_t o_foff = out.take((ns + 1) * 8), o_loff = out.take((ns + 1) * 8), o_stats = out.take(16);
  const size_t o_small = out.off;
  const size_t o_fx = out.take(np * 12), o_fn = out.take(np * 12), o_lx = out.take(np * 12), o_ln = out.take(np * 12),
               o_rc = out.take(np * 8);
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
  s->launches = launch_lidar_feat(d, c->stream);
  SQLM_HIP_OK(hipGetLastError());
  SQLM_HIP_OK(hipMemcpyAsync(s->out.host, s->out.dev, o_small, hipMemcpyDeviceToHost, c->stream));
  SQLM_HIP_OK(hipStreamSynchronize(c->stream));
  char *oh = s->out.host;
  std::memcpy(flat_off, oh + o_foff, (ns + 1) * 8);
  std::memcpy(less_off, oh + o_loff, (ns + 1) * 8);
  std::memcpy(s->stats, oh + o_stats, 16);
  const int64_t kf = flat_off[n_sweep], kl = less_off[n_sweep];
  if (kf < 0 || kl < 0 || kf > n || kl > n) return SQLM_ERR_HIP;  // never: a scan point is picked once
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
  std::memcpy(flat_xyz, oh + o_fx, (size_t)kf * 12);
  std::memcpy(flat_normal, oh + o_fn, (size_t)kf * 12);
  std::memcpy(less_xyz, oh + o_lx, (size_t)kl * 12);
  std::memcpy(less_normal, oh + o_ln, (size_t)kl * 12);
  std::memcpy(less_row_col, oh + o_rc, (size_t)kl * 8);
  s->have = true;
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
