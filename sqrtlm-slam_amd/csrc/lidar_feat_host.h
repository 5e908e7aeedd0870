// lidar_feat_host.h — the host side of the LiDAR feature extraction that needs
// no device: the argument and limit checks of sqlm_lidar_features and
// sqlm_lidar_features_all, the packing of the intermediate state, and the host
// twin of both branches (the reference's loops run sequentially over the text of
// lidar_feat_dev.h and lidar_corner_dev.h). Plain C++: sqlm_lidar_feat.cpp
// includes it, and so does tools/corner_check.cpp, a stand-alone program that
// runs it under sanitizers. Built with -ffp-contract=off.
#pragma once
#include <algorithm>
#include <cstring>
#include <limits>
#include <vector>

#include "lidar_corner_dev.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace sqlm {

// The checks every entry point shares; fills `p` when they pass.
inline int lf_check(int n_sweep, const int64_t *sweep_off, const float *xyz, const sqlm_lidar_feat_params *prm,
             const void *const *outs, int n_outs, LfParams *p, bool allow_sharp = false) {
  if (n_sweep < 0 || !sweep_off || !prm || sweep_off[0] != 0) return SQLM_ERR_INVALID_ARG;
  for (int s = 0; s < n_sweep; ++s) {
    if (sweep_off[s + 1] < sweep_off[s]) return SQLM_ERR_INVALID_ARG;
    if (sweep_off[s + 1] - sweep_off[s] >= (int64_t)std::numeric_limits<int32_t>::max()) return SQLM_ERR_INVALID_ARG;
  }
  const int64_t n = sweep_off[n_sweep];
  if (n_outs && (!outs[0] || !outs[1])) return SQLM_ERR_INVALID_ARG;  // the offset arrays
  if (n > 0) {
    if (!xyz) return SQLM_ERR_INVALID_ARG;
    for (int k = 2; k < n_outs; ++k)
      if (!outs[k]) return SQLM_ERR_INVALID_ARG;
  }
  if (prm->num_scan_subregions < 1 || prm->num_curvature_regions_flat < 1 || prm->num_curvature_regions_corner < 0 ||
      prm->max_surf_flat < 0 || prm->max_surf_less_flat < 0 || !(prm->deg_diff > 0.0) || prm->row_num < 1 ||
      prm->col_num < 1)
    return SQLM_ERR_INVALID_ARG;
  if (prm->using_sharp_point != 0 && !allow_sharp) return SQLM_ERR_UNSUPPORTED;
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

// The checks of the corner stage; fills `q` when they pass.
inline int lc_check(int64_t n, const sqlm_lidar_feat_params *prm, const sqlm_lidar_corner_params *cp,
             const void *const *outs, int n_outs, LcParams *q) {
  if (!outs[0] || !outs[2]) return SQLM_ERR_INVALID_ARG;  // the offset arrays
  if (n > 0)
    for (int k = 0; k < n_outs; ++k)
      if (!outs[k]) return SQLM_ERR_INVALID_ARG;
  if (prm->num_curvature_regions_corner < 1 || cp->max_corner_sharp < 0 || cp->max_corner_less_sharp < 0)
    return SQLM_ERR_INVALID_ARG;
  const double inf = std::numeric_limits<double>::infinity();
  if (!(cp->sharp_curv_th > -inf && cp->sharp_curv_th < inf) || !(cp->ground_z_bound > -inf && cp->ground_z_bound < inf))
    return SQLM_ERR_INVALID_ARG;
  q->ncr = prm->num_curvature_regions_corner;
  q->max_sharp = cp->max_corner_sharp;
  q->max_less = cp->max_corner_less_sharp;
  q->curv_th = cp->sharp_curv_th;
  q->ground_z = cp->ground_z_bound;
  std::memcpy(q->ring_enabled, cp->corner_ring_enabled, sizeof(q->ring_enabled));
  return SQLM_OK;
}

// The outputs of the corner stage
struct LcOut {
  int64_t *sharp_off, *less_off;
  float *sharp_xyz, *less_xyz;
  int32_t *less_label, *less_rc;
};

// The per-scan-point arrays as both sides hold them: [n_rows][col_num]
struct LfStrided {
  const int32_t *scan_n, *scan_src, *scan_col, *image_index, *nbr, *sorted;
  const uint8_t *mask, *reason;
  const float *curv;
};

inline void lf_pack_state(const LfParams &p, int n_rows, int64_t n, const int32_t *ring, const LfStrided &a,
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

inline void lf_put_host(const double *ext, const float *p, float *out) {
  if (ext)
    lf_transform(ext, p, out);
  else
    std::memcpy(out, p, 3 * sizeof(float));
}

// The corner state's per-scan-point arrays from their strided form, and the per-cell ones
inline void lc_pack_state(const LfParams &p, int n_rows, const int32_t *scan_n, const int32_t *cstate, const uint8_t *mask,
                   const float *curv, const int32_t *sorted, const uint8_t *reason, const uint8_t *edge,
                   const float *angle, sqlm_lidar_corner_state *st) {
  const size_t cells = (size_t)n_rows * p.col_num;
  if (st->cell_state && cells) std::memcpy(st->cell_state, cstate, cells * sizeof(int32_t));
  if (st->edge && cells) std::memcpy(st->edge, edge, cells);
  if (st->angle && cells && angle) std::memcpy(st->angle, angle, cells * kLcOffsets * sizeof(float));
  int64_t off = 0;
  for (int q = 0; q < n_rows; ++q) {
    const int m = scan_n[q];
    const size_t b = (size_t)q * p.col_num;
    if (st->mask) std::copy(mask + b, mask + b + m, st->mask + off);
    if (st->curvature) std::copy(curv + b, curv + b + m, st->curvature + off);
    if (st->sorted) std::copy(sorted + b, sorted + b + m, st->sorted + off);
    if (st->reason) std::copy(reason + b, reason + b + m, st->reason + off);
    off += m;
  }
}

// The host twin of both branches: `p` has passed lf_check; do_flat = the flat
// outputs exist; lc = null: no corner stage.
inline int lf_host(int n_sweep, const int64_t *sweep_off, const float *xyz, const LfParams &p, const double *extrinsic,
            bool do_flat, int64_t *flat_off, float *flat_xyz, float *flat_normal, int64_t *less_off, float *less_xyz,
            float *less_normal, int32_t *less_row_col, sqlm_lidar_feat_state *state, const LcParams *lc,
            const LcOut &co, sqlm_lidar_corner_state *cstate_out) {
  const int64_t n = sweep_off[n_sweep];
  const int rows = p.row_num, cols = p.col_num, n_rows = n_sweep * rows;
  const size_t cells = (size_t)n_rows * cols;
  std::vector<int32_t> ring((size_t)n, -1), scan_n((size_t)n_rows, 0), scan_src(cells, 0), scan_col(cells, 0),
      image_index(cells, -1), nbr(cells, 0), sorted(cells, -1);
  std::vector<uint8_t> mask(cells, 0), reason(cells, 0);
  std::vector<float> curv(cells, 0.f), scan_xyz(3 * cells, 0.f), azi;
  std::vector<unsigned long long> cell_key, keys;
  std::vector<uint32_t> cell_first;
  const size_t ccells = lc ? cells : 0;
  std::vector<int32_t> cstate(ccells, -3), csorted(ccells, -1), queue;
  std::vector<uint8_t> cmask(ccells, 0), creason(ccells, 0), cedge(ccells, 0);
  std::vector<float> ccurv(ccells, 0.f), cangle;
  if (lc && cstate_out && cstate_out->angle) cangle.assign(ccells * kLcOffsets, lc_quiet_nan());
  int64_t n_flat = 0, n_less = 0, n_sharp = 0, n_lsharp = 0;
  for (int s = 0; s < n_sweep; ++s) {
    if (do_flat) {
      flat_off[s] = n_flat;
      less_off[s] = n_less;
    }
    if (lc) {
      co.sharp_off[s] = n_sharp;
      co.less_off[s] = n_lsharp;
    }
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
      if (!do_flat || !p.ring_enabled[r] || m <= p.min_scan) continue;
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
      if (!do_flat || !p.ring_enabled[r] || m <= p.min_scan) continue;
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
    if (!lc) continue;
    // the corner branch of the sweep, :861-1037
    int32_t *cst = &cstate[sbase];
    for (int r = 0; r < rows; ++r)
      for (int c = 0; c < cols; ++c) {
        const int idx = image_index[sbase + (size_t)r * cols + c];
        cst[(size_t)r * cols + c] =
            idx < 0 ? -3 : lc_initial_state(&scan_xyz[3 * (sbase + (size_t)r * cols + idx)], lc->ground_z);
      }
    for (int r = 0; r < rows; ++r)
      for (int c = 0; c < cols; ++c) {
        const size_t cell = sbase + (size_t)r * cols + c;
        cedge[cell] = (uint8_t)lc_edges(v, cst, r, c, cangle.empty() ? nullptr : &cangle[kLcOffsets * cell]);
      }
    int label = 1;
    const int cw = lc->ncr;
    for (int r = 0; r < rows; ++r) {
      const size_t base = sbase + (size_t)r * cols;
      const int m = scan_n[(size_t)s * rows + r];
      if (!lc->ring_enabled[r] || m <= p.min_scan) continue;
      const float *scan = &scan_xyz[3 * base];
      for (int i = cw; i + cw < m; ++i) {
        const int rule = lf_mask_rule(scan, i);
        if (rule == 1)
          std::fill_n(&cmask[base + i - cw], cw + 1, (uint8_t)1);
        else if (rule == 2)
          std::fill_n(&cmask[base + i + 1], cw, (uint8_t)1);
        else if (lc_mask_rule3(scan, i))
          cmask[base + i] = 1;
      }
      for (int j = 0; j < p.n_sub; ++j) {
        int64_t sp, ep;
        lf_region(m, cw, p.n_sub, j, &sp, &ep);
        if (ep <= sp) continue;
        const int size = (int)(ep - sp + 1);
        keys.resize((size_t)size);
        for (int k = 0; k < size; ++k) {
          const int i = (int)sp + k;
          const float cv = lc_curvature(scan, i, cw);
          ccurv[base + i] = cv;
          keys[k] = ((unsigned long long)lf_bits(cv) << 32) | (unsigned)i;
        }
        std::sort(keys.begin(), keys.end());
        for (int k = 0; k < size; ++k) csorted[base + sp + k] = (int32_t)(keys[k] & 0xffffffffull);
        int num = 0;
        for (int k = size - 1; k >= 0; --k) {
          const int idx = csorted[base + sp + k];
          const int cell = r * cols + scan_col[base + idx];
          if (cst[cell] == -1) {
            creason[base + idx] = SQLM_LC_GROUND;
            continue;
          }
          if (cmask[base + idx]) {
            creason[base + idx] = SQLM_LC_MASKED;
            continue;
          }
          if (!((double)ccurv[base + idx] > lc->curv_th)) {
            creason[base + idx] = SQLM_LC_CURVATURE;
            continue;
          }
          if (cst[cell] == 0) {  // :908-1006
            bool line[SQLM_LF_MAX_ROWS] = {false};
            queue.assign(1, cell);
            cst[cell] = label;
            for (size_t h = 0; h < queue.size(); ++h) {
              const int from = queue[h], fr = from / cols, fc = from - fr * cols;
              const uint32_t e = cedge[sbase + from];
              for (int o = 0; o < kLcOffsets; ++o) {
                int tr, tc;
                if (!((e >> o) & 1u) || !lc_target(o, fr, fc, rows, cols, &tr, &tc)) continue;
                const int to = tr * cols + tc;
                if (cst[to] != 0) continue;
                cst[to] = label;
                queue.push_back(to);
                line[tr] = true;
              }
            }
            int lines = 0;
            for (int q = 0; q < rows; ++q) lines += line[q] ? 1 : 0;
            if (lines >= 3)
              ++label;
            else
              for (int cellq : queue) cst[cellq] = -2;
          }
          if (cst[cell] < 1) {
            creason[base + idx] = SQLM_LC_UNSTABLE;
            continue;
          }
          if (num < lc->max_less) {
            creason[base + idx] = SQLM_LC_PICKED;
            lf_put_host(extrinsic, scan + 3 * idx, co.less_xyz + 3 * n_lsharp);
            co.less_label[n_lsharp] = cst[cell];
            co.less_rc[2 * n_lsharp] = r;
            co.less_rc[2 * n_lsharp + 1] = scan_col[base + idx];
            ++n_lsharp;
            if (num < lc->max_sharp) {
              lf_put_host(extrinsic, scan + 3 * idx, co.sharp_xyz + 3 * n_sharp);
              ++n_sharp;
            }
            ++num;
          } else {
            creason[base + idx] = SQLM_LC_OVER_CAP;
          }
          if (num >= lc->max_less) {
            for (int kk = 0; kk < k; ++kk) creason[base + csorted[base + sp + kk]] = SQLM_LC_OVER_CAP;
            break;
          }
        }
      }
    }
  }
  if (do_flat) {
    flat_off[n_sweep] = n_flat;
    less_off[n_sweep] = n_less;
  }
  if (lc) {
    co.sharp_off[n_sweep] = n_sharp;
    co.less_off[n_sweep] = n_lsharp;
    if (cstate_out)
      lc_pack_state(p, n_rows, scan_n.data(), cstate.data(), cmask.data(), ccurv.data(), csorted.data(), creason.data(),
                    cedge.data(), cangle.empty() ? nullptr : cangle.data(), cstate_out);
  }
  if (state) {
    LfStrided a{scan_n.data(), scan_src.data(), scan_col.data(), image_index.data(), nbr.data(),
                sorted.data(), mask.data(),     reason.data(),   curv.data()};
    lf_pack_state(p, n_rows, n, ring.data(), a, state);
  }
  return SQLM_OK;
}

}  // namespace sqlm
