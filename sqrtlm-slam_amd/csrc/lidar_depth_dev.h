// lidar_depth_dev.h — the arithmetic of the LiDAR depth image and the keypoint
// depth association (sqlm_lidar_depth, include/sqrtlm.h), written once for the
// kernels (sqlm_lidar_depth.hip), for the host twin (sqlm_lidar_depth_host, the
// same text compiled for the CPU) and for tools/depth_check.cpp (plain g++, no
// HIP), and the launch interface between sqlm_lidar_depth.cpp and the kernels.
// Every translation unit is built with -ffp-contract=off: every result comes
// from IEEE float / double operations in the order written here.
//
// Every function restates a piece of the reference's Frame.cc with C++'s usual
// arithmetic conversions; the line numbers are that file's.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#ifndef SQLM_HD
#if defined(__HIPCC__)
#define SQLM_HD __host__ __device__
#else
#define SQLM_HD
#endif
#endif

#include "../../include/sqrtlm.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace sqlm {

constexpr int kLdBlock = 256;                      // lanes of every workgroup
constexpr int kLdLanes = 2 * SQLM_LD_HALF_W;       // lanes per keypoint: one per dx, adjacent lanes on adjacent columns
constexpr int kLdRows = 2 * SQLM_LD_HALF_H;        // patch rows, one per dy
constexpr int32_t kLdNoKey = 0x7fffffff;           // no seen cell
constexpr int64_t kLdMaxKeys = (int64_t)1 << 27;   // keypoints of a batch (kLdLanes lanes each)

struct LdCfg {
  int32_t rows = 0, cols = 0, has_un = 0;
  double M[12];   // intrinsic * extrinsic
  double E2[4];   // row 2 of extrinsic
  float cam[4];   // fx, fy, cx, cy
};

SQLM_HD inline uint32_t ld_bits(float v) {
  union {
    float f;
    uint32_t u;
  } b;
  b.f = v;
  return b.u;
}
SQLM_HD inline bool ld_finite(float v) { return (ld_bits(v) & 0x7f800000u) != 0x7f800000u; }
inline bool ld_finite_d(double v) { return v - v == 0.0; }

// M = intrinsic (3x4) * extrinsic (4x4), :301
inline void ld_mul(const double *a, const double *b, double *M) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c)
      M[4 * r + c] = ((a[4 * r] * b[c] + a[4 * r + 1] * b[4 + c]) + a[4 * r + 2] * b[8 + c]) + a[4 * r + 3] * b[12 + c];
}

SQLM_HD inline double ld_row(const double *m, double x, double y, double z) {
  return ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
}

// (extrinsicMatrix * P_lidar).z(), :309
SQLM_HD inline double ld_depth(const LdCfg &c, const float *p) {
  return ld_row(c.E2, (double)p[0], (double)p[1], (double)p[2]);
}

// int(q) of a quotient or of a float cell coordinate, as a cell of [0, n): a
// value in (-1, 0) truncates to 0; -1 = outside, NaN included
SQLM_HD inline int32_t ld_cell(double q, int32_t n) { return (q > -1.0 && q < (double)n) ? (int32_t)q : -1; }

// :293-308: the pixel v * cols + u the point writes, -1 when it writes none
SQLM_HD inline int32_t ld_project(const LdCfg &c, const float *p) {
  if (!(ld_finite(p[0]) && ld_finite(p[1]) && ld_finite(p[2]))) return -1;
  if (!(p[0] > SQLM_LD_MIN_X)) return -1;
  const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
  const double zu = ld_row(c.M, x, y, z), zv = ld_row(c.M + 4, x, y, z), zw = ld_row(c.M + 8, x, y, z);
  const int32_t u = ld_cell(zu / zw, c.cols), v = ld_cell(zv / zw, c.rows);
  return (u < 0 || v < 0) ? -1 : v * c.cols + u;
}

// :366-367, the double read into a uchar
SQLM_HD inline bool ld_seen(double d) {
  const int32_t t = (d > -2147483648.0 && d < 2147483648.0) ? (int32_t)d : INT32_MIN;
  return (t & 255) != 0;
}

// What a patch holds: the seen cells' least and greatest depth and least nearest key
struct LdPatch {
  double lo, hi;
  int32_t key;
};
SQLM_HD inline void ld_patch_init(LdPatch *a) {
  a->lo = 0.0;
  a->hi = 0.0;
  a->key = kLdNoKey;
}
SQLM_HD inline int32_t ld_key(int dx, int dy) {
  return (dx * dx + dy * dy) * 128 + ((dx + SQLM_LD_HALF_W) * kLdRows + (dy + SQLM_LD_HALF_H));
}
SQLM_HD inline void ld_patch_merge(LdPatch *a, const LdPatch &b) {
  if (b.key == kLdNoKey) return;
  if (a->key == kLdNoKey) {
    *a = b;
    return;
  }
  if (b.lo < a->lo) a->lo = b.lo;
  if (b.hi > a->hi) a->hi = b.hi;
  if (b.key < a->key) a->key = b.key;
}
// the cell of (dx, dy) around pt, :366-378; image = the frame's [rows][cols]
SQLM_HD inline void ld_patch_cell(const LdCfg &c, const double *image, float px, float py, int dx, int dy, LdPatch *a) {
  const int32_t row = ld_cell((double)(py + (float)dy), c.rows), col = ld_cell((double)(px + (float)dx), c.cols);
  if (row < 0 || col < 0) return;
  const double d = image[(int64_t)row * c.cols + col];
  if (!ld_seen(d)) return;
  LdPatch b;
  b.lo = b.hi = d;
  b.key = ld_key(dx, dy);
  ld_patch_merge(a, b);
}

struct LdKeyOut {
  int32_t cls, u, v;
  float depth, cam[3];
};
// :356-401 from the reduced patch (below = pt.y < min_v), then :1710-1723
SQLM_HD inline void ld_classify(const LdCfg &c, const double *image, bool below, const LdPatch &a, float px, float py,
                                const float *un, LdKeyOut *o) {
  o->cls = 0;
  o->u = o->v = -1;
  o->depth = -1.0f;
  o->cam[0] = o->cam[1] = o->cam[2] = 0.0f;
  if (below || a.key == kLdNoKey) return;
  const int slot = a.key & 127, dx = slot / kLdRows - SQLM_LD_HALF_W, dy = slot % kLdRows - SQLM_LD_HALF_H;
  o->v = ld_cell((double)(py + (float)dy), c.rows);
  o->u = ld_cell((double)(px + (float)dx), c.cols);
  if (a.hi - a.lo > SQLM_LD_MAX_RANGE) {
    o->cls = 2;
    return;
  }
  o->cls = 1;
  o->depth = (float)image[(int64_t)o->v * c.cols + o->u];
  if (un && o->depth > 0.0f) {
    const float z = o->depth, invfx = 1.0f / c.cam[0], invfy = 1.0f / c.cam[1];
    o->cam[0] = ((un[0] - c.cam[2]) * z) * invfx;
    o->cam[1] = ((un[1] - c.cam[3]) * z) * invfy;
    o->cam[2] = z;
  }
}

// The argument and limit checks every entry point shares; fills cfg when they
// pass. Reads the offsets and the matrices only.
inline int ld_check(int n_frame, const int64_t *sweep_off, const float *xyz, const int64_t *key_off, const float *key_xy,
                    const float *key_un_xy, int rows, int cols, const double *intrinsic, const double *extrinsic,
                    const float *cam, const int32_t *class_id, const float *depth, const int32_t *nearest_uv,
                    const float *xyz_cam, const int32_t *stats, LdCfg *cfg) {
  if (n_frame < 0 || !sweep_off || !key_off || !intrinsic || !extrinsic) return SQLM_ERR_INVALID_ARG;
  if (rows < 1 || cols < 1 || sweep_off[0] != 0 || key_off[0] != 0) return SQLM_ERR_INVALID_ARG;
  if (n_frame > 0 && !stats) return SQLM_ERR_INVALID_ARG;
  for (int f = 0; f < n_frame; ++f) {
    if (sweep_off[f + 1] < sweep_off[f] || key_off[f + 1] < key_off[f]) return SQLM_ERR_INVALID_ARG;
    if (sweep_off[f + 1] - sweep_off[f] >= (int64_t)INT32_MAX) return SQLM_ERR_INVALID_ARG;
  }
  const int64_t n = sweep_off[n_frame], m = key_off[n_frame];
  if (n > 0 && !xyz) return SQLM_ERR_INVALID_ARG;
  if (m > 0 && (!key_xy || !class_id || !depth || !nearest_uv)) return SQLM_ERR_INVALID_ARG;
  if (xyz_cam && (!cam || (m > 0 && !key_un_xy))) return SQLM_ERR_INVALID_ARG;
  for (int k = 0; k < 12; ++k)
    if (!ld_finite_d(intrinsic[k])) return SQLM_ERR_INVALID_ARG;
  for (int k = 0; k < 16; ++k)
    if (!ld_finite_d(extrinsic[k])) return SQLM_ERR_INVALID_ARG;
  if (rows > SQLM_LD_MAX_DIM || cols > SQLM_LD_MAX_DIM) return SQLM_ERR_UNSUPPORTED;
  if ((int64_t)n_frame * rows * cols > (int64_t)SQLM_LD_MAX_CELLS) return SQLM_ERR_UNSUPPORTED;
  if (n > (int64_t)INT32_MAX || m >= kLdMaxKeys) return SQLM_ERR_UNSUPPORTED;
  cfg->rows = rows;
  cfg->cols = cols;
  cfg->has_un = (xyz_cam && cam && key_un_xy) ? 1 : 0;
  ld_mul(intrinsic, extrinsic, cfg->M);
  std::memcpy(cfg->E2, extrinsic + 8, sizeof(cfg->E2));
  for (int k = 0; k < 4; ++k) cfg->cam[k] = cam ? cam[k] : 0.0f;
  return SQLM_OK;
}

// One frame on the host, sequentially, over the functions above. winner and
// image are the frame's [rows][cols] (any contents); pixel [n] may be NULL.
inline void ld_host_frame(const LdCfg &c, int32_t n, const float *xyz, int64_t m, const float *key_xy,
                          const float *key_un_xy, int32_t *class_id, float *depth, int32_t *nearest_uv, float *xyz_cam,
                          int32_t *stats, int32_t *pixel, int32_t *winner, double *image) {
  const int64_t cells = (int64_t)c.rows * c.cols;
  for (int64_t p = 0; p < cells; ++p) winner[p] = 0;
  int32_t n_written = 0, n_occupied = 0, n_with = 0, min_v = 0;
  for (int32_t i = 0; i < n; ++i) {
    const int32_t pix = ld_project(c, xyz + 3 * (int64_t)i);
    if (pixel) pixel[i] = pix;
    if (pix < 0) continue;
    if (i + 1 > winner[pix]) winner[pix] = i + 1;
    ++n_written;
  }
  bool found = false;
  for (int64_t p = 0; p < cells; ++p) {
    const int32_t w = winner[p];
    image[p] = w > 0 ? ld_depth(c, xyz + 3 * (int64_t)(w - 1)) : 0.0;
    if (w > 0) ++n_occupied;
    if (!found && image[p] > 0.0) {
      found = true;
      min_v = (int32_t)(p / c.cols);
    }
  }
  for (int64_t k = 0; k < m; ++k) {
    const float px = key_xy[2 * k], py = key_xy[2 * k + 1];
    LdPatch a;
    ld_patch_init(&a);
    const bool below = py < (float)min_v;
    if (!below)
      for (int dx = -SQLM_LD_HALF_W; dx < SQLM_LD_HALF_W; ++dx)
        for (int dy = -SQLM_LD_HALF_H; dy < SQLM_LD_HALF_H; ++dy) ld_patch_cell(c, image, px, py, dx, dy, &a);
    LdKeyOut o;
    ld_classify(c, image, below, a, px, py, c.has_un ? key_un_xy + 2 * k : nullptr, &o);
    class_id[k] = o.cls;
    depth[k] = o.depth;
    nearest_uv[2 * k] = o.u;
    nearest_uv[2 * k + 1] = o.v;
    if (c.has_un) {
      xyz_cam[3 * k] = o.cam[0];
      xyz_cam[3 * k + 1] = o.cam[1];
      xyz_cam[3 * k + 2] = o.cam[2];
    }
    if (o.depth > 0.0f) ++n_with;
  }
  stats[0] = min_v;
  stats[1] = n_written;
  stats[2] = n_occupied;
  stats[3] = n_with;
}

#if defined(__HIPCC__)
// Device pointers of one call. Cells are f * rows * cols + v * cols + u.
struct LdDev {
  LdCfg c;
  int32_t n_frame = 0;
  int64_t n = 0, m = 0, cells = 0;  // points, keypoints, cells of the batch
  const int64_t *sweep_off = nullptr, *key_off = nullptr;
  const float *xyz = nullptr, *key_xy = nullptr, *key_un_xy = nullptr;
  int32_t *pixel = nullptr;   // [n]
  int32_t *winner = nullptr;  // [cells], zeroed per call
  double *image = nullptr;    // [cells], every cell written per call
  int32_t *stats = nullptr;   // [n_frame][4], zeroed per call: rows - min positive row (0 = none), n_written, n_occupied, n_with_depth
  int32_t *class_id = nullptr, *nearest_uv = nullptr;
  float *depth = nullptr, *xyz_cam = nullptr;
};

// The launches of one call, in order; returns how many kernels were launched.
int launch_lidar_depth(const LdDev &d, hipStream_t st);
#endif

}  // namespace sqlm
