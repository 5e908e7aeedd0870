// lidar_corner_dev.h — the arithmetic of the LiDAR corner-feature extraction
// (sqlm_lidar_features_all, include/sqrtlm.h), written once for the kernels
// (sqlm_lidar_corner.hip) and for the host twin (sqlm_lidar_features_all_host,
// the same text compiled for the CPU), and the launch interface between
// sqlm_lidar_feat.cpp and the kernels. Built with -ffp-contract=off like
// lidar_feat_dev.h, whose range image, scans and helpers it reuses; acos / sin /
// cos / atan2 are sqlm_libm.h's. Line numbers are the reference's Frame.cc.
#pragma once
#include "lidar_feat_dev.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace sqlm {

constexpr int kLcOffsets = 6;  // the distinct entries of :929-938, in their order of first appearance

struct LcParams {  // sqlm_lidar_corner_params as the kernels read it
  int32_t ncr, max_sharp, max_less;
  double curv_th, ground_z;
  uint8_t ring_enabled[SQLM_LF_MAX_ROWS];
};

// Device pointers of the corner stage of one call; cells and per-scan-point
// arrays are laid out as LfDev's ([n_rows][col_num]), regions are g = q * n_sub + j.
struct LcDev {
  LfDev f;  // the range image and the scans (sqlm_lidar_feat.hip made them)
  LcParams p;
  int32_t *state = nullptr;       // [n_rows][col_num] cell state
  uint8_t *edge = nullptr;        // [n_rows][col_num] edge mask
  float *angle = nullptr;         // [n_rows][col_num][6] or null: not stored
  uint8_t *mask = nullptr, *reason = nullptr;
  float *curv = nullptr;
  int32_t *sorted = nullptr;      // ascending rank
  int32_t *cand = nullptr;        // at row start + sp + t: the t-th statically passing candidate, highest rank first
  int32_t *cand_n = nullptr;      // [regions]
  int32_t *queue = nullptr;       // [n_rows][col_num] one BFS queue of cells per sweep
  int32_t *ord = nullptr, *label = nullptr;  // of a picked scan point
  int32_t *region_cnt = nullptr;
  int64_t *region_less = nullptr, *region_sharp = nullptr;
  int32_t *stats = nullptr;  // seeds, labelled, unstable, largest segment, most levels, less-sharp, sharp
  int64_t *sharp_off = nullptr, *less_off = nullptr;
  float *sharp_xyz = nullptr, *less_xyz = nullptr;
  int32_t *less_label = nullptr, *less_rc = nullptr;
};

#if defined(__HIPCC__)
// The first stages of sqlm_lidar_feat.hip (range image, scans, flat ring mask),
// then its flat stages; each returns how many kernels it launched.
int launch_lidar_feat_image(const LfDev &d, hipStream_t st);
int launch_lidar_feat_flat(const LfDev &d, hipStream_t st);
// The corner stages, after the image.
int launch_lidar_corner(const LcDev &d, hipStream_t st);
// The edge kernel alone, storing d.angle.
int launch_lidar_corner_angles(const LcDev &d, hipStream_t st);
#endif

SQLM_HD inline float lc_quiet_nan() {
  union {
    uint32_t u;
    float f;
  } b;
  b.u = 0x7fc00000u;
  return b.f;
}

// :596-601 / :618-623 for the final occupant of an occupied cell
SQLM_HD inline int lc_initial_state(const float *p, double ground_z) { return (double)p[2] < ground_z ? -1 : 0; }

// The third rule of PrepareRing_corner :686-692 for scan point i (i - 1 and i + 1 exist)
SQLM_HD inline bool lc_mask_rule3(const float *scan, int i) {
  const float *pc = scan + 3 * (int64_t)i;
  const float dn = lf_sqdiff(pc, pc + 3), dp = lf_sqdiff(pc, pc - 3);
  const float dis2 = pc[0] * pc[0] + pc[1] * pc[1] + pc[2] * pc[2];
  return (double)dn > 0.0002 * (double)dis2 && (double)dp > 0.0002 * (double)dis2;
}

// PrepareSubregion_corner :766-780 for scan point i (c <= i < size - c)
SQLM_HD inline float lc_curvature(const float *scan, int i, int c) {
  const float *p = scan + 3 * (int64_t)i;
  const int nn = 2 * c;
  float dx = (float)(-nn) * p[0], dy = (float)(-nn) * p[1], dz = (float)(-nn) * p[2];
  for (int j = 1; j <= c; ++j) {
    const float *a = p + 3 * (int64_t)j, *b = p - 3 * (int64_t)j;
    dx += a[0] + b[0];
    dy += a[1] + b[1];
    dz += a[2] + b[2];
  }
  return (dx * dx + dy * dy + dz * dz) / (float)nn;
}

// :966-973: the angle of the edge predicate, symmetric in p1 and p2 bit for bit
SQLM_HD inline float lc_angle(const float *p1, const float *p2) {
  const double x1 = (double)p1[0], y1 = (double)p1[1], z1 = (double)p1[2];
  const double x2 = (double)p2[0], y2 = (double)p2[1], z2 = (double)p2[2];
  const double n1 = sqrt((x1 * x1 + y1 * y1) + z1 * z1), n2 = sqrt((x2 * x2 + y2 * y2) + z2 * z2);
  const double dot = (x1 * x2 + y1 * y2) + z1 * z2;
  const float d1 = (float)(n1 > n2 ? n1 : n2), d2 = (float)(n1 > n2 ? n2 : n1);
  const float alpha = (float)sqlm_acos(dot / (n1 * n2));
  const float sa = (float)sqlm_sin((double)alpha), ca = (float)sqlm_cos((double)alpha);
  const float ys = d2 * sa, xs = d1 - d2 * ca;
  return (float)sqlm_atan2((double)ys, (double)xs);
}
SQLM_HD inline bool lc_is_edge(float angle) { return angle > 1.0f; }

// Offset k of :929-938 from (row, col): the target cell's row and column, false = none
SQLM_HD inline bool lc_target(int k, int row, int col, int row_num, int col_num, int *tr, int *tc) {
  const int dr = k == 0 || k == 4 ? -1 : (k == 1 || k == 5 ? 1 : 0);
  const int dc = k == 3 ? 1 : (k < 2 ? 0 : -1);
  const int r = row + dr;
  if (r < 0 || r >= row_num) return false;
  int c = col + dc;
  if (c < 0) c = col_num - 1;
  if (c >= col_num) c = 0;
  *tr = r;
  *tc = c;
  return true;
}

// occupied and not ground: true of a cell before the walk exactly when it is after it
SQLM_HD inline bool lc_live(int32_t state) { return state != -3 && state != -1; }

// The edge mask of cell (row, col) of one sweep; `state` is the sweep's cell
// state, before or after the walk; `angle` (6 floats) may be null
SQLM_HD inline uint32_t lc_edges(const LfView &v, const int32_t *state, int row, int col, float *angle) {
  uint32_t bits = 0;
  const int64_t cell = (int64_t)row * v.col_num + col;
  const bool own = lc_live(state[cell]);
  const float *p1 = v.scan_xyz + 3 * ((int64_t)row * v.col_num + (own ? v.image_index[cell] : 0));
  for (int k = 0; k < kLcOffsets; ++k) {
    float a = lc_quiet_nan();
    int tr, tc;
    if (own && lc_target(k, row, col, v.row_num, v.col_num, &tr, &tc)) {
      const int64_t t = (int64_t)tr * v.col_num + tc;
      if (lc_live(state[t])) {
        a = lc_angle(p1, v.scan_xyz + 3 * ((int64_t)tr * v.col_num + v.image_index[t]));
        if (lc_is_edge(a)) bits |= 1u << k;
        if (a != a) a = lc_quiet_nan();  // one NaN for every producer
      }
    }
    if (angle) angle[k] = a;
  }
  return bits;
}

}  // namespace sqlm
