// lidar_feat_dev.h — the arithmetic of the LiDAR flat-feature extraction
// (sqlm_lidar_features, include/sqrtlm.h), written once for the kernels
// (sqlm_lidar_feat.hip) and for the host twin (sqlm_lidar_features_host, the
// same text compiled for the CPU), and the launch interface between
// sqlm_lidar_feat.cpp and the kernels. Both translation units are built with
// -ffp-contract=off: every result comes from IEEE float / double operations in
// the order written here; atan / atan2 are sqlm_libm.h's.
//
// Every function restates a piece of the reference's Frame.cc with C++'s usual
// arithmetic conversions; the line numbers are that file's.
#pragma once
#include <cstdint>

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

#include "../../include/sqlm_libm.h"
#include "../../include/sqrtlm.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace sqlm {

constexpr double kLfPi = 3.14159265358979323846;  // M_PI
constexpr int kLfScans = 64;                       // N_SCANS of CalculateRingAndTime
constexpr int kLfMaxHalf = SQLM_LF_MAX_HALF_WIDTH;
constexpr int kLfMaxNear = 3 * (2 * kLfMaxHalf + 1);
constexpr double kLfPivotTol2 = 1e-24;  // a pivot column's squared norm against the largest initial one
constexpr int kLfBlock = 256;           // lanes of every workgroup but the emit kernel's
constexpr uint32_t kLfNoIndex = 0xffffffffu;

struct LfParams {  // sqlm_lidar_feat_params as the kernels read it
  int32_t row_num, col_num, n_sub, ncr, min_scan;  // min_scan: a processed row has more scan points than this
  int32_t max_flat, max_less;
  double curv_th, max_sq_dis, deg_diff;
  uint8_t ring_enabled[SQLM_LF_MAX_ROWS];
};

// Device pointers of one call. Rows are q = sweep * row_num + ring; every
// per-scan-point array is [n_rows][col_num] (a row's scan has at most col_num
// points), regions are g = q * n_sub + j.
struct LfDev {
  LfParams p;
  int32_t n_sweep = 0, n_rows = 0, has_ext = 0;
  int64_t n = 0;
  double ext[12];
  const int64_t *sweep_off = nullptr;
  const float *xyz = nullptr;
  int32_t *ring = nullptr;
  float *azi = nullptr;
  uint32_t *sweep_first = nullptr, *sweep_half = nullptr;  // kLfNoIndex = none
  int32_t *sweep_last = nullptr;                           // -1 = none
  unsigned long long *cell_key = nullptr;                  // (distance bits, index), all ones = unoccupied
  uint32_t *cell_first = nullptr;
  int32_t *image_index = nullptr, *scan_n = nullptr, *scan_src = nullptr, *scan_col = nullptr;
  float *scan_xyz = nullptr, *curv = nullptr, *normal = nullptr;
  uint8_t *mask = nullptr, *reason = nullptr;
  int32_t *nbr = nullptr, *sorted = nullptr, *ord = nullptr;
  int32_t *region_cnt = nullptr;
  int64_t *region_less = nullptr, *region_flat = nullptr;  // a region's first output slot
  int32_t *stats = nullptr;                                // largest region, candidates, evaluated, picked
  int64_t *flat_off = nullptr, *less_off = nullptr;
  float *flat_xyz = nullptr, *flat_normal = nullptr, *less_xyz = nullptr, *less_normal = nullptr;
  int32_t *less_rc = nullptr;
};

SQLM_HD inline uint32_t lf_bits(float v) {
  union {
    float f;
    uint32_t u;
  } b;
  b.f = v;
  return b.u;
}
SQLM_HD inline bool lf_finite(float v) { return (lf_bits(v) & 0x7f800000u) != 0x7f800000u; }
SQLM_HD inline float lf_sqrtf(float v) { return (float)sqrt((double)v); }
SQLM_HD inline float lf_atanf(float v) { return (float)sqlm_atan((double)v); }
SQLM_HD inline float lf_atan2f(float y, float x) { return (float)sqlm_atan2((double)y, (double)x); }

// CalculateRingAndTime :516-532; -1 = dropped
SQLM_HD inline int lf_ring(float x, float y, float z) {
  const float s = lf_sqrtf(x * x + y * y);
  const float t = lf_atanf(z / s) * 180.0f;
  const float ang = (float)((double)t / kLfPi);
  if (ang != ang) return -1;
  int id;
  if ((double)ang >= -8.83)
    id = (int)((double)(2.0f - ang) * 3.0 + 0.5);
  else
    id = kLfScans / 2 + (int)((-8.83 - (double)ang) * 2.0 + 0.5);
  return (id > kLfScans - 1 || id < 0) ? -1 : id;
}

// PointToImage :551-558 from the raw azimuths -atan2f(y, x) of the first and last kept point
SQLM_HD inline void lf_oris(float azi_first, float azi_last, float *start, float *end) {
  const float s = (float)((double)azi_first + kLfPi);
  float e = (float)((double)azi_last + 3.0 * kLfPi);
  const float d = e - s;
  if ((double)d > 3.0 * kLfPi)
    e = (float)((double)e - 2.0 * kLfPi);
  else if ((double)d < kLfPi)
    e = (float)((double)e + 2.0 * kLfPi);
  *start = s;
  *end = e;
}

// :568-572, the branch of a point met before halfPassed
SQLM_HD inline float lf_unpassed(float azi, float start) {
  if ((double)azi < (double)start - kLfPi / 2.0) return (float)((double)azi + 2.0 * kLfPi);
  if ((double)azi > (double)start + kLfPi * 3.0 / 2.0) return (float)((double)azi - 2.0 * kLfPi);
  return azi;
}
SQLM_HD inline bool lf_turns_half(float a, float start) { return (double)(a - start) > kLfPi; }

// :577-582, the branch after halfPassed
SQLM_HD inline float lf_passed(float azi, float end) {
  const float a = (float)((double)azi + 2.0 * kLfPi);
  if ((double)a < (double)end - kLfPi * 3.0 / 2.0) return (float)((double)a + 2.0 * kLfPi);
  if ((double)a > (double)end + kLfPi / 2.0) return (float)((double)a - 2.0 * kLfPi);
  return a;
}

// :585-592; -1 = no cell
SQLM_HD inline int lf_col(float a, float start, int col_num) {
  const float rel = a - start;
  const double t = (double)rel / (2.0 * kLfPi) * (double)col_num;
  if (!(t > -2147483000.0 && t < 2147483000.0 - (double)col_num)) return -1;
  const int col = ((int)t + col_num) % col_num;
  return (col < 0 || col >= col_num) ? -1 : col;
}

SQLM_HD inline float lf_dist(const float *p) { return lf_sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]); }
SQLM_HD inline float lf_sqdiff(const float *a, const float *b) {
  const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
  return dx * dx + dy * dy + dz * dz;
}
SQLM_HD inline float lf_sqdiff_w(const float *a, const float *b, float wb) {
  const float dx = a[0] - b[0] * wb, dy = a[1] - b[1] * wb, dz = a[2] - b[2] * wb;
  return dx * dx + dy * dy + dz * dz;
}

// PrepareRing_flat :710-736 for scan point i (i + 1 exists): 0 = writes nothing,
// 1 = masks [i - c, i], 2 = masks [i + 1, i + c]
SQLM_HD inline int lf_mask_rule(const float *scan, int i) {
  const float *pc = scan + 3 * (int64_t)i, *pn = pc + 3;
  const float d2 = lf_sqdiff(pc, pn);
  if ((double)d2 > 0.1) {
    const float depth = lf_dist(pc), dn = lf_dist(pn);
    if (depth > dn) {
      const float wd = lf_sqrtf(lf_sqdiff_w(pn, pc, dn / depth)) / dn;
      if ((double)wd < 0.1) return 1;
    } else {
      const float wd = lf_sqrtf(lf_sqdiff_w(pc, pn, depth / dn)) / depth;
      if ((double)wd < 0.1) return 2;
    }
  }
  return 0;
}

// PrepareSubregion_flat :808-826 for scan point i of a scan of `size` points
// (ncr <= i < size - ncr); *nbr = the half-width used
SQLM_HD inline float lf_curvature(const float *scan, int i, int size, int ncr, int *nbr) {
  const float *p = scan + 3 * (int64_t)i;
  const double q = 25.0 / (double)lf_dist(p) + 0.5;
  int n = ncr;
  if (q < 1073741824.0) {
    n = (int)q + 1;
    if (i < n || (int64_t)i + n >= size) n = ncr;
  }
  const int nn = 2 * n;
  float dx = (float)(-nn) * p[0], dy = (float)(-nn) * p[1], dz = (float)(-nn) * p[2];
  for (int j = 1; j <= n; ++j) {
    const float *a = p + 3 * (int64_t)j, *b = p - 3 * (int64_t)j;
    dx += a[0] + b[0];
    dy += a[1] + b[1];
    dz += a[2] + b[2];
  }
  *nbr = n;
  return (dx * dx + dy * dy + dz * dz) / (float)nn;
}

// :1053-1056
SQLM_HD inline void lf_region(int size, int ncr, int n_sub, int j, int64_t *sp, int64_t *ep) {
  *sp = ((int64_t)ncr * (n_sub - j) + (int64_t)(size - ncr) * j) / n_sub;
  *ep = ((int64_t)ncr * (n_sub - 1 - j) + (int64_t)(size - ncr) * (j + 1)) / n_sub - 1;
}

// The least-squares solution of A x = b by the column-pivoted Householder QR
// the header defines; A [m][3] and b [m] are overwritten. false = degenerate.
SQLM_HD inline bool lf_qr_solve(double (*A)[3], double *b, int m, double x[3]) {
  int perm[3] = {0, 1, 2};
  double max0 = 0.0;
  for (int k = 0; k < 3; ++k) {
    double nrm[3] = {0.0, 0.0, 0.0};
    for (int j = k; j < 3; ++j) {
      double s = 0.0;
      for (int r = k; r < m; ++r) s += A[r][j] * A[r][j];
      nrm[j] = s;
    }
    if (k == 0) {
      max0 = nrm[0];
      if (nrm[1] > max0) max0 = nrm[1];
      if (nrm[2] > max0) max0 = nrm[2];
    }
    int best = k;
    for (int j = k + 1; j < 3; ++j)
      if (nrm[j] > nrm[best]) best = j;
    if (!(nrm[best] > kLfPivotTol2 * max0)) return false;
    if (best != k) {
      for (int r = 0; r < m; ++r) {
        const double t = A[r][k];
        A[r][k] = A[r][best];
        A[r][best] = t;
      }
      const int t = perm[k];
      perm[k] = perm[best];
      perm[best] = t;
    }
    const double alpha = A[k][k];
    const double nx = sqrt(nrm[best]);
    const double beta = alpha >= 0.0 ? -nx : nx;
    const double v0 = alpha - beta, tau = (beta - alpha) / beta;
    for (int r = k + 1; r < m; ++r) A[r][k] = A[r][k] / v0;
    for (int j = k + 1; j < 4; ++j) {
      double w = j < 3 ? A[k][j] : b[k];
      for (int r = k + 1; r < m; ++r) w += A[r][k] * (j < 3 ? A[r][j] : b[r]);
      w = tau * w;
      if (j < 3) {
        A[k][j] -= w;
        for (int r = k + 1; r < m; ++r) A[r][j] -= A[r][k] * w;
      } else {
        b[k] -= w;
        for (int r = k + 1; r < m; ++r) b[r] -= A[r][k] * w;
      }
    }
    A[k][k] = beta;
  }
  const double x2 = b[2] / A[2][2];
  const double x1 = (b[1] - A[1][2] * x2) / A[1][1];
  const double x0 = ((b[0] - A[0][1] * x1) - A[0][2] * x2) / A[0][0];
  x[perm[0]] = x0;
  x[perm[1]] = x1;
  x[perm[2]] = x2;
  return true;
}

// One sweep's range image and scans as a candidate reads them
struct LfView {
  const int32_t *image_index;  // [row_num][col_num]
  const float *scan_xyz;       // [row_num][col_num][3]
  const int32_t *scan_col;     // [row_num][col_num]
  int32_t row_num, col_num;
};

SQLM_HD inline void lf_visit(const LfView &v, int row, int col, const float *P, double max_sq_dis, int *n_search,
                             double (*A)[3], int *m) {
  const int idx = v.image_index[(int64_t)row * v.col_num + col];
  if (idx < 0) return;
  ++*n_search;
  const float *q = v.scan_xyz + 3 * ((int64_t)row * v.col_num + idx);
  if ((double)lf_sqdiff(P, q) < max_sq_dis && *m < kLfMaxNear) {
    A[*m][0] = (double)q[0];
    A[*m][1] = (double)q[1];
    A[*m][2] = (double)q[2];
    ++*m;
  }
}

SQLM_HD inline void lf_visit_row(const LfView &v, int row, int col, int cw, bool centre, const float *P,
                                 double max_sq_dis, int *n_search, double (*A)[3], int *m) {
  if (centre) lf_visit(v, row, col, P, max_sq_dis, n_search, A, m);
  for (int c = 1; c <= cw; ++c) {
    if (col + c < v.col_num) lf_visit(v, row, col + c, P, max_sq_dis, n_search, A, m);
    if (col >= c) lf_visit(v, row, col - c, P, max_sq_dis, n_search, A, m);
  }
}

// ExtractFeaturePoints :1080-1214 for the unmasked, flat-enough scan point idx
// of row `row`: SQLM_LF_FEW_SEARCH / DEGENERATE / PLANE_INVALID, or
// SQLM_LF_PICKED for a valid plane with its float normal.
SQLM_HD inline int lf_candidate(const LfView &v, const LfParams &p, int row, int idx, float normal[3]) {
  const float *P = v.scan_xyz + 3 * ((int64_t)row * v.col_num + idx);
  const int col = v.scan_col[(int64_t)row * v.col_num + idx];
  const double d = (double)lf_dist(P);
  const double q = d * 0.01 / (p.deg_diff / 180.0 * kLfPi * d) + 0.5;
  const int cw = q != q ? 0 : (q >= (double)(kLfMaxHalf + 1) ? kLfMaxHalf : (int)q);
  double A[kLfMaxNear][3], b[kLfMaxNear];
  int n_search = 1, m = 0;
  if (0.0 < p.max_sq_dis) {  // the point itself, :1088
    A[0][0] = (double)P[0];
    A[0][1] = (double)P[1];
    A[0][2] = (double)P[2];
    m = 1;
  }
  lf_visit_row(v, row, col, cw, false, P, p.max_sq_dis, &n_search, A, &m);
  if (row > 0) lf_visit_row(v, row - 1, col, cw, true, P, p.max_sq_dis, &n_search, A, &m);
  if (row + 1 < v.row_num) lf_visit_row(v, row + 1, col, cw, true, P, p.max_sq_dis, &n_search, A, &m);
  if (n_search < 5) return SQLM_LF_FEW_SEARCH;
  if (m < 3) return SQLM_LF_DEGENERATE;
  double pts[kLfMaxNear][3];
  for (int s = 0; s < m; ++s) {
    pts[s][0] = A[s][0];
    pts[s][1] = A[s][1];
    pts[s][2] = A[s][2];
    b[s] = -1.0;
  }
  double x[3];
  if (!lf_qr_solve(A, b, m, x)) return SQLM_LF_DEGENERATE;
  const double nrm = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
  const double d0 = 1.0 / nrm;
  const double n0 = x[0] / nrm, n1 = x[1] / nrm, n2 = x[2] / nrm;
  for (int s = 0; s < m; ++s) {
    const double r = n0 * pts[s][0] + n1 * pts[s][1] + n2 * pts[s][2] + d0;
    if ((r < 0.0 ? -r : r) > 0.1) return SQLM_LF_PLANE_INVALID;
  }
  normal[0] = (float)n0;
  normal[1] = (float)n1;
  normal[2] = (float)n2;
  return SQLM_LF_PICKED;
}

// pcl::transformPointCloud as sqlm_lidar_associate defines it; ext = the top three rows
SQLM_HD inline void lf_transform(const double *ext, const float *p, float *out) {
  for (int k = 0; k < 3; ++k) {
    const double *m = ext + 4 * k;
    out[k] = (float)(((m[0] * (double)p[0] + m[1] * (double)p[1]) + m[2] * (double)p[2]) + m[3]);
  }
}

#if defined(__HIPCC__)
// Device helpers the kernels of sqlm_lidar_feat.hip and sqlm_lidar_corner.hip share
// ascending bitonic sort of key[0 .. npow) by the whole workgroup; npow a power of two
__device__ __forceinline__ void lf_sort(unsigned long long *key, int npow) {
  for (int k = 2; k <= npow; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < npow; i += kLfBlock) {
        const int l = i ^ j;
        if (l > i) {
          const unsigned long long a = key[i], b = key[l];
          if ((a > b) == ((i & k) == 0)) {
            key[i] = b;
            key[l] = a;
          }
        }
      }
      __syncthreads();
    }
  }
}

__device__ __forceinline__ int lf_pow2(int n) {
  int p = 2;
  while (p < n) p <<= 1;
  return p;
}

__device__ __forceinline__ void lf_put(const LfDev &d, const float *p, float *out) {
  if (d.has_ext) {
    lf_transform(d.ext, p, out);
  } else {
    out[0] = p[0];
    out[1] = p[1];
    out[2] = p[2];
  }
}
#endif

}  // namespace sqlm
