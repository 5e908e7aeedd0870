// mappoint_dev.h — the arithmetic of LocalMapping's map-point steps, written
// once for the kernels (sqlm_mappoint.hip) and for the host twins
// (sqlm_triangulate_pairs_host / sqlm_map_points_update_host, the same text
// compiled for the CPU). Both translation units are built with
// -ffp-contract=off: every result comes from IEEE float / double operations
// (+ - * / sqrt and conversions) in the order written here; no libm function is
// called.
//
// tri_match: one match of LocalMapping::CreateNewMapPoints
// (src/backend/LocalMapping.cc:436-624 of the reference), monocular branch.
// The cv::Mat expressions are restated as sqlm_orb.hip restates them (a second
// copy of its small helpers: those are host functions of that translation
// unit): a 3x3 * 3x1 product is a float dot left to right, Mat::dot and
// cv::norm sum in double, Mat / s is a float scale by (float)(1 / s).
// cv::SVD::compute of the 4x4 A is the library's own definition:
// a one-sided Jacobi SVD in double on the columns of A.
//
// mp_row_median / mp_normal_depth: MapPoint::ComputeDistinctiveDescriptors and
// UpdateNormalAndDepth (src/data_structure/MapPoint.cc:382-481, :531-578).
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

#pragma clang fp contract(off)

namespace sqlm {

constexpr int kTriSweeps = 13;         // one-sided Jacobi sweeps of the 4x4 A (measured: DESIGN.md 8h)
constexpr double kTriOrthTol = 1e-15;  // |a_p . a_q| <= tol * |a_p| |a_q|: the two columns count as orthogonal
constexpr int kTriBlock = 256;         // lanes (matches) of a k_triangulate workgroup
constexpr int kMpLdsMax = 128;         // observations of a point whose descriptors k_mp_descriptor keeps in LDS
constexpr int kMpNormalBlock = 256;    // lanes (points) of a k_mp_normal workgroup

// reason codes of a match (include/sqrtlm_orb.h)
enum : uint8_t {
  kTriCreated = 0, kTriParallax = 1, kTriWZero = 2, kTriZ1 = 3, kTriZ2 = 4, kTriReproj1 = 5, kTriReproj2 = 6,
  kTriZeroDist = 7, kTriScale = 8
};

struct TriPair {      // one keyframe pair as the kernel reads it
  float T1[12], T2[12];  // Tcw of both keyframes, 3x4 row-major
  float cam1[6], cam2[6];  // fx fy cx cy invfx invfy
  float Ow1[3], Ow2[3];  // GetCameraCenter() = -Rcw.t() * tcw (KeyFrame::SetPose)
  float ratio_factor;
  int32_t pad;
};

struct TriMatch {     // one match, gathered by the host after its range checks
  float x1, y1, x2, y2;  // mvKeysUn[idx].pt of both keypoints
  float sig1, sig2;      // mvLevelSigma2[octave]
  float sf1, sf2;        // mvScaleFactors[octave]
};

namespace mp_detail {

// -Rcw.t() * tcw: the float dot left to right, negated (alpha = -1 in double is exact)
SQLM_HD inline void center(const float *T, float *Ow) {
  for (int i = 0; i < 3; ++i) {
    const float t0 = T[i] * T[3] + T[4 + i] * T[7] + T[8 + i] * T[11];
    Ow[i] = -t0;
  }
}

SQLM_HD inline double dot3d(const float *a, const float *b) {
  double s = 0;
  s += (double)a[0] * (double)b[0];
  s += (double)a[1] * (double)b[1];
  s += (double)a[2] * (double)b[2];
  return s;
}

// cv::norm of a 3x1 CV_32F as a double
SQLM_HD inline double norm3d(const float *v) { return __builtin_sqrt(dot3d(v, v)); }

// Rcw.row(r).dot(x3Dt) + tcw(r), rounded to float
SQLM_HD inline float row_dot(const float *T, int r, const float *x) {
  return (float)(dot3d(T + 4 * r, x) + (double)T[4 * r + 3]);
}

SQLM_HD inline double absd(double x) { return x < 0 ? -x : x; }

// squared reprojection error of x3D in one keyframe (:543-556), z > 0 given
SQLM_HD inline float reproj2(const float *T, const float *cam, const float *x3D, float z, float kx, float ky) {
  const float x = row_dot(T, 0, x3D), y = row_dot(T, 1, x3D);
  const float invz = (float)(1.0 / (double)z);
  const float u = cam[0] * x * invz + cam[2], v = cam[1] * y * invz + cam[3];
  const float ex = u - kx, ey = v - ky;
  return ex * ex + ey * ey;
}

}  // namespace mp_detail

SQLM_HD inline void tri_pair_finish(TriPair &p) {
  mp_detail::center(p.T1, p.Ow1);
  mp_detail::center(p.T2, p.Ow2);
}

// The right singular vector of the smallest singular value of the 4x4 float A
// (row-major), rounded to float: vt.row(3) up to its sign. One-sided Jacobi in
// double: the column pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) are rotated in
// that order, `sweeps` times, a pair that is orthogonal to kTriOrthTol skipped;
// the rotations' product is V. The column of smallest squared norm wins, the
// highest of equals.
SQLM_HD inline void tri_null_vector(const float *A, int sweeps, float *x4) {
  double W[16], V[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    W[k] = (double)A[k];
    V[k] = (k % 5 == 0) ? 1.0 : 0.0;
  }
#pragma unroll 1
  for (int sweep = 0; sweep < sweeps; ++sweep) {
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        const double al = W[p] * W[p] + W[4 + p] * W[4 + p] + W[8 + p] * W[8 + p] + W[12 + p] * W[12 + p];
        const double be = W[q] * W[q] + W[4 + q] * W[4 + q] + W[8 + q] * W[8 + q] + W[12 + q] * W[12 + q];
        const double ga = W[p] * W[q] + W[4 + p] * W[4 + q] + W[8 + p] * W[8 + q] + W[12 + p] * W[12 + q];
        if (!(mp_detail::absd(ga) <= kTriOrthTol * __builtin_sqrt(al * be))) {
          const double zeta = (be - al) / (ga + ga);
          const double az = mp_detail::absd(zeta);
          double t = 1.0 / (az + __builtin_sqrt(zeta * zeta + 1.0));
          if (zeta < 0) t = -t;
          const double c = 1.0 / __builtin_sqrt(t * t + 1.0);
          const double s = t * c;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const double wp = W[4 * r + p], wq = W[4 * r + q];
            W[4 * r + p] = c * wp - s * wq;
            W[4 * r + q] = s * wp + c * wq;
            const double vp = V[4 * r + p], vq = V[4 * r + q];
            V[4 * r + p] = c * vp - s * vq;
            V[4 * r + q] = s * vp + c * vq;
          }
        }
      }
    }
  }
  double n2[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) n2[k] = W[k] * W[k] + W[4 + k] * W[4 + k] + W[8 + k] * W[8 + k] + W[12 + k] * W[12 + k];
  double best = n2[0];
  int m = 0;
#pragma unroll
  for (int k = 1; k < 4; ++k)
    if (n2[k] <= best) {
      best = n2[k];
      m = k;
    }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const double v = m == 0 ? V[4 * r] : m == 1 ? V[4 * r + 1] : m == 2 ? V[4 * r + 2] : V[4 * r + 3];
    x4[r] = (float)v;
  }
}

// One match of CreateNewMapPoints (:436-624). Returns the reason code; x3D is
// the triangulated point for reasons 0 and 3 to 8 and zero otherwise. Every
// test after the parallax test is written in its accepting form, so an
// unordered (NaN) comparison rejects the match; for ordered values each is the
// reference's test.
SQLM_HD inline uint8_t tri_match(const TriPair &P, const TriMatch &m, int sweeps, float *x3D) {
  using namespace mp_detail;
  x3D[0] = x3D[1] = x3D[2] = 0.f;
  const float xn1[3] = {(m.x1 - P.cam1[2]) * P.cam1[4], (m.y1 - P.cam1[3]) * P.cam1[5], 1.0f};  // :461-462
  const float xn2[3] = {(m.x2 - P.cam2[2]) * P.cam2[4], (m.y2 - P.cam2[3]) * P.cam2[5], 1.0f};
  float ray1[3], ray2[3];  // Rwc * xn (:465-466)
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    ray1[i] = P.T1[i] * xn1[0] + P.T1[4 + i] * xn1[1] + P.T1[8 + i] * xn1[2];
    ray2[i] = P.T2[i] * xn2[0] + P.T2[4 + i] * xn2[1] + P.T2[8 + i] * xn2[2];
  }
  const float cosr = (float)(dot3d(ray1, ray2) / (norm3d(ray1) * norm3d(ray2)));  // :468
  const float cosst = cosr + 1.0f;                                                // :471, no stereo keypoint
  if (!(cosr < cosst && cosr > 0 && (double)cosr < 0.9998)) return kTriParallax;  // :496
  float A[16];  // :500-504
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    A[j] = xn1[0] * P.T1[8 + j] - P.T1[j];
    A[4 + j] = xn1[1] * P.T1[8 + j] - P.T1[4 + j];
    A[8 + j] = xn2[0] * P.T2[8 + j] - P.T2[j];
    A[12 + j] = xn2[1] * P.T2[8 + j] - P.T2[4 + j];
  }
  float x4[4];
  tri_null_vector(A, sweeps, x4);
  if (x4[3] == 0) return kTriWZero;  // :511
  const float inv = (float)(1.0 / (double)x4[3]);  // :514
  const float X[3] = {x4[0] * inv, x4[1] * inv, x4[2] * inv};
  x3D[0] = X[0];
  x3D[1] = X[1];
  x3D[2] = X[2];
  const float z1 = row_dot(P.T1, 2, X);  // :533
  if (!(z1 > 0)) return kTriZ1;
  const float z2 = row_dot(P.T2, 2, X);  // :537
  if (!(z2 > 0)) return kTriZ2;
  const float e1 = reproj2(P.T1, P.cam1, X, z1, m.x1, m.y1);
  if (!((double)e1 <= 5.991 * (double)m.sig1)) return kTriReproj1;  // :556
  const float e2 = reproj2(P.T2, P.cam2, X, z2, m.x2, m.y2);
  if (!((double)e2 <= 5.991 * (double)m.sig2)) return kTriReproj2;  // :586
  const float n1[3] = {X[0] - P.Ow1[0], X[1] - P.Ow1[1], X[2] - P.Ow1[2]};  // :605-609
  const float n2[3] = {X[0] - P.Ow2[0], X[1] - P.Ow2[1], X[2] - P.Ow2[2]};
  const float dist1 = (float)norm3d(n1), dist2 = (float)norm3d(n2);
  if (dist1 == 0 || dist2 == 0) return kTriZeroDist;  // :611
  const float ratioDist = dist2 / dist1;
  const float ratioOctave = m.sf1 / m.sf2;
  if (!(ratioDist * P.ratio_factor >= ratioOctave && ratioDist <= ratioOctave * P.ratio_factor)) return kTriScale;  // :623
  return kTriCreated;
}

// DescriptorDistance over the 256 bits of two descriptors held as 8 words
SQLM_HD inline int mp_hamming(const uint32_t *a, const uint32_t *b) {
  int d = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) d += __builtin_popcount(a[k] ^ b[k]);
  return d;
}

// The element at index (size_t)(0.5 * (N - 1)) of the ascending row of
// distances from descriptor `a` to the N descriptors D (a's own among them):
// the smallest v with at least that index + 1 distances <= v, found by
// bisection over 0..256 in nine counting passes. Exact, and no row is stored.
SQLM_HD inline int mp_row_median(const uint32_t *a, const uint32_t *D, int N) {
  const int need = (N - 1) / 2 + 1;
  int lo = 0, hi = 256;
#pragma unroll 1
  for (int it = 0; it < 9; ++it) {
    const int mid = (lo + hi) >> 1;
    int cnt = 0;
#pragma unroll 1
    for (int j = 0; j < N; ++j) cnt += mp_hamming(a, D + 8 * (int64_t)j) <= mid ? 1 : 0;
    if (cnt >= need)
      hi = mid;
    else
      lo = mid + 1;
  }
  return hi;
}

// UpdateNormalAndDepth (:554-576) of one point over its n camera centres in list order.
// out = normal[3], max_dist, min_dist; n = 0 (the reference returns early) gives zeros.
SQLM_HD inline void mp_normal_depth(const float *pos, const float *centers, int64_t n, const float *ref_center,
                                    float level_scale, float max_scale, float *normal, float *max_dist,
                                    float *min_dist) {
  using namespace mp_detail;
  float acc[3] = {0.f, 0.f, 0.f};
  if (n <= 0) {
    normal[0] = normal[1] = normal[2] = 0.f;
    *max_dist = *min_dist = 0.f;
    return;
  }
#pragma unroll 1
  for (int64_t i = 0; i < n; ++i) {
    const float *O = centers + 3 * i;
    const float d[3] = {pos[0] - O[0], pos[1] - O[1], pos[2] - O[2]};
    const float inv = (float)(1.0 / norm3d(d));
    acc[0] = acc[0] + d[0] * inv;
    acc[1] = acc[1] + d[1] * inv;
    acc[2] = acc[2] + d[2] * inv;
  }
  const float pc[3] = {pos[0] - ref_center[0], pos[1] - ref_center[1], pos[2] - ref_center[2]};
  const float dist = (float)norm3d(pc);
  const float mx = dist * level_scale;
  *max_dist = mx;
  *min_dist = mx / max_scale;
  const float invn = (float)(1.0 / (double)n);
  normal[0] = acc[0] * invn;
  normal[1] = acc[1] * invn;
  normal[2] = acc[2] * invn;
}

}  // namespace sqlm
