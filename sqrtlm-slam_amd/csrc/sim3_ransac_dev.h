// sim3_ransac_dev.h — the arithmetic of one Sim3 RANSAC hypothesis
// (Sim3Solver::ComputeSim3 and CheckInliers, src/algorithm/Sim3Solver.cc
// :319-490 of the reference), written once for the kernel (sqlm_sim3_ransac.hip)
// and for the host (sqlm_sim3_ransac_hypothesis_host, the same text compiled
// for the CPU). Both translation units are built with -ffp-contract=off: every
// result comes from IEEE operations in the order written here.
//
// The rule (tests/sim3_ransac_ref.py is its numpy statement): a float
// operation written out in the source is that float operation; where the
// source hands arithmetic to OpenCV (reduce, matrix products, scaling by a
// scalar, dot, norm) products and sums accumulate in double in index order and
// round to float once per stored element. Step 4 deviates on purpose: the
// eigenvector comes from a cyclic Jacobi iteration in double with a fixed sweep
// count and rotation order, and R12 is the unit quaternion's rotation matrix.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SQLM_HD __host__ __device__
#else
#define SQLM_HD
#endif

#pragma clang fp contract(off)

namespace sqlm {

constexpr int kRansacSweeps = 8;  // Jacobi sweeps over the 6 off-diagonal pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)

struct RansacHyp {  // what a hypothesis stores, all float as in the reference
  float R[9], t[3], s;
  float sR[9], sRinv[9], tinv[3];  // T12 = [sR t], T21 = [sRinv tinv]
};
constexpr int kRansacHypFloats = sizeof(RansacHyp) / sizeof(float);  // 34

// The pair indices of three RandomInt draws from a freshly reset
// vAvailableIndices with swap-remove (:236-256): draw i is in [0, n-1-i].
SQLM_HD inline void ransac_indices(int n, const int32_t r[3], int32_t idx[3]) {
  idx[0] = r[0];
  idx[1] = r[1] == r[0] ? n - 1 : r[1];
  const int back1 = r[0] == n - 2 ? n - 1 : n - 2;  // what the second removal moves into slot r[1]
  idx[2] = r[2] == r[1] ? back1 : (r[2] == r[0] ? n - 1 : r[2]);
}

namespace ransac_detail {

// sum_k a[k] b[k] in double, k ascending
SQLM_HD inline double dot3(float a0, float a1, float a2, float b0, float b1, float b2) {
  return ((double)a0 * (double)b0 + (double)a1 * (double)b1) + (double)a2 * (double)b2;
}

// centroid and relative coordinates of the 3x3 P (column i = point i)
SQLM_HD inline void centroid(const float P[9], float Pr[9], float C[3]) {
  for (int r = 0; r < 3; ++r) {
    const float sum = (float)(((double)P[3 * r] + (double)P[3 * r + 1]) + (double)P[3 * r + 2]);
    C[r] = (float)((double)sum * (1.0 / 3.0));
    for (int i = 0; i < 3; ++i) Pr[3 * r + i] = P[3 * r + i] - C[r];
  }
}

}  // namespace ransac_detail

// Unit eigenvector (w x y z), w >= 0, of the largest eigenvalue of the
// symmetric 4x4 A (row-major, destroyed): cyclic Jacobi, kRansacSweeps sweeps.
// The double square root and division are the correctly rounded IEEE ones on
// both targets.
SQLM_HD inline void ransac_top_eigenvector(double A[16], double q[4]) {
  double V[16];
  for (int k = 0; k < 16; ++k) V[k] = (k % 5 == 0) ? 1.0 : 0.0;
#pragma unroll 1
  for (int sweep = 0; sweep < kRansacSweeps; ++sweep) {
    for (int p = 0; p < 3; ++p) {
      for (int qq = p + 1; qq < 4; ++qq) {
        const double apq = A[4 * p + qq];
        if (!(apq != 0.0)) continue;
        const double theta = (A[5 * qq] - A[5 * p]) / (apq + apq);
        const double at = theta < 0 ? -theta : theta;
        double t = 1.0 / (at + __builtin_sqrt(theta * theta + 1.0));
        if (theta < 0) t = -t;
        const double c = 1.0 / __builtin_sqrt(t * t + 1.0);
        const double s = t * c;
        const double app = A[5 * p] - t * apq, aqq = A[5 * qq] + t * apq;
        for (int r = 0; r < 4; ++r) {
          if (r == p || r == qq) continue;
          const double arp = A[4 * r + p], arq = A[4 * r + qq];
          const double np_ = c * arp - s * arq, nq_ = s * arp + c * arq;
          A[4 * r + p] = A[4 * p + r] = np_;
          A[4 * r + qq] = A[4 * qq + r] = nq_;
        }
        A[5 * p] = app;
        A[5 * qq] = aqq;
        A[4 * p + qq] = A[4 * qq + p] = 0.0;
        for (int r = 0; r < 4; ++r) {
          const double vrp = V[4 * r + p], vrq = V[4 * r + qq];
          V[4 * r + p] = c * vrp - s * vrq;
          V[4 * r + qq] = s * vrp + c * vrq;
        }
      }
    }
  }
  int best = 0;
  double lam = A[0];
  for (int k = 1; k < 4; ++k)
    if (A[5 * k] > lam) {
      lam = A[5 * k];
      best = k;
    }
  // a select per component, not a dynamically indexed read: V stays in registers
  double v[4];
  for (int r = 0; r < 4; ++r)
    v[r] = best == 0 ? V[4 * r] : best == 1 ? V[4 * r + 1] : best == 2 ? V[4 * r + 2] : V[4 * r + 3];
  const double nrm = __builtin_sqrt(((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + v[3] * v[3]);
  for (int r = 0; r < 4; ++r) v[r] = v[r] / nrm;
  const bool neg = v[0] < 0;
  for (int r = 0; r < 4; ++r) q[r] = neg ? -v[r] : v[r];
}

// ComputeSim3 on P1, P2 (3x3 row-major, column i = point i, camera 1 / 2)
SQLM_HD inline void ransac_closed_form(const float P1[9], const float P2[9], bool fix_scale, RansacHyp &h) {
  using namespace ransac_detail;
  float Pr1[9], Pr2[9], O1[3], O2[3];
  centroid(P1, Pr1, O1);
  centroid(P2, Pr2, O2);
  float M[9];  // Pr2 * Pr1^T
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      M[3 * i + j] = (float)dot3(Pr2[3 * i], Pr2[3 * i + 1], Pr2[3 * i + 2], Pr1[3 * j], Pr1[3 * j + 1], Pr1[3 * j + 2]);
  // float expressions, left to right, as the source writes them
  const float N11 = M[0] + M[4] + M[8];
  const float N12 = M[5] - M[7];
  const float N13 = M[6] - M[2];
  const float N14 = M[1] - M[3];
  const float N22 = M[0] - M[4] - M[8];
  const float N23 = M[1] + M[3];
  const float N24 = M[6] + M[2];
  const float N33 = -M[0] + M[4] - M[8];
  const float N34 = M[5] + M[7];
  const float N44 = -M[0] - M[4] + M[8];
  double A[16] = {N11, N12, N13, N14, N12, N22, N23, N24, N13, N23, N33, N34, N14, N24, N34, N44};
  double q[4];
  ransac_top_eigenvector(A, q);
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  h.R[0] = (float)(1.0 - 2.0 * (y * y + z * z));
  h.R[1] = (float)(2.0 * (x * y - w * z));
  h.R[2] = (float)(2.0 * (x * z + w * y));
  h.R[3] = (float)(2.0 * (x * y + w * z));
  h.R[4] = (float)(1.0 - 2.0 * (x * x + z * z));
  h.R[5] = (float)(2.0 * (y * z - w * x));
  h.R[6] = (float)(2.0 * (x * z - w * y));
  h.R[7] = (float)(2.0 * (y * z + w * x));
  h.R[8] = (float)(1.0 - 2.0 * (x * x + y * y));
  const float *R = h.R;
  float P3[9];  // R * Pr2
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      P3[3 * i + j] = (float)dot3(R[3 * i], R[3 * i + 1], R[3 * i + 2], Pr2[j], Pr2[3 + j], Pr2[6 + j]);
  if (!fix_scale) {
    double nom = 0.0, den = 0.0;
    for (int k = 0; k < 9; ++k) {
      nom = nom + (double)Pr1[k] * (double)P3[k];
      den = den + (double)(P3[k] * P3[k]);
    }
    h.s = (float)(nom / den);
  } else {
    h.s = 1.0f;
  }
  const double s = (double)h.s;
  for (int i = 0; i < 3; ++i)
    h.t[i] = (float)((double)O1[i] - s * dot3(R[3 * i], R[3 * i + 1], R[3 * i + 2], O2[0], O2[1], O2[2]));
  const double inv_s = 1.0 / s;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      h.sR[3 * i + j] = (float)(s * (double)R[3 * i + j]);
      h.sRinv[3 * i + j] = (float)(inv_s * (double)R[3 * j + i]);
    }
  for (int i = 0; i < 3; ++i)
    h.tinv[i] = (float)(-dot3(h.sRinv[3 * i], h.sRinv[3 * i + 1], h.sRinv[3 * i + 2], h.t[0], h.t[1], h.t[2]));
}

// (fx x + cx, fy y + cy) of a camera-frame point: FromCameraToImage / the tail of Project (:533-537)
SQLM_HD inline void ransac_image(const float P[3], const float K[4], float uv[2]) {
  const float invz = 1 / P[2];
  const float x = P[0] * invz;
  const float y = P[1] * invz;
  uv[0] = K[0] * x + K[2];
  uv[1] = K[1] * y + K[3];
}

// Rcw * X + tcw of Project (:531): one float gemm, double accumulation, one rounding
SQLM_HD inline void ransac_map(const float sR[9], const float t[3], const float X[3], float out[3]) {
  for (int i = 0; i < 3; ++i)
    out[i] = (float)(ransac_detail::dot3(sR[3 * i], sR[3 * i + 1], sR[3 * i + 2], X[0], X[1], X[2]) + (double)t[i]);
}

// the test of CheckInliers (:474-482) for one pair; false for any NaN
SQLM_HD inline bool ransac_is_inlier(const RansacHyp &h, const float X1[3], const float X2[3], const float K1[4],
                                     const float K2[4], int32_t max_err1, int32_t max_err2) {
  float p1im1[2], p2im2[2], p2im1[2], p1im2[2], c[3];
  ransac_image(X1, K1, p1im1);
  ransac_image(X2, K2, p2im2);
  ransac_map(h.sR, h.t, X2, c);
  ransac_image(c, K1, p2im1);
  ransac_map(h.sRinv, h.tinv, X1, c);
  ransac_image(c, K2, p1im2);
  const float d1x = p1im1[0] - p2im1[0], d1y = p1im1[1] - p2im1[1];
  const float d2x = p1im2[0] - p2im2[0], d2y = p1im2[1] - p2im2[1];
  const float err1 = (float)((double)d1x * (double)d1x + (double)d1y * (double)d1y);
  const float err2 = (float)((double)d2x * (double)d2x + (double)d2y * (double)d2y);
  return err1 < (float)max_err1 && err2 < (float)max_err2;
}

}  // namespace sqlm
