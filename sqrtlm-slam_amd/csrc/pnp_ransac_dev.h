// pnp_ransac_dev.h — the arithmetic of one EPnP solve and of the inlier test of
// the PnP RANSAC (PnPsolver::compute_pose and CheckInliers,
// src/algorithm/PnPsolver.cc:430-467 and :520-1418 of the reference), written
// once for the kernels (sqlm_pnp_ransac.hip) and for the host
// (sqlm_pnp_ransac_hypothesis_host / _refine_host, the same text compiled for
// the CPU). Both translation units are built with -ffp-contract=off: every
// result comes from IEEE double operations (+ - * / sqrt fabs) in the order
// written here; no libm function is called.
//
// One routine, pnp_epnp, serves a 4-point hypothesis and a refine on n inliers.
// A sum over the points (centroid, the 3x3 and 12x12 Gram matrices, pc0 / pw0,
// ABt, the reprojection error) has one order, pnp_sum: lane l of 64 adds the
// terms of points l, l+64, ... in index order to +0.0, then the partials of
// lanes 0 .. min(n, 64)-1 are added in lane order to +0.0. On the device the
// lanes are a wavefront's, on the host a loop replays them.
//
// Everything that is not such a sum is computed by every lane alike on the
// arrays of a PnpWork, which a kernel keeps in LDS (one per wavefront) and the
// host on its stack: no array lives in registers, none in scratch.
//
// Where the reference hands arithmetic to OpenCV the library defines its own
// (DESIGN.md 8g): cyclic Jacobi with a fixed rotation order and sweep count for
// the symmetric eigenproblems, the inverse of CC from its orthogonal columns,
// the reference's own qr_solve for the small least-squares systems, and a
// one-sided Jacobi SVD for the polar factor of ABt.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SQLM_HD __host__ __device__
#else
#define SQLM_HD
#endif

#pragma clang fp contract(off)

namespace sqlm {

constexpr int kPnpSweeps3 = 6;    // Jacobi sweeps of the 3x3 PW0^T PW0
constexpr int kPnpSweeps12 = 12;  // Jacobi sweeps of the 12x12 M^T M
constexpr int kPnpSweepsR = 6;    // one-sided Jacobi sweeps of the 3x3 ABt
constexpr double kPnpRankTol = 1e-6;   // k_i <= tol * k_0: control direction i spans nothing (coplanar points)
constexpr double kPnpOrthTol = 1e-15;   // |w_p . w_q| <= tol * |w_p| |w_q|: the two columns of ABt count as orthogonal
constexpr double kPnpPolarTol = 1e-12;  // sigma_min <= tol * sigma_max: that direction of ABt is completed by a cross product

struct PnpSweeps {
  int s3 = kPnpSweeps3, s12 = kPnpSweeps12, sR = kPnpSweepsR;
};

// The pair indices of four RandomInt draws from a freshly reset
// vAvailableIndices with swap-remove (:281-297): draw i is in [0, n-1-i].
SQLM_HD inline void pnp_indices(int n, const int32_t r[4], int32_t idx[4]) {
  idx[0] = r[0];
  idx[1] = r[1] == r[0] ? n - 1 : r[1];
  const int b1 = r[0] == n - 2 ? n - 1 : n - 2;  // what the second removal moves into slot r[1]
  idx[2] = r[2] == r[1] ? b1 : (r[2] == r[0] ? n - 1 : r[2]);
  const int s = n - 3;  // the third removal moves slot n-3 into slot r[2]
  const int b2 = s == r[1] ? b1 : (s == r[0] ? n - 1 : s);
  idx[3] = r[3] == r[2] ? b2 : (r[3] == r[1] ? b1 : (r[3] == r[0] ? n - 1 : r[3]));
}

// the points of one EPnP solve: the four of a hypothesis (list == nullptr) or
// list[0 .. n) of a refine, out of the n_pair pairs of a problem
struct PnpPts {
  const float *Xw = nullptr, *uv = nullptr;  // [n_pair][3], [n_pair][2]
  const int32_t *list = nullptr;
  int32_t q[4] = {0, 0, 0, 0};
  int n = 0, n_pair = 0;
};

struct PnpWork {
  double A[144], V[144];  // Jacobi workspace
  double ut[144], d[12];  // rows: eigenvectors of M^T M by descending eigenvalue (what cvSVD(.. U_T) yields)
  double uct[9], dc[3];   // the same of PW0^T PW0
  double cws[12], cci[9];  // control points; rows of the inverse of CC
  double L[60], rho[6];
  double qa[30], qb[6], qx[5], q1[5], q2[5];  // qr_solve: A, b, X, A1, A2
  double betas[12];                           // [3][4], candidates N = 4, 2, 3 in the reference's order
  double ccs[12];
  double Rs[27], ts[9], rep[3];
  double pc0[3], pw0[3];
};

namespace pnp_detail {

SQLM_HD inline double absd(double x) { return __builtin_fabs(x); }

// sum over points i in [0, n) of term(i, t[K]) in the order of the header comment
template <int K, class Term>
SQLM_HD inline void pnp_sum(int n, Term term, double (&total)[K]) {
  const int nl = n < 64 ? n : 64;
#if defined(__HIP_DEVICE_COMPILE__)
  const int lane = threadIdx.x & 63;
  double p[K];
#pragma unroll
  for (int k = 0; k < K; ++k) p[k] = 0.0;
  for (int i = lane; i < n; i += 64) {
    double t[K];
    term(i, t);
#pragma unroll
    for (int k = 0; k < K; ++k) p[k] = p[k] + t[k];
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double acc = 0.0;
#pragma unroll 1
    for (int l = 0; l < nl; ++l) acc = acc + __shfl(p[k], l);
    total[k] = acc;
  }
#else
  for (int k = 0; k < K; ++k) total[k] = 0.0;
  for (int l = 0; l < nl; ++l) {
    double p[K];
    for (int k = 0; k < K; ++k) p[k] = 0.0;
    for (int i = l; i < n; i += 64) {
      double t[K];
      term(i, t);
      for (int k = 0; k < K; ++k) p[k] = p[k] + t[k];
    }
    for (int k = 0; k < K; ++k) total[k] = total[k] + p[k];
  }
#endif
}

// point i of the solve as add_correspondence stores it (:505-516): float values in doubles
SQLM_HD inline void point(const PnpPts &P, int i, double &x, double &y, double &z, double &u, double &v) {
  int j = P.list ? P.list[i] : (i == 0 ? P.q[0] : i == 1 ? P.q[1] : i == 2 ? P.q[2] : P.q[3]);
  j = j < 0 ? 0 : (j >= P.n_pair ? P.n_pair - 1 : j);  // in bounds whatever the index is
  x = (double)P.Xw[3 * (int64_t)j];
  y = (double)P.Xw[3 * (int64_t)j + 1];
  z = (double)P.Xw[3 * (int64_t)j + 2];
  u = (double)P.uv[2 * (int64_t)j];
  v = (double)P.uv[2 * (int64_t)j + 1];
}

// Cyclic Jacobi on the symmetric n x n A (row-major, destroyed; the diagonal
// ends as the eigenvalues), V's columns the eigenvectors. Rotations in
// row-major order over p < q, a zero off-diagonal skipped, `sweeps` sweeps.
SQLM_HD inline void jacobi(double *A, double *V, int n, int sweeps) {
  for (int k = 0; k < n * n; ++k) V[k] = (k % (n + 1) == 0) ? 1.0 : 0.0;
#pragma unroll 1
  for (int sweep = 0; sweep < sweeps; ++sweep) {
#pragma unroll 1
    for (int p = 0; p < n - 1; ++p) {
#pragma unroll 1
      for (int q = p + 1; q < n; ++q) {
        const double apq = A[n * p + q];
        if (!(apq != 0.0)) continue;
        const double theta = (A[(n + 1) * q] - A[(n + 1) * p]) / (apq + apq);
        const double at = absd(theta);
        double t = 1.0 / (at + __builtin_sqrt(theta * theta + 1.0));
        if (theta < 0) t = -t;
        const double c = 1.0 / __builtin_sqrt(t * t + 1.0);
        const double s = t * c;
        const double app = A[(n + 1) * p] - t * apq, aqq = A[(n + 1) * q] + t * apq;
#pragma unroll 1
        for (int r = 0; r < n; ++r) {
          if (r == p || r == q) continue;
          const double arp = A[n * r + p], arq = A[n * r + q];
          const double np_ = c * arp - s * arq, nq_ = s * arp + c * arq;
          A[n * r + p] = np_;
          A[n * p + r] = np_;
          A[n * r + q] = nq_;
          A[n * q + r] = nq_;
        }
        A[(n + 1) * p] = app;
        A[(n + 1) * q] = aqq;
        A[n * p + q] = 0.0;
        A[n * q + p] = 0.0;
#pragma unroll 1
        for (int r = 0; r < n; ++r) {
          const double vrp = V[n * r + p], vrq = V[n * r + q];
          V[n * r + p] = c * vrp - s * vrq;
          V[n * r + q] = s * vrp + c * vrq;
        }
      }
    }
  }
}

// eigenpairs by descending eigenvalue, ties by index; row k of ut the k-th eigenvector
SQLM_HD inline void sorted_rows(const double *A, const double *V, int n, double *ut, double *d) {
  for (int k = 0; k < n * n; ++k) ut[k] = 0.0;
  for (int k = 0; k < n; ++k) d[k] = 0.0;
#pragma unroll 1
  for (int k = 0; k < n; ++k) {
    const double ak = A[(n + 1) * k];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      const double aj = A[(n + 1) * j];
      if (aj > ak || (aj == ak && j < k)) ++rank;
    }
    d[rank] = ak;
    for (int r = 0; r < n; ++r) ut[n * rank + r] = V[n * r + k];
  }
}

// qr_solve (:1284-1418) on the nr x nc A (row-major, destroyed) and b
// (destroyed); X is all zeros on its eta == 0 exit
SQLM_HD inline void qr_solve(double *A, double *b, double *X, int nr, int nc, double *A1, double *A2) {
  for (int k = 0; k < nc; ++k) X[k] = 0.0;
#pragma unroll 1
  for (int k = 0; k < nc; ++k) {
    double eta = absd(A[k * nc + k]);
    for (int i = k + 1; i < nr; ++i) {  // as written there: rows k .. nr-2
      const double elt = absd(A[(i - 1) * nc + k]);
      if (eta < elt) eta = elt;
    }
    if (eta == 0) {
      A1[k] = A2[k] = 0.0;
      return;
    }
    double sum = 0.0;
    const double inv_eta = 1. / eta;
    for (int i = k; i < nr; ++i) {
      A[i * nc + k] = A[i * nc + k] * inv_eta;
      sum = sum + A[i * nc + k] * A[i * nc + k];
    }
    double sigma = __builtin_sqrt(sum);
    if (A[k * nc + k] < 0) sigma = -sigma;
    A[k * nc + k] = A[k * nc + k] + sigma;
    A1[k] = sigma * A[k * nc + k];
    A2[k] = -eta * sigma;
#pragma unroll 1
    for (int j = k + 1; j < nc; ++j) {
      double s2 = 0;
      for (int i = k; i < nr; ++i) s2 = s2 + A[i * nc + k] * A[i * nc + j];
      const double tau = s2 / A1[k];
      for (int i = k; i < nr; ++i) A[i * nc + j] = A[i * nc + j] - tau * A[i * nc + k];
    }
  }
#pragma unroll 1
  for (int j = 0; j < nc; ++j) {  // b <- Qt b
    double tau = 0;
    for (int i = j; i < nr; ++i) tau = tau + A[i * nc + j] * b[i];
    tau = tau / A1[j];
    for (int i = j; i < nr; ++i) b[i] = b[i] - tau * A[i * nc + j];
  }
  X[nc - 1] = b[nc - 1] / A2[nc - 1];
#pragma unroll 1
  for (int i = nc - 2; i >= 0; --i) {
    double sum = 0;
    for (int j = i + 1; j < nc; ++j) sum = sum + A[i * nc + j] * X[j];
    X[i] = (b[i] - sum) / A2[i];
  }
}

// alphas of a point (:609-629)
SQLM_HD inline void alphas(const PnpWork &w, double x, double y, double z, double &a0, double &a1, double &a2,
                           double &a3) {
  const double d0 = x - w.cws[0], d1 = y - w.cws[1], d2 = z - w.cws[2];
  a1 = w.cci[0] * d0 + w.cci[1] * d1 + w.cci[2] * d2;
  a2 = w.cci[3] * d0 + w.cci[4] * d1 + w.cci[5] * d2;
  a3 = w.cci[6] * d0 + w.cci[7] * d1 + w.cci[8] * d2;
  a0 = 1.0 - a1 - a2 - a3;
}

// pcs of point i (:685-697) under the control points w.ccs
SQLM_HD inline void pcs(const PnpWork &w, const PnpPts &P, int i, double pc[3], double pw[3]) {
  double u, v, a0, a1, a2, a3;
  point(P, i, pw[0], pw[1], pw[2], u, v);
  alphas(w, pw[0], pw[1], pw[2], a0, a1, a2, a3);
#pragma unroll
  for (int j = 0; j < 3; ++j) pc[j] = a0 * w.ccs[j] + a1 * w.ccs[3 + j] + a2 * w.ccs[6 + j] + a3 * w.ccs[9 + j];
}

// dot(dv[x][pair], dv[y][pair]) of compute_L_6x10 (:1096-1129): v[x] = ut row 11 - x
SQLM_HD inline double dvdot(const double *ut, int x, int y, int a, int b) {
  const double *vx = ut + 12 * (11 - x), *vy = ut + 12 * (11 - y);
  const double x0 = vx[3 * a] - vx[3 * b], x1 = vx[3 * a + 1] - vx[3 * b + 1], x2 = vx[3 * a + 2] - vx[3 * b + 2];
  const double y0 = vy[3 * a] - vy[3 * b], y1 = vy[3 * a + 1] - vy[3 * b + 1], y2 = vy[3 * a + 2] - vy[3 * b + 2];
  return x0 * y0 + x1 * y1 + x2 * y2;
}

SQLM_HD inline double dist2(const double *p1, const double *p2) {
  return (p1[0] - p2[0]) * (p1[0] - p2[0]) + (p1[1] - p2[1]) * (p1[1] - p2[1]) + (p1[2] - p2[2]) * (p1[2] - p2[2]);
}

SQLM_HD inline double dot3(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// the least-squares solve of find_betas_approx_* on nc columns of L: qx
SQLM_HD inline void solve_cols(PnpWork &w, int nc, int c0, int c1, int c2, int c3, int c4) {
  for (int i = 0; i < 6; ++i) {
    for (int j = 0; j < nc; ++j) {
      const int c = j == 0 ? c0 : j == 1 ? c1 : j == 2 ? c2 : j == 3 ? c3 : c4;
      w.qa[i * nc + j] = w.L[10 * i + c];
    }
    w.qb[i] = w.rho[i];
  }
  qr_solve(w.qa, w.qb, w.qx, 6, nc, w.q1, w.q2);
}

// gauss_newton (:1245-1279), five steps of compute_A_and_b_gauss_newton + qr_solve
SQLM_HD inline void gauss_newton(PnpWork &w, double *betas) {
#pragma unroll 1
  for (int it = 0; it < 5; ++it) {
    const double b0 = betas[0], b1 = betas[1], b2 = betas[2], b3 = betas[3];
    for (int i = 0; i < 6; ++i) {
      const double *rowL = w.L + 10 * i;
      double *rowA = w.qa + 4 * i;
      rowA[0] = 2 * rowL[0] * b0 + rowL[1] * b1 + rowL[3] * b2 + rowL[6] * b3;
      rowA[1] = rowL[1] * b0 + 2 * rowL[2] * b1 + rowL[4] * b2 + rowL[7] * b3;
      rowA[2] = rowL[3] * b0 + rowL[4] * b1 + 2 * rowL[5] * b2 + rowL[8] * b3;
      rowA[3] = rowL[6] * b0 + rowL[7] * b1 + rowL[8] * b2 + 2 * rowL[9] * b3;
      w.qb[i] = w.rho[i] - (rowL[0] * b0 * b0 + rowL[1] * b0 * b1 + rowL[2] * b1 * b1 + rowL[3] * b0 * b2 +
                            rowL[4] * b1 * b2 + rowL[5] * b2 * b2 + rowL[6] * b0 * b3 + rowL[7] * b1 * b3 +
                            rowL[8] * b2 * b3 + rowL[9] * b3 * b3);
    }
    qr_solve(w.qa, w.qb, w.qx, 6, 4, w.q1, w.q2);
    for (int i = 0; i < 4; ++i) betas[i] = betas[i] + w.qx[i];
  }
}

// R = U V^T of ABt = U S V^T (estimate_R_and_t :886-891) from a one-sided
// Jacobi SVD: the columns of W = ABt are rotated in the order (0,1) (0,2) (1,2),
// sR sweeps, a pair that is orthogonal to kPnpOrthTol skipped; W = U S, the rotations' product is V.
// A direction with sigma <= kPnpPolarTol * sigma_max is the cross product of
// the other two.
SQLM_HD inline void polar(const double abt[9], int sweeps, double *R) {
  double W[9], Vr[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    W[k] = abt[k];
    Vr[k] = (k % 4 == 0) ? 1.0 : 0.0;
  }
#pragma unroll 1
  for (int sweep = 0; sweep < sweeps; ++sweep) {
#pragma unroll
    for (int pq = 0; pq < 3; ++pq) {
      const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
      const double al = W[p] * W[p] + W[3 + p] * W[3 + p] + W[6 + p] * W[6 + p];
      const double be = W[q] * W[q] + W[3 + q] * W[3 + q] + W[6 + q] * W[6 + q];
      const double ga = W[p] * W[q] + W[3 + p] * W[3 + q] + W[6 + p] * W[6 + q];
      if (!(absd(ga) <= kPnpOrthTol * __builtin_sqrt(al * be))) {  // without it rounding noise keeps rotating
        const double zeta = (be - al) / (ga + ga);
        const double az = absd(zeta);
        double t = 1.0 / (az + __builtin_sqrt(zeta * zeta + 1.0));
        if (zeta < 0) t = -t;
        const double c = 1.0 / __builtin_sqrt(t * t + 1.0);
        const double s = t * c;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const double wp = W[3 * r + p], wq = W[3 * r + q];
          W[3 * r + p] = c * wp - s * wq;
          W[3 * r + q] = s * wp + c * wq;
          const double vp = Vr[3 * r + p], vq = Vr[3 * r + q];
          Vr[3 * r + p] = c * vp - s * vq;
          Vr[3 * r + q] = s * vp + c * vq;
        }
      }
    }
  }
  double sg[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) sg[k] = __builtin_sqrt(W[k] * W[k] + W[3 + k] * W[3 + k] + W[6 + k] * W[6 + k]);
  const int m = (sg[1] < sg[0]) ? (sg[2] < sg[1] ? 2 : 1) : (sg[2] < sg[0] ? 2 : 0);  // the smallest, the first of equals
  const double smax = sg[0] > sg[1] ? (sg[0] > sg[2] ? sg[0] : sg[2]) : (sg[1] > sg[2] ? sg[1] : sg[2]);
  const double smin = m == 0 ? sg[0] : m == 1 ? sg[1] : sg[2];
  double U[9];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int r = 0; r < 3; ++r) U[3 * r + k] = W[3 * r + k] / sg[k];
  if (smin <= kPnpPolarTol * smax) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (k != m) continue;
      const int a = (k + 1) % 3, b = (k + 2) % 3;
      U[k] = U[3 + a] * U[6 + b] - U[6 + a] * U[3 + b];
      U[3 + k] = U[6 + a] * U[b] - U[a] * U[6 + b];
      U[6 + k] = U[a] * U[3 + b] - U[3 + a] * U[b];
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) R[3 * i + j] = U[3 * i] * Vr[3 * j] + U[3 * i + 1] * Vr[3 * j + 1] + U[3 * i + 2] * Vr[3 * j + 2];
}

// compute_R_and_t (:942-957) of candidate c: w.Rs, w.ts, w.rep
SQLM_HD inline void candidate(PnpWork &w, const PnpPts &P, const double K[4], int c, int sweepsR) {
  const double *betas = w.betas + 4 * c;
  const int n = P.n;
  const double dn = (double)n;
  for (int k = 0; k < 12; ++k) w.ccs[k] = 0.0;
  for (int i = 0; i < 4; ++i) {  // compute_ccs (:664-680)
    const double *v = w.ut + 12 * (11 - i);
    for (int k = 0; k < 12; ++k) w.ccs[k] = w.ccs[k] + betas[i] * v[k];
  }
  {  // solve_for_sign (:921-938) on point 0; the negation of pcs is the pcs of the negated ccs
    double pc[3], pw[3];
    pcs(w, P, 0, pc, pw);
    if (pc[2] < 0.0)
      for (int k = 0; k < 12; ++k) w.ccs[k] = -w.ccs[k];
  }
  double s6[6];
  pnp_sum<6>(n, [&](int i, double (&t)[6]) {
    double pc[3], pw[3];
    pcs(w, P, i, pc, pw);
    t[0] = pc[0]; t[1] = pc[1]; t[2] = pc[2];
    t[3] = pw[0]; t[4] = pw[1]; t[5] = pw[2];
  }, s6);
  for (int j = 0; j < 3; ++j) {
    w.pc0[j] = s6[j] / dn;
    w.pw0[j] = s6[3 + j] / dn;
  }
  double abt[9];
  pnp_sum<9>(n, [&](int i, double (&t)[9]) {
    double pc[3], pw[3];
    pcs(w, P, i, pc, pw);
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int k = 0; k < 3; ++k) t[3 * j + k] = (pc[j] - w.pc0[j]) * (pw[k] - w.pw0[k]);
  }, abt);
  double *R = w.Rs + 9 * c, *t = w.ts + 3 * c;
  polar(abt, sweepsR, R);
  const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] -
                     R[1] * R[3] * R[8] - R[0] * R[5] * R[7];
  if (det < 0) {
    R[6] = -R[6];
    R[7] = -R[7];
    R[8] = -R[8];
  }
  t[0] = w.pc0[0] - dot3(R, w.pw0);
  t[1] = w.pc0[1] - dot3(R + 3, w.pw0);
  t[2] = w.pc0[2] - dot3(R + 6, w.pw0);
  double s1[1];
  pnp_sum<1>(n, [&](int i, double (&e)[1]) {  // reprojection_error (:811-834)
    double pw[3], u, v;
    point(P, i, pw[0], pw[1], pw[2], u, v);
    const double Xc = dot3(R, pw) + t[0];
    const double Yc = dot3(R + 3, pw) + t[1];
    const double inv_Zc = 1.0 / (dot3(R + 6, pw) + t[2]);
    const double ue = K[2] + K[0] * Xc * inv_Zc;
    const double ve = K[3] + K[1] * Yc * inv_Zc;
    e[0] = __builtin_sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
  }, s1);
  w.rep[c] = s1[0] / dn;
}

}  // namespace pnp_detail

// compute_pose (:701-776) on the points P, camera K = fu fv uc vc. Returns the
// chosen candidate (0, 1, 2 for the reference's N = 1, 2, 3); its pose is
// w.Rs + 9 c, w.ts + 3 c. Every lane of a wavefront calls it with the same
// arguments and its wavefront's w.
SQLM_HD inline int pnp_epnp(const PnpPts &P, const double K[4], const PnpSweeps &sw, PnpWork &w) {
  using namespace pnp_detail;
  const int n = P.n;
  const double dn = (double)n;
  // choose_control_points (:520-575)
  double c0[3];
  pnp_sum<3>(n, [&](int i, double (&t)[3]) {
    double u, v;
    point(P, i, t[0], t[1], t[2], u, v);
  }, c0);
  for (int j = 0; j < 3; ++j) w.cws[j] = c0[j] / dn;
  double g[6];
  pnp_sum<6>(n, [&](int i, double (&t)[6]) {
    double x, y, z, u, v;
    point(P, i, x, y, z, u, v);
    const double d0 = x - w.cws[0], d1 = y - w.cws[1], d2 = z - w.cws[2];
    t[0] = d0 * d0; t[1] = d0 * d1; t[2] = d0 * d2;
    t[3] = d1 * d1; t[4] = d1 * d2; t[5] = d2 * d2;
  }, g);
  w.A[0] = g[0]; w.A[1] = g[1]; w.A[2] = g[2];
  w.A[3] = g[1]; w.A[4] = g[3]; w.A[5] = g[4];
  w.A[6] = g[2]; w.A[7] = g[4]; w.A[8] = g[5];
  jacobi(w.A, w.V, 3, sw.s3);
  sorted_rows(w.A, w.V, 3, w.uct, w.dc);
  double kk[3];
  for (int i = 0; i < 3; ++i) {
    const double dci = w.dc[i] > 0.0 ? w.dc[i] : 0.0;  // a singular value is not negative
    kk[i] = __builtin_sqrt(dci / dn);
    for (int j = 0; j < 3; ++j) w.cws[3 * (i + 1) + j] = w.cws[j] + kk[i] * w.uct[3 * i + j];
  }
  // compute_barycentric_coordinates (:586-630): CC's columns are k_i u_i, its inverse the rows u_i / k_i
  for (int i = 0; i < 3; ++i) {
    const bool ok = kk[i] > kPnpRankTol * kk[0];
    for (int j = 0; j < 3; ++j) w.cci[3 * i + j] = ok ? w.uct[3 * i + j] / kk[i] : 0.0;
  }
  // M^T M (:709-724), a row at a time: element (r, c) is the sum over the points of M1[r] M1[c] + M2[r] M2[c]
#pragma unroll 1
  for (int r = 0; r < 12; ++r) {
    double row[12];
    pnp_sum<12>(n, [&](int i, double (&t)[12]) {
      double x, y, z, u, v, a[4];
      point(P, i, x, y, z, u, v);
      alphas(w, x, y, z, a[0], a[1], a[2], a[3]);
      double m1[12], m2[12];
#pragma unroll
      for (int j = 0; j < 4; ++j) {  // fill_M (:642-659)
        m1[3 * j] = a[j] * K[0];
        m1[3 * j + 1] = 0.0;
        m1[3 * j + 2] = a[j] * (K[2] - u);
        m2[3 * j] = 0.0;
        m2[3 * j + 1] = a[j] * K[1];
        m2[3 * j + 2] = a[j] * (K[3] - v);
      }
      double m1r = m1[0], m2r = m2[0];
#pragma unroll
      for (int c = 1; c < 12; ++c) {
        m1r = c == r ? m1[c] : m1r;
        m2r = c == r ? m2[c] : m2r;
      }
#pragma unroll
      for (int c = 0; c < 12; ++c) t[c] = m1r * m1[c] + m2r * m2[c];
    }, row);
#pragma unroll
    for (int c = 0; c < 12; ++c) w.A[12 * r + c] = row[c];
  }
  jacobi(w.A, w.V, 12, sw.s12);
  sorted_rows(w.A, w.V, 12, w.ut, w.d);
  // compute_L_6x10 (:1071-1130), compute_rho (:1134-1143)
  {
    int a = 0, b = 1;
    for (int i = 0; i < 6; ++i) {
      double *row = w.L + 10 * i;
      row[0] = dvdot(w.ut, 0, 0, a, b);
      row[1] = 2.0 * dvdot(w.ut, 0, 1, a, b);
      row[2] = dvdot(w.ut, 1, 1, a, b);
      row[3] = 2.0 * dvdot(w.ut, 0, 2, a, b);
      row[4] = 2.0 * dvdot(w.ut, 1, 2, a, b);
      row[5] = dvdot(w.ut, 2, 2, a, b);
      row[6] = 2.0 * dvdot(w.ut, 0, 3, a, b);
      row[7] = 2.0 * dvdot(w.ut, 1, 3, a, b);
      row[8] = 2.0 * dvdot(w.ut, 2, 3, a, b);
      row[9] = dvdot(w.ut, 3, 3, a, b);
      w.rho[i] = dist2(w.cws + 3 * a, w.cws + 3 * b);
      b++;
      if (b > 3) {
        a++;
        b = a + 1;
      }
    }
  }
  // find_betas_approx_1 (:963-992)
  {
    double *be = w.betas;
    solve_cols(w, 4, 0, 1, 3, 6, 0);
    const double *b4 = w.qx;
    if (b4[0] < 0) {
      be[0] = __builtin_sqrt(-b4[0]);
      be[1] = -b4[1] / be[0];
      be[2] = -b4[2] / be[0];
      be[3] = -b4[3] / be[0];
    } else {
      be[0] = __builtin_sqrt(b4[0]);
      be[1] = b4[1] / be[0];
      be[2] = b4[2] / be[0];
      be[3] = b4[3] / be[0];
    }
    gauss_newton(w, be);
    candidate(w, P, K, 0, sw.sR);
  }
  // find_betas_approx_2 (:998-1029)
  {
    double *be = w.betas + 4;
    solve_cols(w, 3, 0, 1, 2, 0, 0);
    const double *b3 = w.qx;
    if (b3[0] < 0) {
      be[0] = __builtin_sqrt(-b3[0]);
      be[1] = (b3[2] < 0) ? __builtin_sqrt(-b3[2]) : 0.0;
    } else {
      be[0] = __builtin_sqrt(b3[0]);
      be[1] = (b3[2] > 0) ? __builtin_sqrt(b3[2]) : 0.0;
    }
    if (b3[1] < 0) be[0] = -be[0];
    be[2] = 0.0;
    be[3] = 0.0;
    gauss_newton(w, be);
    candidate(w, P, K, 1, sw.sR);
  }
  // find_betas_approx_3 (:1035-1067)
  {
    double *be = w.betas + 8;
    solve_cols(w, 5, 0, 1, 2, 3, 4);
    const double *b5 = w.qx;
    if (b5[0] < 0) {
      be[0] = __builtin_sqrt(-b5[0]);
      be[1] = (b5[2] < 0) ? __builtin_sqrt(-b5[2]) : 0.0;
    } else {
      be[0] = __builtin_sqrt(b5[0]);
      be[1] = (b5[2] > 0) ? __builtin_sqrt(b5[2]) : 0.0;
    }
    if (b5[1] < 0) be[0] = -be[0];
    be[2] = b5[3] / be[0];
    be[3] = 0.0;
    gauss_newton(w, be);
    candidate(w, P, K, 2, sw.sR);
  }
  int N = 0;
  if (w.rep[1] < w.rep[0]) N = 1;
  if (w.rep[2] < w.rep[N]) N = 2;
  return N;
}

// the test of CheckInliers (:438-457) for one pair, in the precisions written there; false for any NaN
SQLM_HD inline bool pnp_is_inlier(const double *R, const double *t, const double K[4], float X, float Y, float Z,
                                  float u, float v, float max_err) {
  const float Xc = (float)(R[0] * (double)X + R[1] * (double)Y + R[2] * (double)Z + t[0]);
  const float Yc = (float)(R[3] * (double)X + R[4] * (double)Y + R[5] * (double)Z + t[1]);
  const float invZc = (float)(1 / (R[6] * (double)X + R[7] * (double)Y + R[8] * (double)Z + t[2]));
  const double ue = K[2] + K[0] * (double)Xc * (double)invZc;
  const double ve = K[3] + K[1] * (double)Yc * (double)invZc;
  const float distX = (float)((double)u - ue);
  const float distY = (float)((double)v - ve);
  const float xx = distX * distX, yy = distY * distY;
  const float error2 = xx + yy;
  return error2 < max_err;
}

}  // namespace sqlm
