// sqlm_pose.hip — batched motion-only bundle adjustment on the GPU:
// g2oOptimizer::PoseOptimization (src/backend/g2oOptimizer.cc:385-679) = LM over
// ONE free VertexSE3Expmap with an EdgeSE3ProjectXYZOnlyPose per monocular
// correspondence (analytic Jacobian, Huber), four rounds that each restart from
// the input pose and reclassify every edge, an optional stage with LiDAR edges
// on the same vertex (numeric Jacobians), the final classification.
//
// A sibling of sqlm_sim3.hip: one workgroup per problem, the whole schedule and
// the LM loop in one launch. Lanes stride over the edges (an edge always
// belongs to the same lane, so its level and chi2 are private to it); sums go
// through wave shuffles and then through LDS in wave order, so a problem's bits
// depend on nothing but its own inputs. Thread 0 solves the damped 6x6 system
// and applies lm_decide; every thread reads the outcome from LDS after a
// barrier, so control flow around the barriers is uniform. No atomics, no waits
// on other workgroups; a stage is bounded by iters x 10 trials.
#include <hip/hip_runtime.h>

#include "../../include/sqrtlm.h"
#include "se3_dev.h"
#include "sqlm_internal.h"
#include "sqlm_small_lm.h"

namespace sqlm {

namespace {

constexpr int kPBlock = 256, kPWaves = kPBlock / 64;
constexpr int kPAcc = 28;  // H upper triangle (21, row-major packed), b (6), robust chi2

struct PShared {
  double P0[8];      // input pose: q (4), t (3)
  double S[8], T[8];  // current and trial estimate
  double E[8];       // state of the last computed errors (g2o: e->chi2() reads these)
  double Pq[12][8];  // oplus(S, +-delta e_d), [2 d + sign]: the LiDAR edges' central differences
  double red[kPWaves][kPAcc];
  double Hb[kPAcc];
  double dx[6];
  double bsum;       // block_sum's broadcast slot
  double scale, lambda;
  int ok, iter_end, have_step;
  LMCtl L;
};

struct PProb {
  int64_t o0, l0;  // first mono edge, first LiDAR edge
  int np, nl;
  double th2, delta, dsqr;
  float th2f;
  double K[4];
};

// plain chi2 of mono edge g at the pose A
__device__ __forceinline__ double mono_chi2(const PoseDev &d, const PProb &pb, const double *A, int64_t g) {
  const double X[3] = {d.Xw[3 * g], d.Xw[3 * g + 1], d.Xw[3 * g + 2]}, uv[2] = {d.uv[2 * g], d.uv[2 * g + 1]};
  const double w = d.info[g];
  double xc[3], e[2];
  pose_mono_error(A, A + 4, pb.K, X, uv, xc, e);
  return e[0] * (w * e[0]) + e[1] * (w * e[1]);
}

__device__ __forceinline__ double lidar_err(const PoseDev &d, const double *A, int64_t g) {
  return d.lid_kind[g] ? lidar_corner_error(A, A + 4, d.lid_pc + 3 * g, d.lid_pw + 3 * g)
                       : lidar_error(A, A + 4, d.lid_pc + 3 * g, d.lid_pw + 3 * g, d.lid_n + 3 * g);
}

// The 12 perturbed estimates of the LiDAR edges' central differences: they do
// not depend on the edge, so they are computed once per linearization.
__device__ void perturb(PShared &sh) {
  const int t = threadIdx.x;
  if (t < 12) {
    double u[6] = {0, 0, 0, 0, 0, 0}, s[8];
    u[t >> 1] = (t & 1) ? -1e-9 : 1e-9;
#pragma unroll
    for (int k = 0; k < 8; ++k) s[k] = sh.S[k];
    se3_oplus(s, s + 4, u);
#pragma unroll
    for (int k = 0; k < 8; ++k) sh.Pq[t][k] = s[k];
  }
  __syncthreads();
}

// computeActiveErrors + buildSystem at S over the level-0 mono edges and (lidar)
// every LiDAR edge: H, b, robust chi2 into sh.Hb. BaseUnaryEdge::
// constructQuadraticForm (base_unary_edge.hpp:50-88); the LiDAR Jacobians are
// BaseUnaryEdge::linearizeOplus (numeric, :90-127). write: e and J of every
// edge (level-1 mono edges too) go to the introspection buffers.
__device__ void linearize(PShared &sh, const PoseDev &d, const PProb &pb, bool robust, bool lidar, bool write) {
  if (lidar) perturb(sh);
  double acc[kPAcc];
#pragma unroll
  for (int k = 0; k < kPAcc; ++k) acc[k] = 0.0;
  double S[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) S[k] = sh.S[k];
  for (int i = threadIdx.x; i < pb.np; i += kPBlock) {
    const int64_t g = pb.o0 + i;
    const bool act = d.outlier[g] == 0;
    if (!act && !write) continue;
    const double X[3] = {d.Xw[3 * g], d.Xw[3 * g + 1], d.Xw[3 * g + 2]}, uv[2] = {d.uv[2 * g], d.uv[2 * g + 1]};
    const double w = d.info[g];
    double xc[3], e[2], J[12];
    pose_mono_error(S, S + 4, pb.K, X, uv, xc, e);
    pose_mono_jacobian(xc, pb.K, J);
    if (write) {
      d.lin_e[2 * g] = e[0];
      d.lin_e[2 * g + 1] = e[1];
#pragma unroll
      for (int c = 0; c < 12; ++c) d.lin_J[12 * g + c] = J[c];
    }
    if (!act) continue;
    double rho0, rho1;
    huber(e[0] * (w * e[0]) + e[1] * (w * e[1]), robust, pb.delta, pb.dsqr, rho0, rho1);
    const double ww = rho1 * w;                                    // weightedOmega = rho' Omega
    const double r0 = -(w * e[0]) * rho1, r1 = -(w * e[1]) * rho1;  // omega_r * rho'
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      const double a0 = J[a] * ww, a1 = J[6 + a] * ww;
#pragma unroll
      for (int b = a; b < 6; ++b) acc[k++] += a0 * J[b] + a1 * J[6 + b];
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) acc[21 + a] += J[a] * r0 + J[6 + a] * r1;
    acc[27] += rho0;
  }
  if (lidar) {
    const double scalar = 1.0 / (2 * 1e-9);
    for (int i = threadIdx.x; i < pb.nl; i += kPBlock) {
      const int64_t g = pb.l0 + i;
      const double w = d.lid_info[g];
      const double e = lidar_err(d, S, g);
      double J[6];
#pragma unroll 1
      for (int c = 0; c < 6; ++c) J[c] = scalar * (lidar_err(d, sh.Pq[2 * c], g) - lidar_err(d, sh.Pq[2 * c + 1], g));
      if (write) {
        d.lid_e[g] = e;
#pragma unroll
        for (int c = 0; c < 6; ++c) d.lid_J[6 * g + c] = J[c];
      }
      const double r = -(w * e);
      int k = 0;
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        const double a0 = J[a] * w;
#pragma unroll
        for (int b = a; b < 6; ++b) acc[k++] += a0 * J[b];
      }
#pragma unroll
      for (int a = 0; a < 6; ++a) acc[21 + a] += J[a] * r;
      acc[27] += e * (w * e);
    }
  }
  reduce_acc<kPAcc, kPWaves>(sh, acc);
}

// activeRobustChi2 at the pose A over the same edges.
__device__ double robust_chi2(PShared &sh, const PoseDev &d, const PProb &pb, const double *Ash, bool robust,
                              bool lidar) {
  double A[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) A[k] = Ash[k];
  double chi = 0.0;
  for (int i = threadIdx.x; i < pb.np; i += kPBlock) {
    const int64_t g = pb.o0 + i;
    if (d.outlier[g]) continue;
    double rho0, rho1;
    huber(mono_chi2(d, pb, A, g), robust, pb.delta, pb.dsqr, rho0, rho1);
    chi += rho0;
  }
  if (lidar)
    for (int i = threadIdx.x; i < pb.nl; i += kPBlock) {
      const int64_t g = pb.l0 + i;
      const double e = lidar_err(d, A, g);
      chi += e * (d.lid_info[g] * e);
    }
  return block_sum<kPWaves>(sh, chi);
}

// initializeOptimization(0); optimize(niter) on the level-0 edges
// (sparse_optimizer.cpp:354-419, optimization_algorithm_levenberg.cpp:61-164).
// Returns whether a trial ran, i.e. whether the level-0 edges' errors were
// computed (at sh.E): no level-0 edge means no active vertex and optimize()
// returns before computing anything (sparse_optimizer.cpp:356).
__device__ bool run_stage(PShared &sh, const PoseDev &d, const PProb &pb, int stage, int niter, bool robust,
                          bool lidar, bool write, sqlm_pose_stats *st) {
  double na = 0.0;
  for (int i = threadIdx.x; i < pb.np; i += kPBlock) na += d.outlier[pb.o0 + i] == 0 ? 1.0 : 0.0;
  const int n_act = (int)block_sum<kPWaves>(sh, na) + (lidar ? pb.nl : 0);
  const bool run = niter > 0 && n_act > 0;
  LMCtl &L = sh.L;
  if (threadIdx.x == 0) {
    lm_reset(L, niter, !run);
    st->active[stage] = n_act;
  }
  __syncthreads();
  if (!run) {
    if (write) linearize(sh, d, pb, robust, lidar, true);  // for sqlm_pose_get_linearization only
    return false;
  }
  for (int it = 0; it < niter; ++it) {
    if (L.done) break;  // LDS, the same for every thread
    linearize(sh, d, pb, robust, lidar, write && it == 0);  // the input-pose e and J are recorded on the way
    if (threadIdx.x == 0 && it == 0) {  // levenberg.cpp:66-97 at iteration 0
      L.currentChi = L.iniChi = sh.Hb[27];
      st->chi2_begin[stage] = sh.Hb[27];
      L.lambda = lm_lambda_init<6>(sh.Hb, d.user_lambda);
      L.ni = 2;
    }
    for (int q = 0; q < 10; ++q) {
      if (threadIdx.x == 0) {
        double dx[6], t[8];
        const bool ok = chol_solve<6>(sh.Hb, L.lambda, dx);
        const double scale = lm_scale<6>(sh.Hb, dx, L.lambda);
        for (int k = 0; k < 8; ++k) t[k] = sh.S[k];
        se3_oplus(t, t + 4, dx);
        for (int k = 0; k < 8; ++k) { sh.T[k] = t[k]; sh.E[k] = t[k]; }
        for (int j = 0; j < 6; ++j) sh.dx[j] = dx[j];
        sh.scale = scale;
        sh.lambda = L.lambda;
        sh.ok = ok;
        sh.have_step = 1;
      }
      __syncthreads();
      const double chi_new = robust_chi2(sh, d, pb, sh.T, robust, lidar);
      if (threadIdx.x == 0) {
        if (lm_decide(L, sh.Hb[27], chi_new, sh.scale, sh.ok != 0, false)) {
          for (int k = 0; k < 8; ++k) sh.S[k] = sh.T[k];
        }
        sh.iter_end = L.qmax == 0;
      }
      __syncthreads();
      if (sh.iter_end) break;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    lm_store_stage(st, stage, L);
  }
  return true;
}

// One classification of every mono edge (g2oOptimizer.cc:518-547, :650-675).
// A level-1 edge gets computeError() at the current estimate; a level-0 edge
// keeps the error last computed: at E if this stage ran a trial, else the value
// the previous check read (column prev, none: 0). The rounds compare
// (float)chi2 > (float)th2, the final classification (double)(float)chi2 > th2.
// Returns the number of level-1 edges afterwards.
__device__ int check_edges(PShared &sh, const PoseDev &d, const PProb &pb, int col, int prev, bool ran, bool final) {
  double S[8], E[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) { S[k] = sh.S[k]; E[k] = sh.E[k]; }
  double bad = 0.0;
  for (int i = threadIdx.x; i < pb.np; i += kPBlock) {
    const int64_t g = pb.o0 + i;
    double c;
    if (d.outlier[g]) c = mono_chi2(d, pb, S, g);
    else if (ran) c = mono_chi2(d, pb, E, g);
    else c = prev >= 0 ? d.edge_chi2[kPoseChecks * g + prev] : 0.0;
    d.edge_chi2[kPoseChecks * g + col] = c;
    const float cf = (float)c;  // const float chi2 = e->chi2()
    const bool out = final ? (double)cf > pb.th2 : cf > pb.th2f;
    d.outlier[g] = out ? 1 : 0;
    bad += out ? 1.0 : 0.0;
  }
  return (int)block_sum<kPWaves>(sh, bad);
}

__global__ __launch_bounds__(kPBlock) void k_pose(PoseDev d) {
  __shared__ PShared sh;
  const int prob = blockIdx.x;
  PProb pb;
  pb.o0 = d.obs_off[prob];
  pb.np = (int)(d.obs_off[prob + 1] - pb.o0);
  pb.l0 = d.refine ? d.lid_off[prob] : 0;
  pb.nl = d.refine ? (int)(d.lid_off[prob + 1] - pb.l0) : 0;
  pb.th2 = d.th2;
  pb.th2f = (float)d.th2;
  pb.delta = (double)(float)sqrt(d.th2);  // const float deltaMono = sqrt(5.991)
  pb.dsqr = pb.delta * pb.delta;
#pragma unroll
  for (int k = 0; k < 4; ++k) pb.K[k] = d.intr[4 * prob + k];
  sqlm_pose_stats *st = d.stats + prob;  // zeroed by the host
  if (threadIdx.x == 0) {
    for (int k = 0; k < 8; ++k) {
      const double v = d.pose[8 * prob + k];
      sh.P0[k] = v; sh.S[k] = v; sh.T[k] = v; sh.E[k] = v;
      d.pose_out[8 * prob + k] = v;
    }
    sh.have_step = 0;
    st->n_corr = pb.np;
    st->n_lidar = pb.nl;
    d.n_inliers[prob] = 0;
  }
  __syncthreads();
  if (pb.np < 3) {  // nInitialCorrespondences < 3: return 0, every flag cleared
    for (int i = threadIdx.x; i < pb.np; i += kPBlock) d.outlier[pb.o0 + i] = 0;
    return;
  }

  int prev = -1;
  bool ran = false;
  if (d.refine)  // the level-1 edges of the vision call (an edge's flag is private to its lane)
    for (int i = threadIdx.x; i < pb.np; i += kPBlock) d.outlier[pb.o0 + i] = d.outlier_in[pb.o0 + i] != 0;
  if (!d.refine) {
    int rounds = 0;
    for (int r = 0; r < 4; ++r) {
      if (threadIdx.x == 0)
        for (int k = 0; k < 8; ++k) sh.S[k] = sh.P0[k];  // every round restarts from the input pose
      __syncthreads();
      ran = run_stage(sh, d, pb, r, d.iters[r], r < 3, false, r == 0, st);
      const int n_bad = check_edges(sh, d, pb, r, prev, ran, false);
      if (threadIdx.x == 0) st->n_bad[r] = n_bad;
      prev = r;
      ++rounds;
      if (pb.np < 10) break;  // optimizer.edges().size() < 10
    }
    if (threadIdx.x == 0) st->rounds = rounds;
    ran = false;  // nothing is optimized between the last round's check and the final one
  } else {
    ran = run_stage(sh, d, pb, 4, d.iters[4], d.robust_on[prob] != 0, true, true, st);
  }
  const int n_bad = check_edges(sh, d, pb, kPoseChecks - 1, prev, ran, true);
  if (threadIdx.x == 0) {
    st->n_bad_final = n_bad;
    d.n_inliers[prob] = pb.np - n_bad;
    for (int k = 0; k < 8; ++k) d.pose_out[8 * prob + k] = sh.S[k];
    if (sh.have_step) {  // sqlm_pose_get_last_step
      double *o = d.last_step + kPoseStepLen * (int64_t)prob;
      store_last_step<6>(o, sh.Hb, sh.dx);
      o[48] = sh.lambda;
      o[49] = 1.0;
    }
  }
}

}  // namespace

void launch_pose(const PoseDev &d, hipStream_t st) {
  if (d.n_prob > 0) hipLaunchKernelGGL(k_pose, dim3(d.n_prob), dim3(kPBlock), 0, st, d);
}

}  // namespace sqlm
