// sqlm_sim3.hip — batched Sim3 alignment of loop candidates on the GPU:
// g2oOptimizer::OptimizeSim3 (src/backend/g2oOptimizer.cc:1560-1793) = LM over
// ONE free VertexSim3Expmap with an EdgeSim3ProjectXYZ and an
// EdgeInverseSim3ProjectXYZ per correspondence (numeric Jacobians, Huber),
// stage 1, outlier removal, stage 2, inlier count.
//
// One workgroup per problem, the whole schedule in one launch. Unlike the
// bundle adjustments (host LM loop, sqlm_api.cpp lm_host) the LM loop runs on
// the device here: a trial is a few hundred projections and a 7x7 solve, so a
// launch and a host round trip per phase would cost more than the arithmetic.
// Lanes stride over the pairs; sums go through wave shuffles and then through
// LDS in a fixed order, so a problem's bits depend on nothing but its own
// inputs. Thread 0 solves the 7x7 system and applies lm_decide (the rules the
// host loops use); every thread reads the outcome from LDS after a barrier, so
// control flow is uniform. No atomics, no waits on other workgroups; the loops
// are bounded by (iters[0] + max(iters[1], iters[2])) * 10 trials.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/sqrtlm.h"
#include "sim3_dev.h"
#include "sqlm_internal.h"
#include "sqlm_small_lm.h"

namespace sqlm {

namespace {

constexpr int kS3Block = 256, kS3Waves = kS3Block / 64;
constexpr int kS3Acc = 36;  // H upper triangle (28, row-major packed), b (7), robust chi2

struct S3Shared {
  double S[8], Si[8];      // current estimate and its inverse
  double T[8], Ti[8];      // trial estimate
  double E[8], Ei[8];      // state of the last computed errors (g2o: e->chi2() reads these)
  double P[14][8], Pi[14][8];  // oplus(S, +-delta e_d) and inverses, [2 d + sign]
  double red[kS3Waves][kS3Acc];
  double Hb[kS3Acc];
  double dx[7];
  double bsum;             // block_sum's broadcast slot
  double scale;
  int ok, iter_end, have_err, have_step;
  LMCtl L;
};

struct S3Prob {
  int64_t p0;
  int np;
  bool fix;
  double th2, delta, dsqr;
  double K1[4], K2[4];
};

__device__ __forceinline__ double edge_chi2(const double e[2], double w) { return e[0] * (w * e[0]) + e[1] * (w * e[1]); }

// The 14 perturbed estimates of the central differences and all inverses:
// they do not depend on the edge, so they are computed once per linearization.
__device__ void perturb(S3Shared &sh, const S3Prob &pb) {
  const int t = threadIdx.x;
  if (t < 14) {
    double u[7] = {0, 0, 0, 0, 0, 0, 0}, s[8];
    u[t >> 1] = (t & 1) ? -1e-9 : 1e-9;
#pragma unroll
    for (int k = 0; k < 8; ++k) s[k] = sh.S[k];
    sim3_oplus(s, u, pb.fix);
    double si[8];
    sim3_inverse(s, si);
#pragma unroll
    for (int k = 0; k < 8; ++k) { sh.P[t][k] = s[k]; sh.Pi[t][k] = si[k]; }
  }
  __syncthreads();
}

// computeActiveErrors + buildSystem at S: robust chi2, H, b into sh.Hb.
// BaseBinaryEdge::linearizeOplus (numeric, base_binary_edge.hpp:131-205) and
// constructQuadraticForm (:55-120) with the Sim3 vertex the only free one.
__device__ void linearize(S3Shared &sh, const Sim3Dev &d, const S3Prob &pb, bool write) {
  perturb(sh, pb);
  double acc[kS3Acc];
#pragma unroll
  for (int k = 0; k < kS3Acc; ++k) acc[k] = 0.0;
  const double scalar = 1.0 / (2 * 1e-9);
  for (int i = threadIdx.x; i < pb.np; i += kS3Block) {
    const int64_t g = pb.p0 + i;
    if (d.pair_state[g]) continue;
#pragma unroll 1
    for (int side = 0; side < 2; ++side) {
      const double *Xp = (side == 0 ? d.X2c : d.X1c) + 3 * g, *op = (side == 0 ? d.obs1 : d.obs2) + 2 * g;
      const double X[3] = {Xp[0], Xp[1], Xp[2]}, ob[2] = {op[0], op[1]};
      const double w = (side == 0 ? d.info1 : d.info2)[g];
      const double *K = side == 0 ? pb.K1 : pb.K2;
      double e[2], J[2][7];
      sim3_project_error(side == 0 ? sh.S : sh.Si, X, K, ob, e);
#pragma unroll
      for (int c = 0; c < 7; ++c) {
        double ep[2], em[2];
        sim3_project_error(side == 0 ? sh.P[2 * c] : sh.Pi[2 * c], X, K, ob, ep);
        sim3_project_error(side == 0 ? sh.P[2 * c + 1] : sh.Pi[2 * c + 1], X, K, ob, em);
        J[0][c] = scalar * (ep[0] - em[0]);
        J[1][c] = scalar * (ep[1] - em[1]);
      }
      if (write) {
        d.lin_e[4 * g + 2 * side] = e[0];
        d.lin_e[4 * g + 2 * side + 1] = e[1];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
          for (int c = 0; c < 7; ++c) d.lin_J[28 * g + 14 * side + 7 * r + c] = J[r][c];
      }
      double rho0, rho1;
      huber(edge_chi2(e, w), true, pb.delta, pb.dsqr, rho0, rho1);
      const double ww = rho1 * w;                                    // weightedOmega = rho' Omega
      const double r0 = -(w * e[0]) * rho1, r1 = -(w * e[1]) * rho1;  // omega_r * rho'
      int k = 0;
#pragma unroll
      for (int a = 0; a < 7; ++a) {
        const double a0 = J[0][a] * ww, a1 = J[1][a] * ww;
#pragma unroll
        for (int b = a; b < 7; ++b) acc[k++] += a0 * J[0][b] + a1 * J[1][b];
      }
#pragma unroll
      for (int a = 0; a < 7; ++a) acc[28 + a] += J[0][a] * r0 + J[1][a] * r1;
      acc[35] += rho0;
    }
  }
  reduce_acc<kS3Acc, kS3Waves>(sh, acc);
}

// activeRobustChi2 at the Sim3 (A, Ai) over the active pairs.
__device__ double robust_chi2(S3Shared &sh, const Sim3Dev &d, const S3Prob &pb, const double *A, const double *Ai) {
  double chi = 0.0;
  for (int i = threadIdx.x; i < pb.np; i += kS3Block) {
    const int64_t g = pb.p0 + i;
    if (d.pair_state[g]) continue;
    const double X2[3] = {d.X2c[3 * g], d.X2c[3 * g + 1], d.X2c[3 * g + 2]};
    const double X1[3] = {d.X1c[3 * g], d.X1c[3 * g + 1], d.X1c[3 * g + 2]};
    const double o1[2] = {d.obs1[2 * g], d.obs1[2 * g + 1]}, o2[2] = {d.obs2[2 * g], d.obs2[2 * g + 1]};
    double e[2], rho0, rho1;
    sim3_project_error(A, X2, pb.K1, o1, e);
    huber(edge_chi2(e, d.info1[g]), true, pb.delta, pb.dsqr, rho0, rho1);
    chi += rho0;
    sim3_project_error(Ai, X1, pb.K2, o2, e);
    huber(edge_chi2(e, d.info2[g]), true, pb.delta, pb.dsqr, rho0, rho1);
    chi += rho0;
  }
  return block_sum<kS3Waves>(sh, chi);
}

// initializeOptimization(); optimize(niter) on the active pairs
// (sparse_optimizer.cpp:354-419, optimization_algorithm_levenberg.cpp:61-164).
__device__ void run_stage(S3Shared &sh, const Sim3Dev &d, const S3Prob &pb, int stage, int niter,
                          sqlm_sim3_stats *st) {
  LMCtl &L = sh.L;
  if (threadIdx.x == 0) lm_reset(L, niter, niter <= 0);
  __syncthreads();
  for (int it = 0; it < niter; ++it) {
    if (L.done) break;  // LDS, the same for every thread
    linearize(sh, d, pb, stage == 0 && it == 0);  // the input-state e and J are recorded on the way
    if (threadIdx.x == 0 && it == 0) {  // levenberg.cpp:66-97 at iteration 0
      L.currentChi = L.iniChi = sh.Hb[35];
      st->chi2_begin[stage] = sh.Hb[35];
      L.lambda = lm_lambda_init<7>(sh.Hb, d.user_lambda);
      L.ni = 2;
    }
    for (int q = 0; q < 10; ++q) {
      if (threadIdx.x == 0) {
        double dx[7], t[8], ti[8];
        const bool ok = chol_solve<7>(sh.Hb, L.lambda, dx);
        const double scale = lm_scale<7>(sh.Hb, dx, L.lambda);
        for (int k = 0; k < 8; ++k) t[k] = sh.S[k];
        sim3_oplus(t, dx, pb.fix);
        sim3_inverse(t, ti);
        for (int k = 0; k < 8; ++k) { sh.T[k] = t[k]; sh.Ti[k] = ti[k]; sh.E[k] = t[k]; sh.Ei[k] = ti[k]; }
        for (int j = 0; j < 7; ++j) sh.dx[j] = dx[j];
        sh.scale = scale;
        sh.ok = ok;
        sh.have_err = 1;
        sh.have_step = 1;
      }
      __syncthreads();
      const double chi_new = robust_chi2(sh, d, pb, sh.T, sh.Ti);
      if (threadIdx.x == 0) {
        if (lm_decide(L, sh.Hb[35], chi_new, sh.scale, sh.ok != 0, false)) {
          for (int k = 0; k < 8; ++k) { sh.S[k] = sh.T[k]; sh.Si[k] = sh.Ti[k]; }
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
    const int n = L.its < SQLM_SIM3_TRACE_MAX ? L.its : SQLM_SIM3_TRACE_MAX;
    st->trace_len[stage] = n;
    for (int k = 0; k < n; ++k) {
      st->trace_chi2[stage][k] = L.trace_chi2[k];
      st->trace_lambda[stage][k] = L.trace_lambda[k];
      st->trace_trials[stage][k] = L.trace_trials[k];
    }
  }
}

// The chi2 > th2 test on both edges of every still active pair, from the last
// computed errors (g2oOptimizer.cc:1733-1750 and :1770-1785); failing pairs get
// `tag`. Returns the number of failing pairs.
__device__ int check_pairs(S3Shared &sh, const Sim3Dev &d, const S3Prob &pb, int check, uint8_t tag) {
  double bad = 0.0;
  for (int i = threadIdx.x; i < pb.np; i += kS3Block) {
    const int64_t g = pb.p0 + i;
    if (d.pair_state[g]) continue;
    double c12 = 0.0, c21 = 0.0;
    if (sh.have_err) {
      const double X2[3] = {d.X2c[3 * g], d.X2c[3 * g + 1], d.X2c[3 * g + 2]};
      const double X1[3] = {d.X1c[3 * g], d.X1c[3 * g + 1], d.X1c[3 * g + 2]};
      const double o1[2] = {d.obs1[2 * g], d.obs1[2 * g + 1]}, o2[2] = {d.obs2[2 * g], d.obs2[2 * g + 1]};
      double e[2];
      sim3_project_error(sh.E, X2, pb.K1, o1, e);
      c12 = edge_chi2(e, d.info1[g]);
      sim3_project_error(sh.Ei, X1, pb.K2, o2, e);
      c21 = edge_chi2(e, d.info2[g]);
    }
    d.pair_chi2[4 * g + 2 * check] = c12;
    d.pair_chi2[4 * g + 2 * check + 1] = c21;
    if (check == 0) {  // a removed edge keeps its error
      d.pair_chi2[4 * g + 2] = c12;
      d.pair_chi2[4 * g + 3] = c21;
    }
    if (c12 > pb.th2 || c21 > pb.th2) {
      d.pair_state[g] = tag;
      bad += 1.0;
    }
  }
  return (int)block_sum<kS3Waves>(sh, bad);
}

__global__ __launch_bounds__(kS3Block) void k_sim3(Sim3Dev d) {
  __shared__ S3Shared sh;
  const int prob = blockIdx.x;
  S3Prob pb;
  pb.p0 = d.pair_off[prob];
  pb.np = (int)(d.pair_off[prob + 1] - pb.p0);
  pb.fix = d.fix_scale[prob] != 0;
  pb.th2 = d.th2[prob];
  pb.delta = (double)sqrtf((float)pb.th2);  // const float deltaHuber = sqrt(th2)
  pb.dsqr = pb.delta * pb.delta;
#pragma unroll
  for (int k = 0; k < 4; ++k) { pb.K1[k] = d.intr1[4 * prob + k]; pb.K2[k] = d.intr2[4 * prob + k]; }
  sqlm_sim3_stats *st = d.stats + prob;  // zeroed by the host
  if (threadIdx.x == 0) {
    double s[8], si[8];
    for (int k = 0; k < 8; ++k) s[k] = d.S12[8 * prob + k];
    sim3_inverse(s, si);
    for (int k = 0; k < 8; ++k) { sh.S[k] = s[k]; sh.Si[k] = si[k]; d.S12_out[8 * prob + k] = s[k]; }
    sh.have_err = 0;
    sh.have_step = 0;
    st->n_corr = pb.np;
    d.n_inliers[prob] = 0;
  }
  __syncthreads();
  if (pb.np == 0) return;  // nothing to optimize

  if (d.iters[0] <= 0) linearize(sh, d, pb, true);  // for sqlm_sim3_get_linearization only
  run_stage(sh, d, pb, 0, d.iters[0], st);

  const int n_bad = check_pairs(sh, d, pb, 0, 1);
  if (threadIdx.x == 0) st->n_bad = n_bad;
  if (pb.np - n_bad >= 10) {
    run_stage(sh, d, pb, 1, n_bad > 0 ? d.iters[1] : d.iters[2], st);
    const int n_out = check_pairs(sh, d, pb, 1, 2);
    if (threadIdx.x == 0) {
      d.n_inliers[prob] = pb.np - n_bad - n_out;
      for (int k = 0; k < 8; ++k) d.S12_out[8 * prob + k] = sh.S[k];
    }
  }
  if (threadIdx.x == 0 && sh.have_step) {  // sqlm_sim3_get_last_step
    double *o = d.last_step + 64 * (int64_t)prob;
    store_last_step<7>(o, sh.Hb, sh.dx);
    o[63] = 1.0;
  }
}

}  // namespace

void launch_sim3(const Sim3Dev &d, hipStream_t st) {
  if (d.n_prob > 0) hipLaunchKernelGGL(k_sim3, dim3(d.n_prob), dim3(kS3Block), 0, st, d);
}

}  // namespace sqlm
