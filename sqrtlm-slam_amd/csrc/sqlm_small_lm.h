// sqlm_small_lm.h — device code shared by the batched small-LM kernels
// (sqlm_sim3.hip: one Sim3 vertex, N = 7; sqlm_pose.hip: one SE3 vertex,
// N = 6): one workgroup per problem, lanes stride over the edges, thread 0
// solves the damped N x N system and applies lm_decide.
//
// Layout shared by both: the accumulator a lane carries, and sh.Hb after the
// reduction, is the upper triangle of H packed row-major (N (N + 1) / 2), then
// b (N), then the robust chi2. Sh is the kernel's LDS struct and must have
// double red[NW][NACC], Hb[NACC], bsum.
//
// Every sum is taken in a fixed order (wave butterfly, then the waves in wave
// order), and these kernels are pinned bit for bit to references: change an
// operation's order here and both change.
//
// Not here: the J^T W J / J^T r accumulation of an edge into the lane's
// accumulator. As a function it compiles to a different instruction schedule
// than written out in linearize(), so each kernel keeps its own copy.
#pragma once
#include <hip/hip_runtime.h>

#include "sqlm_internal.h"

namespace sqlm {

namespace {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// Sum over the workgroup, waves added in wave order; every thread gets it.
template <int NW, class Sh>
__device__ double block_sum(Sh &sh, double v) {
  v = wave_sum(v);
  __syncthreads();  // the previous use of red / bsum is over
  if ((threadIdx.x & 63) == 0) sh.red[threadIdx.x >> 6][0] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double r = sh.red[0][0];
    for (int w = 1; w < NW; ++w) r += sh.red[w][0];
    sh.bsum = r;
  }
  __syncthreads();
  return sh.bsum;
}

// The tail of a linearization: every lane's accumulator summed into sh.Hb.
template <int NACC, int NW, class Sh>
__device__ __forceinline__ void reduce_acc(Sh &sh, double (&acc)[NACC]) {
#pragma unroll
  for (int k = 0; k < NACC; ++k) acc[k] = wave_sum(acc[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < NACC; ++k) sh.red[threadIdx.x >> 6][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < NACC) {
    double r = sh.red[0][threadIdx.x];
    for (int w = 1; w < NW; ++w) r += sh.red[w][threadIdx.x];
    sh.Hb[threadIdx.x] = r;
  }
  __syncthreads();
}

// RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91): rho, rho'; no
// kernel (!robust): rho = chi2, rho' = 1
__device__ __forceinline__ void huber(double chi, bool robust, double delta, double dsqr, double &rho0, double &rho1) {
  if (!robust || chi <= dsqr) {
    rho0 = chi;
    rho1 = 1.0;
  } else {
    const double sq = sqrt(chi);
    rho0 = 2 * sq * delta - dsqr;
    rho1 = delta / sq;
  }
}

// (H + lambda I) dx = b by Cholesky (LinearSolverDense, linear_solver_dense.h:
// 100-118: a non-positive pivot is a failed solve, the step is rejected and
// dx = 0). Hb: packed upper triangle, b.
template <int N>
__device__ bool chol_solve(const double *Hb, double lambda, double dx[N]) {
  double A[N][N];
  int k = 0;
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = i; j < N; ++j) A[j][i] = Hb[k++];
#pragma unroll
  for (int i = 0; i < N; ++i) A[i][i] += lambda;
  bool ok = true;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double dj = A[j][j];
#pragma unroll
    for (int c = 0; c < j; ++c) dj -= A[j][c] * A[j][c];
    if (!(dj > 0.0)) ok = false;
    dj = sqrt(dj);
    A[j][j] = dj;
#pragma unroll
    for (int i = j + 1; i < N; ++i) {
      double s = A[i][j];
#pragma unroll
      for (int c = 0; c < j; ++c) s -= A[i][c] * A[j][c];
      A[i][j] = s / dj;
    }
  }
  double y[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double s = Hb[N * (N + 1) / 2 + i];
#pragma unroll
    for (int c = 0; c < i; ++c) s -= A[i][c] * y[c];
    y[i] = s / A[i][i];
  }
#pragma unroll
  for (int i = N - 1; i >= 0; --i) {
    double s = y[i];
#pragma unroll
    for (int c = i + 1; c < N; ++c) s -= A[c][i] * dx[c];
    dx[i] = s / A[i][i];
  }
  if (!ok) {
#pragma unroll
    for (int i = 0; i < N; ++i) dx[i] = 0.0;
  }
  return ok;
}

// The LM state at the head of a stage (one thread).
__device__ __forceinline__ void lm_reset(LMCtl &L, int niter, bool done) {
  L.lambda = 0.0; L.ni = 2.0; L.currentChi = 0.0; L.iniChi = 0.0; L.chi2_end = 0.0; L.lambda_end = 0.0;
  L.qmax = 0; L.nbad = 0; L.its = 0; L.result = 0; L.trials = 0; L.iterations = niter; L.bench = 0;
  L.done = done;
}

// computeLambdaInit: the user's lambda, else 1e-5 max |H_ii|
template <int N>
__device__ __forceinline__ double lm_lambda_init(const double *Hb, double user_lambda) {
  double md = 0.0;
  int k = 0;
  for (int i = 0; i < N; ++i) { md = fmax(fabs(Hb[k]), md); k += N - i; }
  return user_lambda > 0 ? user_lambda : 1e-5 * md;
}

// computeScale: dx^T (lambda dx + b)
template <int N>
__device__ __forceinline__ double lm_scale(const double *Hb, const double *dx, double lambda) {
  double scale = 0.0;
  for (int j = 0; j < N; ++j) scale += dx[j] * (lambda * dx[j] + Hb[N * (N + 1) / 2 + j]);
  return scale;
}

// A finished stage's outcome into the problem's stats (one thread).
template <class Stats>
__device__ __forceinline__ void lm_store_stage(Stats *st, int stage, const LMCtl &L) {
  st->iterations[stage] = L.its;
  st->trials[stage] = L.trials;
  st->result[stage] = L.result;
  st->chi2_end[stage] = L.chi2_end;
  st->lambda_end[stage] = L.lambda_end;
}

// The last trial's system for *_get_last_step: H (N x N, full symmetric), b, dx.
template <int N>
__device__ __forceinline__ void store_last_step(double *o, const double *Hb, const double *dx) {
  int k = 0;
  for (int i = 0; i < N; ++i)
    for (int j = i; j < N; ++j) { o[N * i + j] = Hb[k]; o[N * j + i] = Hb[k]; ++k; }
  for (int j = 0; j < N; ++j) { o[N * N + j] = Hb[N * (N + 1) / 2 + j]; o[N * N + N + j] = dx[j]; }
}

}  // namespace

}  // namespace sqlm
