// sqlm_mappoint.hip — the device stages of LocalMapping's map-point steps
// (sqlm_triangulate_pairs, sqlm_map_points_update; host side: sqlm_mappoint.cpp).
//
// k_triangulate: the match loop of CreateNewMapPoints for every pair of the
// batch in one launch, one lane per match over the concatenated matches. A
// lane finds its pair by bisection over the host-built table of the pairs'
// first matches and evaluates tri_match (mappoint_dev.h) on its own match.
//
// k_mp_descriptor: ComputeDistinctiveDescriptors, a one-wavefront workgroup per
// map point. Lane l owns the rows l, l + 64, ... of the point's N x N distance
// matrix; a row's median is a count-based selection (mp_row_median), so no row
// is stored. A point of at most kMpLdsMax observations has its descriptors
// copied into LDS first (4 KB); a longer track reads them from global memory,
// every lane the same address at a time. The (median, row) minimum goes over
// the lanes by shuffles, the lower row winning among equal medians.
//
// k_mp_normal: UpdateNormalAndDepth, one lane per point: the float
// accumulation runs in list order, so a point is one sequential chain.
//
// No atomics, no wait on another workgroup; every loop is bounded by sizes the
// host set. What a match or a point stores depends on its own inputs alone.
//
// Built with -ffp-contract=off: the arithmetic is mappoint_dev.h, shared with
// the host, IEEE operations in the order written there.
#include "mappoint_dev.h"
#include "sqlm_internal.h"

#pragma clang fp contract(off)

namespace sqlm {

namespace {

__global__ void __launch_bounds__(kTriBlock) k_triangulate(TriDev d) {
  const int64_t i = (int64_t)blockIdx.x * kTriBlock + threadIdx.x;
  if (i >= d.n_match) return;
  // the pair p with first[p] <= i < first[p + 1]; empty pairs share a first match and are skipped
  int lo = 0, hi = d.n_pair - 1;
#pragma unroll 1
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int mid = (lo + hi + 1) >> 1;
    if (d.first[mid] <= i)
      lo = mid;
    else
      hi = mid - 1;
  }
  const TriPair P = d.pair[lo];
  const TriMatch m = d.match[i];
  float X[3];
  const uint8_t reason = tri_match(P, m, kTriSweeps, X);
  d.x3d[3 * i] = X[0];
  d.x3d[3 * i + 1] = X[1];
  d.x3d[3 * i + 2] = X[2];
  d.reason[i] = reason;
}

__device__ __forceinline__ void mp_best_rows(const uint32_t *D, const uint32_t *rows, int N, int lane, int &best_med,
                                             int &best_row) {
#pragma unroll 1
  for (int i = lane; i < N; i += 64) {
    uint32_t a[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] = rows[8 * (int64_t)i + k];
    const int med = mp_row_median(a, D, N);
    if (med < best_med) {  // rows ascend within a lane: the first of equals stays
      best_med = med;
      best_row = i;
    }
  }
}

__global__ void __launch_bounds__(64) k_mp_descriptor(MpDev d) {
  __shared__ uint32_t lds[8 * kMpLdsMax];
  const int pt = blockIdx.x;
  if (pt >= d.n_pt) return;
  const int lane = threadIdx.x & 63;
  const int64_t o0 = d.obs_off[pt];
  const int64_t n64 = d.obs_off[pt + 1] - o0;
  const int N = (int)n64;  // the host checked that a point's count fits an int
  const uint32_t *g = d.desc + 8 * o0;
  int best_med = INT32_MAX, best_row = -1;
  if (N <= kMpLdsMax) {  // uniform over the workgroup
    for (int k = lane; k < 8 * N; k += 64) lds[k] = g[k];
    __syncthreads();
    mp_best_rows(lds, lds, N, lane, best_med, best_row);
  } else {
    mp_best_rows(g, g, N, lane, best_med, best_row);
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const int om = __shfl_xor(best_med, s, 64), orow = __shfl_xor(best_row, s, 64);
    if (orow >= 0 && (best_row < 0 || om < best_med || (om == best_med && orow < best_row))) {
      best_med = om;
      best_row = orow;
    }
  }
  if (lane == 0) {
    d.best_idx[pt] = best_row;
    d.best_median[pt] = best_med;
  }
}

__global__ void __launch_bounds__(kMpNormalBlock) k_mp_normal(MpDev d) {
  const int64_t pt = (int64_t)blockIdx.x * kMpNormalBlock + threadIdx.x;
  if (pt >= d.n_pt) return;
  const int64_t o0 = d.obs_off[pt], n = d.obs_off[pt + 1] - o0;
  float nrm[3], mx, mn;
  mp_normal_depth(d.pos + 3 * pt, d.center + 3 * o0, n, d.ref_center + 3 * pt, d.level_scale[pt], d.max_scale[pt], nrm,
                  &mx, &mn);
  d.normal[3 * pt] = nrm[0];
  d.normal[3 * pt + 1] = nrm[1];
  d.normal[3 * pt + 2] = nrm[2];
  d.max_dist[pt] = mx;
  d.min_dist[pt] = mn;
}

}  // namespace

void launch_triangulate(const TriDev &d, hipStream_t st) {
  if (d.n_match <= 0) return;
  const unsigned grid = (unsigned)((d.n_match + kTriBlock - 1) / kTriBlock);
  hipLaunchKernelGGL(k_triangulate, dim3(grid), dim3(kTriBlock), 0, st, d);
}

void launch_mp_descriptor(const MpDev &d, hipStream_t st) {
  if (d.n_pt > 0) hipLaunchKernelGGL(k_mp_descriptor, dim3((unsigned)d.n_pt), dim3(64), 0, st, d);
}

void launch_mp_normal(const MpDev &d, hipStream_t st) {
  if (d.n_pt <= 0) return;
  const unsigned grid = (unsigned)((d.n_pt + kMpNormalBlock - 1) / kMpNormalBlock);
  hipLaunchKernelGGL(k_mp_normal, dim3(grid), dim3(kMpNormalBlock), 0, st, d);
}

}  // namespace sqlm
