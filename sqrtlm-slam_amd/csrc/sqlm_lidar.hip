// sqlm_lidar.hip — LiDAR nearest-neighbour association on the device: the
// kd-tree search of LocalBundleAdjustment's pass 3 (g2oOptimizer.cc:978-1073)
// and of PoseOptimization (:560-630) restated as an exact brute-force 1-NN.
//
// Three launches on the context's stream:
//   k_lidar_transform  sensor-frame clouds -> world float4 (pcl::transformPointCloud
//                      with an Eigen::Affine3d built from the float Twc, :985-1010)
//   k_lidar_search     a workgroup keeps kLidarW queries in registers and walks one
//                      segment of the map in LDS tiles of kLidarT points; the
//                      distance is FLANN's L2_Simple<float> in float, no FMA
//   k_lidar_emit       threshold test (:1045), exclusive scan of the accept
//                      flags, the accepted queries in query order
// This file is built with -ffp-contract=off: every float that decides a result
// comes from IEEE operations in the order written here.
#include "sqlm_internal.h"

#pragma clang fp contract(off)

namespace sqlm {

namespace {

constexpr unsigned long long kNoBest = ~0ull;

// out = (float)(((m0 x + m1 y) + m2 z) + m3) per row, in double: PCL's dense
// transformPointCloud with an Affine3d whose entries are the float Twc widened
__device__ inline float4 to_world(const float *M, float x, float y, float z) {
  const double dx = (double)x, dy = (double)y, dz = (double)z;
  float4 o;
  o.x = (float)((((double)M[0] * dx + (double)M[1] * dy) + (double)M[2] * dz) + (double)M[3]);
  o.y = (float)((((double)M[4] * dx + (double)M[5] * dy) + (double)M[6] * dz) + (double)M[7]);
  o.z = (float)((((double)M[8] * dx + (double)M[9] * dy) + (double)M[10] * dz) + (double)M[11]);
  o.w = 0.f;
  return o;
}

// one thread per map point, then one per query point
__global__ void __launch_bounds__(256) k_lidar_transform(LidarDev d) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < d.n_map) {
    const float x = d.map_xyz[3 * i], y = d.map_xyz[3 * i + 1], z = d.map_xyz[3 * i + 2];
    if (!d.has_Twc) {
      d.map_w[i] = make_float4(x, y, z, 0.f);
      return;
    }
    // the cloud of point i: the last c with map_off[c] <= i (empty clouds skipped)
    int lo = 0, hi = d.n_clouds;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (d.map_off[mid] <= i) lo = mid;
      else hi = mid;
    }
    d.map_w[i] = to_world(d.map_Twc + 16 * (int64_t)lo, x, y, z);
    return;
  }
  const int64_t j = i - d.n_map;
  if (j < d.n_query) {
    d.query_w[j] = to_world(d.query_Twc, d.query_xyz[3 * j], d.query_xyz[3 * j + 1], d.query_xyz[3 * j + 2]);
    d.best[j] = kNoBest;
  }
}

// grid (query tiles, map segments). Every lane reads the same LDS point at the
// same time (a broadcast); a lane's scan is in ascending map index with a
// strict <, so it keeps the lowest index among equal distances, and the 64-bit
// atomicMin over (bits of d2, index) does the same across segments: d2 >= 0
// makes the float's bit pattern monotone, so the result does not depend on the
// order the segments arrive in, nor on their number.
__global__ void __launch_bounds__(kLidarBlock) k_lidar_search(LidarDev d) {
  __shared__ float4 tile[kLidarT];
  const int tid = threadIdx.x;
  const int64_t q0 = (int64_t)blockIdx.x * kLidarW + tid;
  float qx[kLidarQpl], qy[kLidarQpl], qz[kLidarQpl], bd[kLidarQpl];
  int bi[kLidarQpl];
#pragma unroll
  for (int k = 0; k < kLidarQpl; ++k) {
    const int64_t i = q0 + (int64_t)k * kLidarBlock;
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < d.n_query) q = d.query_w[i];
    qx[k] = q.x; qy[k] = q.y; qz[k] = q.z;
    bd[k] = INFINITY;
    bi[k] = -1;
  }
  const int64_t begin = (int64_t)blockIdx.y * d.seg_len;
  const int64_t end = begin + d.seg_len < (int64_t)d.n_map ? begin + d.seg_len : (int64_t)d.n_map;
  for (int64_t base = begin; base < end; base += kLidarT) {
    const int cnt = end - base < kLidarT ? (int)(end - base) : kLidarT;
    __syncthreads();
    for (int j = tid; j < cnt; j += kLidarBlock) tile[j] = d.map_w[base + j];
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < cnt; ++j) {
      const float4 m = tile[j];
#pragma unroll
      for (int k = 0; k < kLidarQpl; ++k) {
        const float dx = qx[k] - m.x, dy = qy[k] - m.y, dz = qz[k] - m.z;
        const float d2 = ((dx * dx) + dy * dy) + dz * dz;
        if (d2 < bd[k]) {
          bd[k] = d2;
          bi[k] = (int)base + j;
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kLidarQpl; ++k) {
    const int64_t i = q0 + (int64_t)k * kLidarBlock;
    if (i < d.n_query && bi[k] >= 0)
      atomicMin(&d.best[i], ((unsigned long long)__float_as_uint(bd[k]) << 32) | (unsigned)bi[k]);
  }
}

// one workgroup walks the queries in order, kLidarEmitBlock at a time, and
// carries the running pair count: the pairs come out in query order
__global__ void __launch_bounds__(kLidarEmitBlock) k_lidar_emit(LidarDev d) {
  __shared__ int wsum[kLidarEmitBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int carry = 0;  // every thread keeps the same copy
  for (int64_t base = 0; base < d.n_query; base += kLidarEmitBlock) {
    const int64_t i = base + tid;
    int flag = 0;
    if (i < d.n_query) {
      const unsigned long long b = d.best[i];
      const unsigned idx = (unsigned)(b & 0xffffffffull);
      int32_t out_i = -1;
      float d2 = INFINITY;
      float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
      if (b != kNoBest && idx < (unsigned)d.n_map) {
        out_i = (int32_t)idx;
        d2 = __uint_as_float((unsigned)(b >> 32));
        m = d.map_w[idx];
        flag = (double)d2 < d.thr;  // strict, in double (:1045)
      }
      d.nn_index[i] = out_i;
      d.nn_sq_dist[i] = d2;
      d.nn_xyz[3 * i] = m.x;
      d.nn_xyz[3 * i + 1] = m.y;
      d.nn_xyz[3 * i + 2] = m.z;
      d.accepted[i] = (uint8_t)flag;
    }
    const unsigned long long bal = __ballot(flag);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wave] = __popcll(bal);
    __syncthreads();
    int woff = 0, total = 0;
    for (int w = 0; w < kLidarEmitBlock / 64; ++w) {
      if (w < wave) woff += wsum[w];
      total += wsum[w];
    }
    if (flag) d.pair_query[carry + woff + before] = (int32_t)i;
    carry += total;
    __syncthreads();
  }
  if (tid == 0) *d.n_pairs = carry;
}

}  // namespace

void launch_lidar(const LidarDev &d, hipStream_t st) {
  const int64_t n = (int64_t)d.n_map + d.n_query;
  hipLaunchKernelGGL(k_lidar_transform, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d);
  if (d.n_map > 0)
    hipLaunchKernelGGL(k_lidar_search, dim3((unsigned)((d.n_query + kLidarW - 1) / kLidarW), (unsigned)d.n_seg),
                       dim3(kLidarBlock), 0, st, d);
  hipLaunchKernelGGL(k_lidar_emit, dim3(1), dim3(kLidarEmitBlock), 0, st, d);
}

}  // namespace sqlm
