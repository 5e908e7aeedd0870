// sqlm_lidar_depth.hip — the device stages of sqlm_lidar_depth (host side:
// sqlm_lidar_depth.cpp; arithmetic: lidar_depth_dev.h, shared with the host twin).
//
// The reference's loops carry state (the overwritten pixel, the first positive
// row, the strict nearest test, a sorted vector). Each is restated as an
// order-free rule (include/sqrtlm.h) and the stages below evaluate the rules:
//
// k_ld_point  a lane per input point: projection, then one atomicMax of
//             (index in sweep + 1) on the cell's winner (the last write of the
//             reference's loop is the greatest index); the writes are counted
//             with one integer atomicAdd per wavefront and frame.
// k_ld_pixel  a lane per pixel of the batch: the winner's depth (0.0 for an
//             unwritten pixel) into the double image, the occupied pixels
//             counted likewise, and atomicMax of rows - v for a positive pixel
//             (the lowest such row).
// k_ld_key    eight adjacent lanes per keypoint, one per dx: a lane walks the
//             fourteen dy of its column, so a patch row is one contiguous read
//             of the group; (min, max, nearest key) are reduced over the group
//             with three xor shuffles, then lane 0 of the group applies the
//             class rule and the unprojection.
//
// The atomics are integer maxima and sums on vector memory: their result does
// not depend on the order of arrival, so nothing depends on the batch or on the
// launch geometry. No workgroup waits on another; every loop is bounded by
// constants. All stores are plain vector stores; every index is checked
// against the sizes the host checked.
#include "lidar_depth_dev.h"
#include "sqlm_internal.h"

#pragma clang fp contract(off)

namespace sqlm {

namespace {

// the frame that owns item i of a packed array: the last f with off[f] <= i
__device__ __forceinline__ int ld_frame_of(const int64_t *off, int n_frame, int64_t i) {
  int lo = 0, hi = n_frame - 1;
#pragma unroll 1
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= i)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

// stats[4 f + slot] += the number of lanes with `hit`; one atomic per wavefront
// when its hits share a frame (the usual case), one per lane otherwise. Every
// lane of the wavefront calls it.
__device__ __forceinline__ void ld_count(int32_t *stats, int slot, bool hit, int f) {
  const unsigned long long w = __ballot(hit);
  if (!w) return;
  const int lane = threadIdx.x & 63, lead = __ffsll((long long)w) - 1;
  const int f0 = __shfl(f, lead);
  if (__all(!hit || f == f0)) {
    if (lane == lead) atomicAdd(stats + 4 * f0 + slot, __popcll(w));
  } else if (hit) {
    atomicAdd(stats + 4 * f + slot, 1);
  }
}

__global__ void __launch_bounds__(kLdBlock) k_ld_point(LdDev d) {
  const int64_t i = (int64_t)blockIdx.x * kLdBlock + threadIdx.x;
  int f = 0;
  bool writes = false;
  if (i < d.n) {
    f = ld_frame_of(d.sweep_off, d.n_frame, i);
    const int32_t pix = ld_project(d.c, d.xyz + 3 * i);
    d.pixel[i] = pix;
    const int64_t per = (int64_t)d.c.rows * d.c.cols;
    if (pix >= 0 && pix < per) {
      writes = true;
      atomicMax(d.winner + f * per + pix, (int32_t)(i - d.sweep_off[f]) + 1);
    }
  }
  ld_count(d.stats, 1, writes, f);
}

__global__ void __launch_bounds__(kLdBlock) k_ld_pixel(LdDev d) {
  const int64_t p = (int64_t)blockIdx.x * kLdBlock + threadIdx.x;
  int f = 0;
  bool occupied = false;
  if (p < d.cells) {
    const int64_t per = (int64_t)d.c.rows * d.c.cols;
    f = (int)(p / per);
    const int32_t w = d.winner[p];
    const int64_t n_f = d.sweep_off[f + 1] - d.sweep_off[f];
    double v = 0.0;
    if (w > 0 && w <= n_f) {
      occupied = true;
      v = ld_depth(d.c, d.xyz + 3 * (d.sweep_off[f] + (w - 1)));
    }
    d.image[p] = v;
    if (v > 0.0) {
      const int32_t key = d.c.rows - (int32_t)((p - f * per) / d.c.cols);
      int32_t *addr = d.stats + 4 * f;
      if (key > __hip_atomic_load(addr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(addr, key);
    }
  }
  ld_count(d.stats, 2, occupied, f);
}

__global__ void __launch_bounds__(kLdBlock) k_ld_key(LdDev d) {
  const int64_t t = (int64_t)blockIdx.x * kLdBlock + threadIdx.x;
  const int64_t k = t / kLdLanes;
  const int sub = (int)(t % kLdLanes);
  const bool live = k < d.m;  // uniform over a group of kLdLanes
  LdPatch a;
  ld_patch_init(&a);
  int f = 0;
  float px = 0.f, py = 0.f;
  bool below = true;
  const double *image = d.image;
  if (live) {
    f = ld_frame_of(d.key_off, d.n_frame, k);
    px = d.key_xy[2 * k];
    py = d.key_xy[2 * k + 1];
    const int32_t s0 = d.stats[4 * f];
    const int32_t min_v = (s0 > 0 && s0 <= d.c.rows) ? d.c.rows - s0 : 0;
    below = py < (float)min_v;
    image = d.image + (int64_t)f * d.c.rows * d.c.cols;
    if (!below) {
      const int dx = sub - SQLM_LD_HALF_W;
#pragma unroll
      for (int dy = -SQLM_LD_HALF_H; dy < SQLM_LD_HALF_H; ++dy) ld_patch_cell(d.c, image, px, py, dx, dy, &a);
    }
  }
  // every lane of the wavefront takes part; a group's lanes exchange among themselves only
#pragma unroll
  for (int step = 1; step < kLdLanes; step <<= 1) {
    LdPatch b;
    b.lo = __shfl_xor(a.lo, step);
    b.hi = __shfl_xor(a.hi, step);
    b.key = __shfl_xor(a.key, step);
    ld_patch_merge(&a, b);
  }
  bool with_depth = false;
  if (live && sub == 0) {
    LdKeyOut o;
    ld_classify(d.c, image, below, a, px, py, d.c.has_un ? d.key_un_xy + 2 * k : nullptr, &o);
    d.class_id[k] = o.cls;
    d.depth[k] = o.depth;
    d.nearest_uv[2 * k] = o.u;
    d.nearest_uv[2 * k + 1] = o.v;
    if (d.c.has_un) {
      d.xyz_cam[3 * k] = o.cam[0];
      d.xyz_cam[3 * k + 1] = o.cam[1];
      d.xyz_cam[3 * k + 2] = o.cam[2];
    }
    with_depth = o.depth > 0.0f;
  }
  ld_count(d.stats, 3, with_depth, f);
}

unsigned ld_blocks(int64_t items) { return items > 0 ? (unsigned)((items + kLdBlock - 1) / kLdBlock) : 1u; }

}  // namespace

int launch_lidar_depth(const LdDev &d, hipStream_t st) {
  hipLaunchKernelGGL(k_ld_point, dim3(ld_blocks(d.n)), dim3(kLdBlock), 0, st, d);
  hipLaunchKernelGGL(k_ld_pixel, dim3(ld_blocks(d.cells)), dim3(kLdBlock), 0, st, d);
  hipLaunchKernelGGL(k_ld_key, dim3(ld_blocks(d.m * kLdLanes)), dim3(kLdBlock), 0, st, d);
  return 3;
}

}  // namespace sqlm
