// sqlm_lidar_feat.hip — the device stages of sqlm_lidar_features (host side:
// sqlm_lidar_feat.cpp; arithmetic: lidar_feat_dev.h, shared with the host twin).
//
// The reference's loops carry state from one point to the next (halfPassed,
// the range image, index_num, the mask, the pick counter). Each is restated as
// an order-free rule (include/sqrtlm.h) and the stages below evaluate the rules:
//
// k_lf_point   a lane per input point: finite test, ring, raw azimuth; the
//              first / last kept index of the sweep by atomicMin / atomicMax.
// k_lf_half    a lane per kept point: the not-yet-passed branch against
//              startOri; halfPassed is the atomicMin of the indices that turn.
// k_lf_claim   a lane per kept point: column, then one 64-bit atomicMin of
//              (distance bits, index) on its cell (positive floats order as their
//              bits: least distance, lowest index among equals) and one of the
//              index (the cell's first arrival).
// k_lf_row     a workgroup per (sweep, ring): the row's occupied cells sorted
//              by first arrival in LDS (bitonic, at most 4096 keys) give the scan
//              order; the scan arrays, the range image's index and the ring mask.
// k_lf_region  a workgroup per (sweep, ring, subregion): curvature, the
//              (curvature, index) sort in LDS, then the first wavefront walks the
//              candidates in sorted order, a lane each and 64 per ballot, and
//              stops once the cap is met.
// k_lf_offsets one workgroup: the prefix sum of the regions' counts.
// k_lf_emit    a wavefront per region: the picked points to their output slots
//              through the extrinsic.
//
// The atomics are integer minima / maxima / sums on vector memory: their result
// does not depend on the order of arrival, so nothing depends on the batch or on
// the launch geometry. No workgroup waits on another; every loop is bounded by
// sizes the host checked. All stores are plain vector stores.
#include "lidar_corner_dev.h"
#include "sqlm_internal.h"

#pragma clang fp contract(off)

namespace sqlm {

namespace {

constexpr unsigned long long kNoKey = ~0ull;

__device__ __forceinline__ int lf_sweep_of(const LfDev &d, int64_t i) {
  int lo = 0, hi = d.n_sweep - 1;
#pragma unroll 1
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int mid = (lo + hi + 1) >> 1;
    if (d.sweep_off[mid] <= i)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ void lf_min_u32(uint32_t *addr, uint32_t v) {
  if (v < __hip_atomic_load(addr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(addr, v);
}

__global__ void __launch_bounds__(kLfBlock) k_lf_point(LfDev d) {
  const int64_t i = (int64_t)blockIdx.x * kLfBlock + threadIdx.x;
  if (i >= d.n) return;
  const int s = lf_sweep_of(d, i);
  const float x = d.xyz[3 * i], y = d.xyz[3 * i + 1], z = d.xyz[3 * i + 2];
  int ring = -1;
  if (lf_finite(x) && lf_finite(y) && lf_finite(z)) ring = lf_ring(x, y, z);
  d.ring[i] = ring;
  if (ring < 0) return;
  d.azi[i] = -lf_atan2f(y, x);
  const int32_t local = (int32_t)(i - d.sweep_off[s]);
  lf_min_u32(d.sweep_first + s, (uint32_t)local);
  if (local > __hip_atomic_load(d.sweep_last + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    atomicMax(d.sweep_last + s, local);
}

__global__ void __launch_bounds__(kLfBlock) k_lf_half(LfDev d) {
  const int64_t i = (int64_t)blockIdx.x * kLfBlock + threadIdx.x;
  if (i >= d.n || d.ring[i] < 0) return;
  const int s = lf_sweep_of(d, i);
  const int64_t o = d.sweep_off[s];
  const float start = (float)((double)d.azi[o + d.sweep_first[s]] + kLfPi);
  if (lf_turns_half(lf_unpassed(d.azi[i], start), start)) lf_min_u32(d.sweep_half + s, (uint32_t)(i - o));
}

__global__ void __launch_bounds__(kLfBlock) k_lf_claim(LfDev d) {
  const int64_t i = (int64_t)blockIdx.x * kLfBlock + threadIdx.x;
  if (i >= d.n) return;
  const int row = d.ring[i];
  if (row < 0 || row >= d.p.row_num) return;
  const int s = lf_sweep_of(d, i);
  const int64_t o = d.sweep_off[s];
  float start, end;
  lf_oris(d.azi[o + d.sweep_first[s]], d.azi[o + d.sweep_last[s]], &start, &end);
  const uint32_t local = (uint32_t)(i - o);
  const float a = local <= d.sweep_half[s] ? lf_unpassed(d.azi[i], start) : lf_passed(d.azi[i], end);
  const int col = lf_col(a, start, d.p.col_num);
  if (col < 0) return;
  const int64_t cell = ((int64_t)s * d.p.row_num + row) * d.p.col_num + col;
  const unsigned long long key = ((unsigned long long)lf_bits(lf_dist(d.xyz + 3 * i)) << 32) | local;
  atomicMin(d.cell_key + cell, key);
  atomicMin(d.cell_first + cell, local);
}

__global__ void __launch_bounds__(kLfBlock) k_lf_row(LfDev d) {
  __shared__ unsigned long long key[SQLM_LF_MAX_COLS];
  __shared__ uint8_t msk[SQLM_LF_MAX_COLS];
  __shared__ int n_sh;
  const int q = blockIdx.x;
  if (q >= d.n_rows) return;
  const int s = q / d.p.row_num, r = q - s * d.p.row_num;
  const int cols = d.p.col_num, npow = lf_pow2(cols);
  const int64_t base = (int64_t)q * cols;
  for (int c = threadIdx.x; c < npow; c += kLfBlock) {
    unsigned long long k = kNoKey;
    if (c < cols) {
      const uint32_t f = d.cell_first[base + c];
      if (f != kLfNoIndex) k = ((unsigned long long)f << 12) | (unsigned)c;
    }
    key[c] = k;
    if (c < cols) msk[c] = 0;
  }
  if (threadIdx.x == 0) n_sh = 0;
  __syncthreads();
  lf_sort(key, npow);
  for (int p = threadIdx.x; p < npow; p += kLfBlock)
    if (key[p] != kNoKey && (p + 1 == npow || key[p + 1] == kNoKey)) n_sh = p + 1;
  __syncthreads();
  const int n = n_sh < cols ? n_sh : cols;
  const int64_t o = d.sweep_off[s];
  for (int p = threadIdx.x; p < n; p += kLfBlock) {
    const int c = (int)(key[p] & 4095u);
    const uint32_t occ = (uint32_t)(d.cell_key[base + c] & 0xffffffffull);
    d.scan_src[base + p] = (int32_t)occ;
    d.scan_col[base + p] = c;
    const float *src = d.xyz + 3 * (o + occ);
    float *dst = d.scan_xyz + 3 * (base + p);
    dst[0] = src[0];
    dst[1] = src[1];
    dst[2] = src[2];
    d.image_index[base + c] = p;
  }
  if (threadIdx.x == 0) d.scan_n[q] = n;
  if (!d.p.ring_enabled[r] || n <= d.p.min_scan) return;  // uniform: the mask stays zero
  __syncthreads();
  const int c = d.p.ncr;
  const float *scan = d.scan_xyz + 3 * base;
  for (int i = c + threadIdx.x; i + c < n; i += kLfBlock) {
    const int rule = lf_mask_rule(scan, i);
    if (rule == 1)
      for (int t = i - c; t <= i; ++t) msk[t] = 1;
    else if (rule == 2)
      for (int t = i + 1; t <= i + c; ++t) msk[t] = 1;
  }
  __syncthreads();
  for (int p = threadIdx.x; p < n; p += kLfBlock) d.mask[base + p] = msk[p];
}

__global__ void __launch_bounds__(kLfBlock) k_lf_region(LfDev d) {
  __shared__ unsigned long long key[SQLM_LF_MAX_COLS];
  const int g = blockIdx.x;
  if (g >= d.n_rows * d.p.n_sub) return;
  const int q = g / d.p.n_sub, j = g - q * d.p.n_sub;
  const int s = q / d.p.row_num, r = q - s * d.p.row_num;
  const int n = d.scan_n[q], cols = d.p.col_num;
  if (!d.p.ring_enabled[r] || n <= d.p.min_scan) return;
  int64_t sp, ep;
  lf_region(n, d.p.ncr, d.p.n_sub, j, &sp, &ep);
  if (ep <= sp) return;
  const int size = (int)(ep - sp + 1), npow = lf_pow2(size);
  const int64_t base = (int64_t)q * cols;
  const float *scan = d.scan_xyz + 3 * base;
  for (int k = threadIdx.x; k < npow; k += kLfBlock) {
    unsigned long long v = kNoKey;
    if (k < size) {
      const int i = (int)sp + k;
      int nb;
      const float cv = lf_curvature(scan, i, n, d.p.ncr, &nb);
      d.curv[base + i] = cv;
      d.nbr[base + i] = nb;
      v = ((unsigned long long)lf_bits(cv) << 32) | (unsigned)i;
    }
    key[k] = v;
  }
  __syncthreads();
  lf_sort(key, npow);
  for (int k = threadIdx.x; k < size; k += kLfBlock) d.sorted[base + sp + k] = (int32_t)(key[k] & 0xffffffffull);
  if (threadIdx.x >= 64) return;  // no barrier below
  const int lane = threadIdx.x;
  LfView v;
  v.image_index = d.image_index + (int64_t)s * d.p.row_num * cols;
  v.scan_xyz = d.scan_xyz + 3 * (int64_t)s * d.p.row_num * cols;
  v.scan_col = d.scan_col + (int64_t)s * d.p.row_num * cols;
  v.row_num = d.p.row_num;
  v.col_num = cols;
  const int cap = d.p.max_less, target = (cap > 1 ? cap : 1) - 1;
  int picked = 0, evaluated = 0, k0 = 0;
  bool stop = false;
#pragma unroll 1
  for (; k0 < size && !stop; k0 += 64) {
    const int k = k0 + lane;
    int code = SQLM_LF_NONE;
    int64_t slot = 0;
    float nrm[3] = {0.f, 0.f, 0.f};
    if (k < size) {
      const unsigned long long kv = key[k];
      const int idx = (int)(kv & 0xffffffffull);
      slot = base + idx;
      union {
        uint32_t u;
        float f;
      } cb;
      cb.u = (uint32_t)(kv >> 32);
      if (d.mask[slot])
        code = SQLM_LF_MASKED;
      else if (!((double)cb.f < d.p.curv_th))
        code = SQLM_LF_CURVATURE;
      else
        code = lf_candidate(v, d.p, r, idx, nrm);
    }
    const unsigned long long valid = __ballot(code == SQLM_LF_PICKED);
    const int my = picked + __popcll(valid & ((1ull << lane) - 1ull));
    const unsigned long long sm = __ballot(code == SQLM_LF_PICKED && my == target);
    const int stop_lane = sm ? __ffsll((long long)sm) - 1 : 64;
    if (k < size) {
      if (lane > stop_lane || (code == SQLM_LF_PICKED && my >= cap)) code = SQLM_LF_OVER_CAP;
      d.reason[slot] = (uint8_t)code;
      if (code == SQLM_LF_PICKED) {
        d.normal[3 * slot] = nrm[0];
        d.normal[3 * slot + 1] = nrm[1];
        d.normal[3 * slot + 2] = nrm[2];
        d.ord[slot] = my;
      }
    }
    picked += __popcll(__ballot(k < size && code == SQLM_LF_PICKED));
    evaluated += size - k0 < 64 ? size - k0 : 64;
    stop = stop_lane < 64;
  }
  for (int k = k0 + lane; k < size; k += 64) d.reason[base + (int)(key[k] & 0xffffffffull)] = SQLM_LF_OVER_CAP;
  if (lane == 0) {
    d.region_cnt[g] = picked;
    atomicMax(d.stats + 0, size);
    atomicAdd(d.stats + 1, size);
    atomicAdd(d.stats + 2, evaluated);
    atomicAdd(d.stats + 3, picked);
  }
}

__global__ void __launch_bounds__(kLfBlock) k_lf_offsets(LfDev d) {
  __shared__ int64_t sl[kLfBlock], sf[kLfBlock];
  const int G = d.n_rows * d.p.n_sub, per_sweep = d.p.row_num * d.p.n_sub;
  const int chunk = (G + kLfBlock - 1) / kLfBlock;
  const int t = threadIdx.x, g0 = t * chunk, g1 = g0 + chunk < G ? g0 + chunk : G;
  int64_t nl = 0, nf = 0;
  for (int g = g0; g < g1; ++g) {
    const int c = d.region_cnt[g];
    nl += c;
    nf += c < d.p.max_flat ? c : d.p.max_flat;
  }
  sl[t] = nl;
  sf[t] = nf;
  __syncthreads();
  for (int step = 1; step < kLfBlock; step <<= 1) {
    const int64_t al = t >= step ? sl[t - step] : 0, af = t >= step ? sf[t - step] : 0;
    __syncthreads();
    sl[t] += al;
    sf[t] += af;
    __syncthreads();
  }
  int64_t bl = sl[t] - nl, bf = sf[t] - nf;
  for (int g = g0; g < g1; ++g) {
    if (g % per_sweep == 0) {
      d.less_off[g / per_sweep] = bl;
      d.flat_off[g / per_sweep] = bf;
    }
    d.region_less[g] = bl;
    d.region_flat[g] = bf;
    const int c = d.region_cnt[g];
    bl += c;
    bf += c < d.p.max_flat ? c : d.p.max_flat;
  }
  if (t == kLfBlock - 1) {
    d.less_off[d.n_sweep] = sl[t];
    d.flat_off[d.n_sweep] = sf[t];
  }
}

__global__ void __launch_bounds__(64) k_lf_emit(LfDev d) {
  const int g = blockIdx.x;
  if (g >= d.n_rows * d.p.n_sub || d.region_cnt[g] == 0) return;
  const int q = g / d.p.n_sub, j = g - q * d.p.n_sub;
  const int r = q % d.p.row_num;
  int64_t sp, ep;
  lf_region(d.scan_n[q], d.p.ncr, d.p.n_sub, j, &sp, &ep);
  const int size = (int)(ep - sp + 1);
  const int64_t base = (int64_t)q * d.p.col_num;
  for (int k = threadIdx.x; k < size; k += 64) {
    const int64_t slot = base + d.sorted[base + sp + k];
    if (d.reason[slot] != SQLM_LF_PICKED) continue;
    const int o = d.ord[slot];
    const int64_t L = d.region_less[g] + o;
    if (L >= d.n) continue;  // cannot happen: a scan point is picked at most once
    lf_put(d, d.scan_xyz + 3 * slot, d.less_xyz + 3 * L);
    lf_put(d, d.normal + 3 * slot, d.less_normal + 3 * L);
    d.less_rc[2 * L] = r;
    d.less_rc[2 * L + 1] = d.scan_col[slot];
    if (o < d.p.max_flat) {
      const int64_t F = d.region_flat[g] + o;
      lf_put(d, d.scan_xyz + 3 * slot, d.flat_xyz + 3 * F);
      lf_put(d, d.normal + 3 * slot, d.flat_normal + 3 * F);
    }
  }
}

}  // namespace

int launch_lidar_feat_image(const LfDev &d, hipStream_t st) {
  const unsigned pts = (unsigned)((d.n + kLfBlock - 1) / kLfBlock);
  hipLaunchKernelGGL(k_lf_point, dim3(pts), dim3(kLfBlock), 0, st, d);
  hipLaunchKernelGGL(k_lf_half, dim3(pts), dim3(kLfBlock), 0, st, d);
  hipLaunchKernelGGL(k_lf_claim, dim3(pts), dim3(kLfBlock), 0, st, d);
  hipLaunchKernelGGL(k_lf_row, dim3((unsigned)d.n_rows), dim3(kLfBlock), 0, st, d);
  return 4;
}

int launch_lidar_feat_flat(const LfDev &d, hipStream_t st) {
  const unsigned regions = (unsigned)(d.n_rows * d.p.n_sub);
  hipLaunchKernelGGL(k_lf_region, dim3(regions), dim3(kLfBlock), 0, st, d);
  hipLaunchKernelGGL(k_lf_offsets, dim3(1), dim3(kLfBlock), 0, st, d);
  hipLaunchKernelGGL(k_lf_emit, dim3(regions), dim3(64), 0, st, d);
  return 3;
}

}  // namespace sqlm
