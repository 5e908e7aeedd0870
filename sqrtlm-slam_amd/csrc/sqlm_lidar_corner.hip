// sqlm_lidar_corner.hip — the device stages of the corner branch of
// sqlm_lidar_features_all (host side: sqlm_lidar_feat.cpp; arithmetic:
// lidar_corner_dev.h, shared with the host twin). They run after k_lf_row of
// sqlm_lidar_feat.hip has made the range image and the scans.
//
// The reference grows segments over a mutable range image while it walks the
// candidates in curvature order. What is expensive there is order-free and runs
// in parallel; what is sequential is an integer walk whose result does not
// depend on how a growth is evaluated (include/sqrtlm.h):
//
// k_lc_row     a workgroup per (sweep, ring): the initial state of the row's
//              cells (-3 / -1 / 0) and, on a corner ring, the corner mask.
// k_lc_edge    a lane per cell: the six directed offsets' angle and edge bit
//              (one acos, sin, cos, atan2 in double per pair; pairs with an
//              unoccupied or ground cell are skipped).
// k_lc_region  a workgroup per (sweep, ring, subregion): corner curvature, the
//              (curvature, index) sort in LDS, the static reasons (GROUND,
//              MASKED, CURVATURE) and the list of the other candidates, highest
//              rank first.
// k_lc_walk    a workgroup per sweep: rings, subregions and listed candidates in
//              order. A growth is a level-synchronous BFS by the whole workgroup
//              over the edge bits: a cell is claimed by an integer compare-and-swap
//              on its state (0 to the label), so a cell is claimed once whichever
//              lane wins; the claimed cell is appended to the sweep's queue through
//              an LDS counter (the order inside the queue is free, only the set is
//              used); row flags are an LDS OR. Fewer than 3 flagged rows: the queue
//              is rewritten to -2.
// k_lc_offsets one workgroup: the prefix sum of the regions' counts.
// k_lc_emit    a wavefront per region: the picked points to their output slots.
//
// The state image and the queue of a sweep are global memory that only that
// sweep's workgroup touches during the walk. Every access to them there is a
// relaxed agent-scope atomic (served by L2, not by the CU's L1), and a
// __syncthreads() stands between a lane's write and another lane's read, so a
// level sees the claims of the level before. No workgroup waits on another and
// there is no spin: every loop is bounded because a cell is claimed at most once
// and a queue holds at most row_num * col_num cells. All stores are plain vector
// stores or vector atomics. Nothing depends on the batch or on the launch geometry.
#include "lidar_corner_dev.h"
#include "sqlm_internal.h"

#pragma clang fp contract(off)

namespace sqlm {

namespace {

constexpr unsigned long long kNoKey = ~0ull;

__device__ __forceinline__ int32_t lc_ld(const int32_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void lc_st(int32_t *p, int32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ bool lc_row_on(const LcDev &d, int r, int n) {
  return d.p.ring_enabled[r] && n > d.f.p.min_scan;
}

__global__ void __launch_bounds__(kLfBlock) k_lc_row(LcDev d) {
  __shared__ uint8_t msk[SQLM_LF_MAX_COLS];
  const int q = blockIdx.x;
  if (q >= d.f.n_rows) return;
  const int r = q % d.f.p.row_num, cols = d.f.p.col_num;
  const int64_t base = (int64_t)q * cols;
  const float *scan = d.f.scan_xyz + 3 * base;
  for (int c = threadIdx.x; c < cols; c += kLfBlock) {
    const int idx = d.f.image_index[base + c];
    d.state[base + c] = idx < 0 || idx >= cols ? -3 : lc_initial_state(scan + 3 * (int64_t)idx, d.p.ground_z);
    msk[c] = 0;
  }
  const int n = d.f.scan_n[q];
  if (!lc_row_on(d, r, n)) return;  // uniform: the mask stays zero
  __syncthreads();
  const int c = d.p.ncr;
  for (int i = c + threadIdx.x; i + c < n; i += kLfBlock) {
    const int rule = lf_mask_rule(scan, i);
    if (rule == 1) {
      for (int t = i - c; t <= i; ++t) msk[t] = 1;
    } else if (rule == 2) {
      for (int t = i + 1; t <= i + c; ++t) msk[t] = 1;
    } else if (lc_mask_rule3(scan, i)) {
      msk[i] = 1;
    }
  }
  __syncthreads();
  for (int p = threadIdx.x; p < n; p += kLfBlock) d.mask[base + p] = msk[p];
}

__global__ void __launch_bounds__(kLfBlock) k_lc_edge(LcDev d) {
  const int cols = d.f.p.col_num, rows = d.f.p.row_num;
  const int64_t cell = (int64_t)blockIdx.x * kLfBlock + threadIdx.x;
  if (cell >= (int64_t)d.f.n_rows * cols) return;
  const int64_t q = cell / cols;
  const int col = (int)(cell - q * cols);
  const int s = (int)(q / rows), r = (int)(q - (int64_t)s * rows);
  const int64_t sbase = (int64_t)s * rows * cols;
  LfView v;
  v.image_index = d.f.image_index + sbase;
  v.scan_xyz = d.f.scan_xyz + 3 * sbase;
  v.scan_col = d.f.scan_col + sbase;
  v.row_num = rows;
  v.col_num = cols;
  float ang[kLcOffsets];
  const uint32_t bits = lc_edges(v, d.state + sbase, r, col, ang);
  if (!d.angle) {  // the read-back launch stores the angles alone
    d.edge[cell] = (uint8_t)bits;
    return;
  }
  if (d.angle)
    for (int k = 0; k < kLcOffsets; ++k) d.angle[kLcOffsets * cell + k] = ang[k];
}

__global__ void __launch_bounds__(kLfBlock) k_lc_region(LcDev d) {
  __shared__ unsigned long long key[SQLM_LF_MAX_COLS];
  const int n_sub = d.f.p.n_sub;
  const int g = blockIdx.x;
  if (g >= d.f.n_rows * n_sub) return;
  const int q = g / n_sub, j = g - q * n_sub;
  const int r = q % d.f.p.row_num;
  const int n = d.f.scan_n[q], cols = d.f.p.col_num;
  if (!lc_row_on(d, r, n)) return;
  int64_t sp, ep;
  lf_region(n, d.p.ncr, n_sub, j, &sp, &ep);
  if (ep <= sp) return;
  const int size = (int)(ep - sp + 1), npow = lf_pow2(size);
  const int64_t base = (int64_t)q * cols;
  const float *scan = d.f.scan_xyz + 3 * base;
  for (int k = threadIdx.x; k < npow; k += kLfBlock) {
    unsigned long long v = kNoKey;
    if (k < size) {
      const int i = (int)sp + k;
      const float cv = lc_curvature(scan, i, d.p.ncr);
      d.curv[base + i] = cv;
      v = ((unsigned long long)lf_bits(cv) << 32) | (unsigned)i;
    }
    key[k] = v;
  }
  __syncthreads();
  lf_sort(key, npow);
  for (int k = threadIdx.x; k < size; k += kLfBlock) d.sorted[base + sp + k] = (int32_t)(key[k] & 0xffffffffull);
  if (threadIdx.x >= 64) return;  // no barrier below
  const int lane = threadIdx.x;
  int cnt = 0;
#pragma unroll 1
  for (int k0 = size - 1; k0 >= 0; k0 -= 64) {
    const int k = k0 - lane;
    bool pass = false;
    if (k >= 0) {
      const unsigned long long kv = key[k];
      const int idx = (int)(kv & 0xffffffffull);
      const int64_t slot = base + idx;
      union {
        uint32_t u;
        float f;
      } cb;
      cb.u = (uint32_t)(kv >> 32);
      int code = SQLM_LC_NONE;
      if (d.state[base + d.f.scan_col[slot]] == -1)
        code = SQLM_LC_GROUND;
      else if (d.mask[slot])
        code = SQLM_LC_MASKED;
      else if (!((double)cb.f > d.p.curv_th))
        code = SQLM_LC_CURVATURE;
      d.reason[slot] = (uint8_t)code;
      pass = code == SQLM_LC_NONE;
    }
    const unsigned long long b = __ballot(pass);
    if (pass) d.cand[base + sp + cnt + __popcll(b & ((1ull << lane) - 1ull))] = k;
    cnt += __popcll(b);
  }
  if (lane == 0) d.cand_n[g] = cnt;
}

__global__ void __launch_bounds__(kLfBlock) k_lc_walk(LcDev d) {
  __shared__ int q_tail;
  __shared__ unsigned row_flag[SQLM_LF_MAX_ROWS / 32];
  const int s = blockIdx.x;
  if (s >= d.f.n_sweep) return;
  const int rows = d.f.p.row_num, cols = d.f.p.col_num, n_sub = d.f.p.n_sub, tid = threadIdx.x;
  const int n_cells = rows * cols;
  const int64_t sbase = (int64_t)s * n_cells;
  int32_t *state = d.state + sbase, *queue = d.queue + sbase;
  const uint8_t *edge = d.edge + sbase;
  int label = 1;
  int seeds = 0, labelled = 0, unstable = 0, largest = 0, most_levels = 0;  // uniform; lane 0 reports
#pragma unroll 1
  for (int r = 0; r < rows; ++r) {
    const int q = s * rows + r, n = d.f.scan_n[q];
    if (!lc_row_on(d, r, n)) continue;
    const int64_t base = (int64_t)q * cols;
#pragma unroll 1
    for (int j = 0; j < n_sub; ++j) {
      int64_t sp, ep;
      lf_region(n, d.p.ncr, n_sub, j, &sp, &ep);
      if (ep <= sp) continue;
      const int g = q * n_sub + j, nc = d.cand_n[g];
      int num = 0;
#pragma unroll 1
      for (int t = 0; t < nc; ++t) {
        const int k = d.cand[base + sp + t];
        const int64_t slot = base + d.sorted[base + sp + k];
        const int cell = r * cols + d.f.scan_col[slot];
        int st = lc_ld(state + cell);
        // Every lane has read the word before lane 0 may overwrite it below: without this barrier a
        // wavefront that runs behind would read the seed's label instead of 0 and skip the growth.
        // The last write to a state word (a claim or the -2 rewrite of an earlier growth) lies before
        // the barrier that ends that growth, so all lanes read the same value and the branch is uniform.
        __syncthreads();
        if (st == 0) {  // grow
          if (tid == 0) {
            lc_st(state + cell, label);
            lc_st(queue, cell);
            q_tail = 1;
            for (int w = 0; w < SQLM_LF_MAX_ROWS / 32; ++w) row_flag[w] = 0;
          }
          __syncthreads();
          int head = 0, tail = 1, levels = 0;
#pragma unroll 1
          while (head < tail) {
            for (int i = head + tid; i < tail; i += kLfBlock) {
              const int from = lc_ld(queue + i);
              const int fr = from / cols, fc = from - fr * cols;
              const uint32_t e = edge[from];
              for (int o = 0; o < kLcOffsets; ++o) {
                int tr, tc;
                if (!((e >> o) & 1u) || !lc_target(o, fr, fc, rows, cols, &tr, &tc)) continue;
                const int to = tr * cols + tc;
                if (lc_ld(state + to) != 0) continue;
                int expect = 0;
                if (!__hip_atomic_compare_exchange_strong(state + to, &expect, label, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                          __HIP_MEMORY_SCOPE_AGENT))
                  continue;
                const int pos = atomicAdd(&q_tail, 1);
                if (pos < n_cells) lc_st(queue + pos, to);  // always: a cell is claimed once
                atomicOr(&row_flag[tr >> 5], 1u << (tr & 31));
              }
            }
            __syncthreads();
            head = tail;
            tail = q_tail < n_cells ? q_tail : n_cells;
            ++levels;
            __syncthreads();
          }
          int lines = 0;
          for (int w = 0; w < SQLM_LF_MAX_ROWS / 32; ++w) lines += __popc(row_flag[w]);
          ++seeds;
          largest = tail > largest ? tail : largest;
          most_levels = levels > most_levels ? levels : most_levels;
          if (lines >= 3) {
            ++label;
            labelled += tail;
          } else {
            for (int i = tid; i < tail; i += kLfBlock) lc_st(state + lc_ld(queue + i), -2);
            unstable += tail;
          }
          __syncthreads();
          st = lc_ld(state + cell);
        }
        if (st < 1) {
          if (tid == 0) d.reason[slot] = SQLM_LC_UNSTABLE;
          continue;
        }
        if (num < d.p.max_less) {
          if (tid == 0) {
            d.reason[slot] = SQLM_LC_PICKED;
            d.ord[slot] = num;
            d.label[slot] = st;
          }
          ++num;
        } else if (tid == 0) {
          d.reason[slot] = SQLM_LC_OVER_CAP;
        }
        if (num >= d.p.max_less) {
          for (int kk = tid; kk < k; kk += kLfBlock) d.reason[base + d.sorted[base + sp + kk]] = SQLM_LC_OVER_CAP;
          break;
        }
      }
      if (tid == 0) d.region_cnt[g] = num;
    }
  }
  if (tid == 0) {
    atomicAdd(d.stats + 0, seeds);
    atomicAdd(d.stats + 1, labelled);
    atomicAdd(d.stats + 2, unstable);
    atomicMax(d.stats + 3, largest);
    atomicMax(d.stats + 4, most_levels);
  }
}

__global__ void __launch_bounds__(kLfBlock) k_lc_offsets(LcDev d) {
  __shared__ int64_t sl[kLfBlock], sf[kLfBlock];
  const int G = d.f.n_rows * d.f.p.n_sub, per_sweep = d.f.p.row_num * d.f.p.n_sub;
  const int chunk = (G + kLfBlock - 1) / kLfBlock;
  const int t = threadIdx.x, g0 = t * chunk < G ? t * chunk : G, g1 = g0 + chunk < G ? g0 + chunk : G;
  int64_t nl = 0, nf = 0;
  for (int g = g0; g < g1; ++g) {
    const int c = d.region_cnt[g];
    nl += c;
    nf += c < d.p.max_sharp ? c : d.p.max_sharp;
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
      d.sharp_off[g / per_sweep] = bf;
    }
    d.region_less[g] = bl;
    d.region_sharp[g] = bf;
    const int c = d.region_cnt[g];
    bl += c;
    bf += c < d.p.max_sharp ? c : d.p.max_sharp;
  }
  if (t == kLfBlock - 1) {
    d.less_off[d.f.n_sweep] = sl[t];
    d.sharp_off[d.f.n_sweep] = sf[t];
  }
}

__global__ void __launch_bounds__(64) k_lc_emit(LcDev d) {
  const int g = blockIdx.x;
  if (g >= d.f.n_rows * d.f.p.n_sub || d.region_cnt[g] == 0) return;
  const int q = g / d.f.p.n_sub, j = g - q * d.f.p.n_sub;
  const int r = q % d.f.p.row_num;
  int64_t sp, ep;
  lf_region(d.f.scan_n[q], d.p.ncr, d.f.p.n_sub, j, &sp, &ep);
  const int size = (int)(ep - sp + 1);
  const int64_t base = (int64_t)q * d.f.p.col_num;
  for (int k = threadIdx.x; k < size; k += 64) {
    const int64_t slot = base + d.sorted[base + sp + k];
    if (d.reason[slot] != SQLM_LC_PICKED) continue;
    const int o = d.ord[slot];
    const int64_t L = d.region_less[g] + o;
    if (L < 0 || L >= d.f.n) continue;  // cannot happen: a scan point is picked at most once
    lf_put(d.f, d.f.scan_xyz + 3 * slot, d.less_xyz + 3 * L);
    d.less_label[L] = d.label[slot];
    d.less_rc[2 * L] = r;
    d.less_rc[2 * L + 1] = d.f.scan_col[slot];
    if (o < d.p.max_sharp) {
      const int64_t F = d.region_sharp[g] + o;
      if (F >= 0 && F < d.f.n) lf_put(d.f, d.f.scan_xyz + 3 * slot, d.sharp_xyz + 3 * F);
    }
  }
}

}  // namespace

int launch_lidar_corner(const LcDev &d, hipStream_t st) {
  const unsigned regions = (unsigned)(d.f.n_rows * d.f.p.n_sub);
  const unsigned cells = (unsigned)(((int64_t)d.f.n_rows * d.f.p.col_num + kLfBlock - 1) / kLfBlock);
  hipLaunchKernelGGL(k_lc_row, dim3((unsigned)d.f.n_rows), dim3(kLfBlock), 0, st, d);
  hipLaunchKernelGGL(k_lc_edge, dim3(cells), dim3(kLfBlock), 0, st, d);
  hipLaunchKernelGGL(k_lc_region, dim3(regions), dim3(kLfBlock), 0, st, d);
  hipLaunchKernelGGL(k_lc_walk, dim3((unsigned)d.f.n_sweep), dim3(kLfBlock), 0, st, d);
  hipLaunchKernelGGL(k_lc_offsets, dim3(1), dim3(kLfBlock), 0, st, d);
  hipLaunchKernelGGL(k_lc_emit, dim3(regions), dim3(64), 0, st, d);
  return 6;
}

int launch_lidar_corner_angles(const LcDev &d, hipStream_t st) {
  const unsigned cells = (unsigned)(((int64_t)d.f.n_rows * d.f.p.col_num + kLfBlock - 1) / kLfBlock);
  hipLaunchKernelGGL(k_lc_edge, dim3(cells), dim3(kLfBlock), 0, st, d);
  return 1;
}

}  // namespace sqlm
