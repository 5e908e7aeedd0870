// sqlm_bow.hip — the DBoW2 vocabulary on the device (include/sqrtlm_orb.h):
// the per-feature descent of TemplatedVocabulary::transform and the batched
// L1Scoring::score. Both are integer work or one fixed-order double chain, so
// their results equal the sequential definition bit for bit; the file is
// compiled with -ffp-contract=off like the rest of the ORB path.
//
// Both kernels give kBowGroup = 16 adjacent lanes to one item (a feature, a
// database vector), four items to a wavefront. Every loop around a cross-lane
// operation runs a wavefront-uniform number of times and an item that has
// finished is predicated off, so no shuffle reads a lane that is switched off
// and no item's result depends on which items share its wavefront.
#include <hip/hip_runtime.h>

#include "sqlm_internal.h"

namespace sqlm {

namespace {

constexpr int kBowBlock = 256;
constexpr int kBowItems = kBowBlock / kBowGroup;  // items of one workgroup

// One feature per lane group. Each level: the group reads the current node's
// child run (lane s takes children s, s + 16: one coalesced read of 32-byte
// descriptors for k <= 16, a second for 17..20), every lane keeps the smallest
// (distance << 8 | child slot) of its own children with that child's table
// entry, the group takes the minimum — the smallest distance, among equals the
// first child — and the owning lane hands the entry round. One dependent
// memory round trip per level. The descent stops at the first childless node;
// groups of one wavefront stop at different depths in a ragged tree. Beside
// the word and the FeatureVector node the kernel returns the word's weight.
__global__ __launch_bounds__(kBowBlock) void k_bow_descend(BowVocDev v, const uint4 *__restrict__ feat, int n_feat,
                                                           int nid_level, int32_t *__restrict__ word,
                                                           int32_t *__restrict__ node, double *__restrict__ weight) {
  const int lane = threadIdx.x & (kBowGroup - 1);
  const int64_t f = ((int64_t)blockIdx.x * kBowBlock + threadIdx.x) / kBowGroup;
  const bool live = f < n_feat;
  uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0;
  if (live) {
    q0 = feat[2 * f];
    q1 = feat[2 * f + 1];
  }
  // the root is node 0 and its children start at 1
  int begin = 1, count = live ? v.root_count : 0;
  int cur = 0, leaf_word = -1;
  int sel = nid_level <= 0 ? 0 : -1;
  for (int depth = 1; depth <= v.max_depth; ++depth) {
    uint32_t key = 0xffffffffu;
    BowNode mine = {0, 0, 0, -1};
    for (int slot = lane; slot < count; slot += kBowGroup) {
      const size_t c = (size_t)begin + slot;
      const uint4 a = v.desc[2 * c], b = v.desc[2 * c + 1];
      const BowNode t = v.tab[c];
      const int dist = __popc(a.x ^ q0.x) + __popc(a.y ^ q0.y) + __popc(a.z ^ q0.z) + __popc(a.w ^ q0.w) +
                       __popc(b.x ^ q1.x) + __popc(b.y ^ q1.y) + __popc(b.z ^ q1.z) + __popc(b.w ^ q1.w);
      const uint32_t kk = ((uint32_t)dist << 8) | (uint32_t)slot;
      if (kk < key) {
        key = kk;
        mine = t;
      }
    }
    uint32_t best = key;
    for (int o = kBowGroup / 2; o > 0; o >>= 1) best = min(best, (uint32_t)__shfl_xor((int)best, o, kBowGroup));
    const int src = (int)(best & 0xffu) & (kBowGroup - 1);  // the lane that holds the winning child
    BowNode w;
    w.child_begin = __shfl(mine.child_begin, src, kBowGroup);
    w.child_count = __shfl(mine.child_count, src, kBowGroup);
    w.orig = __shfl(mine.orig, src, kBowGroup);
    w.word = __shfl(mine.word, src, kBowGroup);
    if (count > 0) {
      begin = w.child_begin;
      count = w.child_count;
      cur = w.orig;
      leaf_word = w.word;
      if (depth == nid_level) sel = cur;
    }
  }
  if (live && lane == 0) {
    if (sel < 0) sel = cur;  // the leaf sits above depth nid_level
    const bool stop = leaf_word < 0;
    word[f] = stop ? -1 : leaf_word;
    node[f] = stop ? -1 : sel;
    weight[f] = stop ? 0.0 : v.weight[leaf_word];  // gathered here: on the host it is a cache miss per feature
  }
}

// One database vector per lane group, the query in LDS (or, longer than
// kBowScoreLds, in memory). The group reads 16 consecutive entries of its
// vector, every lane looks its word up in the query by binary search and forms
// its term; the terms of the common words are then added in ascending word id
// as one chain, the same chain in all 16 lanes.
template <bool LDS>
__global__ __launch_bounds__(kBowBlock) void k_bow_score(int nq, const int32_t *__restrict__ q_word,
                                                         const double *__restrict__ q_value, int n_db,
                                                         const int64_t *__restrict__ db_off,
                                                         const int32_t *__restrict__ db_word,
                                                         const double *__restrict__ db_value,
                                                         double *__restrict__ score, int32_t *__restrict__ n_common) {
  __shared__ int32_t s_word[LDS ? kBowScoreLds : 1];
  __shared__ double s_value[LDS ? kBowScoreLds : 1];
  if (LDS) {
    for (int i = threadIdx.x; i < nq; i += kBowBlock) {
      s_word[i] = q_word[i];
      s_value[i] = q_value[i];
    }
    __syncthreads();
  }
  const int32_t *qw = LDS ? s_word : q_word;
  const double *qv = LDS ? s_value : q_value;
  const int lane = threadIdx.x & (kBowGroup - 1);
  const int shift = threadIdx.x & (64 - kBowGroup);  // this group's bits in the wavefront's ballot
  const int64_t g = ((int64_t)blockIdx.x * kBowBlock + threadIdx.x) / kBowGroup;
  int64_t b = 0, e = 0;
  if (g < n_db) {
    b = db_off[g];
    e = db_off[g + 1];
  }
  double sum = 0.0;
  int nc = 0;
  for (int64_t base = b; __any(base < e); base += kBowGroup) {
    const int64_t i = base + lane;
    bool found = false;
    double term = 0.0;
    if (i < e) {
      const int32_t w = db_word[i];
      int lo = 0, hi = nq;  // the first query entry >= w
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (qw[mid] < w)
          lo = mid + 1;
        else
          hi = mid;
      }
      if (lo < nq && qw[lo] == w) {
        const double vi = qv[lo], wi = db_value[i];
        found = true;
        term = fabs(vi - wi) - fabs(vi) - fabs(wi);
      }
    }
    uint32_t m = (uint32_t)(__ballot(found) >> shift) & 0xffffu;
    nc += __popc(m);
    while (__any(m != 0)) {
      const int src = m ? __ffs((int)m) - 1 : 0;
      const double t = __shfl(term, src, kBowGroup);
      if (m) {
        sum += t;
        m &= m - 1;
      }
    }
  }
  if (g < n_db && lane == 0) {
    score[g] = -sum / 2.0;
    if (n_common) n_common[g] = nc;
  }
}

}  // namespace

void launch_bow_descend(const BowVocDev &v, const uint4 *feat, int n_feat, int nid_level, int32_t *word, int32_t *node,
                        double *weight, hipStream_t st) {
  if (n_feat <= 0) return;
  const unsigned grid = (unsigned)(((int64_t)n_feat + kBowItems - 1) / kBowItems);
  hipLaunchKernelGGL(k_bow_descend, dim3(grid), dim3(kBowBlock), 0, st, v, feat, n_feat, nid_level, word, node, weight);
}

void launch_bow_score(int nq, const int32_t *q_word, const double *q_value, int n_db, const int64_t *db_off,
                      const int32_t *db_word, const double *db_value, double *score, int32_t *n_common,
                      hipStream_t st) {
  if (n_db <= 0) return;
  const unsigned grid = (unsigned)(((int64_t)n_db + kBowItems - 1) / kBowItems);
  if (nq <= kBowScoreLds)
    hipLaunchKernelGGL(k_bow_score<true>, dim3(grid), dim3(kBowBlock), 0, st, nq, q_word, q_value, n_db, db_off,
                       db_word, db_value, score, n_common);
  else
    hipLaunchKernelGGL(k_bow_score<false>, dim3(grid), dim3(kBowBlock), 0, st, nq, q_word, q_value, n_db, db_off,
                       db_word, db_value, score, n_common);
}

}  // namespace sqlm
