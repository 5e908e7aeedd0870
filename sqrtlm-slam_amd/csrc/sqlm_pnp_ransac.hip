// sqlm_pnp_ransac.hip — the two device stages of the batched PnP RANSAC
// (PnPsolver::iterate and Refine, src/algorithm/PnPsolver.cc:247-426 of the
// reference) without the sequential bookkeeping, which the host replays over
// the inlier counts (sqlm_pnp_ransac.cpp).
//
// k_pnp_hyp: every hypothesis of every problem in one launch. A wavefront owns
// a hypothesis: it maps the four raw draws to pair indices, solves EPnP on the
// four points (pnp_ransac_dev.h, its arrays in the wavefront's PnpWork in LDS),
// then strides over the problem's pairs 64 at a time; the 64-bit ballot of the
// inlier test is the mask word of that chunk and the count is the sum of the
// words' popcounts. A workgroup is kPnpWaves wavefronts on consecutive
// hypotheses of one problem; the host lists (problem, first hypothesis) per
// workgroup.
//
// k_pnp_refine: a one-wavefront workgroup per record-breaking hypothesis. It
// lists the set bits of that hypothesis's mask words in ascending order, solves
// EPnP on those points and runs the same inlier test.
//
// No atomics, no wait on another workgroup; the wavefronts of a k_pnp_hyp
// workgroup never meet at a barrier. Every loop is bounded by sizes the host
// set and every index is clamped before a read. What a hypothesis or a refine
// stores depends on its own inputs alone.
//
// Built with -ffp-contract=off: the arithmetic is pnp_ransac_dev.h, shared with
// the host, IEEE operations in the order written there.
#include "pnp_ransac_dev.h"
#include "sqlm_internal.h"

#pragma clang fp contract(off)

namespace sqlm {

namespace {

// the inlier test over all pairs of the problem: mask words, and the count in every lane
__device__ int pnp_check(const PnpProb &pb, const PnpDev &d, const double *R, const double *t,
                         unsigned long long *mask, int lane) {
  const int n = pb.n_pair, n_words = (n + 63) >> 6;
  const float *Xw = d.Xw + 3 * (int64_t)pb.pair0, *uv = d.uv + 2 * (int64_t)pb.pair0, *me = d.max_err + pb.pair0;
  int count = 0;
  for (int w = 0; w < n_words; ++w) {
    const int j = 64 * w + lane;
    bool in = false;  // a lane past the last pair contributes 0
    if (j < n) {
      const int64_t j3 = 3 * (int64_t)j, j2 = 2 * (int64_t)j;
      in = pnp_is_inlier(R, t, pb.K, Xw[j3], Xw[j3 + 1], Xw[j3 + 2], uv[j2], uv[j2 + 1], me[j]);
    }
    const unsigned long long word = __ballot(in);
    count += __popcll(word);
    if (lane == 0) mask[w] = word;
  }
  return count;
}

// pose and diagnostics of a finished solve, the lanes sharing the copies out of LDS
__device__ void pnp_store(const PnpWork &w, int ch, double *pose, double *diag, int lane) {
  if (lane < 9) pose[lane] = w.Rs[9 * ch + lane];
  if (lane < 3) pose[9 + lane] = w.ts[3 * ch + lane];
  for (int k = lane; k < 144; k += 64) diag[k] = w.ut[k];
  if (lane < 12) {
    diag[144 + lane] = w.d[lane];
    diag[156 + lane] = w.betas[lane];
  }
  if (lane < 3) diag[168 + lane] = w.rep[lane];
  if (lane == 0) diag[171] = (double)ch;
}

__global__ void __launch_bounds__(64 * kPnpWaves) k_pnp_hyp(PnpDev d) {
  __shared__ PnpWork work[kPnpWaves];
  const int wg = blockIdx.x;
  if (wg >= d.n_wg) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const PnpProb pb = d.prob[d.wg_prob[wg]];
  const int h = d.wg_hyp[wg] + wave;  // uniform over the wavefront
  if (h >= pb.hyp0 + pb.n_hyp) return;
  const int n = pb.n_pair;
  PnpWork &w = work[wave];
  int32_t r[4];
  for (int i = 0; i < 4; ++i) r[i] = d.draws[4 * (int64_t)h + i];
  PnpPts P;
  P.Xw = d.Xw + 3 * (int64_t)pb.pair0;
  P.uv = d.uv + 2 * (int64_t)pb.pair0;
  P.n = 4;
  P.n_pair = n;
  pnp_indices(n, r, P.q);  // the host checked every draw; pnp_detail::point clamps whatever comes
  const PnpSweeps sw;
  const int ch = pnp_epnp(P, pb.K, sw, w);
  const int n_words = (n + 63) >> 6;
  const int count = pnp_check(pb, d, w.Rs + 9 * ch, w.ts + 3 * ch, d.mask + pb.mask0 + (int64_t)(h - pb.hyp0) * n_words, lane);
  if (lane == 0) d.count[h] = count;
  if (lane < 4) d.idx[4 * (int64_t)h + lane] = lane == 0 ? P.q[0] : lane == 1 ? P.q[1] : lane == 2 ? P.q[2] : P.q[3];
  pnp_store(w, ch, d.pose + (int64_t)h * kPnpPose, d.diag + (int64_t)h * kPnpDiag, lane);
}

__global__ void __launch_bounds__(64) k_pnp_refine(PnpDev d) {
  __shared__ PnpWork w;
  const int rec = blockIdx.x;
  if (rec >= d.n_rec) return;
  const int lane = threadIdx.x & 63;
  const PnpProb pb = d.prob[d.rec_prob[rec]];
  const int h = d.rec_hyp[rec];
  const int n = pb.n_pair, n_words = (n + 63) >> 6;
  const unsigned long long *hm = d.mask + pb.mask0 + (int64_t)(h - pb.hyp0) * n_words;
  int32_t *list = d.list + d.rec_list0[rec];  // n_pair entries belong to this record
  int m = 0;
  for (int wd = 0; wd < n_words; ++wd) {
    const unsigned long long word = hm[wd];
    const int j = 64 * wd + lane;
    const int pos = m + __popcll(word & ((1ull << lane) - 1ull));
    if (((word >> lane) & 1ull) && j < n && pos < n) list[pos] = j;
    m += __popcll(word);
  }
  if (m > n) m = n;
  __threadfence_block();
  __syncthreads();  // one wavefront: its lanes now read each other's list entries
  PnpPts P;
  P.Xw = d.Xw + 3 * (int64_t)pb.pair0;
  P.uv = d.uv + 2 * (int64_t)pb.pair0;
  P.list = list;
  P.n = m;
  P.n_pair = n;
  const PnpSweeps sw;
  const int ch = pnp_epnp(P, pb.K, sw, w);
  const int count = pnp_check(pb, d, w.Rs + 9 * ch, w.ts + 3 * ch, d.rmask + d.rec_mask0[rec], lane);
  if (lane == 0) d.rcount[rec] = count;
  pnp_store(w, ch, d.rpose + (int64_t)rec * kPnpPose, d.rdiag + (int64_t)rec * kPnpDiag, lane);
}

}  // namespace

void launch_pnp_hyp(const PnpDev &d, hipStream_t st) {
  if (d.n_wg > 0) hipLaunchKernelGGL(k_pnp_hyp, dim3((unsigned)d.n_wg), dim3(64 * kPnpWaves), 0, st, d);
}

void launch_pnp_refine(const PnpDev &d, hipStream_t st) {
  if (d.n_rec > 0) hipLaunchKernelGGL(k_pnp_refine, dim3((unsigned)d.n_rec), dim3(64), 0, st, d);
}

}  // namespace sqlm
