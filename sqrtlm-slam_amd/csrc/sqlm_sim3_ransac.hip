// sqlm_sim3_ransac.hip — every RANSAC hypothesis of every loop candidate in one
// launch: Sim3Solver::iterate's body (src/algorithm/Sim3Solver.cc:236-262 of
// the reference) without its sequential bookkeeping, which the host replays
// over the inlier counts (sqlm_sim3_ransac.cpp).
//
// A wavefront owns a hypothesis. All its lanes compute the closed form from the
// three drawn pairs (the same values in every lane: no exchange, no LDS), then
// stride over the problem's pairs 64 at a time; the 64-bit ballot of the
// inlier test is the mask word of that chunk, written once by lane 0, and the
// count is the sum of the words' popcounts. A workgroup is kRansacWaves
// wavefronts on kRansacHypPerWg consecutive hypotheses of one problem; the host
// lists (problem, first hypothesis) per workgroup. No atomics, no waits on
// other workgroups, no barrier; every loop is bounded by sizes the host set.
// What a hypothesis stores depends on its own inputs alone, not on the batch,
// its place in it or the wavefront that ran it.
//
// Built with -ffp-contract=off: the arithmetic is sim3_ransac_dev.h, shared
// with the host, IEEE operations in the order written there.
#include "sim3_ransac_dev.h"
#include "sqlm_internal.h"

#pragma clang fp contract(off)

namespace sqlm {

namespace {

__global__ void __launch_bounds__(64 * kRansacWaves) k_sim3_ransac(RansacDev d) {
  const int wg = blockIdx.x;
  if (wg >= d.n_wg) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const RansacProb pb = d.prob[d.wg_prob[wg]];
  const int n = pb.n_pair;
  const int n_words = (n + 63) >> 6;
  const float *X1 = d.X1c + 3 * (int64_t)pb.pair0, *X2 = d.X2c + 3 * (int64_t)pb.pair0;
  const int32_t *me1 = d.max_err1 + pb.pair0, *me2 = d.max_err2 + pb.pair0;
  const int h_end = pb.hyp0 + pb.n_hyp;
  for (int k = 0; k < kRansacHypPerWave; ++k) {
    const int h = d.wg_hyp[wg] + wave + k * kRansacWaves;  // uniform over the wavefront
    if (h >= h_end) break;
    int32_t r[3], idx[3];
    for (int i = 0; i < 3; ++i) r[i] = d.draws[3 * (int64_t)h + i];
    ransac_indices(n, r, idx);
    float P1[9], P2[9];
    for (int i = 0; i < 3; ++i) {
      // the host checked every draw: 0 <= idx < n. The clamp keeps a read in bounds whatever happens.
      const int j = idx[i] < 0 ? 0 : (idx[i] >= n ? n - 1 : idx[i]);
      for (int c = 0; c < 3; ++c) {
        P1[3 * c + i] = X1[3 * j + c];
        P2[3 * c + i] = X2[3 * j + c];
      }
    }
    RansacHyp hy;
    ransac_closed_form(P1, P2, pb.fix_scale != 0, hy);

    unsigned long long *mask = d.mask + pb.mask0 + (int64_t)(h - pb.hyp0) * n_words;
    int count = 0;
    for (int w = 0; w < n_words; ++w) {
      const int j = 64 * w + lane;
      bool in = false;  // a lane past the last pair contributes 0
      if (j < n) {
        const float a[3] = {X1[3 * j], X1[3 * j + 1], X1[3 * j + 2]};
        const float b[3] = {X2[3 * j], X2[3 * j + 1], X2[3 * j + 2]};
        in = ransac_is_inlier(hy, a, b, pb.K1, pb.K2, me1[j], me2[j]);
      }
      const unsigned long long word = __ballot(in);
      count += __popcll(word);
      if (lane == 0) mask[w] = word;
    }
    if (lane == 0) {
      d.count[h] = count;
      for (int i = 0; i < 3; ++i) d.idx[3 * (int64_t)h + i] = idx[i];
    }
    // the 34 floats of the hypothesis, one per lane
    const float *src = reinterpret_cast<const float *>(&hy);
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < kRansacHypFloats; ++i)
      if (lane == i) v = src[i];
    if (lane < kRansacHypFloats) d.hyp[(int64_t)h * kRansacHypFloats + lane] = v;
  }
}

}  // namespace

void launch_sim3_ransac(const RansacDev &d, hipStream_t st) {
  if (d.n_wg > 0) hipLaunchKernelGGL(k_sim3_ransac, dim3((unsigned)d.n_wg), dim3(64 * kRansacWaves), 0, st, d);
}

}  // namespace sqlm
