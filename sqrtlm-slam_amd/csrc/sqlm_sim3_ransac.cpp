// sqlm_sim3_ransac.cpp — host side of the batched Sim3 RANSAC
// (sqlm_sim3_ransac): one staged upload, the single launch of k_sim3_ransac
// (sqlm_sim3_ransac.hip) on the context's stream, one download, one
// synchronisation, then the reference's sequential "best so far / return on the
// first good one" bookkeeping (Sim3Solver.cc:264-284) as a scan over the
// downloaded inlier counts. The output arena stays in the solver for the
// getters. Built with -ffp-contract=off like the kernel: the host evaluation of
// a hypothesis (ransac_hypothesis_host) is the same text, sim3_ransac_dev.h.
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "sim3_ransac_dev.h"
#include "sqlm_internal.h"
#include "sqlm_staging.h"

#pragma clang fp contract(off)

namespace sqlm {

struct RansacSolver {
  hipStream_t stream = nullptr;
  Staged in, out;    // one input and one output arena on the device, a pinned mirror of each
  bool ran = false;  // a call has completed: the getters below are valid
  std::vector<RansacProb> prob;  // the last call's problems
  size_t o_count = 0, o_idx = 0, o_hyp = 0, o_mask = 0;  // offsets into out.host of the last call
};

RansacSolver *ransac_create(hipStream_t st) {
  RansacSolver *s = new (std::nothrow) RansacSolver;
  if (s) s->stream = st;
  return s;
}

void ransac_destroy(RansacSolver *s) { delete s; }

// mRansacMaxIts of SetRansacParameters (:145-203), 0 when iterate() gives up at once (:214-218)
int ransac_max_its(int64_t n_pair, double probability, int min_inliers, int max_iterations) {
  if (n_pair < (int64_t)min_inliers) return 0;
  double n_it;
  if ((int64_t)min_inliers == n_pair) {
    n_it = 1.0;
  } else {
    const float epsilon = (float)min_inliers / (float)n_pair;
    n_it = std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)epsilon, 3.0)));
  }
  // clamped in double: the reference converts first, which is undefined for inf and NaN
  if (!(n_it <= (double)max_iterations)) n_it = (double)max_iterations;
  if (!(n_it >= 1.0)) n_it = 1.0;
  return (int)n_it;
}

void ransac_scan(int64_t n_hyp, const int32_t *counts, int min_inliers, uint8_t *flags, int64_t *first_return,
                 int64_t *best) {
  int32_t b = 0;
  int64_t first = -1, ibest = -1;
  for (int64_t h = 0; h < n_hyp; ++h) {
    uint8_t f = 0;
    if (counts[h] >= b) {  // :265
      b = counts[h];
      ibest = h;
      f = 1;
      if (counts[h] > min_inliers) {  // :274
        f = 3;
        if (first < 0) first = h;
      }
    }
    if (flags) flags[h] = f;
  }
  if (first_return) *first_return = first;
  if (best) *best = ibest;
}

int ransac_args_ok(const RansacArgs &a) {
  const int n_prob = a.n_prob;
  if (n_prob < 0 || !a.pair_off || !a.hyp_off) return SQLM_ERR_INVALID_ARG;
  if (n_prob > 0 && (!a.intr1 || !a.intr2 || !a.fix_scale || !a.min_inliers || !a.first_return || !a.best))
    return SQLM_ERR_INVALID_ARG;
  if (a.pair_off[0] < 0 || a.hyp_off[0] < 0) return SQLM_ERR_INVALID_ARG;
  for (int k = 0; k < n_prob; ++k) {
    const int64_t n = a.pair_off[k + 1] - a.pair_off[k], nh = a.hyp_off[k + 1] - a.hyp_off[k];
    if (n < 0 || nh < 0 || n > INT32_MAX - 64) return SQLM_ERR_INVALID_ARG;
    if (nh > 0 && n < 3) return SQLM_ERR_INVALID_ARG;
  }
  const int64_t n_pair = a.pair_off[n_prob] - a.pair_off[0], n_hyp = a.hyp_off[n_prob] - a.hyp_off[0];
  if (n_pair > INT32_MAX - 64 || n_hyp > INT32_MAX / kRansacHypFloats) return SQLM_ERR_INVALID_ARG;
  if (n_pair > 0 && (!a.X1c || !a.X2c || !a.max_err1 || !a.max_err2)) return SQLM_ERR_INVALID_ARG;
  if (n_hyp > 0 && (!a.draws || !a.n_inliers || !a.flags || !a.R12 || !a.t12 || !a.s12)) return SQLM_ERR_INVALID_ARG;
  for (int64_t j = a.pair_off[0]; j < a.pair_off[n_prob]; ++j)
    if (a.max_err1[j] < 0 || a.max_err2[j] < 0) return SQLM_ERR_INVALID_ARG;  // the reference's are size_t
  for (int k = 0; k < n_prob; ++k) {
    const int64_t n = a.pair_off[k + 1] - a.pair_off[k];
    for (int64_t h = a.hyp_off[k]; h < a.hyp_off[k + 1]; ++h)
      for (int i = 0; i < 3; ++i)
        if (a.draws[3 * h + i] < 0 || a.draws[3 * h + i] > n - 1 - i) return SQLM_ERR_INVALID_ARG;
  }
  return SQLM_OK;
}

int ransac_run(RansacSolver *s, const RansacArgs &a) {
  const int n_prob = a.n_prob;
  s->ran = false;
  const int64_t pb = a.pair_off[0], hb = a.hyp_off[0];
  const int64_t n_pair = a.pair_off[n_prob] - pb, n_hyp = a.hyp_off[n_prob] - hb;
  s->prob.assign((size_t)n_prob, RansacProb{});
  int64_t n_words = 0, n_wg = 0;
  for (int k = 0; k < n_prob; ++k) {
    RansacProb &p = s->prob[k];
    for (int i = 0; i < 4; ++i) {
      p.K1[i] = (float)a.intr1[4 * k + i];
      p.K2[i] = (float)a.intr2[4 * k + i];
    }
    p.pair0 = (int32_t)(a.pair_off[k] - pb);
    p.n_pair = (int32_t)(a.pair_off[k + 1] - a.pair_off[k]);
    p.hyp0 = (int32_t)(a.hyp_off[k] - hb);
    p.n_hyp = (int32_t)(a.hyp_off[k + 1] - a.hyp_off[k]);
    p.mask0 = n_words;
    p.fix_scale = a.fix_scale[k] ? 1 : 0;
    n_words += (int64_t)p.n_hyp * ((p.n_pair + 63) / 64);
    n_wg += (p.n_hyp + kRansacHypPerWg - 1) / kRansacHypPerWg;
  }
  if (n_wg > INT32_MAX) return SQLM_ERR_INVALID_ARG;
  const size_t np = (size_t)n_prob, nq = (size_t)n_pair, nh = (size_t)n_hyp, ng = (size_t)n_wg;
  Arena in, out;
  const size_t i_prob = in.take(np * sizeof(RansacProb)), i_wp = in.take(ng * sizeof(int32_t)),
               i_wh = in.take(ng * sizeof(int32_t)), i_X1 = in.take(3 * nq * sizeof(float)),
               i_X2 = in.take(3 * nq * sizeof(float)), i_e1 = in.take(nq * sizeof(int32_t)),
               i_e2 = in.take(nq * sizeof(int32_t)), i_dr = in.take(3 * nh * sizeof(int32_t));
  const size_t o_count = out.take(nh * sizeof(int32_t)), o_idx = out.take(3 * nh * sizeof(int32_t)),
               o_hyp = out.take(nh * kRansacHypFloats * sizeof(float)),
               o_mask = out.take((size_t)n_words * sizeof(unsigned long long));
  if (n_hyp > 0) {
    if (int r = s->in.grow(in.off)) return r;
    if (int r = s->out.grow(out.off)) return r;
    char *h = s->in.host;
    std::memcpy(h + i_prob, s->prob.data(), np * sizeof(RansacProb));
    int32_t *wp = at<int32_t>(h, i_wp), *wh = at<int32_t>(h, i_wh);
    size_t g = 0;
    for (int k = 0; k < n_prob; ++k)
      for (int32_t h0 = 0; h0 < s->prob[k].n_hyp; h0 += kRansacHypPerWg, ++g) {
        wp[g] = k;
        wh[g] = s->prob[k].hyp0 + h0;
      }
    float *X1 = at<float>(h, i_X1), *X2 = at<float>(h, i_X2);
    for (size_t j = 0; j < 3 * nq; ++j) {  // float values carried in doubles, as sqlm_sim3_optimize takes them
      X1[j] = (float)a.X1c[3 * pb + j];
      X2[j] = (float)a.X2c[3 * pb + j];
    }
    std::memcpy(h + i_e1, a.max_err1 + pb, nq * sizeof(int32_t));
    std::memcpy(h + i_e2, a.max_err2 + pb, nq * sizeof(int32_t));
    std::memcpy(h + i_dr, a.draws + 3 * hb, 3 * nh * sizeof(int32_t));
    SQLM_HIP_OK(hipMemcpyAsync(s->in.dev, s->in.host, in.off, hipMemcpyHostToDevice, s->stream));
    SQLM_HIP_OK(hipMemsetAsync(s->out.dev, 0, out.off, s->stream));

    RansacDev d;
    d.n_wg = (int)n_wg;
    char *di = s->in.dev, *dout = s->out.dev;
    d.prob = at<const RansacProb>(di, i_prob);
    d.wg_prob = at<const int32_t>(di, i_wp);
    d.wg_hyp = at<const int32_t>(di, i_wh);
    d.X1c = at<const float>(di, i_X1);
    d.X2c = at<const float>(di, i_X2);
    d.max_err1 = at<const int32_t>(di, i_e1);
    d.max_err2 = at<const int32_t>(di, i_e2);
    d.draws = at<const int32_t>(di, i_dr);
    d.count = at<int32_t>(dout, o_count);
    d.idx = at<int32_t>(dout, o_idx);
    d.hyp = at<float>(dout, o_hyp);
    d.mask = at<unsigned long long>(dout, o_mask);
    launch_sim3_ransac(d, s->stream);
    SQLM_HIP_OK(hipGetLastError());
    SQLM_HIP_OK(hipMemcpyAsync(s->out.host, s->out.dev, out.off, hipMemcpyDeviceToHost, s->stream));
    SQLM_HIP_OK(hipStreamSynchronize(s->stream));

    const char *ho = s->out.host;
    std::memcpy(a.n_inliers + hb, ho + o_count, nh * sizeof(int32_t));
    const float *hyp = at<const float>(s->out.host, o_hyp);
    for (size_t k = 0; k < nh; ++k) {
      const float *v = hyp + k * kRansacHypFloats;  // RansacHyp: R 9, t 3, s
      std::memcpy(a.R12 + 9 * (hb + (int64_t)k), v, 9 * sizeof(float));
      std::memcpy(a.t12 + 3 * (hb + (int64_t)k), v + 9, 3 * sizeof(float));
      a.s12[hb + (int64_t)k] = v[12];
    }
  }
  for (int k = 0; k < n_prob; ++k) {
    const RansacProb &p = s->prob[k];
    int64_t first = -1, best = -1;
    ransac_scan(p.n_hyp, p.n_hyp ? a.n_inliers + a.hyp_off[k] : nullptr, a.min_inliers[k],
                p.n_hyp ? a.flags + a.hyp_off[k] : nullptr, &first, &best);
    a.first_return[k] = (int32_t)first;
    a.best[k] = (int32_t)best;
  }
  s->o_count = o_count;
  s->o_idx = o_idx;
  s->o_hyp = o_hyp;
  s->o_mask = o_mask;
  s->ran = true;
  return SQLM_OK;
}

// One hypothesis of one problem on the CPU: the kernel's arithmetic, compiled for the host.
int ransac_hypothesis_host(int n_pair, const double *intr1, const double *intr2, int fix_scale, const double *X1c,
                           const double *X2c, const int32_t *max_err1, const int32_t *max_err2, const int32_t *draws,
                           int32_t *idx, float *hyp, uint8_t *mask, int32_t *count) {
  if (n_pair < 3) return SQLM_ERR_INVALID_ARG;
  for (int i = 0; i < 3; ++i)
    if (draws[i] < 0 || draws[i] > n_pair - 1 - i) return SQLM_ERR_INVALID_ARG;
  float K1[4], K2[4], P1[9], P2[9];
  for (int i = 0; i < 4; ++i) {
    K1[i] = (float)intr1[i];
    K2[i] = (float)intr2[i];
  }
  ransac_indices(n_pair, draws, idx);
  for (int i = 0; i < 3; ++i)
    for (int c = 0; c < 3; ++c) {
      P1[3 * c + i] = (float)X1c[3 * (size_t)idx[i] + c];
      P2[3 * c + i] = (float)X2c[3 * (size_t)idx[i] + c];
    }
  RansacHyp hy;
  ransac_closed_form(P1, P2, fix_scale != 0, hy);
  std::memcpy(hyp, &hy, sizeof(hy));
  int32_t n_in = 0;
  for (int j = 0; j < n_pair; ++j) {
    const float a[3] = {(float)X1c[3 * (size_t)j], (float)X1c[3 * (size_t)j + 1], (float)X1c[3 * (size_t)j + 2]};
    const float b[3] = {(float)X2c[3 * (size_t)j], (float)X2c[3 * (size_t)j + 1], (float)X2c[3 * (size_t)j + 2]};
    mask[j] = ransac_is_inlier(hy, a, b, K1, K2, max_err1[j], max_err2[j]) ? 1 : 0;
    n_in += mask[j];
  }
  *count = n_in;
  return SQLM_OK;
}

int ransac_get_inliers(const RansacSolver *s, int prob, int hyp, uint8_t *mask) {
  if (!s->ran) return SQLM_ERR_STATE;
  if (prob < 0 || prob >= (int)s->prob.size()) return SQLM_ERR_INVALID_ARG;
  const RansacProb &p = s->prob[prob];
  if (hyp < 0 || hyp >= p.n_hyp) return SQLM_ERR_INVALID_ARG;
  const int n_words = (p.n_pair + 63) / 64;
  const unsigned long long *w = at<const unsigned long long>(s->out.host, s->o_mask) + p.mask0 + (int64_t)hyp * n_words;
  for (int j = 0; j < p.n_pair; ++j) mask[j] = (uint8_t)((w[j >> 6] >> (j & 63)) & 1ull);
  return SQLM_OK;
}

int ransac_get_hypothesis(const RansacSolver *s, int prob, int hyp, int32_t *idx, float *T12, float *T21) {
  if (!s->ran) return SQLM_ERR_STATE;
  if (prob < 0 || prob >= (int)s->prob.size()) return SQLM_ERR_INVALID_ARG;
  const RansacProb &p = s->prob[prob];
  if (hyp < 0 || hyp >= p.n_hyp) return SQLM_ERR_INVALID_ARG;
  const size_t h = (size_t)p.hyp0 + (size_t)hyp;
  if (idx) std::memcpy(idx, at<const int32_t>(s->out.host, s->o_idx) + 3 * h, 3 * sizeof(int32_t));
  RansacHyp hy;
  std::memcpy(&hy, at<const float>(s->out.host, s->o_hyp) + h * kRansacHypFloats, sizeof(hy));
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) {
      if (T12) T12[4 * i + j] = hy.sR[3 * i + j];
      if (T21) T21[4 * i + j] = hy.sRinv[3 * i + j];
    }
    if (T12) T12[4 * i + 3] = hy.t[i];
    if (T21) T21[4 * i + 3] = hy.tinv[i];
  }
  for (int j = 0; j < 4; ++j) {
    if (T12) T12[12 + j] = j == 3 ? 1.f : 0.f;
    if (T21) T21[12 + j] = j == 3 ? 1.f : 0.f;
  }
  return SQLM_OK;
}

}  // namespace sqlm
