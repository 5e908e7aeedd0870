// sqlm_pnp_ransac.cpp — host side of the batched PnP RANSAC (sqlm_pnp_ransac):
// one staged upload, k_pnp_hyp (sqlm_pnp_ransac.hip) on the context's stream,
// a download of the inlier counts, the host scan that finds the record-breaking
// hypotheses (the only ones whose Refine() the reference's outcome depends on,
// PnPsolver.cc:308-344), their table's upload, k_pnp_refine, one download, and
// the final scan: two launches, two synchronisations. The output arenas stay in
// the solver for the getters; the per-hypothesis diagnostics (ut, eigenvalues,
// betas, errors) stay on the device until a getter asks for them. Built with
// -ffp-contract=off like the kernels: the host evaluation of a hypothesis and
// of a refine is the same text, pnp_ransac_dev.h.
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "pnp_ransac_dev.h"
#include "sqlm_internal.h"
#include "sqlm_staging.h"

#pragma clang fp contract(off)

namespace sqlm {

struct PnpRecord {
  int32_t prob, hyp;  // problem, hypothesis within it
};

struct PnpSolver {
  hipStream_t stream = nullptr;
  Staged in, out;    // the call's inputs; counts, indices, poses and masks of the hypotheses
  Staged rin, rout;  // the records' table; their lists, counts, poses, diagnostics and masks
  Staged diag;       // the hypotheses' diagnostics
  bool ran = false;  // a call has completed: the getters below are valid
  bool diag_here = false;  // diag.host holds the last call's diagnostics
  std::vector<PnpProb> prob;
  std::vector<PnpRecord> rec;       // the last call's records, by problem, then by hypothesis
  std::vector<int64_t> rec_mask0;   // a record's first refined mask word
  std::vector<int32_t> rec0;        // [n_prob + 1] a problem's records in rec
  size_t n_hyp = 0;
  size_t o_count = 0, o_idx = 0, o_pose = 0, o_mask = 0;            // offsets into out.host
  size_t r_count = 0, r_pose = 0, r_diag = 0, r_mask = 0;           // offsets into rout.host
};

PnpSolver *pnp_create(hipStream_t st) {
  PnpSolver *s = new (std::nothrow) PnpSolver;
  if (s) s->stream = st;
  return s;
}

void pnp_destroy(PnpSolver *s) { delete s; }

// SetRansacParameters (:178-227): mRansacMaxIts, 0 when iterate() gives up at once (:257-261)
int pnp_max_its(int64_t n_pair, double probability, int min_inliers, int max_iterations, int min_set, float epsilon,
                int *min_inliers_out) {
  const int N = (int)n_pair;
  int n_min = (int)((float)N * epsilon);
  if (n_min < min_inliers) n_min = min_inliers;
  if (n_min < min_set) n_min = min_set;
  if (min_inliers_out) *min_inliers_out = n_min;
  if (N < n_min) return 0;
  if (epsilon < (float)n_min / (float)N) epsilon = (float)n_min / (float)N;
  double n_it;
  if (n_min == N)
    n_it = 1.0;
  else
    n_it = std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)epsilon, 3.0)));
  // clamped in double: the reference converts first, which is undefined for inf and NaN
  if (!(n_it <= (double)max_iterations)) n_it = (double)max_iterations;
  if (!(n_it >= 1.0)) n_it = 1.0;
  return (int)n_it;
}

// The bookkeeping of iterate (:308-344) over the counts. `refined` holds the
// refined inlier counts of the record-breaking hypotheses in their order; with
// fewer than there are records (or none) the later records count as failed.
void pnp_scan(int64_t n_hyp, const int32_t *counts, const int32_t *refined, int64_t n_refined, int min_inliers,
              uint8_t *flags, int64_t *first_return, int64_t *best, int64_t *n_record) {
  int32_t b = 0;
  int64_t first = -1, ibest = -1, n_rec = 0;
  bool refine_ok = false;
  for (int64_t h = 0; h < n_hyp; ++h) {
    uint8_t f = 0;
    if (counts[h] >= min_inliers) {  // :308
      f = 1;
      if (counts[h] > b) {  // :312
        b = counts[h];
        ibest = h;
        f |= 2;
        refine_ok = refined && n_rec < n_refined && refined[n_rec] > min_inliers;  // :412
        ++n_rec;
      }
      if (refine_ok) {  // :327, Refine() of the best mask so far
        f |= 4;
        if (first < 0) first = h;
      }
    }
    if (flags) flags[h] = f;
  }
  if (first_return) *first_return = first;
  if (best) *best = ibest;
  if (n_record) *n_record = n_rec;
}

int pnp_args_ok(const PnpArgs &a) {
  const int n_prob = a.n_prob;
  if (n_prob < 0 || !a.pair_off || !a.hyp_off) return SQLM_ERR_INVALID_ARG;
  if (n_prob > 0 && (!a.intr || !a.min_inliers || !a.first_return || !a.best || !a.Tcw || !a.n_refined))
    return SQLM_ERR_INVALID_ARG;
  if (a.pair_off[0] < 0 || a.hyp_off[0] < 0) return SQLM_ERR_INVALID_ARG;
  for (int k = 0; k < n_prob; ++k) {
    const int64_t n = a.pair_off[k + 1] - a.pair_off[k], nh = a.hyp_off[k + 1] - a.hyp_off[k];
    if (n < 0 || nh < 0 || n > INT32_MAX - 64) return SQLM_ERR_INVALID_ARG;
    if (nh > 0 && (n < 4 || n < (int64_t)a.min_inliers[k])) return SQLM_ERR_INVALID_ARG;  // iterate gives up at once there
  }
  const int64_t n_pair = a.pair_off[n_prob] - a.pair_off[0], n_hyp = a.hyp_off[n_prob] - a.hyp_off[0];
  if (n_pair > INT32_MAX - 64 || n_hyp > INT32_MAX / kPnpDiag) return SQLM_ERR_INVALID_ARG;
  if (n_pair > 0 && (!a.Xw || !a.uv || !a.max_err)) return SQLM_ERR_INVALID_ARG;
  if (n_hyp > 0 && (!a.draws || !a.n_inliers || !a.flags || !a.R || !a.t)) return SQLM_ERR_INVALID_ARG;
  for (int k = 0; k < n_prob; ++k) {
    const int64_t n = a.pair_off[k + 1] - a.pair_off[k];
    for (int64_t h = a.hyp_off[k]; h < a.hyp_off[k + 1]; ++h)
      for (int i = 0; i < 4; ++i)
        if (a.draws[4 * h + i] < 0 || a.draws[4 * h + i] > n - 1 - i) return SQLM_ERR_INVALID_ARG;
  }
  return SQLM_OK;
}

int pnp_run(PnpSolver *s, const PnpArgs &a) {
  const int n_prob = a.n_prob;
  s->ran = false;
  s->diag_here = false;
  const int64_t pb = a.pair_off[0], hb = a.hyp_off[0];
  const int64_t n_pair = a.pair_off[n_prob] - pb, n_hyp = a.hyp_off[n_prob] - hb;
  s->prob.assign((size_t)n_prob, PnpProb{});
  s->rec.clear();
  s->rec_mask0.clear();
  s->rec0.assign((size_t)n_prob + 1, 0);
  s->n_hyp = (size_t)n_hyp;
  int64_t n_words = 0, n_wg = 0;
  for (int k = 0; k < n_prob; ++k) {
    PnpProb &p = s->prob[k];
    for (int i = 0; i < 4; ++i) p.K[i] = a.intr[4 * k + i];
    p.pair0 = (int32_t)(a.pair_off[k] - pb);
    p.n_pair = (int32_t)(a.pair_off[k + 1] - a.pair_off[k]);
    p.hyp0 = (int32_t)(a.hyp_off[k] - hb);
    p.n_hyp = (int32_t)(a.hyp_off[k + 1] - a.hyp_off[k]);
    p.mask0 = n_words;
    n_words += (int64_t)p.n_hyp * ((p.n_pair + 63) / 64);
    n_wg += (p.n_hyp + kPnpHypPerWg - 1) / kPnpHypPerWg;
  }
  if (n_wg > INT32_MAX) return SQLM_ERR_INVALID_ARG;
  const size_t np = (size_t)n_prob, nq = (size_t)n_pair, nh = (size_t)n_hyp, ng = (size_t)n_wg;
  Arena in, out;
  const size_t i_prob = in.take(np * sizeof(PnpProb)), i_wp = in.take(ng * sizeof(int32_t)),
               i_wh = in.take(ng * sizeof(int32_t)), i_X = in.take(3 * nq * sizeof(float)),
               i_uv = in.take(2 * nq * sizeof(float)), i_me = in.take(nq * sizeof(float)),
               i_dr = in.take(4 * nh * sizeof(int32_t));
  const size_t o_count = out.take(nh * sizeof(int32_t)), o_idx = out.take(4 * nh * sizeof(int32_t)),
               o_pose = out.take(nh * kPnpPose * sizeof(double)),
               o_mask = out.take((size_t)n_words * sizeof(unsigned long long));
  PnpDev d;
  if (n_hyp > 0) {
    if (int r = s->in.grow(in.off)) return r;
    if (int r = s->out.grow(out.off)) return r;
    if (int r = s->diag.grow(nh * kPnpDiag * sizeof(double))) return r;
    char *h = s->in.host;
    std::memcpy(h + i_prob, s->prob.data(), np * sizeof(PnpProb));
    int32_t *wp = at<int32_t>(h, i_wp), *wh = at<int32_t>(h, i_wh);
    size_t g = 0;
    for (int k = 0; k < n_prob; ++k)
      for (int32_t h0 = 0; h0 < s->prob[k].n_hyp; h0 += kPnpHypPerWg, ++g) {
        wp[g] = k;
        wh[g] = s->prob[k].hyp0 + h0;
      }
    std::memcpy(h + i_X, a.Xw + 3 * pb, 3 * nq * sizeof(float));
    std::memcpy(h + i_uv, a.uv + 2 * pb, 2 * nq * sizeof(float));
    std::memcpy(h + i_me, a.max_err + pb, nq * sizeof(float));
    std::memcpy(h + i_dr, a.draws + 4 * hb, 4 * nh * sizeof(int32_t));
    SQLM_HIP_OK(hipMemcpyAsync(s->in.dev, s->in.host, in.off, hipMemcpyHostToDevice, s->stream));
    SQLM_HIP_OK(hipMemsetAsync(s->out.dev, 0, out.off, s->stream));

    char *di = s->in.dev, *dout = s->out.dev;
    d.n_wg = (int)n_wg;
    d.prob = at<const PnpProb>(di, i_prob);
    d.wg_prob = at<const int32_t>(di, i_wp);
    d.wg_hyp = at<const int32_t>(di, i_wh);
    d.Xw = at<const float>(di, i_X);
    d.uv = at<const float>(di, i_uv);
    d.max_err = at<const float>(di, i_me);
    d.draws = at<const int32_t>(di, i_dr);
    d.count = at<int32_t>(dout, o_count);
    d.idx = at<int32_t>(dout, o_idx);
    d.pose = at<double>(dout, o_pose);
    d.mask = at<unsigned long long>(dout, o_mask);
    d.diag = at<double>(s->diag.dev, 0);
    launch_pnp_hyp(d, s->stream);
    SQLM_HIP_OK(hipGetLastError());
    SQLM_HIP_OK(hipMemcpyAsync(s->out.host + o_count, s->out.dev + o_count, nh * sizeof(int32_t), hipMemcpyDeviceToHost,
                               s->stream));
    SQLM_HIP_OK(hipStreamSynchronize(s->stream));
    std::memcpy(a.n_inliers + hb, s->out.host + o_count, nh * sizeof(int32_t));
  }

  // the records: a hypothesis that qualifies with a count above every earlier qualifying one
  int64_t list_len = 0, rmask_words = 0;
  std::vector<int64_t> rec_list0;
  for (int k = 0; k < n_prob; ++k) {
    const PnpProb &p = s->prob[k];
    const int32_t *c = p.n_hyp ? a.n_inliers + a.hyp_off[k] : nullptr;
    int32_t b = 0;
    for (int32_t h = 0; h < p.n_hyp; ++h)
      if (c[h] >= a.min_inliers[k] && c[h] > b) {
        b = c[h];
        s->rec.push_back(PnpRecord{k, h});
        rec_list0.push_back(list_len);
        s->rec_mask0.push_back(rmask_words);
        list_len += p.n_pair;
        rmask_words += (p.n_pair + 63) / 64;
      }
    s->rec0[(size_t)k + 1] = (int32_t)s->rec.size();
  }
  const size_t nr = s->rec.size();
  Arena rin, rout;
  const size_t ri_prob = rin.take(nr * sizeof(int32_t)), ri_hyp = rin.take(nr * sizeof(int32_t)),
               ri_l0 = rin.take(nr * sizeof(int64_t)), ri_m0 = rin.take(nr * sizeof(int64_t));
  const size_t r_count = rout.take(nr * sizeof(int32_t)), r_pose = rout.take(nr * kPnpPose * sizeof(double)),
               r_diag = rout.take(nr * kPnpDiag * sizeof(double)),
               r_mask = rout.take((size_t)rmask_words * sizeof(unsigned long long)),
               r_list = rout.take((size_t)list_len * sizeof(int32_t));
  if (nr > 0) {
    if (int r = s->rin.grow(rin.off)) return r;
    if (int r = s->rout.grow(rout.off)) return r;
    char *h = s->rin.host;
    for (size_t i = 0; i < nr; ++i) {
      at<int32_t>(h, ri_prob)[i] = s->rec[i].prob;
      at<int32_t>(h, ri_hyp)[i] = s->prob[s->rec[i].prob].hyp0 + s->rec[i].hyp;
      at<int64_t>(h, ri_l0)[i] = rec_list0[i];
      at<int64_t>(h, ri_m0)[i] = s->rec_mask0[i];
    }
    SQLM_HIP_OK(hipMemcpyAsync(s->rin.dev, s->rin.host, rin.off, hipMemcpyHostToDevice, s->stream));
    SQLM_HIP_OK(hipMemsetAsync(s->rout.dev, 0, r_list, s->stream));  // everything but the lists
    d.n_rec = (int)nr;
    d.rec_prob = at<const int32_t>(s->rin.dev, ri_prob);
    d.rec_hyp = at<const int32_t>(s->rin.dev, ri_hyp);
    d.rec_list0 = at<const int64_t>(s->rin.dev, ri_l0);
    d.rec_mask0 = at<const int64_t>(s->rin.dev, ri_m0);
    d.rcount = at<int32_t>(s->rout.dev, r_count);
    d.rpose = at<double>(s->rout.dev, r_pose);
    d.rdiag = at<double>(s->rout.dev, r_diag);
    d.rmask = at<unsigned long long>(s->rout.dev, r_mask);
    d.list = at<int32_t>(s->rout.dev, r_list);
    launch_pnp_refine(d, s->stream);
    SQLM_HIP_OK(hipGetLastError());
    SQLM_HIP_OK(hipMemcpyAsync(s->rout.host, s->rout.dev, r_list, hipMemcpyDeviceToHost, s->stream));
  }
  if (n_hyp > 0) {
    SQLM_HIP_OK(hipMemcpyAsync(s->out.host + o_idx, s->out.dev + o_idx, out.off - o_idx, hipMemcpyDeviceToHost,
                               s->stream));
    SQLM_HIP_OK(hipStreamSynchronize(s->stream));
    const double *pose = at<const double>(s->out.host, o_pose);
    for (size_t k = 0; k < nh; ++k) {
      std::memcpy(a.R + 9 * (hb + (int64_t)k), pose + k * kPnpPose, 9 * sizeof(double));
      std::memcpy(a.t + 3 * (hb + (int64_t)k), pose + k * kPnpPose + 9, 3 * sizeof(double));
    }
  }
  for (int k = 0; k < n_prob; ++k) {
    const PnpProb &p = s->prob[k];
    const int32_t r0 = s->rec0[(size_t)k], r1 = s->rec0[(size_t)k + 1];
    const int32_t *rc = nr ? at<const int32_t>(s->rout.host, r_count) + r0 : nullptr;
    int64_t first = -1, best = -1;
    pnp_scan(p.n_hyp, p.n_hyp ? a.n_inliers + a.hyp_off[k] : nullptr, rc, r1 - r0, a.min_inliers[k],
             p.n_hyp ? a.flags + a.hyp_off[k] : nullptr, &first, &best, nullptr);
    a.first_return[k] = (int32_t)first;
    a.best[k] = (int32_t)best;
    float *T = a.Tcw + 16 * (size_t)k;
    for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.f : 0.f;
    a.n_refined[k] = 0;
    if (first >= 0) {  // the refine of the best mask at the first return: the last record at or before it
      int32_t r = r0;
      while (r + 1 < r1 && s->rec[(size_t)r + 1].hyp <= first) ++r;
      const double *ps = at<const double>(s->rout.host, r_pose) + (size_t)r * kPnpPose;
      for (int i = 0; i < 3; ++i) {  // Rcw.convertTo(CV_32F) (:415-421)
        for (int j = 0; j < 3; ++j) T[4 * i + j] = (float)ps[3 * i + j];
        T[4 * i + 3] = (float)ps[9 + i];
      }
      a.n_refined[k] = rc[r - r0];
    }
  }
  s->o_count = o_count;
  s->o_idx = o_idx;
  s->o_pose = o_pose;
  s->o_mask = o_mask;
  s->r_count = r_count;
  s->r_pose = r_pose;
  s->r_diag = r_diag;
  s->r_mask = r_mask;
  s->ran = true;
  return SQLM_OK;
}

namespace {

PnpSweeps sweeps_of(const int32_t *sweeps) {
  PnpSweeps sw;
  if (sweeps) {
    if (sweeps[0] > 0) sw.s3 = sweeps[0];
    if (sweeps[1] > 0) sw.s12 = sweeps[1];
    if (sweeps[2] > 0) sw.sR = sweeps[2];
  }
  return sw;
}

// EPnP on P, then the inlier test over all pairs: what a wavefront of either kernel computes
void solve_host(const PnpPts &P, const double *intr, const float *max_err, const PnpSweeps &sw, double *R, double *t,
                uint8_t *mask, int32_t *count, double *diag) {
  PnpWork w;
  const int ch = pnp_epnp(P, intr, sw, w);
  std::memcpy(R, w.Rs + 9 * ch, 9 * sizeof(double));
  std::memcpy(t, w.ts + 3 * ch, 3 * sizeof(double));
  int32_t n_in = 0;
  for (int j = 0; j < P.n_pair; ++j) {
    mask[j] = pnp_is_inlier(R, t, intr, P.Xw[3 * (size_t)j], P.Xw[3 * (size_t)j + 1], P.Xw[3 * (size_t)j + 2],
                            P.uv[2 * (size_t)j], P.uv[2 * (size_t)j + 1], max_err[j])
                  ? 1
                  : 0;
    n_in += mask[j];
  }
  *count = n_in;
  if (diag) {
    std::memcpy(diag, w.ut, 144 * sizeof(double));
    std::memcpy(diag + 144, w.d, 12 * sizeof(double));
    std::memcpy(diag + 156, w.betas, 12 * sizeof(double));
    std::memcpy(diag + 168, w.rep, 3 * sizeof(double));
    diag[171] = (double)ch;
  }
}

}  // namespace

int pnp_hypothesis_host(int n_pair, const double *intr, const float *Xw, const float *uv, const float *max_err,
                        const int32_t *draws, const int32_t *sweeps, int32_t *idx, double *R, double *t,
                        uint8_t *mask, int32_t *count, double *diag) {
  if (n_pair < 4) return SQLM_ERR_INVALID_ARG;
  for (int i = 0; i < 4; ++i)
    if (draws[i] < 0 || draws[i] > n_pair - 1 - i) return SQLM_ERR_INVALID_ARG;
  PnpPts P;
  P.Xw = Xw;
  P.uv = uv;
  P.n = 4;
  P.n_pair = n_pair;
  pnp_indices(n_pair, draws, P.q);
  for (int i = 0; i < 4; ++i) idx[i] = P.q[i];
  solve_host(P, intr, max_err, sweeps_of(sweeps), R, t, mask, count, diag);
  return SQLM_OK;
}

int pnp_refine_host(int n_pair, const double *intr, const float *Xw, const float *uv, const float *max_err,
                    const uint8_t *in_mask, const int32_t *sweeps, double *R, double *t, uint8_t *mask,
                    int32_t *count, double *diag) {
  if (n_pair < 1) return SQLM_ERR_INVALID_ARG;
  std::vector<int32_t> list;
  for (int j = 0; j < n_pair; ++j)
    if (in_mask[j]) list.push_back(j);
  PnpPts P;
  P.Xw = Xw;
  P.uv = uv;
  P.list = list.data();
  P.n = (int)list.size();
  P.n_pair = n_pair;
  solve_host(P, intr, max_err, sweeps_of(sweeps), R, t, mask, count, diag);
  return SQLM_OK;
}

int pnp_get_inliers(const PnpSolver *s, int prob, int hyp, uint8_t *mask) {
  if (!s->ran) return SQLM_ERR_STATE;
  if (prob < 0 || prob >= (int)s->prob.size()) return SQLM_ERR_INVALID_ARG;
  const PnpProb &p = s->prob[prob];
  if (hyp < 0 || hyp >= p.n_hyp) return SQLM_ERR_INVALID_ARG;
  const int n_words = (p.n_pair + 63) / 64;
  const unsigned long long *w = at<const unsigned long long>(s->out.host, s->o_mask) + p.mask0 + (int64_t)hyp * n_words;
  for (int j = 0; j < p.n_pair; ++j) mask[j] = (uint8_t)((w[j >> 6] >> (j & 63)) & 1ull);
  return SQLM_OK;
}

int pnp_get_refined(PnpSolver *s, int prob, int hyp, double *R, double *t, uint8_t *mask, int32_t *n_inliers,
                    double *diag) {
  if (!s->ran) return SQLM_ERR_STATE;
  if (prob < 0 || prob >= (int)s->prob.size()) return SQLM_ERR_INVALID_ARG;
  const PnpProb &p = s->prob[prob];
  if (hyp < 0 || hyp >= p.n_hyp) return SQLM_ERR_INVALID_ARG;
  int32_t r = -1;
  for (int32_t i = s->rec0[(size_t)prob]; i < s->rec0[(size_t)prob + 1]; ++i)
    if (s->rec[(size_t)i].hyp == hyp) r = i;
  if (r < 0) return SQLM_ERR_STATE;  // not a record-breaking hypothesis: the reference never refines its mask
  const double *ps = at<const double>(s->rout.host, s->r_pose) + (size_t)r * kPnpPose;
  if (R) std::memcpy(R, ps, 9 * sizeof(double));
  if (t) std::memcpy(t, ps + 9, 3 * sizeof(double));
  if (n_inliers) *n_inliers = at<const int32_t>(s->rout.host, s->r_count)[r];
  if (mask) {
    const unsigned long long *w = at<const unsigned long long>(s->rout.host, s->r_mask) + s->rec_mask0[(size_t)r];
    for (int j = 0; j < p.n_pair; ++j) mask[j] = (uint8_t)((w[j >> 6] >> (j & 63)) & 1ull);
  }
  if (diag) std::memcpy(diag, at<const double>(s->rout.host, s->r_diag) + (size_t)r * kPnpDiag, kPnpDiag * sizeof(double));
  return SQLM_OK;
}

int pnp_get_hypothesis(PnpSolver *s, int prob, int hyp, int32_t *idx, double *diag) {
  if (!s->ran) return SQLM_ERR_STATE;
  if (prob < 0 || prob >= (int)s->prob.size()) return SQLM_ERR_INVALID_ARG;
  const PnpProb &p = s->prob[prob];
  if (hyp < 0 || hyp >= p.n_hyp) return SQLM_ERR_INVALID_ARG;
  const size_t h = (size_t)p.hyp0 + (size_t)hyp;
  if (idx) std::memcpy(idx, at<const int32_t>(s->out.host, s->o_idx) + 4 * h, 4 * sizeof(int32_t));
  if (diag) {
    if (!s->diag_here) {  // fetched on the first request after a call
      SQLM_HIP_OK(hipMemcpyAsync(s->diag.host, s->diag.dev, s->n_hyp * kPnpDiag * sizeof(double), hipMemcpyDeviceToHost,
                                 s->stream));
      SQLM_HIP_OK(hipStreamSynchronize(s->stream));
      s->diag_here = true;
    }
    std::memcpy(diag, at<const double>(s->diag.host, 0) + h * kPnpDiag, kPnpDiag * sizeof(double));
  }
  return SQLM_OK;
}

}  // namespace sqlm
