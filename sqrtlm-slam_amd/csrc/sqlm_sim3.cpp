// sqlm_sim3.cpp — host side of the batched Sim3 alignment (sqlm_sim3_optimize):
// one staged upload, the single launch of k_sim3 (sqlm_sim3.hip) on the
// context's stream, one synchronisation, results out. The device and staging
// buffers belong to the solver and are reused.
#include <cstring>
#include <new>

#include "sqlm_internal.h"
#include "sqlm_staging.h"

namespace sqlm {

struct Sim3Solver {
  hipStream_t stream = nullptr;
  Staged in, out;    // one input and one output arena on the device, a pinned mirror of each
  bool ran = false;  // a call has completed: the introspection below is valid
  int n_prob = 0;
  int64_t n_pair = 0;
  size_t o_chi2 = 0, o_line = 0, o_linJ = 0, o_step = 0;  // offsets into out.host of the last call
};

Sim3Solver *sim3_create(hipStream_t st) {
  Sim3Solver *s = new (std::nothrow) Sim3Solver;
  if (s) s->stream = st;
  return s;
}

void sim3_destroy(Sim3Solver *s) { delete s; }

int sim3_optimize(Sim3Solver *s, const Sim3Args &a) {
  const int n_prob = a.n_prob;
  if (n_prob == 0) {  // nothing to launch
    s->n_prob = 0;
    s->n_pair = 0;
    s->ran = true;
    return SQLM_OK;
  }
  const int64_t b = a.pair_off[0], n_pair = a.pair_off[n_prob] - b;
  const size_t np = (size_t)n_prob, nq = (size_t)n_pair, D = sizeof(double);
  Arena in, out;
  const size_t i_S = in.take(8 * np * D), i_k1 = in.take(4 * np * D), i_k2 = in.take(4 * np * D),
               i_th = in.take(np * D), i_off = in.take((np + 1) * sizeof(int64_t)), i_fix = in.take(np),
               i_X1 = in.take(3 * nq * D), i_X2 = in.take(3 * nq * D), i_o1 = in.take(2 * nq * D),
               i_o2 = in.take(2 * nq * D), i_w1 = in.take(nq * D), i_w2 = in.take(nq * D);
  const size_t o_S = out.take(8 * np * D), o_nin = out.take(np * sizeof(int32_t)),
               o_st = out.take(np * sizeof(sqlm_sim3_stats)), o_state = out.take(nq), o_chi2 = out.take(4 * nq * D),
               o_line = out.take(4 * nq * D), o_linJ = out.take(28 * nq * D), o_step = out.take(64 * np * D);
  s->ran = false;
  if (int r = s->in.grow(in.off)) return r;
  if (int r = s->out.grow(out.off)) return r;

  char *h = s->in.host;
  std::memcpy(h + i_S, a.S12, 8 * np * D);
  std::memcpy(h + i_k1, a.intr1, 4 * np * D);
  std::memcpy(h + i_k2, a.intr2, 4 * np * D);
  std::memcpy(h + i_th, a.th2, np * D);
  int64_t *off = at<int64_t>(h, i_off);
  for (size_t k = 0; k <= np; ++k) off[k] = a.pair_off[k] - b;
  std::memcpy(h + i_fix, a.fix_scale, np);
  if (nq) {
    std::memcpy(h + i_X1, a.X1c + 3 * b, 3 * nq * D);
    std::memcpy(h + i_X2, a.X2c + 3 * b, 3 * nq * D);
    std::memcpy(h + i_o1, a.obs1 + 2 * b, 2 * nq * D);
    std::memcpy(h + i_o2, a.obs2 + 2 * b, 2 * nq * D);
    std::memcpy(h + i_w1, a.info1 + b, nq * D);
    std::memcpy(h + i_w2, a.info2 + b, nq * D);
  }
  SQLM_HIP_OK(hipMemcpyAsync(s->in.dev, s->in.host, in.off, hipMemcpyHostToDevice, s->stream));
  SQLM_HIP_OK(hipMemsetAsync(s->out.dev, 0, out.off, s->stream));

  Sim3Dev d;
  d.n_prob = n_prob;
  if (a.iters)
    for (int k = 0; k < 3; ++k) d.iters[k] = a.iters[k];
  d.user_lambda = a.user_lambda;
  char *di = s->in.dev, *dout = s->out.dev;
  d.S12 = at<const double>(di, i_S);
  d.intr1 = at<const double>(di, i_k1);
  d.intr2 = at<const double>(di, i_k2);
  d.th2 = at<const double>(di, i_th);
  d.pair_off = at<const int64_t>(di, i_off);
  d.fix_scale = at<const uint8_t>(di, i_fix);
  d.X1c = at<const double>(di, i_X1);
  d.X2c = at<const double>(di, i_X2);
  d.obs1 = at<const double>(di, i_o1);
  d.obs2 = at<const double>(di, i_o2);
  d.info1 = at<const double>(di, i_w1);
  d.info2 = at<const double>(di, i_w2);
  d.S12_out = at<double>(dout, o_S);
  d.n_inliers = at<int32_t>(dout, o_nin);
  d.stats = at<sqlm_sim3_stats>(dout, o_st);
  d.pair_state = at<uint8_t>(dout, o_state);
  d.pair_chi2 = at<double>(dout, o_chi2);
  d.lin_e = at<double>(dout, o_line);
  d.lin_J = at<double>(dout, o_linJ);
  d.last_step = at<double>(dout, o_step);
  launch_sim3(d, s->stream);
  SQLM_HIP_OK(hipGetLastError());
  SQLM_HIP_OK(hipMemcpyAsync(s->out.host, s->out.dev, out.off, hipMemcpyDeviceToHost, s->stream));
  SQLM_HIP_OK(hipStreamSynchronize(s->stream));

  const char *ho = s->out.host;
  std::memcpy(a.S12_out, ho + o_S, 8 * np * D);
  std::memcpy(a.n_inliers, ho + o_nin, np * sizeof(int32_t));
  if (nq) std::memcpy(a.pair_state + b, ho + o_state, nq);
  if (a.stats) std::memcpy(a.stats, ho + o_st, np * sizeof(sqlm_sim3_stats));
  s->n_prob = n_prob;
  s->n_pair = n_pair;
  s->o_chi2 = o_chi2;
  s->o_line = o_line;
  s->o_linJ = o_linJ;
  s->o_step = o_step;
  s->ran = true;
  return SQLM_OK;
}

int sim3_get_pair_chi2(const Sim3Solver *s, double *chi2) {
  if (!s->ran) return SQLM_ERR_STATE;
  std::memcpy(chi2, s->out.host + s->o_chi2, 4 * (size_t)s->n_pair * sizeof(double));
  return SQLM_OK;
}

int sim3_get_linearization(const Sim3Solver *s, double *e, double *J) {
  if (!s->ran) return SQLM_ERR_STATE;
  if (e) std::memcpy(e, s->out.host + s->o_line, 4 * (size_t)s->n_pair * sizeof(double));
  if (J) std::memcpy(J, s->out.host + s->o_linJ, 28 * (size_t)s->n_pair * sizeof(double));
  return SQLM_OK;
}

int sim3_get_last_step(const Sim3Solver *s, int prob, double *H, double *b, double *dx) {
  if (!s->ran) return SQLM_ERR_STATE;
  if (prob < 0 || prob >= s->n_prob) return SQLM_ERR_INVALID_ARG;
  const double *o = at<const double>(s->out.host, s->o_step) + 64 * (size_t)prob;
  if (o[63] == 0.0) return SQLM_ERR_STATE;  // the problem ran no trial
  std::memcpy(H, o, 49 * sizeof(double));
  std::memcpy(b, o + 49, 7 * sizeof(double));
  std::memcpy(dx, o + 56, 7 * sizeof(double));
  return SQLM_OK;
}

}  // namespace sqlm
