// sqlm_pose.cpp — host side of the batched motion-only BA (sqlm_pose_optimize,
// sqlm_pose_refine_lidar): one staged upload, the single launch of k_pose
// (sqlm_pose.hip) on the context's stream, one synchronisation, results out.
// The device and staging buffers belong to the solver and grow on demand.
#include <cstring>
#include <new>

#include "sqlm_internal.h"
#include "sqlm_staging.h"

namespace sqlm {

struct PoseSolver {
  hipStream_t stream = nullptr;
  Staged in, out;    // one input and one output arena on the device, a pinned mirror of each
  bool ran = false;  // a call has completed: the introspection below is valid
  int n_prob = 0;
  int64_t n_obs = 0, n_lid = 0;
  size_t o_chi2 = 0, o_line = 0, o_linJ = 0, o_lide = 0, o_lidJ = 0, o_step = 0;  // offsets into out.host of the last call
};

PoseSolver *pose_create(hipStream_t st) {
  PoseSolver *s = new (std::nothrow) PoseSolver;
  if (s) s->stream = st;
  return s;
}

void pose_destroy(PoseSolver *s) { delete s; }

int pose_run(PoseSolver *s, const PoseArgs &a) {
  const int n_prob = a.n_prob;
  if (n_prob == 0) {  // nothing to launch
    s->n_prob = 0;
    s->n_obs = s->n_lid = 0;
    s->ran = true;
    return SQLM_OK;
  }
  const int64_t b = a.obs_off[0], n_obs = a.obs_off[n_prob] - b;
  const int64_t lb = a.refine ? a.lid_off[0] : 0, n_lid = a.refine ? a.lid_off[n_prob] - lb : 0;
  const size_t np = (size_t)n_prob, nq = (size_t)n_obs, nl = (size_t)n_lid, D = sizeof(double);
  Arena in, out;
  const size_t i_pose = in.take(8 * np * D), i_k = in.take(4 * np * D), i_off = in.take((np + 1) * sizeof(int64_t)),
               i_X = in.take(3 * nq * D), i_uv = in.take(2 * nq * D), i_w = in.take(nq * D), i_oin = in.take(nq),
               i_rob = in.take(np), i_loff = in.take((np + 1) * sizeof(int64_t)), i_kind = in.take(nl),
               i_pc = in.take(3 * nl * D), i_pw = in.take(3 * nl * D), i_n = in.take(3 * nl * D), i_lw = in.take(nl * D);
  const size_t o_pose = out.take(8 * np * D), o_nin = out.take(np * sizeof(int32_t)),
               o_st = out.take(np * sizeof(sqlm_pose_stats)), o_flag = out.take(nq),
               o_chi2 = out.take(kPoseChecks * nq * D), o_line = out.take(2 * nq * D), o_linJ = out.take(12 * nq * D),
               o_lide = out.take(nl * D), o_lidJ = out.take(6 * nl * D), o_step = out.take(kPoseStepLen * np * D);
  s->ran = false;
  if (int r = s->in.grow(in.off)) return r;
  if (int r = s->out.grow(out.off)) return r;

  char *h = s->in.host;
  double *hp = at<double>(h, i_pose);
  for (size_t k = 0; k < np; ++k) {
    for (int c = 0; c < 4; ++c) hp[8 * k + c] = a.pose_q[4 * k + c];
    for (int c = 0; c < 3; ++c) hp[8 * k + 4 + c] = a.pose_t[3 * k + c];
    hp[8 * k + 7] = 0.0;
  }
  std::memcpy(h + i_k, a.intr, 4 * np * D);
  int64_t *off = at<int64_t>(h, i_off), *loff = at<int64_t>(h, i_loff);
  for (size_t k = 0; k <= np; ++k) {
    off[k] = a.obs_off[k] - b;
    loff[k] = a.refine ? a.lid_off[k] - lb : 0;
  }
  if (nq) {
    std::memcpy(h + i_X, a.Xw + 3 * b, 3 * nq * D);
    std::memcpy(h + i_uv, a.uv + 2 * b, 2 * nq * D);
    std::memcpy(h + i_w, a.info + b, nq * D);
    if (a.refine) std::memcpy(h + i_oin, a.outlier_in + b, nq);
  }
  if (a.refine) std::memcpy(h + i_rob, a.robust_on, np);
  if (nl) {
    std::memcpy(h + i_kind, a.lid_kind + lb, nl);
    std::memcpy(h + i_pc, a.lid_pc + 3 * lb, 3 * nl * D);
    std::memcpy(h + i_pw, a.lid_pw + 3 * lb, 3 * nl * D);
    std::memcpy(h + i_n, a.lid_n + 3 * lb, 3 * nl * D);
    std::memcpy(h + i_lw, a.lid_info + lb, nl * D);
  }
  SQLM_HIP_OK(hipMemcpyAsync(s->in.dev, s->in.host, in.off, hipMemcpyHostToDevice, s->stream));
  SQLM_HIP_OK(hipMemsetAsync(s->out.dev, 0, out.off, s->stream));

  PoseDev d;
  d.n_prob = n_prob;
  d.refine = a.refine;
  for (int k = 0; k < 5; ++k) d.iters[k] = a.iters[k];
  d.user_lambda = a.user_lambda;
  d.th2 = a.th2;
  char *di = s->in.dev, *dout = s->out.dev;
  auto cd = [&](size_t o) { return at<const double>(di, o); };
  auto od = [&](size_t o) { return at<double>(dout, o); };
  d.pose = cd(i_pose);
  d.intr = cd(i_k);
  d.obs_off = at<const int64_t>(di, i_off);
  d.Xw = cd(i_X);
  d.uv = cd(i_uv);
  d.info = cd(i_w);
  d.outlier_in = at<const uint8_t>(di, i_oin);
  d.robust_on = at<const uint8_t>(di, i_rob);
  d.lid_off = at<const int64_t>(di, i_loff);
  d.lid_kind = at<const uint8_t>(di, i_kind);
  d.lid_pc = cd(i_pc);
  d.lid_pw = cd(i_pw);
  d.lid_n = cd(i_n);
  d.lid_info = cd(i_lw);
  d.pose_out = od(o_pose);
  d.n_inliers = at<int32_t>(dout, o_nin);
  d.stats = at<sqlm_pose_stats>(dout, o_st);
  d.outlier = at<uint8_t>(dout, o_flag);
  d.edge_chi2 = od(o_chi2);
  d.lin_e = od(o_line);
  d.lin_J = od(o_linJ);
  d.lid_e = od(o_lide);
  d.lid_J = od(o_lidJ);
  d.last_step = od(o_step);
  launch_pose(d, s->stream);
  SQLM_HIP_OK(hipGetLastError());
  SQLM_HIP_OK(hipMemcpyAsync(s->out.host, s->out.dev, out.off, hipMemcpyDeviceToHost, s->stream));
  SQLM_HIP_OK(hipStreamSynchronize(s->stream));

  const double *po = at<const double>(s->out.host, o_pose);
  for (size_t k = 0; k < np; ++k) {
    for (int c = 0; c < 4; ++c) a.pose_q_out[4 * k + c] = po[8 * k + c];
    for (int c = 0; c < 3; ++c) a.pose_t_out[3 * k + c] = po[8 * k + 4 + c];
  }
  std::memcpy(a.n_inliers, s->out.host + o_nin, np * sizeof(int32_t));
  if (nq) std::memcpy(a.outlier + b, s->out.host + o_flag, nq);
  if (a.stats) std::memcpy(a.stats, s->out.host + o_st, np * sizeof(sqlm_pose_stats));
  s->n_prob = n_prob;
  s->n_obs = n_obs;
  s->n_lid = n_lid;
  s->o_chi2 = o_chi2;
  s->o_line = o_line;
  s->o_linJ = o_linJ;
  s->o_lide = o_lide;
  s->o_lidJ = o_lidJ;
  s->o_step = o_step;
  s->ran = true;
  return SQLM_OK;
}

int pose_get_edge_chi2(const PoseSolver *s, double *chi2) {
  if (!s->ran) return SQLM_ERR_STATE;
  if (s->n_obs) std::memcpy(chi2, s->out.host + s->o_chi2, kPoseChecks * (size_t)s->n_obs * sizeof(double));
  return SQLM_OK;
}

int pose_get_linearization(const PoseSolver *s, double *e, double *J, double *lid_e, double *lid_J) {
  if (!s->ran) return SQLM_ERR_STATE;
  const size_t nq = (size_t)s->n_obs, nl = (size_t)s->n_lid, D = sizeof(double);
  if (e && nq) std::memcpy(e, s->out.host + s->o_line, 2 * nq * D);
  if (J && nq) std::memcpy(J, s->out.host + s->o_linJ, 12 * nq * D);
  if (lid_e && nl) std::memcpy(lid_e, s->out.host + s->o_lide, nl * D);
  if (lid_J && nl) std::memcpy(lid_J, s->out.host + s->o_lidJ, 6 * nl * D);
  return SQLM_OK;
}

int pose_get_last_step(const PoseSolver *s, int prob, double *H, double *b, double *dx) {
  if (!s->ran) return SQLM_ERR_STATE;
  if (prob < 0 || prob >= s->n_prob) return SQLM_ERR_INVALID_ARG;
  const double *o = at<const double>(s->out.host, s->o_step) + kPoseStepLen * (size_t)prob;
  if (o[49] == 0.0) return SQLM_ERR_STATE;  // the problem ran no trial
  std::memcpy(H, o, 36 * sizeof(double));
  std::memcpy(b, o + 36, 6 * sizeof(double));
  std::memcpy(dx, o + 42, 6 * sizeof(double));
  return SQLM_OK;
}

}  // namespace sqlm
