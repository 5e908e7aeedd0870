// sqlm_sim3.cpp — host side of the batched Sim3 alignment (sqlm_sim3_optimize):
// argument checks, one staged upload, the single launch of k_sim3
// (sqlm_sim3.hip) on the context's stream, one synchronisation, results out.
// The device and staging buffers belong to the solver and are reused.
#include <cstring>
#include <new>
#include <vector>

#include "sqlm_internal.h"

namespace sqlm {

#define S3_HIP(x)                             \
  do {                                        \
    if ((x) != hipSuccess) return SQLM_ERR_HIP; \
  } while (0)

struct Sim3Solver {
  hipStream_t stream = nullptr;
  // one input arena and one output arena on the device, one pinned mirror of each
  char *d_in = nullptr, *d_out = nullptr, *h_in = nullptr, *h_out = nullptr;
  size_t cap_in = 0, cap_out = 0;
  bool ran = false;  // a call has completed: the introspection below is valid
  int n_prob = 0;
  int64_t n_pair = 0;
  size_t o_chi2 = 0, o_line = 0, o_linJ = 0, o_step = 0;  // offsets into h_out of the last call

  ~Sim3Solver() {
    if (d_in) (void)hipFree(d_in);
    if (d_out) (void)hipFree(d_out);
    if (h_in) (void)hipHostFree(h_in);
    if (h_out) (void)hipHostFree(h_out);
  }
};

Sim3Solver *sim3_create(hipStream_t st) {
  Sim3Solver *s = new (std::nothrow) Sim3Solver;
  if (s) s->stream = st;
  return s;
}

void sim3_destroy(Sim3Solver *s) { delete s; }

namespace {

int grow(char **dev, char **host, size_t *cap, size_t need) {
  if (need <= *cap) return SQLM_OK;
  if (*dev) (void)hipFree(*dev);
  if (*host) (void)hipHostFree(*host);
  *dev = *host = nullptr;
  *cap = 0;
  const size_t n = need + need / 2;
  if (hipMalloc((void **)dev, n) != hipSuccess) return SQLM_ERR_OOM;
  if (hipHostMalloc((void **)host, n, hipHostMallocDefault) != hipSuccess) return SQLM_ERR_OOM;
  *cap = n;
  return SQLM_OK;
}

// bump allocation in 16-byte steps
struct Arena {
  size_t off = 0;
  size_t take(size_t bytes) {
    const size_t o = off;
    off += (bytes + 15) & ~(size_t)15;
    return o;
  }
};

}  // namespace

int sim3_optimize(Sim3Solver *s, int n_prob, const double *S12, const double *intr1, const double *intr2,
                  const uint8_t *fix_scale, const double *th2, const int64_t *pair_off, const double *X1c,
                  const double *X2c, const double *obs1, const double *obs2, const double *info1, const double *info2,
                  const int32_t iters[3], double user_lambda, double *S12_out, int32_t *n_inliers, uint8_t *pair_state,
                  sqlm_sim3_stats *stats) {
  if (n_prob == 0) {  // nothing to launch
    s->n_prob = 0;
    s->n_pair = 0;
    s->ran = true;
    return SQLM_OK;
  }
  const int64_t n_pair = pair_off[n_prob] - pair_off[0];
  const size_t np = (size_t)n_prob, nq = (size_t)n_pair;
  Arena in, out;
  const size_t i_S = in.take(8 * np * sizeof(double)), i_k1 = in.take(4 * np * sizeof(double)),
               i_k2 = in.take(4 * np * sizeof(double)), i_th = in.take(np * sizeof(double)),
               i_off = in.take((np + 1) * sizeof(int64_t)), i_fix = in.take(np), i_X1 = in.take(3 * nq * sizeof(double)),
               i_X2 = in.take(3 * nq * sizeof(double)), i_o1 = in.take(2 * nq * sizeof(double)),
               i_o2 = in.take(2 * nq * sizeof(double)), i_w1 = in.take(nq * sizeof(double)),
               i_w2 = in.take(nq * sizeof(double));
  const size_t o_S = out.take(8 * np * sizeof(double)), o_nin = out.take(np * sizeof(int32_t)),
               o_st = out.take(np * sizeof(sqlm_sim3_stats)), o_state = out.take(nq),
               o_chi2 = out.take(4 * nq * sizeof(double)), o_line = out.take(4 * nq * sizeof(double)),
               o_linJ = out.take(28 * nq * sizeof(double)), o_step = out.take(64 * np * sizeof(double));
  s->ran = false;
  if (int r = grow(&s->d_in, &s->h_in, &s->cap_in, in.off)) return r;
  if (int r = grow(&s->d_out, &s->h_out, &s->cap_out, out.off)) return r;

  char *h = s->h_in;
  std::memcpy(h + i_S, S12, 8 * np * sizeof(double));
  std::memcpy(h + i_k1, intr1, 4 * np * sizeof(double));
  std::memcpy(h + i_k2, intr2, 4 * np * sizeof(double));
  std::memcpy(h + i_th, th2, np * sizeof(double));
  int64_t *off = reinterpret_cast<int64_t *>(h + i_off);
  for (size_t k = 0; k <= np; ++k) off[k] = pair_off[k] - pair_off[0];
  std::memcpy(h + i_fix, fix_scale, np);
  const int64_t b = pair_off[0];
  if (nq) {
    std::memcpy(h + i_X1, X1c + 3 * b, 3 * nq * sizeof(double));
    std::memcpy(h + i_X2, X2c + 3 * b, 3 * nq * sizeof(double));
    std::memcpy(h + i_o1, obs1 + 2 * b, 2 * nq * sizeof(double));
    std::memcpy(h + i_o2, obs2 + 2 * b, 2 * nq * sizeof(double));
    std::memcpy(h + i_w1, info1 + b, nq * sizeof(double));
    std::memcpy(h + i_w2, info2 + b, nq * sizeof(double));
  }
  S3_HIP(hipMemcpyAsync(s->d_in, s->h_in, in.off, hipMemcpyHostToDevice, s->stream));
  S3_HIP(hipMemsetAsync(s->d_out, 0, out.off, s->stream));

  Sim3Dev d;
  d.n_prob = n_prob;
  if (iters)
    for (int k = 0; k < 3; ++k) d.iters[k] = iters[k];
  d.user_lambda = user_lambda;
  const char *di = s->d_in;
  char *dout = s->d_out;
  d.S12 = reinterpret_cast<const double *>(di + i_S);
  d.intr1 = reinterpret_cast<const double *>(di + i_k1);
  d.intr2 = reinterpret_cast<const double *>(di + i_k2);
  d.th2 = reinterpret_cast<const double *>(di + i_th);
  d.pair_off = reinterpret_cast<const int64_t *>(di + i_off);
  d.fix_scale = reinterpret_cast<const uint8_t *>(di + i_fix);
  d.X1c = reinterpret_cast<const double *>(di + i_X1);
  d.X2c = reinterpret_cast<const double *>(di + i_X2);
  d.obs1 = reinterpret_cast<const double *>(di + i_o1);
  d.obs2 = reinterpret_cast<const double *>(di + i_o2);
  d.info1 = reinterpret_cast<const double *>(di + i_w1);
  d.info2 = reinterpret_cast<const double *>(di + i_w2);
  d.S12_out = reinterpret_cast<double *>(dout + o_S);
  d.n_inliers = reinterpret_cast<int32_t *>(dout + o_nin);
  d.stats = reinterpret_cast<sqlm_sim3_stats *>(dout + o_st);
  d.pair_state = reinterpret_cast<uint8_t *>(dout + o_state);
  d.pair_chi2 = reinterpret_cast<double *>(dout + o_chi2);
  d.lin_e = reinterpret_cast<double *>(dout + o_line);
  d.lin_J = reinterpret_cast<double *>(dout + o_linJ);
  d.last_step = reinterpret_cast<double *>(dout + o_step);
  launch_sim3(d, s->stream);
  S3_HIP(hipGetLastError());
  S3_HIP(hipMemcpyAsync(s->h_out, s->d_out, out.off, hipMemcpyDeviceToHost, s->stream));
  S3_HIP(hipStreamSynchronize(s->stream));

  std::memcpy(S12_out, s->h_out + o_S, 8 * np * sizeof(double));
  std::memcpy(n_inliers, s->h_out + o_nin, np * sizeof(int32_t));
  if (nq) std::memcpy(pair_state + b, s->h_out + o_state, nq);
  if (stats) std::memcpy(stats, s->h_out + o_st, np * sizeof(sqlm_sim3_stats));
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
  std::memcpy(chi2, s->h_out + s->o_chi2, 4 * (size_t)s->n_pair * sizeof(double));
  return SQLM_OK;
}

int sim3_get_linearization(const Sim3Solver *s, double *e, double *J) {
  if (!s->ran) return SQLM_ERR_STATE;
  if (e) std::memcpy(e, s->h_out + s->o_line, 4 * (size_t)s->n_pair * sizeof(double));
  if (J) std::memcpy(J, s->h_out + s->o_linJ, 28 * (size_t)s->n_pair * sizeof(double));
  return SQLM_OK;
}

int sim3_get_last_step(const Sim3Solver *s, int prob, double *H, double *b, double *dx) {
  if (!s->ran) return SQLM_ERR_STATE;
  if (prob < 0 || prob >= s->n_prob) return SQLM_ERR_INVALID_ARG;
  const double *o = reinterpret_cast<const double *>(s->h_out + s->o_step) + 64 * (size_t)prob;
  if (o[63] == 0.0) return SQLM_ERR_STATE;  // the problem ran no trial
  std::memcpy(H, o, 49 * sizeof(double));
  std::memcpy(b, o + 49, 7 * sizeof(double));
  std::memcpy(dx, o + 56, 7 * sizeof(double));
  return SQLM_OK;
}

}  // namespace sqlm
