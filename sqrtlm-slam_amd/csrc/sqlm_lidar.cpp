// sqlm_lidar.cpp — host side of the LiDAR association (sqlm_lidar_associate,
// sqlm_set_lidar_from_clouds): one staged upload, the three launches of
// sqlm_lidar.hip on the context's stream, one synchronisation, results out.
// The device and staging buffers belong to the solver and grow on demand.
#include <cstdlib>
#include <cstring>
#include <limits>
#include <new>

#include "sqlm_internal.h"
#include "sqlm_staging.h"

namespace sqlm {

struct LidarSolver {
  hipStream_t stream = nullptr;
  int n_cu = 256;
  // input arena, work arena (world clouds, best words) and output arena on the
  // device; pinned mirrors of the input and the output
  Staged in, work, out;
  bool ran = false;
  int64_t n_map = 0, n_query = 0, n_pairs = 0;
  int n_seg = 0;
  size_t o_xyz = 0, o_pq = 0;  // offsets into out.host of the last call
};

LidarSolver *lidar_create(hipStream_t st, int n_cu) {
  LidarSolver *s = new (std::nothrow) LidarSolver;
  if (s) {
    s->stream = st;
    if (n_cu > 0) s->n_cu = n_cu;
  }
  return s;
}

void lidar_destroy(LidarSolver *s) { delete s; }

int lidar_args_ok(const LidarArgs &a) {
  if (a.n_map_clouds < 0 || a.n_query < 0 || !a.map_off) return 0;
  if (a.map_off[0] < 0) return 0;
  for (int c = 0; c < a.n_map_clouds; ++c)
    if (a.map_off[c + 1] < a.map_off[c]) return 0;
  const int64_t n_map = a.map_off[a.n_map_clouds] - a.map_off[0];
  if (n_map > std::numeric_limits<int32_t>::max() || a.n_query > std::numeric_limits<int32_t>::max()) return 0;
  if (n_map > 0 && !a.map_xyz) return 0;
  if (a.n_query > 0 && (!a.query_xyz || !a.query_Twc)) return 0;
  return 1;
}

int lidar_run(LidarSolver *s, const LidarArgs &a) {
  const int64_t b = a.map_off[0], n_map = a.map_off[a.n_map_clouds] - b, nq = a.n_query;
  const size_t nm = (size_t)n_map, nqs = (size_t)nq, nc = (size_t)a.n_map_clouds;
  s->ran = false;
  if (nq == 0 || n_map == 0) {
    // no query: nothing to do. No map: the reference would hand an empty cloud
    // to the kd-tree; every query answers "none" and the device is not touched
    s->n_pairs = 0;
    s->n_seg = 0;
    for (size_t i = 0; i < nqs; ++i) {
      if (a.nn_index) a.nn_index[i] = -1;
      if (a.nn_sq_dist) a.nn_sq_dist[i] = std::numeric_limits<float>::infinity();
      if (a.nn_xyz) a.nn_xyz[3 * i] = a.nn_xyz[3 * i + 1] = a.nn_xyz[3 * i + 2] = 0.f;
      if (a.accepted) a.accepted[i] = 0;
    }
    if (a.n_pairs) *a.n_pairs = 0;
    s->n_map = n_map;
    s->n_query = nq;
    s->ran = true;
    return SQLM_OK;
  }

  Arena in, work, out;
  const size_t i_map = in.take(3 * nm * sizeof(float)), i_off = in.take((nc + 1) * sizeof(int64_t)),
               i_Twc = in.take(16 * nc * sizeof(float)), i_q = in.take(3 * nqs * sizeof(float)),
               i_qT = in.take(16 * sizeof(float));
  const size_t w_map = work.take(nm * sizeof(float4)), w_q = work.take(nqs * sizeof(float4)),
               w_best = work.take(nqs * sizeof(unsigned long long));
  const size_t o_idx = out.take(nqs * sizeof(int32_t)), o_d2 = out.take(nqs * sizeof(float)),
               o_xyz = out.take(3 * nqs * sizeof(float)), o_acc = out.take(nqs), o_pq = out.take(nqs * sizeof(int32_t)),
               o_np = out.take(sizeof(int32_t));
  if (int r = s->in.grow(in.off)) return r;
  if (int r = s->work.grow(work.off, false)) return r;  // device only
  if (int r = s->out.grow(out.off)) return r;

  char *h = s->in.host;
  std::memcpy(h + i_map, a.map_xyz + 3 * b, 3 * nm * sizeof(float));
  int64_t *off = at<int64_t>(h, i_off);
  for (size_t c = 0; c <= nc; ++c) off[c] = a.map_off[c] - b;
  if (a.map_Twc) std::memcpy(h + i_Twc, a.map_Twc, 16 * nc * sizeof(float));
  std::memcpy(h + i_q, a.query_xyz, 3 * nqs * sizeof(float));
  std::memcpy(h + i_qT, a.query_Twc, 16 * sizeof(float));
  SQLM_HIP_OK(hipMemcpyAsync(s->in.dev, s->in.host, in.off, hipMemcpyHostToDevice, s->stream));

  // Map segments: enough workgroups to cover every CU about twice, no segment
  // shorter than four LDS tiles; SQLM_LIDAR_SPLIT=s forces s (an A/B switch:
  // the result does not depend on it). Segments are whole tiles.
  const int64_t n_tiles = (n_map + kLidarT - 1) / kLidarT, q_tiles = (nq + kLidarW - 1) / kLidarW;
  int64_t split = (2 * (int64_t)s->n_cu + q_tiles - 1) / q_tiles;
  if (split > (n_tiles + 3) / 4) split = (n_tiles + 3) / 4;
  if (const char *e = std::getenv("SQLM_LIDAR_SPLIT")) {
    const long v = std::atol(e);
    if (v >= 1) split = v;
  }
  if (split < 1) split = 1;
  if (split > n_tiles) split = n_tiles;
  if (split > 65535) split = 65535;  // grid.y
  const int64_t seg_tiles = (n_tiles + split - 1) / split;

  LidarDev d;
  d.n_map = (int)n_map;
  d.n_clouds = a.n_map_clouds;
  d.n_query = (int)nq;
  d.seg_len = (int)(seg_tiles * kLidarT);
  d.n_seg = (int)((n_tiles + seg_tiles - 1) / seg_tiles);
  d.has_Twc = a.map_Twc != nullptr;
  d.thr = a.thr;
  d.map_xyz = at<const float>(s->in.dev, i_map);
  d.map_off = at<const int64_t>(s->in.dev, i_off);
  d.map_Twc = at<const float>(s->in.dev, i_Twc);
  d.query_xyz = at<const float>(s->in.dev, i_q);
  d.query_Twc = at<const float>(s->in.dev, i_qT);
  d.map_w = at<float4>(s->work.dev, w_map);
  d.query_w = at<float4>(s->work.dev, w_q);
  d.best = at<unsigned long long>(s->work.dev, w_best);
  d.nn_index = at<int32_t>(s->out.dev, o_idx);
  d.nn_sq_dist = at<float>(s->out.dev, o_d2);
  d.nn_xyz = at<float>(s->out.dev, o_xyz);
  d.accepted = at<uint8_t>(s->out.dev, o_acc);
  d.pair_query = at<int32_t>(s->out.dev, o_pq);
  d.n_pairs = at<int32_t>(s->out.dev, o_np);
  launch_lidar(d, s->stream);
  SQLM_HIP_OK(hipGetLastError());
  SQLM_HIP_OK(hipMemcpyAsync(s->out.host, s->out.dev, out.off, hipMemcpyDeviceToHost, s->stream));
  SQLM_HIP_OK(hipStreamSynchronize(s->stream));

  char *ho = s->out.host;
  s->n_pairs = *at<const int32_t>(ho, o_np);
  if (a.nn_index) std::memcpy(a.nn_index, ho + o_idx, nqs * sizeof(int32_t));
  if (a.nn_sq_dist) std::memcpy(a.nn_sq_dist, ho + o_d2, nqs * sizeof(float));
  if (a.nn_xyz) std::memcpy(a.nn_xyz, ho + o_xyz, 3 * nqs * sizeof(float));
  if (a.accepted) std::memcpy(a.accepted, ho + o_acc, nqs);
  if (a.n_pairs) *a.n_pairs = s->n_pairs;
  s->o_xyz = o_xyz;
  s->o_pq = o_pq;
  s->n_map = n_map;
  s->n_query = nq;
  s->n_seg = d.n_seg;
  s->ran = true;
  return SQLM_OK;
}

int64_t lidar_n_pairs(const LidarSolver *s) { return s->ran ? s->n_pairs : 0; }
const int32_t *lidar_pair_query(const LidarSolver *s) { return at<const int32_t>(s->out.host, s->o_pq); }
const float *lidar_nn_xyz(const LidarSolver *s) { return at<const float>(s->out.host, s->o_xyz); }

int lidar_get_exec_info(const LidarSolver *s, int out[8]) {
  if (!s->ran) return SQLM_ERR_STATE;
  out[0] = (int)s->n_map;
  out[1] = (int)s->n_query;
  out[2] = s->n_seg;
  out[3] = kLidarT;
  out[4] = (int)s->n_pairs;
  out[5] = kLidarW;
  out[6] = out[7] = 0;
  return SQLM_OK;
}

}  // namespace sqlm
