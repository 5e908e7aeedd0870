// sqlm_lidar.cpp — host side of the LiDAR association (sqlm_lidar_associate,
// sqlm_set_lidar_from_clouds): one staged upload, the three launches of
// sqlm_lidar.hip on the context's stream, one synchronisation, results out.
// The device and staging buffers belong to the solver and grow on demand.
#include <cstdlib>
#include <cstring>
#include <limits>
#include <new>

#include "sqlm_internal.h"

namespace sqlm {

#define LS_HIP(x)                              \
  do {                                         \
    if ((x) != hipSuccess) return SQLM_ERR_HIP; \
  } while (0)

struct LidarSolver {
  hipStream_t stream = nullptr;
  int n_cu = 256;
  // input arena, work arena (world clouds, best words) and output arena on the
  // device; pinned mirrors of the input and the output
  char *d_in = nullptr, *d_work = nullptr, *d_out = nullptr, *h_in = nullptr, *h_out = nullptr;
  size_t cap_in = 0, cap_work = 0, cap_out = 0;
  bool ran = false;
  int64_t n_map = 0, n_query = 0, n_pairs = 0;
  int n_seg = 0;
  size_t o_xyz = 0, o_pq = 0;  // offsets into h_out of the last call

  ~LidarSolver() {
    if (d_in) (void)hipFree(d_in);
    if (d_work) (void)hipFree(d_work);
    if (d_out) (void)hipFree(d_out);
    if (h_in) (void)hipHostFree(h_in);
    if (h_out) (void)hipHostFree(h_out);
  }
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

namespace {

// host == nullptr: device memory only
int grow(char **dev, char **host, size_t *cap, size_t need) {
  if (need <= *cap) return SQLM_OK;
  if (*dev) (void)hipFree(*dev);
  if (host && *host) (void)hipHostFree(*host);
  *dev = nullptr;
  if (host) *host = nullptr;
  *cap = 0;
  const size_t n = need + need / 2;
  if (hipMalloc((void **)dev, n) != hipSuccess) return SQLM_ERR_OOM;
  if (host && hipHostMalloc((void **)host, n, hipHostMallocDefault) != hipSuccess) return SQLM_ERR_OOM;
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
  if (int r = grow(&s->d_in, &s->h_in, &s->cap_in, in.off)) return r;
  if (int r = grow(&s->d_work, nullptr, &s->cap_work, work.off)) return r;
  if (int r = grow(&s->d_out, &s->h_out, &s->cap_out, out.off)) return r;

  char *h = s->h_in;
  std::memcpy(h + i_map, a.map_xyz + 3 * b, 3 * nm * sizeof(float));
  int64_t *off = reinterpret_cast<int64_t *>(h + i_off);
  for (size_t c = 0; c <= nc; ++c) off[c] = a.map_off[c] - b;
  if (a.map_Twc) std::memcpy(h + i_Twc, a.map_Twc, 16 * nc * sizeof(float));
  std::memcpy(h + i_q, a.query_xyz, 3 * nqs * sizeof(float));
  std::memcpy(h + i_qT, a.query_Twc, 16 * sizeof(float));
  LS_HIP(hipMemcpyAsync(s->d_in, s->h_in, in.off, hipMemcpyHostToDevice, s->stream));

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
  d.map_xyz = reinterpret_cast<const float *>(s->d_in + i_map);
  d.map_off = reinterpret_cast<const int64_t *>(s->d_in + i_off);
  d.map_Twc = reinterpret_cast<const float *>(s->d_in + i_Twc);
  d.query_xyz = reinterpret_cast<const float *>(s->d_in + i_q);
  d.query_Twc = reinterpret_cast<const float *>(s->d_in + i_qT);
  d.map_w = reinterpret_cast<float4 *>(s->d_work + w_map);
  d.query_w = reinterpret_cast<float4 *>(s->d_work + w_q);
  d.best = reinterpret_cast<unsigned long long *>(s->d_work + w_best);
  d.nn_index = reinterpret_cast<int32_t *>(s->d_out + o_idx);
  d.nn_sq_dist = reinterpret_cast<float *>(s->d_out + o_d2);
  d.nn_xyz = reinterpret_cast<float *>(s->d_out + o_xyz);
  d.accepted = reinterpret_cast<uint8_t *>(s->d_out + o_acc);
  d.pair_query = reinterpret_cast<int32_t *>(s->d_out + o_pq);
  d.n_pairs = reinterpret_cast<int32_t *>(s->d_out + o_np);
  launch_lidar(d, s->stream);
  LS_HIP(hipGetLastError());
  LS_HIP(hipMemcpyAsync(s->h_out, s->d_out, out.off, hipMemcpyDeviceToHost, s->stream));
  LS_HIP(hipStreamSynchronize(s->stream));

  const char *ho = s->h_out;
  s->n_pairs = *reinterpret_cast<const int32_t *>(ho + o_np);
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
const int32_t *lidar_pair_query(const LidarSolver *s) { return reinterpret_cast<const int32_t *>(s->h_out + s->o_pq); }
const float *lidar_nn_xyz(const LidarSolver *s) { return reinterpret_cast<const float *>(s->h_out + s->o_xyz); }

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
