// sqlm_ctx.h — the context behind the C ABI (include/sqrtlm.h): the host copy
// of the graph, the setup plan, the device and page-locked buffer arenas and
// the streams / events of the LM driver. Shared by sqlm_prepare.cpp (setup),
// sqlm_lm.cpp (LM driver) and sqlm_api.cpp (ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/sqrtlm.h"
#include "sqlm_comm.h"
#include "sqlm_host_par.h"
#include "sqlm_internal.h"
#include "sqlm_plan.h"

namespace sqlm {

struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  size_t map = 0;  // page-locked buffers: mapped length of a registered huge-page mapping (0: hipHostMalloc)
};

}  // namespace sqlm

struct sqlm_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  // ---- host copy of the graph (caller order) ----
  bool has_problem = false;
  bool prepared = false;  // the last prepare() completed (CR plan, buffers valid)
  bool step_valid = false;  // a trial has run since the last prepare() (d.g / d.dx hold its system)
  int n_pose = 0, n_pt = 0;
  int64_t n_obs = 0, n_lid = 0;
  std::vector<double> pose_q, pose_t, intr, pt;
  std::vector<uint8_t> pose_fixed;
  sqlm::HVec<int32_t> obs_pose, obs_pt;
  sqlm::HVec<double> obs_uv, obs_info, obs_delta, obs_err;
  sqlm::HVec<uint8_t> obs_level;
  bool has_stereo = false;           // some edge is an EdgeStereoSE3ProjectXYZ
  std::vector<double> obs_ur, pose_bf, obs_err3;
  std::vector<int32_t> lid_pose;
  std::vector<double> lid_pc, lid_pw, lid_n, lid_info, lid_err;
  std::vector<uint8_t> lid_level;
  std::vector<uint8_t> lid_kind;     // 0 EdgeLidarFlatPoint, 1 EdgeLidarCornerPoint (sqlm_set_lidar_kind)
  // ---- structure of the current optimize() call ----
  sqlm::DevProblem d;
  // what the planner decided (buckets, update launch, S pattern, solver plan,
  // slot and LiDAR orders) and the host scratch it keeps across calls
  // (capacity reused: prepare() allocates and first-touches none of its large
  // arrays after the first call)
  sqlm::SetupPlan plan;
  sqlm::PlanScratch scratch;
  sqlm::HVec<int64_t> dev_edge;      // device obs -> edge id
  int n_active_edges = 0;
  int n_cu = 0;
  bool use_tiles = false;
  // the last optimize()'s per-edge errors are still on the device only
  // (fetched when an edge chi2 is asked for, or before the next prepare())
  bool err_pending = false;
  bool err_zero = false;  // obs_err is still to be sized and zeroed (a new problem: no error computed yet)
  // The state buffer the last error evaluation of this setup used: -1 none yet,
  // 0 a full linearize(), 1 a trial (an accepted trial's swap_state makes it 0).
  // fetch_errors evaluates the edge errors there (k_edge_errors); the LM loop
  // itself stores none unless trial_stores (SQLM_TRIAL_STORES=1, per prepare)
  int err_state = -1;
  bool trial_stores = false;
  bool opt_done = false;  // an optimize() has finished on this problem's current LiDAR edge set (sqlm_get_lidar_error)
  // ---- device memory ----
  std::vector<sqlm::DevBuf> bufs;
  std::vector<sqlm::DevBuf> pins;  // page-locked host staging of the large uploads (async DMA)
  double *h_scalars = nullptr;  // pinned
  sqlm::CRSync crs;                   // completion words of the one-launch back substitution
  // the trial scalars' mailbox (mapped, coherent page-locked memory written by
  // k_reduce): the host polls its sequence number instead of a copy + stream
  // synchronize; timing runs and sharded runs copy
  double *mbox = nullptr, *mbox_dev = nullptr;
  unsigned long long mbox_seq = 0;
  // SQLM_HOST_TRACE=1: host-side time points of every trial (diagnostic)
  bool htrace = false;
  std::chrono::steady_clock::time_point ht_prev{};
  double ht_acc[10] = {};
  int ht_n = 0;
  // ---- comm ----
  sqlm::Comm comm;
  // ---- essential graph (sqlm_eg.hip) ----
  // sharded runs: every rank's nonzero S block-row range [lo, hi), the BSR
  // row pointer (host), and on rank 0 the gather table into xstage
  std::vector<int> sh_lo, sh_hi, s_row_host;
  sqlm::GatherTab gather;
  bool need_maxdiag = false;
  sqlm::EGSolver *eg = nullptr;
  sqlm::Sim3Solver *sim3 = nullptr;
  sqlm::RansacSolver *ransac = nullptr;  // sqlm_sim3_ransac (sqlm_sim3_ransac.cpp)
  sqlm::PnpSolver *pnp = nullptr;  // sqlm_pnp_ransac (sqlm_pnp_ransac.cpp)
  sqlm::PoseSolver *pose = nullptr;
  sqlm::LidarSolver *lidar = nullptr;
  sqlm::OrbEngine *orb = nullptr;
  sqlm::BowSolver *bow = nullptr;  // staging of sqlm_bow_transform / sqlm_bow_score (sqlm_bow.cpp)
  sqlm::MapPointSolver *mappoint = nullptr;  // sqlm_triangulate_pairs / sqlm_map_points_update (sqlm_mappoint.cpp)
  sqlm::LidarFeatSolver *lidar_feat = nullptr;  // sqlm_lidar_features (sqlm_lidar_feat.cpp)
  sqlm::LidarDepthSolver *lidar_depth = nullptr;  // sqlm_lidar_depth (sqlm_lidar_depth.cpp)
  // ---- timing ----
  hipEvent_t ev[2 * SQLM_NKERNEL_TIMERS] = {};
  // side stream: the camera pass runs concurrently with the landmark QR
  // (independent inputs and outputs); fork / join through two events
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  // speculative linearization: every trial's k_landmark_update also linearizes
  // at the trial state (into the *_nx buffers) and the camera pass for that
  // state runs on the side stream; an accepted trial swaps them in, so the next
  // iteration starts without a linearization pass (g2o linearizes at exactly
  // that state: same device code, same bits). SQLM_NO_SPEC=1 turns it off.
  bool spec = false;
  bool no_pose_fuse = false;       // SQLM_NO_POSE_FUSE=1 (per prepare): the pose update as its own launch
  bool lin_valid = false;          // the current buffers hold the linearization at the current state
  bool spec_outstanding = false;   // a speculative camera pass may still run on the side stream
  bool cam_inline = false;         // small problem: the speculative camera pass on the context stream
  hipEvent_t ev_spec_fork = nullptr, ev_spec_join = nullptr;
  sqlm::TileStreams tiles;  // RCS tile classes run on stream + these two
  hipEvent_t ev_cam[2][2] = {};    // timing of the speculative camera passes (ping-pong)
  bool cam_pending[2] = {false, false};
  int cam_par = 0;
  int lin_timers = 2;               // timers the last linearize() recorded
  bool timing = false;
  double kernel_ms_acc[SQLM_NKERNEL_TIMERS] = {};
  int kernel_ms_n = 0;
};

namespace sqlm {

template <class T>
int ensure(sqlm_ctx *c, int idx, size_t n, T **out) {
  if ((int)c->bufs.size() <= idx) c->bufs.resize(idx + 1);
  DevBuf &b = c->bufs[idx];
  size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
  bytes = (bytes + 255) & ~size_t(255);
  if (b.cap < bytes) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
    if (hipMalloc(&b.p, bytes) != hipSuccess) return SQLM_ERR_OOM;
    b.cap = bytes;
  }
  *out = static_cast<T *>(b.p);
  return SQLM_OK;
}

template <class T>
int upload(sqlm_ctx *c, int idx, const std::vector<T> &v, T **out) {
  int s = ensure(c, idx, v.size(), out);
  if (s) return s;
  if (!v.empty()) SQLM_HIP_OK(hipMemcpyAsync(*out, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, c->stream));
  return SQLM_OK;
}

// A page-locked host array from the context's arena (grown, never shrunk):
// the large observation arrays are built in place and copied to the device
// asynchronously while the host goes on with the setup.
template <class T>
struct PinVec {
  T *p = nullptr;
  size_t n = 0;
  T &operator[](size_t i) const { return p[i]; }
  T *data() const { return p; }
  size_t size() const { return n; }
  T *begin() const { return p; }
  T *end() const { return p + n; }
};

inline void free_pinned(DevBuf &b) {
  if (b.p && b.map) {
    (void)hipHostUnregister(b.p);
    munmap(b.p, b.map);
  } else if (b.p) {
    (void)hipHostFree(b.p);
  }
  b.p = nullptr;
  b.cap = b.map = 0;
}

template <class T>
int pinned(sqlm_ctx *c, int idx, size_t n, PinVec<T> &out) {
  if ((int)c->pins.size() <= idx) c->pins.resize(idx + 1);
  DevBuf &b = c->pins[idx];
  const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
  if (b.cap < bytes) {
    free_pinned(b);
    // large arrays: a huge-page mapping, touched, then page-locked for the DMA
    if (SQLM_HOST_HUGE && bytes >= kHugePage) {
      if (void *p = huge_map(bytes)) {
        std::memset(p, 0, huge_len(bytes));
        if (hipHostRegister(p, huge_len(bytes), hipHostRegisterDefault) == hipSuccess) {
          b.p = p;
          b.cap = bytes;
          b.map = huge_len(bytes);
        } else {
          munmap(p, huge_len(bytes));
        }
      }
    }
    if (!b.p) {
      if (hipHostMalloc(&b.p, bytes, hipHostMallocDefault) != hipSuccess) return SQLM_ERR_OOM;
      b.cap = bytes;
    }
  }
  out.p = static_cast<T *>(b.p);
  out.n = n;
  return SQLM_OK;
}

template <class T>
int upload(sqlm_ctx *c, int idx, const PinVec<T> &v, T **out) {
  int s = ensure(c, idx, v.size(), out);
  if (s) return s;
  if (v.size()) SQLM_HIP_OK(hipMemcpyAsync(*out, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, c->stream));
  return SQLM_OK;
}

enum PinId { P_OBSLM, P_OBSCAM, P_OBSCAMH, P_OBSUV, P_OBSINFO, P_OBSDELTA, P_OBSUR, P_RQT, P_RX, P_RERR, P_RERR3, P_RLERR, P_OBSQ,
             P_X, P_OBSLOC, P_ARENA };

enum BufId {
  B_QT0, B_QT1, B_RT0, B_RT1, B_INTR, B_PHIDX, B_HIDXP, B_X0, B_X1, B_LMBEG, B_LMR, B_LMB, B_LMM, B_LMV,
  B_OBSLM, B_OBSCAM, B_OBSCAMH, B_OBSUV, B_OBSINFO, B_OBSDELTA, B_OBSS, B_OBSP, B_OBSJP, B_OBSERR, B_CAMPTR, B_CAMOBS, B_CAMSLOT, B_CAMUV, B_SROWIDX,
  B_HPP, B_BP, B_LIDPTR, B_LIDDATA, B_LIDPOSE, B_LIDERR, B_SROW, B_SCOL, B_S, B_G, B_DX, B_DENSE, B_PART,
  B_SCAL, B_MAXD, B_FLAGS, B_CRD, B_CRE, B_CRA, B_CRC, B_CRG, B_CRX, B_LMRP, B_TLM, B_TCAMP, B_TCAMS, B_TORDER,
  B_TPART, B_OBSLOC, B_PART2, B_GPART, B_REDP, B_REDI, B_GREDP, B_GREDI, B_TGPART, B_TLD, B_URANGE,
  B_OBSUR, B_OBSERR3, B_POSEBF, B_CAMUR, B_HDIAG, B_XSTAGE, B_DENSEL, B_DENSELI, B_DENSER, B_DENSEX,
  B_LMR_NX, B_LMB_NX, B_OBSS_NX, B_HPP_NX, B_BP_NX, B_CAMPOS, B_ARWS, B_ARWG, B_ARWZ, B_BDA, B_BDL, B_BDLI,
  B_BDR, B_BDX, B_LONGS, B_LONGG, B_UPDRNG, B_CRL, B_CAMKEY0, B_CAMKEY1, B_CAMVAL, B_SORTTMP, B_OBSQ, B_CAMQ,
  B_CRDONE, B_ARENA
};

// The small host arrays of a setup go to the device in one copy: their bytes
// are gathered into one block (256-byte aligned pieces) and their device
// pointers point into one arena buffer. A local-BA setup is otherwise ~35
// hipMemcpyAsync calls of a few KB at 3-10 us of host time each.
constexpr size_t kSmallUpload = 64 << 10;
template <class T>
struct is_pinvec : std::false_type {};
template <class T>
struct is_pinvec<PinVec<T>> : std::true_type {};
struct SmallUploads {
  std::vector<uint8_t> host;
  std::vector<std::pair<size_t, void **>> dst;
  template <class T>
  void add(const std::vector<T> &v, T **out) {
    const size_t off = host.size(), bytes = v.size() * sizeof(T);
    host.resize(off + ((std::max<size_t>(bytes, 1) + 255) & ~size_t(255)));
    if (bytes) std::memcpy(host.data() + off, v.data(), bytes);
    dst.push_back({off, reinterpret_cast<void **>(out)});
    *out = nullptr;  // set when the arena is copied: a kernel launched before that reads null, not stale memory
  }
};

inline bool stopped(const volatile uint8_t *s) { return s && *s; }

// sqlm_prepare.cpp: initializeOptimization(level) + BlockSolver::buildStructure
// (the planner's stages, sqlm_plan.h) and the uploads
int prepare(sqlm_ctx *c, int level);
// sqlm_lm.cpp
void ensure_host_errors(sqlm_ctx *c);
int fetch_errors(sqlm_ctx *c);
int finish(sqlm_ctx *c);
int run_lm(sqlm_ctx *c, int iterations, double user_lambda, const volatile uint8_t *stop, sqlm_stats *st,
           int *n_iter, bool bench);
int optimize_impl(sqlm_ctx *c, int level, int iterations, double user_lambda, const volatile uint8_t *stop,
                  sqlm_stats *st, int *n_iter);

}  // namespace sqlm
