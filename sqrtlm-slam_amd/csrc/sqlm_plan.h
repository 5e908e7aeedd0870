// sqlm_plan.h — the host-only planner of a BA setup: active set, landmark
// slots and buckets, observation scatter, update windows, RCS tiles, the S
// pattern, the solver plan and the LiDAR grouping. Everything here decides
// what the kernels compute -- the slot order, the tile boundaries and the
// reduction lists fix the summation order of S and g -- and none of it calls
// HIP: prepare() (sqlm_prepare.cpp) runs the stages and uploads their results,
// tools/plan_check.cpp runs them on a CPU against naive references.
#pragma once
#include <cstdint>
#include <vector>

#include "sqlm_host_par.h"
#include "sqlm_internal.h"

namespace sqlm {

// Landmark tiles for the RCS assembly: runs of consecutive slots whose free
// cameras fit a window of <= kTileMaxCams cameras (sorted), plus the reduction
// lists that sum each S block / g row from its tiles in tile order.
struct TilePlan {
  std::vector<int> lm_ptr{0}, cam_ptr{0}, cams, ld, red_ptr, gred_ptr;
  std::vector<int2> urange, gred_idx;
  std::vector<int64_t> red_off;   // absolute offset (doubles) of each contribution's 6x6 block in part
  std::vector<int64_t> gred_off;  // ... and of each g contribution's 6 doubles in gpart
  std::vector<int> long_s, long_g;  // S blocks / cameras with more than kRedLong contributions
  std::vector<int64_t> part_ptr{0}, gpart_ptr{0};
  int max_cp = 0;
  bool dups = false;
  std::vector<int> order;  // tile ids grouped by nt class (ascending id within a class)
  int cls_off[kTileNtMax + 2] = {}, cls_cnt[kTileNtMax + 1] = {};
  // back to the empty plan, keeping every vector's memory (a context reuses
  // its plan across calls: no reallocation, no first-touch page faults)
  void reset() {
    lm_ptr.assign(1, 0);
    cam_ptr.assign(1, 0);
    part_ptr.assign(1, 0);
    gpart_ptr.assign(1, 0);
    for (auto *v : {&cams, &ld, &red_ptr, &gred_ptr, &long_s, &long_g, &order}) v->clear();
    urange.clear();
    gred_idx.clear();
    red_off.clear();
    gred_off.clear();
    max_cp = 0;
    dups = false;
    std::fill(cls_off, cls_off + kTileNtMax + 2, 0);
    std::fill(cls_cnt, cls_cnt + kTileNtMax + 1, 0);
  }
};

// Intermediate state of build_tiles between the tiles (passes 1-2) and the
// reduction lists, which need the S pattern (built from the tiles' camera
// pairs in between).
struct TileBuild {
  struct Red { int key, tile, code, j; };  // key: camera i until the pattern exists, then the S block
  struct TileOut { std::vector<int> cams; std::vector<Red> red; };
  std::vector<int> tstart;
  std::vector<TileOut> out;
};

void build_tiles(int nP, int nL, const std::vector<int> &lm_begin, const int *obs_camh, int lm_cap, TilePlan &tp,
                 TileBuild &tb, int *obs_local);
void pattern_from_tiles(int nP, const TileBuild &tb, std::vector<int> &s_row, std::vector<int> &s_col);
void build_tiles_finish(int nP, const std::vector<int> &s_row, const std::vector<int> &s_col, TilePlan &tp,
                        TileBuild &tb);
int cr_superblock_width(int bmin, int nband);

// Level arithmetic of the block cyclic reduction over p superblocks numbered
// lo .. p + lo - 1 (CRPlan::lo): level l runs at stride h[l] = 2^l, eliminates
// the n_odd[l] odd multiples of h[l] (I = h + 2 h q) and updates the n_even[l]
// even ones (J = 2 h (q + lo)); levels run while two superblocks are alive and
// `top` is the survivor. lo = 0: ceil(log2 p) levels, top 0. lo = 1:
// floor(log2 p) levels, top the largest power of two <= p. The one-launch back
// substitution holds back_grid workgroups, the levels coarsest first
// (cr_back_block). launch_cr_core takes its grids from here and
// tools/cr_levels_check.cpp checks them against a simulated elimination.
struct CRLevels {
  static constexpr int kMax = 32;
  int lo = 0, top = 0, count = 0, back_grid = 0;
  int h[kMax] = {}, n_odd[kMax] = {}, n_even[kMax] = {};
};
inline CRLevels cr_levels(int p, int lo) {
  CRLevels L;
  L.lo = lo;
  const int last = p + lo - 1;  // highest superblock index
  int h = 1;
  for (; L.count < CRLevels::kMax && last / h + 1 - lo >= 2; h *= 2) {  // multiples of h in [lo, last]
    L.h[L.count] = h;
    L.n_odd[L.count] = (last + h) / (2 * h);
    L.n_even[L.count] = last / (2 * h) + 1 - lo;
    L.back_grid += L.n_odd[L.count];
    ++L.count;
  }
  L.top = lo ? h : 0;
  return L;
}
// Workgroup b of the one-launch back substitution -> (level, superblock I):
// what k_cr_back_all computes from its block index.
inline void cr_back_block(const CRLevels &L, int b, int &level, int &I) {
  level = L.count - 1;
  while (level > 0 && b >= L.n_odd[level]) b -= L.n_odd[level--];
  I = L.h[level] + 2 * L.h[level] * b;
}
bool plan_rcs(int nP, const std::vector<int> &s_row, const std::vector<int> &s_col, CRPlan &pl,
              std::vector<int> &cam_pos);

// Lanes per landmark segment in the per-landmark kernels: up to kObsPerLane
// observations per lane, at least 2 lanes.
inline int seg_width(int k) {
  int w = 2;
  while (kObsPerLane * w < k && w < 64) w <<= 1;
  return w;
}

// The caller-order graph of one setup, read-only.
struct GraphView {
  int n_pose = 0, n_pt = 0;
  int64_t n_obs = 0, n_lid = 0;
  const int32_t *obs_pose = nullptr, *obs_pt = nullptr;
  const double *obs_uv = nullptr, *obs_info = nullptr, *obs_delta = nullptr;
  const uint8_t *obs_level = nullptr;
  const double *obs_ur = nullptr;  // null: no stereo edge
  const uint8_t *pose_fixed = nullptr;
  const int32_t *lid_pose = nullptr;
  const double *lid_pc = nullptr, *lid_pw = nullptr, *lid_n = nullptr, *lid_info = nullptr;
  const uint8_t *lid_level = nullptr;
  const uint8_t *lid_kind = nullptr;  // 0 flat, 1 corner; null: every edge flat
  int level = 0;
};

// Host plan scratch a context keeps across calls (capacity reused: a setup
// allocates and first-touches none of its large arrays after the first call).
struct PlanScratch {
  TilePlan tp;
  TileBuild tb;
  std::vector<std::vector<int>> scat_base;  // per-thread counting-sort bases (slots)
  std::vector<int> kcount, span_lo, span_hi, pt_slot, key;
  std::vector<int> efirst, elast;  // first / last active edge of every landmark (contiguity test)
  std::vector<int> btot;           // landmark-slot bucket totals
  std::vector<uint8_t> pose_act, pt_act;
};

// The slot-ordered observation arrays a setup writes (nE entries; obs_q 4 nE,
// obs_uv 2 nE). prepare() passes its page-locked upload buffers.
struct ObsArrays {
  int64_t *dev_edge = nullptr;  // device obs -> edge id
  int *obs_lm = nullptr, *obs_cam = nullptr, *obs_camh = nullptr;
  float *obs_q = nullptr;        // u v info delta as float32, exact when obs_f32
  double *obs_ur = nullptr;      // stereo only
  double *obs_uv = nullptr, *obs_info = nullptr, *obs_delta = nullptr;  // only when !obs_f32
};

// What the stages decide. Lives in the context: the LM driver reads the
// buckets, the update launch and the solver plan.
struct SetupPlan {
  // stage 1
  int64_t n_ae = 0;               // active mono / stereo edges
  std::vector<int64_t> lid_act;   // active LiDAR edges (free pose, this level)
  // stage 2
  std::vector<int> phidx, hidxp;  // pose -> free hidx or -1, and back
  int nP = 0, nL = 0;
  std::vector<int> slot_pt;       // device slot -> point id
  std::vector<Bucket> buckets;
  std::vector<int> bucket_part_off;
  int n_lm_parts = 0;
  std::vector<int> lm_begin;
  int64_t nE = 0;
  // stage 3
  bool obs_f32 = true, any_robust = false;
  std::vector<int> cam_ptr, cam_obs;  // host camera CSR (sharded runs only)
  int64_t n_cam_obs = 0;
  // stage 4
  std::vector<int2> upd_rng;
  UpdLaunch upd;  // every bucket's landmark update in one launch (nb = 0: per bucket)
  // stages 5-6
  std::vector<int> s_row, s_col;
  int max_row_blocks = 0;
  CRPlan cr;
  std::vector<int> cam_pos;  // hidx -> band position or -(1 + border index)
  // stage 7
  std::vector<int> lid_ptr, lid_pose;
  std::vector<double> lid_data;
  std::vector<int64_t> dev_lid_edge;  // device lidar -> lidar edge id
};

// 1. Active set: pose_act / pt_act, track lengths, camera spans and edge runs
// of every landmark, then the active LiDAR edges (with_lidar: rank 0 of a
// sharded run, or an unsharded one).
void plan_active_set(const GraphView &g, bool with_lidar, PlanScratch &ps, SetupPlan &pl, PhaseTimer &phase);
// 2. Indexing and slots: phidx / hidxp, the landmark slot order, the buckets
// and lm_begin. Returns a status (SQLM_ERR_UNSUPPORTED, SQLM_ERR_STATE).
int plan_slots(const GraphView &g, PlanScratch &ps, SetupPlan &pl, PhaseTimer &phase);
// 3. Observation scatter into slot order (o.dev_edge .. o.obs_ur), the
// double arrays when some input is no float32 value, and the camera CSR /
// count of observations seen by a free camera.
void plan_scatter(const GraphView &g, PlanScratch &ps, SetupPlan &pl, const ObsArrays &o, PhaseTimer &phase);
void plan_scatter_doubles(const GraphView &g, const SetupPlan &pl, const ObsArrays &o);
void plan_cam_csr(const GraphView &g, bool host_csr, SetupPlan &pl, const ObsArrays &o);
// 4. Update windows: the pose id window of every per-landmark block tile.
void plan_update_windows(const GraphView &g, SetupPlan &pl, const int *obs_cam);
// 5. Landmarks per tile, then the tiles (build_tiles) and the S pattern:
// pattern_from_tiles, or for a sharded run the local rows, whose union over
// the ranks (made by prepare()) plan_rows_to_pattern turns into s_row / s_col.
int tile_lm_cap(int nL);
void plan_local_rows(const SetupPlan &pl, const ObsArrays &o, std::vector<std::vector<int>> &rows);
void plan_rows_to_pattern(const std::vector<std::vector<int>> &rows, SetupPlan &pl);
// 6. Solver plan: the band (+ border) superblock plan, or none (dense solver).
void plan_solver(SetupPlan &pl);
// 7. LiDAR edges grouped by free camera.
void plan_lidar_groups(const GraphView &g, SetupPlan &pl);

}  // namespace sqlm
