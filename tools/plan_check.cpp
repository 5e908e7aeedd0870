// plan_check: CPU test of the BA setup planner (csrc/sqlm_plan.cpp). Builds
// small graphs with a fixed integer generator, runs the planner's stages in
// prepare()'s order and checks every output against a naive single-threaded
// reference written here. No HIP, no libsqrtlm.so: g++ and sqlm_plan.cpp only.
// One "ok" line per graph on stdout; the first failing check is named on
// stderr and the exit status is 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <string>

#include "../sqrtlm-slam_amd/csrc/sqlm_plan.h"

namespace sqlm {
// The two launch-shape helpers the planner calls live beside the kernels
// (sqlm_kernels.hip); this host-only program links its own copies.
int linearize_blocks(const Bucket &b) {
  const int spb = kBlock / b.W, tiles = (b.slot_end - b.slot_begin + spb - 1) / spb;
  return std::min(tiles, 2048);
}
int upd_launch_plan(const std::vector<Bucket> &bk, const std::vector<int> &part_off, UpdLaunch &u) {
  u = UpdLaunch{};
  if (bk.size() > (size_t)kMaxUpdBuckets) return -1;
  std::vector<int> ord(bk.size());
  for (size_t b = 0; b < ord.size(); ++b) ord[b] = (int)b;
  std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return bk[x].W > bk[y].W; });
  for (int b : ord) {
    const int nb = linearize_blocks(bk[b]);
    if (nb <= 0) continue;
    const int k = u.nb++;
    u.W[k] = bk[b].W; u.slot_begin[k] = bk[b].slot_begin; u.slot_end[k] = bk[b].slot_end;
    u.part_off[k] = part_off[b]; u.rng_off[k] = bk[b].rng_off; u.nblk[k] = nb; u.blk0[k] = u.grid;
    u.grid += nb;
  }
  return 0;
}
}  // namespace sqlm

using namespace sqlm;

namespace {

struct Rng {  // fixed integer generator (LCG)
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed * 2862933555777941757ull + 3037000493ull) {}
  uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
  int below(int n) { return (int)(next() % (uint32_t)n); }
};

struct Graph {
  std::string name;
  int n_pose = 0, n_pt = 0, level = 0;
  std::vector<int32_t> obs_pose, obs_pt;
  std::vector<double> uv, info, delta, ur;  // ur empty: no stereo
  std::vector<uint8_t> obs_level, pose_fixed;
  std::vector<int32_t> lid_pose;
  std::vector<double> lid_pc, lid_pw, lid_n, lid_info;
  std::vector<uint8_t> lid_level;
  std::vector<uint8_t> ext_act;  // a shard of a sharded run: the poses the other ranks' edges make active
  int expect_status = SQLM_OK;
  int expect_solver = 0;  // 0 any, 1 band, 2 band + border, 3 dense
  int expect_f32 = -1, expect_robust = -1, expect_dups = -1, expect_tiles = -1;  // -1 any
  int expect_wide = -1;  // the first bucket's wide flag
  int expect_long = -1;  // 1: reduction lists of exactly kRedLong and of kRedLong + 1 entries exist
  Rng rng{1};
  int64_t n_obs() const { return (int64_t)obs_pose.size(); }
  void edge(int pose, int pt, int lvl = 0) {
    obs_pose.push_back(pose);
    obs_pt.push_back(pt);
    uv.push_back(rng.below(2560) * 0.25);  // float32 values
    uv.push_back(rng.below(1920) * 0.25);
    info.push_back(rng.below(2) ? 1.0 : 0.25);
    delta.push_back(0.0);
    obs_level.push_back((uint8_t)lvl);
  }
  int point() { return n_pt++; }
  // a new point seen by `track` consecutive poses from p0
  int track(int p0, int len, int lvl = 0) {
    const int l = point();
    for (int k = 0; k < len; ++k) edge(p0 + k, l, lvl);
    return l;
  }
  void lidar(int pose, int lvl = 0) {
    lid_pose.push_back(pose);
    for (int k = 0; k < 3; ++k) {
      lid_pc.push_back(rng.below(100) * 0.5);
      lid_pw.push_back(rng.below(100) * 0.5);
      lid_n.push_back(k == 0 ? 1.0 : 0.0);
    }
    lid_info.push_back(1.0 + rng.below(3));
    lid_level.push_back((uint8_t)lvl);
  }
  GraphView view() const {
    GraphView g;
    g.n_pose = n_pose; g.n_pt = n_pt; g.n_obs = n_obs(); g.n_lid = (int64_t)lid_pose.size();
    g.obs_pose = obs_pose.data(); g.obs_pt = obs_pt.data(); g.obs_uv = uv.data(); g.obs_info = info.data();
    g.obs_delta = delta.data(); g.obs_level = obs_level.data(); g.obs_ur = ur.empty() ? nullptr : ur.data();
    g.pose_fixed = pose_fixed.data();
    g.lid_pose = lid_pose.data(); g.lid_pc = lid_pc.data(); g.lid_pw = lid_pw.data(); g.lid_n = lid_n.data();
    g.lid_info = lid_info.data(); g.lid_level = lid_level.data();
    g.level = level;
    return g;
  }
};

// n_pt points, each seen by `window` consecutive poses; the first n_fixed poses fixed
Graph windowed(const char *name, int n_pose, int n_pt, int window, int n_fixed, uint64_t seed) {
  Graph G;
  G.name = name;
  G.rng = Rng(seed);
  G.n_pose = n_pose;
  G.pose_fixed.assign(n_pose, 0);
  for (int p = 0; p < n_fixed; ++p) G.pose_fixed[p] = 1;
  for (int l = 0; l < n_pt; ++l) G.track(G.rng.below(n_pose - window + 1), window);
  return G;
}

// Everything a setup decides, as prepare() would upload it.
struct Out {
  int status = SQLM_OK;
  SetupPlan pl;
  PlanScratch ps;
  std::vector<int64_t> dev_edge;
  std::vector<int> obs_lm, obs_cam, obs_camh, obs_loc;
  std::vector<float> obs_q;
  std::vector<double> obs_ur, obs_uv, obs_info, obs_delta;
  int lm_cap = 0;
  std::vector<int> sh_cam_ptr, sh_cam_obs, sh_s_row, sh_s_col;  // the sharded stages on one rank
};

ObsArrays arrays(Out &r) {
  ObsArrays o;
  o.dev_edge = r.dev_edge.data(); o.obs_lm = r.obs_lm.data(); o.obs_cam = r.obs_cam.data();
  o.obs_camh = r.obs_camh.data(); o.obs_q = r.obs_q.data(); o.obs_ur = r.obs_ur.data();
  o.obs_uv = r.obs_uv.data(); o.obs_info = r.obs_info.data(); o.obs_delta = r.obs_delta.data();
  return o;
}

// the stages in prepare()'s order (unsharded), then the sharded pattern stages as one rank
void run_plan(const Graph &G, Out &r) {
  PhaseTimer phase(kPhasePrepare);
  const GraphView g = G.view();
  SetupPlan &pl = r.pl;
  plan_active_set(g, true, r.ps, pl, phase);
  // prepare() ORs the ranks' pose_act here (all-reduce max)
  for (size_t p = 0; p < G.ext_act.size(); ++p) r.ps.pose_act[p] |= G.ext_act[p];
  if ((r.status = plan_slots(g, r.ps, pl, phase))) return;
  const size_t nE = (size_t)pl.nE;
  r.dev_edge.assign(nE, -1);
  r.obs_lm.assign(nE, -7); r.obs_cam.assign(nE, -7); r.obs_camh.assign(nE, -7); r.obs_loc.assign(nE, -7);
  r.obs_q.assign(4 * nE, -1.f);
  r.obs_ur.assign(G.ur.empty() ? 0 : nE, -7.0);
  plan_scatter(g, r.ps, pl, arrays(r), phase);
  if (!pl.obs_f32) {
    r.obs_uv.assign(2 * nE, -7.0); r.obs_info.assign(nE, -7.0); r.obs_delta.assign(nE, -7.0);
    plan_scatter_doubles(g, pl, arrays(r));
  }
  plan_cam_csr(g, false, pl, arrays(r));
  plan_update_windows(g, pl, r.obs_cam.data());
  r.lm_cap = tile_lm_cap(pl.nL);
  build_tiles(pl.nP, pl.nL, pl.lm_begin, r.obs_camh.data(), r.lm_cap, r.ps.tp, r.ps.tb, r.obs_loc.data());
  pattern_from_tiles(pl.nP, r.ps.tb, pl.s_row, pl.s_col);
  plan_solver(pl);
  build_tiles_finish(pl.nP, pl.s_row, pl.s_col, r.ps.tp, r.ps.tb);
  plan_lidar_groups(g, pl);
  SetupPlan sh = pl;
  std::vector<std::vector<int>> rows;
  plan_cam_csr(g, true, sh, arrays(r));
  plan_local_rows(sh, arrays(r), rows);
  plan_rows_to_pattern(rows, sh);
  r.sh_cam_ptr = sh.cam_ptr; r.sh_cam_obs = sh.cam_obs; r.sh_s_row = sh.s_row; r.sh_s_col = sh.s_col;
}

std::string g_ctx;  // "<graph> grain <g>" of the running check
[[noreturn]] void fail(const char *what) {
  std::fprintf(stderr, "FAIL %s: %s\n", g_ctx.c_str(), what);
  std::exit(1);
}
#define CHECK(cond, what) \
  do {                    \
    if (!(cond)) fail(what); \
  } while (0)

bool eq2(const std::vector<int2> &a, const std::vector<int2> &b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (a[i].x != b[i].x || a[i].y != b[i].y) return false;
  return true;
}

// ---- naive references -----------------------------------------------------

struct Naive {  // active set and slot order
  std::vector<uint8_t> pose_act, pt_act;
  std::vector<int> kcount, lo, hi, phidx, hidxp, pts;
  std::vector<std::vector<int64_t>> edges;  // active edges of every point, by id
  std::vector<int64_t> lid_act;
  int64_t n_ae = 0;
};

Naive naive_active(const Graph &G) {
  Naive n;
  n.pose_act.assign(G.n_pose, 0);
  n.pt_act.assign(G.n_pt, 0);
  n.kcount.assign(G.n_pt, 0);
  n.lo.assign(G.n_pt, 1 << 30);
  n.hi.assign(G.n_pt, -1);
  n.edges.resize(G.n_pt);
  for (int64_t e = 0; e < G.n_obs(); ++e) {
    if (G.obs_level[e] != G.level) continue;
    const int l = G.obs_pt[e], p = G.obs_pose[e];
    n.pt_act[l] = 1;
    n.pose_act[p] = 1;
    n.kcount[l]++;
    n.lo[l] = std::min(n.lo[l], p);
    n.hi[l] = std::max(n.hi[l], p);
    n.edges[l].push_back(e);
    ++n.n_ae;
  }
  for (size_t e = 0; e < G.lid_pose.size(); ++e)
    if (G.lid_level[e] == G.level && !G.pose_fixed[G.lid_pose[e]]) {
      n.lid_act.push_back((int64_t)e);
      n.pose_act[G.lid_pose[e]] = 1;
    }
  for (size_t p = 0; p < G.ext_act.size(); ++p) n.pose_act[p] |= G.ext_act[p];
  n.phidx.assign(G.n_pose, -1);
  for (int p = 0; p < G.n_pose; ++p)
    if (n.pose_act[p] && !G.pose_fixed[p]) { n.phidx[p] = (int)n.hidxp.size(); n.hidxp.push_back(p); }
  for (int l = 0; l < G.n_pt; ++l)
    if (n.pt_act[l]) n.pts.push_back(l);
  std::stable_sort(n.pts.begin(), n.pts.end(), [&](int a, int b) {
    const int wa = seg_width(n.kcount[a]), wb = seg_width(n.kcount[b]);
    if (wa != wb) return wa < wb;
    if (n.lo[a] != n.lo[b]) return n.lo[a] < n.lo[b];
    return n.hi[a] < n.hi[b];
  });
  return n;
}

void check_active_and_scatter(const Graph &G, const Naive &n, const Out &r) {
  const SetupPlan &pl = r.pl;
  CHECK(r.ps.pose_act == n.pose_act, "active set: pose_act");
  CHECK(r.ps.pt_act == n.pt_act, "active set: pt_act");
  CHECK(pl.n_ae == n.n_ae, "active set: n_ae");
  CHECK(pl.lid_act == n.lid_act, "active set: LiDAR active list");
  for (int l = 0; l < G.n_pt; ++l) {
    if (!n.pt_act[l]) continue;
    CHECK(r.ps.kcount[l] == n.kcount[l], "active set: kcount");
    CHECK(r.ps.span_lo[l] == n.lo[l] && r.ps.span_hi[l] == n.hi[l], "active set: spans");
    CHECK(r.ps.efirst[l] == n.edges[l].front() && r.ps.elast[l] == n.edges[l].back(), "active set: efirst / elast");
  }
  CHECK(pl.phidx == n.phidx && pl.hidxp == n.hidxp && pl.nP == (int)n.hidxp.size(), "indexing: phidx / hidxp");
  CHECK(pl.slot_pt == n.pts && pl.nL == (int)n.pts.size(), "slots: order against std::stable_sort");
  for (int s = 0; s < pl.nL; ++s) CHECK(r.ps.pt_slot[n.pts[s]] == s, "slots: pt_slot");
  // lm_begin and the scattered arrays: a stable sort of the active edges by slot
  CHECK((int)pl.lm_begin.size() == pl.nL + 1 && pl.lm_begin[0] == 0, "lm_begin: size");
  bool f32 = true, robust = false;
  int64_t o = 0, n_cam = 0;
  for (int s = 0; s < pl.nL; ++s) {
    CHECK(pl.lm_begin[s] == o, "lm_begin: prefix of the track lengths");
    for (int64_t e : n.edges[n.pts[s]]) {
      CHECK(r.dev_edge[o] == e, "scatter: dev_edge");
      CHECK(r.obs_lm[o] == s, "scatter: obs_lm");
      CHECK(r.obs_cam[o] == G.obs_pose[e], "scatter: obs_cam");
      CHECK(r.obs_camh[o] == n.phidx[G.obs_pose[e]], "scatter: obs_camh");
      const double in[4] = {G.uv[2 * e], G.uv[2 * e + 1], G.info[e], G.delta[e]};
      for (int k = 0; k < 4; ++k) {
        CHECK(r.obs_q[4 * o + k] == (float)in[k], "scatter: obs_q");
        f32 &= (double)(float)in[k] == in[k];
      }
      robust |= G.delta[e] > 0.0;
      if (!G.ur.empty()) CHECK(r.obs_ur[o] == G.ur[e], "scatter: obs_ur");
      n_cam += r.obs_camh[o] >= 0;
      ++o;
    }
  }
  CHECK(pl.lm_begin[pl.nL] == o && pl.nE == o, "lm_begin: nE");
  CHECK(pl.obs_f32 == f32, "scatter: obs_f32 flag");
  CHECK(pl.any_robust == robust, "scatter: any_robust flag");
  CHECK(pl.n_cam_obs == n_cam, "scatter: n_cam_obs");
  if (!f32)
    for (int64_t k = 0; k < o; ++k) {
      const int64_t e = r.dev_edge[k];
      CHECK(r.obs_uv[2 * k] == G.uv[2 * e] && r.obs_uv[2 * k + 1] == G.uv[2 * e + 1] && r.obs_info[k] == G.info[e] &&
                r.obs_delta[k] == G.delta[e],
            "scatter: double arrays");
    }
  // host camera CSR (sharded runs): observations by camera, slot order inside
  std::vector<int> cp(pl.nP + 1, 0), co;
  for (int i = 0; i < pl.nP; ++i) {
    for (int64_t k = 0; k < o; ++k)
      if (r.obs_camh[k] == i) co.push_back((int)k);
    cp[i + 1] = (int)co.size();
    if (pl.nE > 100000) break;  // (quadratic: small graphs only)
  }
  if (pl.nE <= 100000) CHECK(r.sh_cam_ptr == cp && r.sh_cam_obs == co, "camera CSR (host)");
  // LiDAR grouping by free camera
  std::vector<int> lp(pl.nP + 1, 0), lpose;
  std::vector<int64_t> le;
  std::vector<double> ld;
  for (int i = 0; i < pl.nP; ++i) {
    for (int64_t e : n.lid_act)
      if (n.phidx[G.lid_pose[e]] == i) {
        le.push_back(e);
        lpose.push_back(G.lid_pose[e]);
        for (int k = 0; k < 3; ++k) ld.push_back(G.lid_pc[3 * e + k]);
        for (int k = 0; k < 3; ++k) ld.push_back(G.lid_pw[3 * e + k]);
        for (int k = 0; k < 3; ++k) ld.push_back(G.lid_n[3 * e + k]);
        ld.push_back(G.lid_info[e]);
        ld.push_back(0.0);
        ld.push_back(0.0);
      }
    lp[i + 1] = (int)le.size();
  }
  CHECK(pl.lid_ptr == lp && pl.dev_lid_edge == le && pl.lid_pose == lpose && pl.lid_data == ld, "LiDAR grouping");
}

void check_buckets(const Naive &n, const Out &r) {
  const SetupPlan &pl = r.pl;
  int s = 0, parts = 0, prevW = 0;
  size_t rng = 0;
  CHECK(pl.buckets.size() == pl.bucket_part_off.size(), "buckets: part offsets");
  for (size_t b = 0; b < pl.buckets.size(); ++b) {
    const Bucket &bk = pl.buckets[b];
    CHECK(bk.slot_begin == s && bk.slot_end > s, "buckets: cover [0, nL) without gaps");
    const int Ws = seg_width(n.kcount[n.pts[s]]);
    CHECK(Ws > prevW, "buckets: ascending segment width");
    for (int k = bk.slot_begin; k < bk.slot_end; ++k) CHECK(seg_width(n.kcount[n.pts[k]]) == Ws, "buckets: one width per bucket");
    CHECK(bk.W == (Ws >= 4 ? Ws / 2 : Ws), "buckets: half-lane rule");
    CHECK(pl.bucket_part_off[b] == parts, "buckets: bucket_part_off");
    parts += linearize_blocks(bk);
    // update windows: brute-force min / max pose of every block's observations
    CHECK(bk.rng_off == (int)rng, "update windows: rng_off");
    const int spb = kBlock / bk.W;
    bool wide = false;
    for (int s0 = bk.slot_begin; s0 < bk.slot_end; s0 += spb, ++rng) {
      int lo = 1 << 30, hi = -1;
      for (int o = pl.lm_begin[s0]; o < pl.lm_begin[std::min(s0 + spb, bk.slot_end)]; ++o) {
        lo = std::min(lo, r.obs_cam[o]);
        hi = std::max(hi, r.obs_cam[o]);
      }
      CHECK(rng < pl.upd_rng.size() && pl.upd_rng[rng].x == lo && pl.upd_rng[rng].y == hi, "update windows: upd_rng");
      wide |= hi - lo + 1 > kUpdWin;
    }
    CHECK(bk.wide == wide, "update windows: wide");
    prevW = Ws;
    s = bk.slot_end;
  }
  CHECK(s == pl.nL, "buckets: end at nL");
  CHECK(rng == pl.upd_rng.size(), "update windows: count");
  CHECK(pl.n_lm_parts == parts, "buckets: n_lm_parts");
  if (pl.buckets.size() <= (size_t)kMaxUpdBuckets) CHECK(pl.upd.grid == parts, "update windows: one-launch grid");
  else CHECK(pl.upd.nb == 0, "update windows: per-bucket launches");
}

// free cameras (hidx) of slot sl, in observation order
std::vector<int> slot_cams(const Out &r, int sl) {
  std::vector<int> v;
  for (int o = r.pl.lm_begin[sl]; o < r.pl.lm_begin[sl + 1]; ++o)
    if (r.obs_camh[o] >= 0) v.push_back(r.obs_camh[o]);
  return v;
}

void check_tiles(const Out &r, std::vector<std::set<std::pair<int, int>>> &tile_pairs) {
  const SetupPlan &pl = r.pl;
  const TilePlan &tp = r.ps.tp;
  const int nL = pl.nL;
  // the greedy cut, single-threaded: chunk starts depend on the problem only
  const int nchunk = (int)std::max<int64_t>(1, std::min<int64_t>(16, pl.nE / 131072));
  std::vector<int> start;
  bool dups = false;
  for (int ch = 0; ch < nchunk; ++ch) {
    std::set<int> win;
    int nlm = 0;
    for (int sl = (int)((int64_t)nL * ch / nchunk); sl < (int)((int64_t)nL * (ch + 1) / nchunk); ++sl) {
      const std::vector<int> cams = slot_cams(r, sl);
      const std::set<int> cs(cams.begin(), cams.end());
      dups |= cs.size() != cams.size();
      std::set<int> merged = win;
      merged.insert(cs.begin(), cs.end());
      if (nlm == 0 || (int)merged.size() > kTileMaxCams || nlm >= r.lm_cap) {
        start.push_back(sl);
        win.clear();
        nlm = 0;
        merged = cs;
      }
      win = merged;
      ++nlm;
    }
  }
  if (start.empty() || start[0] != 0) start.insert(start.begin(), 0);
  if (nL > 0) start.push_back(nL);
  CHECK(tp.lm_ptr == start, "tiles: lm_ptr against the single-threaded greedy cut");
  CHECK(tp.dups == dups, "tiles: dups");
  const int nt = (int)tp.lm_ptr.size() - 1;
  CHECK((int)tp.cam_ptr.size() == nt + 1 && (int)tp.ld.size() == nt && (int)tp.part_ptr.size() == nt + 1 &&
            (int)tp.gpart_ptr.size() == nt + 1,
        "tiles: array sizes");
  CHECK((int)tp.urange.size() == nL, "tiles: urange size");
  tile_pairs.assign(nt, {});
  int max_cp = 0;
  std::set<int> chunk_starts;
  for (int ch = 0; ch < nchunk; ++ch) chunk_starts.insert((int)((int64_t)nL * ch / nchunk));
  for (int t = 0; t < nt; ++t) {
    const int s0 = tp.lm_ptr[t], s1 = tp.lm_ptr[t + 1];
    CHECK(s0 < s1, "tiles: lm_ptr partitions the slots");
    for (int sl = s0 + 1; sl < s1; ++sl) CHECK(!chunk_starts.count(sl), "tiles: no tile crosses a chunk start");
    std::set<int> cs;
    for (int sl = s0; sl < s1; ++sl)
      for (int h : slot_cams(r, sl)) cs.insert(h);
    const std::vector<int> cams(cs.begin(), cs.end());
    const int cp = (int)cams.size();
    CHECK(tp.cam_ptr[t + 1] - tp.cam_ptr[t] == cp &&
              std::equal(cams.begin(), cams.end(), tp.cams.begin() + tp.cam_ptr[t]),
          "tiles: cams is the sorted set of free cameras");
    CHECK(cp <= kTileMaxCams || s1 - s0 == 1, "tiles: closing rule (cameras)");
    CHECK(s1 - s0 <= r.lm_cap, "tiles: closing rule (landmarks)");
    CHECK(tp.ld[t] == (6 * cp + 15) / 16 * 16, "tiles: ld");
    CHECK(tp.part_ptr[t + 1] - tp.part_ptr[t] == 36 * (int64_t)(cp * (cp + 1) / 2), "tiles: part_ptr");
    CHECK(tp.gpart_ptr[t + 1] - tp.gpart_ptr[t] == tp.ld[t], "tiles: gpart_ptr");
    max_cp = std::max(max_cp, cp);
    for (int sl = s0; sl < s1; ++sl) {
      int lo = cp, hi = -1;
      std::vector<int> loc;
      for (int o = pl.lm_begin[sl]; o < pl.lm_begin[sl + 1]; ++o) {
        const int h = r.obs_camh[o];
        const int u = h < 0 ? -1 : (int)(std::lower_bound(cams.begin(), cams.end(), h) - cams.begin());
        CHECK(r.obs_loc[o] == u, "tiles: obs_local indexes into the tile's cameras");
        if (u >= 0) { lo = std::min(lo, u); hi = std::max(hi, u); loc.push_back(u); }
      }
      if (hi < 0) lo = -1;
      CHECK(tp.urange[sl].x == lo && tp.urange[sl].y == hi, "tiles: urange");
      for (int a : loc)
        for (int b : loc)
          if (a <= b) tile_pairs[t].insert({a, b});
    }
  }
  CHECK(tp.max_cp == max_cp, "tiles: max_cp");
  // launch classes
  bool any4 = false;
  for (int t = 0; t < nt; ++t) any4 |= tp.ld[t] / 16 == 4;
  std::vector<std::vector<int>> by(kTileNtMax + 1);
  for (int t = 0; t < nt; ++t) {
    const int w = tp.ld[t] / 16;
    by[w <= 3 && !any4 ? 3 : w <= 4 ? 4 : w <= 6 ? 6 : w <= 8 ? 8 : kTileNtMax].push_back(t);
  }
  int off = 0;
  for (int k = 0; k <= kTileNtMax; ++k) {
    CHECK(tp.cls_off[k] == off && tp.cls_cnt[k] == (int)by[k].size(), "tiles: cls_off / cls_cnt");
    CHECK(by[k].empty() || std::equal(by[k].begin(), by[k].end(), tp.order.begin() + off), "tiles: order by class");
    off += (int)by[k].size();
  }
  CHECK(tp.cls_off[kTileNtMax + 1] == nt && (int)tp.order.size() == std::max(nt, 1), "tiles: classes partition the tiles");
}

void check_pattern_and_lists(const Out &r, const std::vector<std::set<std::pair<int, int>>> &tile_pairs) {
  const SetupPlan &pl = r.pl;
  const TilePlan &tp = r.ps.tp;
  const int nP = pl.nP;
  // brute-force co-observation set: upper, diagonal first, columns sorted
  std::vector<std::set<int>> co(nP);
  for (int sl = 0; sl < pl.nL; ++sl) {
    const std::vector<int> cams = slot_cams(r, sl);
    for (int a : cams)
      for (int b : cams)
        if (a < b) co[a].insert(b);
  }
  std::vector<int> s_row(nP + 1, 0), s_col;
  for (int i = 0; i < nP; ++i) {
    s_col.push_back(i);
    s_col.insert(s_col.end(), co[i].begin(), co[i].end());
    s_row[i + 1] = (int)s_col.size();
  }
  CHECK(pl.s_row == s_row && pl.s_col == s_col, "S pattern: brute-force co-observation set");
  CHECK(r.sh_s_row == s_row && r.sh_s_col == s_col, "S pattern: sharded row stages on one rank");
  int mx = 0;
  for (int i = 0; i < nP; ++i) mx = std::max(mx, s_row[i + 1] - s_row[i]);
  CHECK(pl.max_row_blocks == mx, "S pattern: max_row_blocks");
  // reduction lists: every marked (tile, u <= v) once under its S block, ascending by tile
  const int nnzb = s_row[nP], nt = (int)tile_pairs.size();
  std::vector<std::vector<int64_t>> red(nnzb), gred(nP);
  for (int t = 0; t < nt; ++t) {
    const int *cams = tp.cams.data() + tp.cam_ptr[t];
    const int cp = tp.cam_ptr[t + 1] - tp.cam_ptr[t];
    for (const auto &uv : tile_pairs[t]) {
      const int i = cams[uv.first], j = cams[uv.second];
      const int k = (int)(std::lower_bound(s_col.begin() + s_row[i], s_col.begin() + s_row[i + 1], j) - s_col.begin());
      CHECK(k < s_row[i + 1] && s_col[k] == j, "reduction lists: pair outside the S pattern");
      red[k].push_back(tp.part_ptr[t] + 36 * (int64_t)tile_blk(uv.first, uv.second, cp));
    }
    for (int u = 0; u < cp; ++u) gred[cams[u]].push_back(tp.gpart_ptr[t] + 6 * (int64_t)u);
  }
  auto flat = [&](const std::vector<std::vector<int64_t>> &lists, const std::vector<int> &ptr,
                  const std::vector<int64_t> &off, const std::vector<int> &lng, const char *what) {
    CHECK(ptr.size() == lists.size() + 1 && ptr[0] == 0, what);
    std::vector<int> want_long;
    for (size_t k = 0; k < lists.size(); ++k) {
      CHECK(ptr[k + 1] - ptr[k] == (int)lists[k].size() &&
                std::equal(lists[k].begin(), lists[k].end(), off.begin() + ptr[k]),
            what);
      if ((int)lists[k].size() > kRedLong) want_long.push_back((int)k);
    }
    CHECK((size_t)ptr.back() == off.size(), what);
    CHECK(lng == want_long, "reduction lists: long_s / long_g are the lists longer than kRedLong");
  };
  flat(red, tp.red_ptr, tp.red_off, tp.long_s, "reduction lists: red_ptr / red_off");
  flat(gred, tp.gred_ptr, tp.gred_off, tp.long_g, "reduction lists: gred_ptr / gred_off");
}

void check_solver(const Graph &G, const Out &r) {
  const SetupPlan &pl = r.pl;
  const CRPlan &cr = pl.cr;
  const int nP = pl.nP;
  const int kind = nP == 0 ? 0 : !cr.enabled ? 3 : cr.nbc ? 2 : 1;
  if (G.expect_solver && nP) CHECK(kind == G.expect_solver, "plan_rcs: solver kind (band / border / dense)");
  std::vector<std::pair<int, int>> longe;
  for (int i = 0; i < nP; ++i)
    for (int k = pl.s_row[i]; k < pl.s_row[i + 1]; ++k)
      if (pl.s_col[k] - i > kBandMaxCams) longe.push_back({i, pl.s_col[k]});
  if (!cr.enabled) {
    if (nP == 0) return;
    // dense: no cover of the long blocks may fit a third of the cameras -- a
    // maximal matching of them bounds every cover from below -- unless the band
    // alone is too wide for a superblock
    std::vector<uint8_t> used(nP, 0);
    int m = 0;
    for (auto &e : longe)
      if (!used[e.first] && !used[e.second]) { used[e.first] = used[e.second] = 1; ++m; }
    if (G.expect_solver == 3) CHECK(3 * m > nP, "plan_rcs: dense fallback although a small border exists");
    return;
  }
  CHECK((int)pl.cam_pos.size() == nP, "plan_rcs: cam_pos size");
  int pos = 0, b = 0;
  for (int i = 0; i < nP; ++i) {
    if (pl.cam_pos[i] < 0) CHECK(pl.cam_pos[i] == -1 - b++, "plan_rcs: border indices ascend");
    else CHECK(pl.cam_pos[i] == pos++, "plan_rcs: band positions ascend");
  }
  CHECK(b == cr.nbc && pos == cr.nband && cr.nband + cr.nbc == nP, "plan_rcs: nband / nbc");
  CHECK(3 * cr.nbc <= nP, "plan_rcs: border at most a third of the cameras");
  for (auto &e : longe) CHECK(pl.cam_pos[e.first] < 0 || pl.cam_pos[e.second] < 0, "plan_rcs: far block without a border endpoint");
  int bw = 0;
  std::set<int> init;
  for (int i = 0; i < nP; ++i)
    for (int k = pl.s_row[i]; k < pl.s_row[i + 1]; ++k) {
      const int a = pl.cam_pos[i], c = pl.cam_pos[pl.s_col[k]];
      if (a >= 0 && c >= 0) bw = std::max(bw, c - a);
      else if ((a < 0) != (c < 0)) init.insert((a >= 0 ? a : c) / cr.B);
    }
  CHECK(cr.B >= std::min(bw + 1, std::max(cr.nband, 1)), "plan_rcs: B >= bandwidth + 1");
  if (cr.nbc) CHECK(cr.B == std::min(bw + 1, cr.nband), "plan_rcs: B of a bordered plan");
  CHECK(6 * cr.B <= kCRMaxN && cr.n <= kCRMaxN, "plan_rcs: 6 B <= kCRMaxN");
  CHECK(cr.p == (cr.nband + cr.B - 1) / cr.B && cr.n == (6 * cr.B + 15) / 16 * 16, "plan_rcs: p / n");
  CHECK(cr.R == (cr.nbc ? (6 * cr.nbc + 15) / 16 * 16 : 0), "plan_rcs: R");
  CHECK(cr.Rp == (cr.R + kCRMaxN - 1) / kCRMaxN * kCRMaxN, "plan_rcs: Rp");
  if (cr.nbc) {
    CHECK(cr.init_off == 0 && cr.init_cnt == (int)init.size() &&
              std::equal(init.begin(), init.end(), cr.sched.begin() + cr.init_off),
          "plan_rcs: initial list is the superblocks holding a band-border block");
    CHECK((int)cr.sched.size() == cr.elim_off + cr.elim_cnt, "plan_rcs: schedule ends with the elimination list");
  }
}

void check_all(const Graph &G, const Out &r) {
  CHECK(r.status == G.expect_status, "status");
  if (r.status) return;
  const Naive n = naive_active(G);
  check_active_and_scatter(G, n, r);
  check_buckets(n, r);
  std::vector<std::set<std::pair<int, int>>> tile_pairs;
  check_tiles(r, tile_pairs);
  check_pattern_and_lists(r, tile_pairs);
  check_solver(G, r);
  const bool use_tiles = r.pl.nP > 0 && r.ps.tp.max_cp <= kTileHardCams;
  if (G.expect_f32 >= 0) CHECK(r.pl.obs_f32 == (G.expect_f32 != 0), "expected obs_f32");
  if (G.expect_robust >= 0) CHECK(r.pl.any_robust == (G.expect_robust != 0), "expected any_robust");
  if (G.expect_dups >= 0) CHECK(r.ps.tp.dups == (G.expect_dups != 0), "expected dups");
  if (G.expect_tiles >= 0) CHECK(use_tiles == (G.expect_tiles != 0), "expected use_tiles");
  if (G.expect_wide >= 0) CHECK(r.pl.buckets[0].wide == (G.expect_wide != 0), "expected wide");
  if (G.expect_long == 1) {  // the graph does sit on the kRedLong step
    bool at = false, over = false;
    const std::vector<int> &rp = r.ps.tp.red_ptr;
    for (size_t k = 0; k + 1 < rp.size(); ++k) { at |= rp[k + 1] - rp[k] == kRedLong; over |= rp[k + 1] - rp[k] == kRedLong + 1; }
    CHECK(at && over, "expected reduction lists of kRedLong and kRedLong + 1 entries");
  }
}

// every output of two runs is identical (edge ids through `relabel` when given)
void check_same(const Out &a, const Out &b, const std::vector<int64_t> *relabel = nullptr) {
  const SetupPlan &p = a.pl, &q = b.pl;
  const TilePlan &s = a.ps.tp, &t = b.ps.tp;
  CHECK(a.status == b.status, "same: status");
  if (a.status) return;
  std::vector<int64_t> de = b.dev_edge;
  if (relabel)
    for (auto &e : de) e = (*relabel)[e];
  CHECK(a.dev_edge == de, "same: dev_edge");
  CHECK(a.obs_lm == b.obs_lm && a.obs_cam == b.obs_cam && a.obs_camh == b.obs_camh && a.obs_loc == b.obs_loc &&
            a.obs_q == b.obs_q && a.obs_ur == b.obs_ur && a.obs_uv == b.obs_uv && a.obs_info == b.obs_info &&
            a.obs_delta == b.obs_delta,
        "same: observation arrays");
  CHECK(p.phidx == q.phidx && p.hidxp == q.hidxp && p.slot_pt == q.slot_pt && p.lm_begin == q.lm_begin &&
            p.nE == q.nE && p.obs_f32 == q.obs_f32 && p.any_robust == q.any_robust && p.n_cam_obs == q.n_cam_obs &&
            p.n_lm_parts == q.n_lm_parts && p.bucket_part_off == q.bucket_part_off,
        "same: slots");
  CHECK(p.buckets.size() == q.buckets.size() && eq2(p.upd_rng, q.upd_rng), "same: update windows");
  for (size_t k = 0; k < p.buckets.size(); ++k)
    CHECK(p.buckets[k].W == q.buckets[k].W && p.buckets[k].slot_end == q.buckets[k].slot_end &&
              p.buckets[k].rng_off == q.buckets[k].rng_off && p.buckets[k].wide == q.buckets[k].wide,
          "same: buckets");
  CHECK(s.lm_ptr == t.lm_ptr && s.cam_ptr == t.cam_ptr && s.cams == t.cams && s.ld == t.ld && s.order == t.order &&
            s.part_ptr == t.part_ptr && s.gpart_ptr == t.gpart_ptr && eq2(s.urange, t.urange) && s.dups == t.dups &&
            s.max_cp == t.max_cp,
        "same: tiles");
  CHECK(s.red_ptr == t.red_ptr && s.red_off == t.red_off && s.gred_ptr == t.gred_ptr && s.gred_off == t.gred_off &&
            s.long_s == t.long_s && s.long_g == t.long_g,
        "same: reduction lists");
  CHECK(p.s_row == q.s_row && p.s_col == q.s_col && p.cam_pos == q.cam_pos && p.cr.enabled == q.cr.enabled &&
            p.cr.B == q.cr.B && p.cr.p == q.cr.p && p.cr.n == q.cr.n && p.cr.nbc == q.cr.nbc && p.cr.sched == q.cr.sched &&
            p.cr.lvl == q.cr.lvl,
        "same: S pattern and solver plan");
  CHECK(p.lid_ptr == q.lid_ptr && p.dev_lid_edge == q.dev_lid_edge && p.lid_data == q.lid_data, "same: LiDAR groups");
}

// The graph at the default grain (one thread unless it is large), at three
// threads for the edge passes and at the most threads the host gives; every
// run against the naive references, and all three identical.
int check_graph(const Graph &G, Out *keep = nullptr) {
  const int64_t grains[3] = {kHostGrain, std::max<int64_t>(1, G.n_obs() / 3), 1};
  Out first;
  int nth[3];
  for (int k = 0; k < 3; ++k) {
    g_host_grain = grains[k];
    nth[k] = host_threads(G.n_obs());
    g_ctx = G.name + " grain " + std::to_string(grains[k]);
    Out r;
    run_plan(G, r);
    check_all(G, r);
    if (k == 0) first = r;
    else check_same(first, r);
  }
  g_host_grain = kHostGrain;
  const SetupPlan &pl = first.pl;
  std::printf("ok %-14s status %d threads %d/%d/%d nP %d nL %d nE %lld tiles %zu nnzb %d solver %s dups %d f32 %d\n",
              G.name.c_str(), first.status, nth[0], nth[1], nth[2], pl.nP, pl.nL, (long long)pl.nE,
              first.status ? (size_t)0 : first.ps.tp.lm_ptr.size() - 1, first.status ? 0 : pl.s_row[pl.nP],
              first.status || pl.nP == 0 ? "-" : !pl.cr.enabled ? "dense" : pl.cr.nbc ? "border" : "band",
              (int)first.ps.tp.dups, (int)pl.obs_f32);
  if (keep) *keep = first;
  return 0;
}

// The same graph with its edges interleaved across landmarks (each landmark's
// own edge order kept): the general scatter route. relabel: new id -> old id.
Graph shuffled(const Graph &G, std::vector<int64_t> &relabel) {
  Graph S = G;
  S.name = G.name + "-shuf";
  const int64_t n = G.n_obs();
  Rng rng(99);
  std::vector<int64_t> pos(n);
  for (int64_t i = 0; i < n; ++i) pos[i] = i;
  for (int64_t i = n - 1; i > 0; --i) std::swap(pos[i], pos[rng.below((int)i + 1)]);
  // the edges of a point take the positions drawn for them, in ascending order
  std::map<int, std::vector<int64_t>> by_pt;
  for (int64_t e = 0; e < n; ++e) by_pt[G.obs_pt[e]].push_back(e);
  relabel.assign(n, -1);
  for (auto &kv : by_pt) {
    std::vector<int64_t> where;
    for (int64_t e : kv.second) where.push_back(pos[e]);
    std::sort(where.begin(), where.end());
    for (size_t k = 0; k < where.size(); ++k) relabel[where[k]] = kv.second[k];
  }
  for (int64_t j = 0; j < n; ++j) {
    const int64_t e = relabel[j];
    S.obs_pose[j] = G.obs_pose[e]; S.obs_pt[j] = G.obs_pt[e]; S.uv[2 * j] = G.uv[2 * e]; S.uv[2 * j + 1] = G.uv[2 * e + 1];
    S.info[j] = G.info[e]; S.delta[j] = G.delta[e]; S.obs_level[j] = G.obs_level[e];
  }
  return S;
}

// A rank of a sharded run that owns no landmark (n_pt = n_obs = 0): the
// other ranks' cameras are free here too, every list is empty, S is its diagonal
void check_empty_shard() {
  Graph es;
  es.name = "empty-shard";
  es.n_pose = 12;
  es.pose_fixed.assign(12, 0);
  es.pose_fixed[0] = es.pose_fixed[1] = 1;
  es.ext_act.assign(12, 1);
  es.ext_act[11] = 0;
  es.expect_tiles = 1;
  Out eo;
  check_graph(es, &eo);
  g_ctx = "empty-shard";
  CHECK(eo.pl.nP == 9 && eo.pl.nL == 0 && eo.pl.nE == 0 && eo.pl.n_lm_parts == 0, "empty shard: sizes");
  CHECK(eo.pl.buckets.empty() && eo.pl.upd.nb == 0 && eo.pl.upd_rng.empty(), "empty shard: no update launch");
  CHECK(eo.ps.tp.lm_ptr.size() == 1 && eo.ps.tp.red_off.empty() && eo.ps.tp.gred_off.empty(), "empty shard: no tiles");
  CHECK((int)eo.ps.tp.red_ptr.size() == eo.pl.s_row[eo.pl.nP] + 1 && (int)eo.ps.tp.gred_ptr.size() == eo.pl.nP + 1,
        "empty shard: reduction list pointers cover the pattern");
  CHECK(eo.sh_cam_ptr == std::vector<int>(10, 0) && eo.sh_cam_obs.empty(), "empty shard: camera CSR");
  CHECK(eo.pl.lm_begin == std::vector<int>(1, 0) && eo.pl.slot_pt.empty(), "empty shard: lm_begin");
}

}  // namespace

// No argument: the graphs of an unsharded setup. "shard": the graphs that stand
// for one rank of a sharded run.
int main(int argc, char **argv) {
  if (argc > 1 && std::string(argv[1]) == "shard") {
    check_empty_shard();
    return 0;
  }
  // 1. the smoke shape: band only
  Graph smoke = windowed("smoke", 12, 300, 3, 2, 1);
  smoke.expect_solver = 1; smoke.expect_f32 = 1; smoke.expect_robust = 0; smoke.expect_dups = 0; smoke.expect_tiles = 1;
  Out smoke_out;
  check_graph(smoke, &smoke_out);
  {  // route equivalence: contiguous edge runs against the same graph through the general route
    std::vector<int64_t> relabel;
    const Graph S = shuffled(smoke, relabel);
    Out so;
    check_graph(S, &so);
    g_ctx = "smoke vs smoke-shuf";
    check_same(smoke_out, so, &relabel);
  }
  // 2. ~45 free poses, a handful of points seen by two poses 40 apart: a border
  Graph border = windowed("border", 47, 400, 3, 2, 2);
  for (int k = 0; k < 5; ++k) { const int l = border.point(); border.edge(2, l); border.edge(42, l); }
  border.expect_solver = 2;
  check_graph(border);
  // 3. the same with disjoint closures, one border camera each: 15 of them are
  // still a third of the 45 cameras, 16 exceed it -- the dense fallback
  Graph border15 = windowed("border-15", 47, 400, 3, 2, 2);
  for (int i = 2; i < 17; ++i) { const int l = border15.point(); border15.edge(i, l); border15.edge(i + 22, l); }
  border15.expect_solver = 2;
  check_graph(border15);
  Graph dense = windowed("dense", 47, 400, 3, 2, 2);
  for (int i = 2; i < 18; ++i) { const int l = dense.point(); dense.edge(i, l); dense.edge(i + 22, l); }
  dense.expect_solver = 3;
  check_graph(dense);
  // 4. a landmark whose edges come in two separate runs (the atomic pass at > 1 thread)
  Graph split = windowed("two-runs", 12, 300, 3, 2, 3);
  split.edge(7, 100); split.edge(8, 100);
  split.edge(1, 5);
  check_graph(split);
  // 5. half the edges at level 1; inactive point / pose; LiDAR on a fixed pose and at the other level
  for (int level = 0; level < 2; ++level) {
    Graph lv;
    lv.name = level ? "levels-1" : "levels-0";
    lv.rng = Rng(5);
    lv.n_pose = 16;
    lv.level = level;
    lv.pose_fixed.assign(16, 0);
    lv.pose_fixed[0] = lv.pose_fixed[1] = 1;
    for (int l = 0; l < 240; ++l) {
      const int p0 = lv.rng.below(11), pt = lv.point();
      for (int k = 0; k < 4; ++k) lv.edge(p0 + k, pt, lv.rng.below(2));
    }
    lv.track(3, 3, 1);    // a point whose edges are all at level 1
    lv.track(15, 1, 1);   // pose 15 is seen by a level-1 edge only
    lv.track(14, 1, 1);
    for (int k = 0; k < 3; ++k) lv.lidar(0);      // fixed pose
    for (int k = 0; k < 3; ++k) lv.lidar(6, 0);
    for (int k = 0; k < 2; ++k) lv.lidar(4, 1);   // the other level
    lv.lidar(6, 0);
    lv.lidar(13, 1);
    check_graph(lv);
  }
  // 6. track lengths on the seg_width steps and at the 64-lane cap
  {
    Graph tr;
    tr.name = "tracks";
    tr.rng = Rng(6);
    tr.n_pose = 210;
    tr.pose_fixed.assign(210, 0);
    tr.pose_fixed[0] = 1;
    const int lens[11] = {1, 2, 6, 7, 12, 13, 24, 25, 96, 97, 200};
    for (int rep = 0; rep < 5; ++rep)
      for (int len : lens) tr.track(tr.rng.below(210 - len + 1), len);
    tr.expect_tiles = 0;
    check_graph(tr);
  }
  // 7. one landmark seen by 70 cameras: byte-matrix pair path, tiles off
  Graph wide = windowed("wide-70", 80, 300, 3, 1, 7);
  wide.track(5, 70);
  wide.expect_tiles = 0;
  check_graph(wide);
  // 7b. one block of landmark-update slots whose pose window is exactly kUpdWin
  // wide, and one pose wider
  for (int extra = 0; extra < 2; ++extra) {
    Graph win;
    win.name = extra ? "window-65" : "window-64";
    win.rng = Rng(70);
    win.n_pose = 80;
    win.pose_fixed.assign(80, 0);
    win.track(5, 2);
    for (int k = 0; k < 18; ++k) win.track(6 + win.rng.below(55), 2);
    win.track(5 + kUpdWin - 2 + extra, 2);
    win.expect_wide = extra;
    check_graph(win);
  }
  // 7c. S blocks / cameras with 20 .. 28 tile contributions: both sides of kRedLong
  {
    Graph lg;
    lg.name = "long-lists";
    lg.rng = Rng(71);
    lg.n_pose = 18;
    lg.pose_fixed.assign(18, 0);
    for (int i = 0; i < 9; ++i)
      for (int k = 0; k < 16 * (20 + i); ++k) lg.track(2 * i, 2);
    lg.expect_long = 1;
    check_graph(lg);
  }
  // 8. a landmark observing the same pose twice
  Graph dup = windowed("dup", 12, 300, 3, 2, 8);
  { const int l = dup.point(); dup.edge(4, l); dup.edge(5, l); dup.edge(4, l); }
  dup.expect_dups = 1;
  check_graph(dup);
  // 9. one uv value that is no float32; one robust edge
  Graph inexact = windowed("non-f32", 12, 300, 3, 2, 9);
  inexact.uv[2 * 100 + 1] = 0.1;
  inexact.expect_f32 = 0; inexact.expect_robust = 0;
  check_graph(inexact);
  Graph robust = windowed("robust", 12, 300, 3, 2, 9);
  robust.delta[77] = 2.5;
  robust.expect_f32 = 1; robust.expect_robust = 1;
  check_graph(robust);
  // 10. stereo edges (obs_ur travels with the scatter)
  Graph stereo = windowed("stereo", 12, 300, 3, 2, 10);
  for (int64_t e = 0; e < stereo.n_obs(); ++e) stereo.ur.push_back(e % 3 ? stereo.rng.below(2000) * 0.25 : -1.0);
  check_graph(stereo);
  // 11. an empty active set
  Graph empty = windowed("empty", 12, 50, 3, 2, 11);
  empty.level = 1;
  empty.expect_status = SQLM_ERR_STATE;
  check_graph(empty);
  // 12. at least 2 x 131072 observations: two tile chunks, several threads at the default grain
  Graph big = windowed("big", 60, 66000, 4, 2, 12);
  big.expect_solver = 1;
  check_graph(big);
  return 0;
}
