// sqlm_prepare.cpp — the setup of one optimize() call: the planner's stages
// (sqlm_plan.h), the exchanges of a sharded run between them, and the uploads.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "sqlm_ctx.h"

namespace sqlm {

namespace {

// The page-locked slot-ordered arrays of one setup (uploaded as they are).
struct ObsPins {
  PinVec<int> obs_lm, obs_cam, obs_camh, obs_loc;
  PinVec<double> obs_uv, obs_info, obs_delta, obs_ur;
  PinVec<float> obs_q;  // u v info delta as float32, exact when obs_f32
};

GraphView graph_view(const sqlm_ctx *c, int level) {
  GraphView g;
  g.n_pose = c->n_pose;
  g.n_pt = c->n_pt;
  g.n_obs = c->n_obs;
  g.n_lid = c->n_lid;
  g.obs_pose = c->obs_pose.data();
  g.obs_pt = c->obs_pt.data();
  g.obs_uv = c->obs_uv.data();
  g.obs_info = c->obs_info.data();
  g.obs_delta = c->obs_delta.data();
  g.obs_level = c->obs_level.data();
  g.obs_ur = c->has_stereo ? c->obs_ur.data() : nullptr;
  g.pose_fixed = c->pose_fixed.data();
  g.lid_pose = c->lid_pose.data();
  g.lid_pc = c->lid_pc.data();
  g.lid_pw = c->lid_pw.data();
  g.lid_n = c->lid_n.data();
  g.lid_info = c->lid_info.data();
  g.lid_level = c->lid_level.data();
  g.lid_kind = c->lid_kind.data();
  g.level = level;
  return g;
}

// Every rank of a sharded run needs the same S pattern: the union of the
// shards' rows. Blocks within kNearCams of the diagonal as one flag per (row,
// offset), OR-ed by an all-reduce (max); the few far blocks (loop closures) as
// (row, column) pairs all-gathered through a summed, zero-padded buffer.
int union_rows(sqlm_ctx *c, int nP, std::vector<std::vector<int>> &rows) {
  constexpr int kNearCams = 64;
  std::vector<uint8_t> near((size_t)nP * kNearCams, 0);
  std::vector<int> far;
  for (int i = 0; i < nP; ++i)
    for (size_t k = 1; k < rows[i].size(); ++k) {
      const int off = rows[i][k] - i;
      if (off < kNearCams) near[(size_t)i * kNearCams + off] = 1;
      else { far.push_back(i); far.push_back(rows[i][k]); }
    }
  if (comm_allreduce_host(c->comm, near.data(), (int64_t)near.size(), SQLM_DT_U8, SQLM_OP_MAX, c->stream))
    return SQLM_ERR_COMM;
  const int R = c->comm.nranks, me = c->comm.rank;
  std::vector<int> cnt(R, 0);
  cnt[me] = (int)far.size();
  if (comm_allreduce_host(c->comm, cnt.data(), R, SQLM_DT_I32, SQLM_OP_SUM, c->stream)) return SQLM_ERR_COMM;
  int64_t tot = 0, mine = 0;
  for (int r = 0; r < R; ++r) { if (r < me) mine += cnt[r]; tot += cnt[r]; }
  std::vector<int> all((size_t)tot, 0);
  std::copy(far.begin(), far.end(), all.begin() + mine);
  if (tot && comm_allreduce_host(c->comm, all.data(), tot, SQLM_DT_I32, SQLM_OP_SUM, c->stream))
    return SQLM_ERR_COMM;
  for (int i = 0; i < nP; ++i) {
    rows[i].assign(1, i);
    for (int off = 1; off < kNearCams && i + off < nP; ++off)
      if (near[(size_t)i * kNearCams + off]) rows[i].push_back(i + off);
  }
  for (int64_t k = 0; k < tot; k += 2) rows[all[k]].push_back(all[k + 1]);
  for (int i = 0; i < nP; ++i) {
    std::sort(rows[i].begin() + 1, rows[i].end());
    rows[i].erase(std::unique(rows[i].begin() + 1, rows[i].end()), rows[i].end());
  }
  return SQLM_OK;
}

// plan shape (SQLM_PREP_TIMING=1): tile count, longest reduction lists, solver layout
void print_plan(const SetupPlan &pl, const TilePlan &tp) {
  int rmax = 0, gmax = 0;
  for (size_t s = 0; s + 1 < tp.red_ptr.size(); ++s) rmax = std::max(rmax, tp.red_ptr[s + 1] - tp.red_ptr[s]);
  for (size_t s = 0; s + 1 < tp.gred_ptr.size(); ++s) gmax = std::max(gmax, tp.gred_ptr[s + 1] - tp.gred_ptr[s]);
  std::fprintf(stderr,
               "prepare plan: nP %d nL %d nnzb %d tiles %zu max_cp %d red %zu (max/block %d, long %zu) gred max %d "
               "(long %zu) | CR %d B %d p %d n %d border %d R %d init %d elim %d\n",
               pl.nP, pl.nL, pl.s_row[pl.nP], tp.lm_ptr.size() - 1, tp.max_cp, tp.red_off.size(), rmax, tp.long_s.size(),
               gmax, tp.long_g.size(),
               (int)pl.cr.enabled, pl.cr.B, pl.cr.p, pl.cr.n, pl.cr.nbc, pl.cr.R, pl.cr.init_cnt, pl.cr.elim_cnt);
}

// std::vector: small ones into the arena (one copy at the end of the setup)
template <class V, class P>
int up(sqlm_ctx *c, SmallUploads &small, int id, V &vec, P **ptr) {
  if constexpr (!is_pinvec<std::remove_const_t<V>>::value) {
    if (vec.size() * sizeof(typename V::value_type) <= kSmallUpload) {
      small.add(vec, ptr);
      return SQLM_OK;
    }
  }
  return upload(c, id, vec, ptr);
}
// UP: small arrays' device pointers are set when the arena is copied (before
// the first kernel that reads them); UPD: a direct copy, pointer set now
#define UP(id, vec, ptr) \
  if (int st_ = up(c, small, id, vec, &ptr)) return st_;
#define UPD(id, vec, ptr) \
  if (int st_ = upload(c, id, vec, &ptr)) return st_;
#define AL(id, n, ptr) \
  if (int st_ = ensure(c, id, n, &ptr)) return st_;

// The observation arrays go to the device as soon as they are scattered,
// overlapped with the rest of the setup.
int upload_observations(sqlm_ctx *c, const ObsPins &o) {
  DevProblem &d = c->d;
  const bool obs_f32 = c->plan.obs_f32;
  UPD(B_OBSLM, o.obs_lm, d.obs_lm);
  UPD(B_OBSCAM, o.obs_cam, d.obs_cam);
  UPD(B_OBSCAMH, o.obs_camh, d.obs_camh);
  d.obs_f32 = obs_f32 ? 1 : 0;
  if (obs_f32) {
    UPD(B_OBSQ, o.obs_q, d.obs_q);
    d.obs_uv = d.obs_info = d.obs_delta = nullptr;
  } else {
    UPD(B_OBSUV, o.obs_uv, d.obs_uv);
    UPD(B_OBSINFO, o.obs_info, d.obs_info);
    UPD(B_OBSDELTA, o.obs_delta, d.obs_delta);
    d.obs_q = nullptr;
  }
  if (c->has_stereo) UPD(B_OBSUR, o.obs_ur, d.obs_ur);
  (void)hipStreamQuery(c->stream);  // submit now: the runtime would otherwise batch them until the next sync
  return SQLM_OK;
}

// Problem sizes, pose and landmark state, index maps and the landmark buffers.
int upload_state(sqlm_ctx *c, SmallUploads &small) {
  DevProblem &d = c->d;
  const SetupPlan &pl = c->plan;
  const int nP = pl.nP, nL = pl.nL;
  d.n_pose = c->n_pose;
  d.sharded = c->comm.enabled() ? 1 : 0;
  d.rank = c->comm.rank;
  d.nP = nP;
  d.nL = nL;
  d.nE = pl.nE;
  d.nLid = (int64_t)pl.lid_act.size();
  d.nnzb = pl.s_row[nP];
  // single-GPU tiled path: k_rcs_reduce writes the CR superblocks directly
  d.cr_direct = (pl.cr.enabled && c->use_tiles && !c->comm.enabled()) ? 1 : 0;
  d.cr_B = pl.cr.B;
  d.cr_n = pl.cr.n;
  d.cr_p = pl.cr.p;
  d.cr_nband = pl.cr.nband;
  d.arw_R = pl.cr.R;
  d.arw_Rp = pl.cr.Rp;
  std::vector<double> qt(8 * (size_t)c->n_pose, 0.0);
  for (int p = 0; p < c->n_pose; ++p) {
    for (int k = 0; k < 4; ++k) qt[8 * p + k] = c->pose_q[4 * p + k];
    for (int k = 0; k < 3; ++k) qt[8 * p + 4 + k] = c->pose_t[3 * p + k];
  }
  // the landmark states in slot order go through a page-locked buffer filled
  // on host threads, like obs_local (a pageable copy is staged by the runtime
  // on the calling thread: ~3 ms for these two arrays, 36 MB)
  PinVec<double> X;
  {
    if (int e = pinned(c, P_X, 4 * (size_t)nL, X)) return e;
    const int nth = host_threads(c->n_obs);
    run_threads(nth, [&](int t) {
      for (int sl = (int)((int64_t)nL * t / nth); sl < (int)((int64_t)nL * (t + 1) / nth); ++sl) {
        const double *src = c->pt.data() + 3 * (size_t)pl.slot_pt[sl];
        double *dst = X.data() + 4 * (size_t)sl;
        dst[0] = src[0];
        dst[1] = src[1];
        dst[2] = src[2];
        dst[3] = 0.0;
      }
    });
  }
  UP(B_QT0, qt, d.pose_qt[0]);
  UP(B_QT1, qt, d.pose_qt[1]);
  AL(B_RT0, 16 * (size_t)c->n_pose, d.pose_rt[0]);
  AL(B_RT1, 16 * (size_t)c->n_pose, d.pose_rt[1]);
  UP(B_INTR, c->intr, d.intr);
  UP(B_PHIDX, pl.phidx, d.pose_hidx);
  UP(B_HIDXP, pl.hidxp, d.hidx_pose);
  UP(B_X0, X, d.X[0]);
  AL(B_X1, 4 * (size_t)nL, d.X[1]);
  if (nL) SQLM_HIP_OK(hipMemcpyAsync(d.X[1], d.X[0], 4 * (size_t)nL * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  UP(B_LMBEG, pl.lm_begin, d.lm_begin);
  AL(B_LMR, 8 * (size_t)nL, d.lm_R);
  AL(B_LMB, 4 * (size_t)nL, d.lm_b);
  AL(B_LMM, 8 * (size_t)nL, d.lm_M);
  AL(B_LMV, 4 * (size_t)nL, d.lm_v);
  return SQLM_OK;
}

// The RCS tiles, their reduction lists and the update windows.
int upload_tiles(sqlm_ctx *c, SmallUploads &small, const PinVec<int> &obs_loc) {
  DevProblem &d = c->d;
  const SetupPlan &pl = c->plan;
  const TilePlan &tp = c->scratch.tp;
  const int nL = pl.nL;
  d.n_tiles = c->use_tiles ? (int)tp.lm_ptr.size() - 1 : 0;
  std::copy(tp.cls_off, tp.cls_off + kTileNtMax + 2, d.tile_cls_off);
  std::copy(tp.cls_cnt, tp.cls_cnt + kTileNtMax + 1, d.tile_cls_cnt);
  d.tile_dups = tp.dups ? 1 : 0;
  {
    const char *tw = std::getenv("SQLM_TILE_PROD");  // read per setup: tests/test_gpu_first_trial.py switches it
    d.tile_prod = tw && std::atoi(tw) == 0 ? 0 : 1;
  }
  {
    int mk = 0;
    for (int sl = 0; sl < nL; ++sl) mk = std::max(mk, pl.lm_begin[sl + 1] - pl.lm_begin[sl]);
    d.tile_maxk = mk;
  }
  d.n_long_s = d.n_long_g = 0;
  if (c->use_tiles) {
    UP(B_TLM, tp.lm_ptr, d.tile_lm_ptr);
    UP(B_TCAMP, tp.cam_ptr, d.tile_cam_ptr);
    UP(B_TORDER, tp.order, d.tile_order);
    UP(B_TCAMS, tp.cams, d.tile_cams);
    UP(B_TPART, tp.part_ptr, d.tile_part_ptr);
    UP(B_TGPART, tp.gpart_ptr, d.tile_gpart_ptr);
    UP(B_TLD, tp.ld, d.tile_ld);
    UP(B_URANGE, tp.urange, d.lm_urange);
    UP(B_OBSLOC, obs_loc, d.obs_local);
    AL(B_PART2, (size_t)tp.part_ptr.back(), d.part);
    AL(B_GPART, (size_t)tp.gpart_ptr.back(), d.gpart);
    UP(B_REDP, tp.red_ptr, d.red_ptr);
    UP(B_REDI, tp.red_off, d.red_off);
    UP(B_GREDP, tp.gred_ptr, d.gred_ptr);
    UP(B_GREDI, tp.gred_off, d.gred_off);
    UP(B_LONGS, tp.long_s, d.long_s);
    UP(B_LONGG, tp.long_g, d.long_g);
    d.n_long_s = (int)tp.long_s.size();
    d.n_long_g = (int)tp.long_g.size();
  }
  UP(B_UPDRNG, pl.upd_rng, d.upd_rng);
  return SQLM_OK;
}

// The per-edge work buffers, the camera CSR and the camera-ordered copies of
// the camera pass inputs, the speculative buffers and the LiDAR groups.
int upload_camera_side(sqlm_ctx *c, SmallUploads &small) {
  DevProblem &d = c->d;
  const SetupPlan &pl = c->plan;
  const int nP = pl.nP, nL = pl.nL;
  const int64_t nE = pl.nE, n_cam_obs = pl.n_cam_obs;
  const bool sharded = c->comm.enabled();
  AL(B_OBSS, (size_t)nE, d.obs_s);
  if (c->use_tiles) {
    d.obs_P = nullptr;  // consumers recompute the H_lp blocks from obs_s
  } else {
    AL(B_OBSP, 18 * (size_t)nE, d.obs_P);
  }
  AL(B_OBSERR, 2 * (size_t)nE, d.obs_err);
  if (sharded) {
    UPD(B_CAMPTR, pl.cam_ptr, d.cam_obs_ptr);  // (k_cam_gather below reads them)
    UPD(B_CAMOBS, pl.cam_obs, d.cam_obs);
  } else {  // the stable counting sort on the device (same result as the host's)
    unsigned *k0 = nullptr, *k1 = nullptr;
    int *v0 = nullptr;
    unsigned char *tmp = nullptr;
    const size_t sort_bytes = cam_csr_temp_bytes(nE, nP);
    AL(B_CAMKEY0, (size_t)nE, k0);
    AL(B_CAMKEY1, (size_t)nE, k1);
    AL(B_CAMVAL, (size_t)nE, v0);
    AL(B_SORTTMP, sort_bytes, tmp);
    AL(B_CAMOBS, (size_t)nE, d.cam_obs);
    AL(B_CAMPTR, (size_t)nP + 1, d.cam_obs_ptr);
    if (launch_cam_csr(d.obs_camh, nE, nP, k0, k1, v0, d.cam_obs, d.cam_obs_ptr, tmp, sort_bytes, c->stream))
      return SQLM_ERR_HIP;
  }
  d.has_stereo = c->has_stereo ? 1 : 0;
  if (c->has_stereo) {
    UP(B_POSEBF, c->pose_bf, d.pose_bf);
    AL(B_OBSERR3, (size_t)nE, d.obs_err3);
    AL(B_CAMUR, (size_t)n_cam_obs, d.cam_ur);
  } else {
    d.obs_ur = d.obs_err3 = d.pose_bf = d.cam_ur = nullptr;
  }
  // camera-ordered copies of the camera pass inputs (one coalesced stream +
  // the X gather), gathered on the device from the slot-ordered arrays
  AL(B_CAMSLOT, (size_t)n_cam_obs, d.cam_slot);
  if (d.obs_f32) {
    AL(B_CAMQ, 4 * (size_t)n_cam_obs, d.cam_q);
    d.cam_uv = nullptr;
  } else {
    AL(B_CAMUV, 4 * (size_t)n_cam_obs, d.cam_uv);
    d.cam_q = nullptr;
  }
  launch_cam_gather(d, n_cam_obs, c->stream);
  AL(B_HPP, 36 * (size_t)nP, d.Hpp);
  AL(B_BP, 8 * (size_t)nP, d.bp);
  {
    const bool no_spec = getenv("SQLM_NO_SPEC") && atoi(getenv("SQLM_NO_SPEC")) != 0;
    c->no_pose_fuse = getenv("SQLM_NO_POSE_FUSE") != nullptr;
    c->spec = c->use_tiles && d.obs_P == nullptr && !no_spec;
    c->trial_stores = getenv("SQLM_TRIAL_STORES") && atoi(getenv("SQLM_TRIAL_STORES")) != 0;
    d.trial_stores = c->trial_stores ? 1 : 0;
    // no robust edge: the weights are sqrt(info) at every state, written once by k_linearize
    d.s_const = !pl.any_robust && !c->trial_stores ? 1 : 0;
    // the side stream's fork / join (two event records, two waits: ~20 us of
    // host API time per trial) pays only when the pass is long enough to hide
    // (profiles/r03/ab_lba_cam_inline.log)
    c->cam_inline = d.nE < (1 << 18);
    if (sharded) c->cam_inline = false;
  }
  c->lin_valid = false;
  d.pc_lm = kPartChiCurLm;
  d.pc_lid = kPartChiCurLid;
  d.px_lm = kPartChiCurLm2;
  d.px_lid = kPartChiCurLid2;
  if (c->spec) {
    AL(B_LMR_NX, 8 * (size_t)nL, d.lm_R_nx);
    AL(B_LMB_NX, 4 * (size_t)nL, d.lm_b_nx);
    if (d.s_const) d.obs_s_nx = d.obs_s;
    else AL(B_OBSS_NX, (size_t)nE, d.obs_s_nx);
    AL(B_HPP_NX, 36 * (size_t)nP, d.Hpp_nx);
    AL(B_BP_NX, 8 * (size_t)nP, d.bp_nx);
  } else {
    d.lm_R_nx = d.lm_b_nx = d.obs_s_nx = d.Hpp_nx = d.bp_nx = nullptr;
  }
  UP(B_LIDPTR, pl.lid_ptr, d.lid_cam_ptr);
  UP(B_LIDDATA, pl.lid_data, d.lid_data);
  d.has_corner = 0;
  for (size_t t = 10; t < pl.lid_data.size(); t += 12) d.has_corner |= pl.lid_data[t] != 0.0;
  UP(B_LIDPOSE, pl.lid_pose, d.lid_pose);
  AL(B_LIDERR, (size_t)d.nLid, d.lid_err);
  return SQLM_OK;
}

// The S pattern and the solver's buffers: cyclic reduction (band, or band +
// border) or the dense Cholesky, then the reduction scalars.
int upload_solver(sqlm_ctx *c, SmallUploads &small) {
  DevProblem &d = c->d;
  SetupPlan &pl = c->plan;
  const int nP = pl.nP;
  const std::vector<int> &s_row = pl.s_row, &s_col = pl.s_col;
  UP(B_SROW, s_row, d.s_row_ptr);
  UP(B_SCOL, s_col, d.s_col);
  {
    std::vector<int> srow(s_col.size());
    for (int i = 0; i < nP; ++i)
      for (int k = s_row[i]; k < s_row[i + 1]; ++k) srow[k] = i;
    UP(B_SROWIDX, srow, d.s_row);
  }
  AL(B_S, 36 * (size_t)d.nnzb, d.S);
  AL(B_G, 6 * (size_t)nP, d.g);
  AL(B_DX, 6 * (size_t)nP + 1, d.dx);
  d.cam_pos = nullptr;
  if (pl.cr.enabled) {
    const size_t nb = (size_t)pl.cr.p * pl.cr.n * pl.cr.n;
    AL(B_CRD, nb, d.cr_D);
    AL(B_CRL, nb, d.cr_L);
    AL(B_CRE, nb, d.cr_E);
    AL(B_CRA, nb, d.cr_A);
    AL(B_CRC, nb, d.cr_C);
    AL(B_CRG, (size_t)pl.cr.p * pl.cr.n, d.cr_g);
    AL(B_CRX, (size_t)pl.cr.p * pl.cr.n, d.cr_x);
    {  // completion words of the one-launch back substitution, from epoch 0
      int *dn = nullptr;
      AL(B_CRDONE, (size_t)pl.cr.p, dn);
      SQLM_HIP_OK(hipMemsetAsync(dn, 0, (size_t)pl.cr.p * sizeof(int), c->stream));
      c->crs = CRSync{dn, pl.cr.p, 0};
    }
    if (pl.cr.R) {  // band + border layout
      const size_t fr = (size_t)pl.cr.p * pl.cr.n * pl.cr.R, rp = (size_t)pl.cr.Rp;
      UP(B_CAMPOS, pl.cam_pos, d.cam_pos);
      int *sd = nullptr;
      UPD(B_ARWS, pl.cr.sched, sd);
      pl.cr.sched_dev = sd;
      AL(B_ARWG, fr, d.arw_G);
      AL(B_ARWZ, fr, d.arw_Z);
      AL(B_BDA, rp * rp, d.bd_A);
      AL(B_BDL, rp * rp, d.bd_L);
      AL(B_BDLI, rp * kCRMaxN, d.bd_Linv);
      AL(B_BDR, rp, d.bd_r);
      AL(B_BDX, rp, d.bd_x);
    }
  } else {  // blocked MFMA Cholesky of the dense S (sqlm_rcs_solve.hip)
    const int np_ = (6 * nP + kCRMaxN - 1) / kCRMaxN * kCRMaxN;
    {  // two np_ x np_ matrices: refuse what the device cannot hold instead of failing mid-solve
      size_t fr = 0, tot = 0;
      if (hipMemGetInfo(&fr, &tot) == hipSuccess && 2.0 * 8.0 * np_ * (double)np_ > 0.9 * (double)fr)
        return SQLM_ERR_OOM;
    }
    d.dense_n = np_;
    AL(B_DENSE, (size_t)np_ * np_, d.dense);
    AL(B_DENSEL, (size_t)np_ * np_, d.dense_L);
    AL(B_DENSELI, (size_t)np_ * kCRMaxN, d.dense_Linv);
    AL(B_DENSER, (size_t)np_, d.dense_r);
    AL(B_DENSEX, (size_t)np_, d.dense_x);
  }
  AL(B_PART, (size_t)kMaxPartials, d.partials);
  AL(B_SCAL, (size_t)kNScalars, d.scalars);
  AL(B_MAXD, 1, d.maxdiag);
  AL(B_FLAGS, 4, d.flags);
  SQLM_HIP_OK(hipMemsetAsync(d.flags, 0, 4 * sizeof(int), c->stream));  // flags[1]: sticky device error of the solves
  return SQLM_OK;
}

// Sharded runs: every rank's nonzero S rows -- the free cameras its own edges
// (and, on rank 0, the LiDAR edges) touch -- and rank 0's gather table and
// staging buffer for the others' rows.
int upload_gather_table(sqlm_ctx *c, const int *obs_camh) {
  DevProblem &d = c->d;
  const SetupPlan &pl = c->plan;
  const int nP = pl.nP;
  const std::vector<int> &s_row = pl.s_row;
  AL(B_HDIAG, 6 * (size_t)nP, d.hdiag);
  c->s_row_host = s_row;
  int lo = nP, hi = 0;
  for (int64_t o = 0; o < pl.nE; ++o)
    if (obs_camh[o] >= 0) { lo = std::min(lo, obs_camh[o]); hi = std::max(hi, obs_camh[o] + 1); }
  for (int i = 0; i < nP; ++i)
    if (pl.lid_ptr[i + 1] > pl.lid_ptr[i]) { lo = std::min(lo, i); hi = std::max(hi, i + 1); }
  if (lo >= hi) lo = hi = 0;
  const int R = c->comm.nranks, me = c->comm.rank;
  if (R > kMaxRanks) return SQLM_ERR_UNSUPPORTED;
  std::vector<int> rng(2 * R, 0);
  rng[2 * me] = lo;
  rng[2 * me + 1] = hi;
  if (comm_allreduce_host(c->comm, rng.data(), 2 * R, SQLM_DT_I32, SQLM_OP_SUM, c->stream)) return SQLM_ERR_COMM;
  c->sh_lo.assign(R, 0);
  c->sh_hi.assign(R, 0);
  for (int r = 0; r < R; ++r) { c->sh_lo[r] = rng[2 * r]; c->sh_hi[r] = rng[2 * r + 1]; }
  GatherTab &t = c->gather;
  t.n = 0;
  int64_t off = 0;
  for (int r = 1; r < R; ++r) {
    const int a = c->sh_lo[r], b = c->sh_hi[r];
    t.s_lo[t.n] = 36 * (int64_t)s_row[a];
    t.s_hi[t.n] = 36 * (int64_t)s_row[b];
    t.s_src[t.n] = off;
    off += t.s_hi[t.n] - t.s_lo[t.n];
    t.g_lo[t.n] = 6 * (int64_t)a;
    t.g_hi[t.n] = 6 * (int64_t)b;
    t.g_src[t.n] = off;
    off += t.g_hi[t.n] - t.g_lo[t.n];
    ++t.n;
  }
  if (me == 0) AL(B_XSTAGE, (size_t)std::max<int64_t>(off, 1), d.xstage);
  return SQLM_OK;
}

// The arena of the small arrays: one page-locked block, one copy; their
// device pointers are set here.
int upload_arena(sqlm_ctx *c, SmallUploads &small) {
  if (small.host.empty()) return SQLM_OK;
  uint8_t *dev = nullptr;
  AL(B_ARENA, small.host.size(), dev);
  PinVec<uint8_t> stg;
  if (int st = pinned(c, P_ARENA, small.host.size(), stg)) return st;
  std::memcpy(stg.data(), small.host.data(), small.host.size());
  SQLM_HIP_OK(hipMemcpyAsync(dev, stg.data(), small.host.size(), hipMemcpyHostToDevice, c->stream));
  for (const auto &[off, p] : small.dst) *p = dev + off;
  return SQLM_OK;
}
#undef UP
#undef UPD
#undef AL

// Everything after the planning: buffers, copies and the setup kernels, in
// stream order.
int upload_all(sqlm_ctx *c, const ObsPins &o) {
  DevProblem &d = c->d;
  SmallUploads small;
  int st = 0;
  if ((st = upload_state(c, small)) || (st = upload_tiles(c, small, o.obs_loc)) ||
      (st = upload_camera_side(c, small)) || (st = upload_solver(c, small)))
    return st;
  d.hdiag = nullptr;
  d.xstage = nullptr;
  if (c->comm.enabled() && (st = upload_gather_table(c, o.obs_camh.data()))) return st;
  if ((st = upload_arena(c, small))) return st;
  SQLM_HIP_OK(hipMemsetAsync(d.partials, 0, sizeof(double) * kMaxPartials, c->stream));
  SQLM_HIP_OK(hipMemsetAsync(d.maxdiag, 0, sizeof(unsigned long long), c->stream));
  c->err_state = -1;  // no error evaluated yet (fetch_errors then delivers zeros)
  launch_pose_prep(d, 0, c->stream);
  return SQLM_OK;
}

// Stages 5-6 of the plan: RCS tiles (passes 1-2: windows, local cameras,
// camera pairs), then the reduced-camera-system pattern (upper, diagonal
// first) from the tiles' camera pairs -- sharded: the union of the ranks'
// rows -- the solver plan, then the tiles' reduction lists over that pattern.
int plan_tiles_and_solver(sqlm_ctx *c, const ObsArrays &oa, int *obs_loc, PhaseTimer &phase) {
  SetupPlan &pl = c->plan;
  TilePlan &tp = c->scratch.tp;
  TileBuild &tb = c->scratch.tb;
  const int nP = pl.nP;
  build_tiles(nP, pl.nL, pl.lm_begin, oa.obs_camh, tile_lm_cap(pl.nL), tp, tb, obs_loc);
  phase("tiles");
  if (!c->comm.enabled()) {
    pattern_from_tiles(nP, tb, pl.s_row, pl.s_col);
    phase("  S rows");
  } else {
    std::vector<std::vector<int>> rows;
    plan_local_rows(pl, oa, rows);
    if (int s = union_rows(c, nP, rows)) return s;
    plan_rows_to_pattern(rows, pl);
  }
  plan_solver(pl);
  phase("S pattern");
  build_tiles_finish(nP, pl.s_row, pl.s_col, tp, tb);
  phase("tile lists");
  if (phase.on) print_plan(pl, tp);
  c->use_tiles = nP > 0 && tp.max_cp <= kTileHardCams;
  if (!c->use_tiles && pl.max_row_blocks > 128) return SQLM_ERR_UNSUPPORTED;
  return SQLM_OK;
}

}  // namespace

int prepare(sqlm_ctx *c, int level) {
  // edges outside this call's level keep their last error (g2o semantics):
  // bring the previous call's errors home before the device copies change
  if (int s = fetch_errors(c)) return s;
  c->prepared = false;
  c->step_valid = false;
  // the page-locked staging arrays are rewritten (or regrown) below: no DMA of
  // an earlier call, finished or abandoned on an error path, may still read them
  SQLM_HIP_OK(hipStreamSynchronize(c->stream));
  PhaseTimer phase(kPhasePrepare);
  const GraphView g = graph_view(c, level);
  SetupPlan &pl = c->plan;
  PlanScratch &ps = c->scratch;
  const bool sharded = c->comm.enabled();
  plan_active_set(g, !sharded || c->comm.rank == 0, ps, pl, phase);
  // sharded: every rank must index the same free cameras (union of shards)
  if (sharded &&
      comm_allreduce_host(c->comm, ps.pose_act.data(), c->n_pose, SQLM_DT_U8, SQLM_OP_MAX, c->stream))
    return SQLM_ERR_COMM;
  c->n_active_edges = (int)(pl.n_ae + (int64_t)pl.lid_act.size());
  if (int s = plan_slots(g, ps, pl, phase)) return s;
  const int64_t nE = pl.nE;
  c->dev_edge.resize(nE);  // every entry is written by the scatter below
  ObsPins o;
  {
    int e = 0;
    if ((e = pinned(c, P_OBSLM, nE, o.obs_lm)) || (e = pinned(c, P_OBSCAM, nE, o.obs_cam)) ||
        (e = pinned(c, P_OBSCAMH, nE, o.obs_camh)) || (e = pinned(c, P_OBSQ, 4 * nE, o.obs_q)) ||
        (e = pinned(c, P_OBSUR, c->has_stereo ? nE : 0, o.obs_ur)))
      return e;
  }
  phase("  pinned");
  ObsArrays oa;
  oa.dev_edge = c->dev_edge.data();
  oa.obs_lm = o.obs_lm.data();
  oa.obs_cam = o.obs_cam.data();
  oa.obs_camh = o.obs_camh.data();
  oa.obs_q = o.obs_q.data();
  oa.obs_ur = o.obs_ur.data();
  plan_scatter(g, ps, pl, oa, phase);
  if (!pl.obs_f32) {
    int e = 0;
    if ((e = pinned(c, P_OBSUV, 2 * nE, o.obs_uv)) || (e = pinned(c, P_OBSINFO, nE, o.obs_info)) ||
        (e = pinned(c, P_OBSDELTA, nE, o.obs_delta)))
      return e;
    oa.obs_uv = o.obs_uv.data();
    oa.obs_info = o.obs_info.data();
    oa.obs_delta = o.obs_delta.data();
    plan_scatter_doubles(g, pl, oa);
  }
  plan_cam_csr(g, sharded, pl, oa);
  phase("  camh count");
  if (int s = upload_observations(c, o)) return s;
  phase("obs+camcsr");
  if (phase.on && std::getenv("SQLM_PREP_SYNC")) {  // diagnostic: the early uploads alone
    (void)hipStreamSynchronize(c->stream);
    phase("obs upload");
  }
  plan_update_windows(g, pl, oa.obs_cam);
  // every observation's camera in its tile's window, written straight into the
  // page-locked upload buffer
  if (int e = pinned(c, P_OBSLOC, (size_t)nE, o.obs_loc)) return e;
  if (int s = plan_tiles_and_solver(c, oa, o.obs_loc.data(), phase)) return s;
  plan_lidar_groups(g, pl);
  phase("lidar");
  if (int s = upload_all(c, o)) return s;
  phase("upload");
  if (phase.on) {  // how long the queued copies and setup kernels still run after the host is done
    (void)hipStreamSynchronize(c->stream);
    phase("gpu drain");
  }
  c->prepared = true;
  return SQLM_OK;
}

}  // namespace sqlm
