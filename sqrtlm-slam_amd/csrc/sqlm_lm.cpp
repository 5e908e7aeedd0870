// sqlm_lm.cpp — host LM driver.
//
// The host side owns only control: it mirrors g2o's Levenberg–Marquardt loop
// decision for decision (optimization_algorithm_levenberg.cpp:61-164,
// sparse_optimizer.cpp:354-419) and keeps every array in HBM; one small
// device->host copy of the reduced scalars per LM trial is the only sync.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "sqlm_ctx.h"

namespace sqlm {

// The per-edge errors of the last optimize() (computeActiveErrors' _error of
// every active edge) into the caller-order host arrays: ~90 MB on config 4,
// fetched only when a caller needs an edge chi2 (LBA outlier tags,
// sqlm_get_edge_chi2) or before the next prepare() replaces them on the
// device -- a GBA call that never asks does not pay for the copy. They are
// evaluated only now, by k_edge_errors at the state the last linearization or
// trial evaluated (err_state; that state is still on the device): the LM loop
// stores no per-edge error.
namespace {

// A device -> host staging array of n doubles: page-locked (one DMA), or the
// pageable `fallback` if the page-locked arena cannot grow.
void stage_out(sqlm_ctx *c, int id, size_t n, PinVec<double> &v, std::vector<double> &fallback) {
  if (pinned(c, id, n, v) == SQLM_OK) return;
  fallback.resize(std::max<size_t>(n, 1));
  v.p = fallback.data();
  v.n = n;
}

}  // namespace

void ensure_host_errors(sqlm_ctx *c) {
  if (!c->err_zero) return;
  c->err_zero = false;
  par_assign(c->obs_err, (const double *)nullptr, 2 * (size_t)c->n_obs);
}

int fetch_errors(sqlm_ctx *c) {
  if (!c->err_pending) return SQLM_OK;
  c->err_pending = false;
  if (hipSetDevice(c->device) != hipSuccess) return SQLM_ERR_HIP;
  ensure_host_errors(c);
  DevProblem &d = c->d;
  PinVec<double> err, err3, lerr;
  std::vector<double> fallback[3];
  stage_out(c, P_RERR, 2 * (size_t)d.nE, err, fallback[0]);
  stage_out(c, P_RERR3, d.obs_err3 ? (size_t)d.nE : 0, err3, fallback[1]);
  stage_out(c, P_RLERR, (size_t)d.nLid, lerr, fallback[2]);
  if (c->err_state < 0) {  // nothing evaluated since prepare(): zeros
    if (d.nE) SQLM_HIP_OK(hipMemsetAsync(d.obs_err, 0, sizeof(double) * 2 * (size_t)d.nE, c->stream));
    if (d.nE && d.obs_err3) SQLM_HIP_OK(hipMemsetAsync(d.obs_err3, 0, sizeof(double) * (size_t)d.nE, c->stream));
  } else if (!c->trial_stores) {  // the errors of the last evaluated state, computed now
    launch_edge_errors(d, c->err_state, c->stream);
  }
  if (err3.size())
    SQLM_HIP_OK(hipMemcpyAsync(err3.data(), d.obs_err3, err3.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (d.nE) SQLM_HIP_OK(hipMemcpyAsync(err.data(), d.obs_err, err.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (d.nLid)
    SQLM_HIP_OK(hipMemcpyAsync(lerr.data(), d.lid_err, lerr.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  SQLM_HIP_OK(hipStreamSynchronize(c->stream));
  const int nth = host_threads(d.nE);
  run_threads(nth, [&](int t) {
    for (int64_t o = d.nE * t / nth; o < d.nE * (t + 1) / nth; ++o) {
      c->obs_err[2 * c->dev_edge[o]] = err[2 * o];
      c->obs_err[2 * c->dev_edge[o] + 1] = err[2 * o + 1];
      if (err3.size()) c->obs_err3[c->dev_edge[o]] = err3[o];
    }
  });
  for (int64_t t = 0; t < d.nLid; ++t) c->lid_err[c->plan.dev_lid_edge[t]] = lerr[t];
  return SQLM_OK;
}

int finish(sqlm_ctx *c) {
  DevProblem &d = c->d;
  // device -> page-locked staging (one DMA each; pageable vectors if the
  // page-locked arena cannot grow), then the scatter back to caller order on
  // host threads; the edge errors stay on the device until asked for
  PinVec<double> qt, X;
  std::vector<double> fallback[2];
  stage_out(c, P_RQT, 8 * (size_t)c->n_pose, qt, fallback[0]);
  stage_out(c, P_RX, 4 * (size_t)d.nL, X, fallback[1]);
  SQLM_HIP_OK(hipMemcpyAsync(qt.data(), d.pose_qt[0], qt.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (d.nL) SQLM_HIP_OK(hipMemcpyAsync(X.data(), d.X[0], X.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  SQLM_HIP_OK(hipStreamSynchronize(c->stream));
  for (int p = 0; p < c->n_pose; ++p) {
    for (int k = 0; k < 4; ++k) c->pose_q[4 * p + k] = qt[8 * p + k];
    for (int k = 0; k < 3; ++k) c->pose_t[3 * p + k] = qt[8 * p + 4 + k];
  }
  const int nth = host_threads(d.nL * 8);
  run_threads(nth, [&](int t) {
    for (int s = (int)((int64_t)d.nL * t / nth); s < (int)((int64_t)d.nL * (t + 1) / nth); ++s)
      for (int k = 0; k < 3; ++k) c->pt[3 * c->plan.slot_pt[s] + k] = X[4 * s + k];
  });
  c->err_pending = d.nE > 0 || d.nLid > 0;
  c->opt_done = true;
  return SQLM_OK;
}

namespace {

inline void tmark(sqlm_ctx *c, int i, bool end) {
  if (c->timing) (void)hipEventRecord(c->ev[2 * i + (end ? 1 : 0)], c->stream);
}

// Add the elapsed times of timer pairs [i0, i1) (events already complete).
void acc_events(sqlm_ctx *c, int i0, int i1) {
  if (!c->timing) return;
  for (int i = i0; i < i1; ++i) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, c->ev[2 * i], c->ev[2 * i + 1]) == hipSuccess) c->kernel_ms_acc[i] += ms;
  }
}

// computeActiveErrors + buildSystem for the current state.
int linearize(sqlm_ctx *c) {
  DevProblem &d = c->d;
  c->lin_timers = 1;
  if (c->spec && c->lin_valid) {  // the accepted trial already linearized at this state
    tmark(c, 0, false);
    tmark(c, 0, true);
    return SQLM_OK;
  }
  c->lin_timers = 2;  // + the camera pass on the side stream
  c->err_state = 0;
  // the camera pass (H_pp, b_p, LiDAR) reads only the state, like the landmark
  // QR: fork it onto the side stream and join before anything consumes H_pp
  SQLM_HIP_OK(hipEventRecord(c->ev_fork, c->stream));
  SQLM_HIP_OK(hipStreamWaitEvent(c->side, c->ev_fork, 0));
  if (c->timing) SQLM_HIP_OK(hipEventRecord(c->ev[2], c->side));
  launch_camera_pass(d, c->side);
  if (c->timing) SQLM_HIP_OK(hipEventRecord(c->ev[3], c->side));
  SQLM_HIP_OK(hipEventRecord(c->ev_join, c->side));
  tmark(c, 0, false);  // maxdiag was zeroed by the last k_reduce (or prepare)
  for (size_t b = 0; b < c->plan.buckets.size(); ++b) launch_linearize(d, c->plan.buckets[b], c->plan.bucket_part_off[b], c->stream);
  tmark(c, 0, true);
  SQLM_HIP_OK(hipStreamWaitEvent(c->stream, c->ev_join, 0));
  if (c->comm.enabled() && c->need_maxdiag) {  // lambda_0 needs the summed pose diagonals
    launch_pose_diag(d, c->stream);
    if (comm_allreduce_dev(c->comm, d.hdiag, 6 * (int64_t)d.nP, SQLM_DT_F64, SQLM_OP_SUM, c->stream))
      return SQLM_ERR_COMM;
    launch_pose_maxdiag(d, c->stream);
  }
  return SQLM_OK;
}

struct TrialOut {
  double chi_cur, chi_new, scale, maxdiag;
  bool ok;
  bool dev_err;  // a solve kernel gave up a bounded wait (flags[1]): the result is not trusted
};

// Wait for k_reduce's mailbox entry `seq`. The stream is polled now and then:
// an error ends the wait, and so does a drained stream without the entry
// (the copy path then takes over). Returns the scalars or null.
const double *mbox_wait(sqlm_ctx *c, unsigned long long seq, int &err) {
  err = SQLM_OK;
  const unsigned long long *slot = reinterpret_cast<const unsigned long long *>(c->mbox + kMboxSeq);
  Timer t;
  for (unsigned it = 1;; ++it) {
    if (__atomic_load_n(slot, __ATOMIC_ACQUIRE) == seq) return c->mbox;
    if ((it & 1023) == 0) {
      // bounded: a stream that never drains (an error the query does not report) ends the wait
      const hipError_t q = hipStreamQuery(c->stream);
      if (q == hipSuccess) return __atomic_load_n(slot, __ATOMIC_ACQUIRE) == seq ? c->mbox : nullptr;
      if (q != hipErrorNotReady || t.ms() > 60000.0) {
        err = SQLM_ERR_HIP;
        return nullptr;
      }
    }
    __builtin_ia32_pause();
  }
}

// Add the elapsed time of speculative camera pass p (ping-pong), if one is pending.
void acc_cam_timer(sqlm_ctx *c, int p) {
  if (!c->cam_pending[p]) return;
  float ms = 0.f;
  if (hipEventSynchronize(c->ev_cam[p][1]) == hipSuccess &&
      hipEventElapsedTime(&ms, c->ev_cam[p][0], c->ev_cam[p][1]) == hipSuccess)
    c->kernel_ms_acc[1] += ms;
  c->cam_pending[p] = false;
}

// The speculative camera pass (H_pp / b_p at the trial state) on stream st,
// with its HIP-event timing in the timing run.
int spec_camera_pass(sqlm_ctx *c, hipStream_t st) {
  const int p = c->cam_par;
  if (c->timing) acc_cam_timer(c, p);  // the pass two trials back is long complete
  if (c->timing) SQLM_HIP_OK(hipEventRecord(c->ev_cam[p][0], st));
  launch_camera_pass(c->d, st, true);
  if (c->timing) { SQLM_HIP_OK(hipEventRecord(c->ev_cam[p][1], st)); c->cam_pending[p] = true; }
  c->cam_par ^= 1;
  return SQLM_OK;
}

// The speculative camera pass behind the work enqueued so far: inline on the
// context stream (small problems), else forked to the side stream and joined
// before the next trial's RCS reduce.
int spec_camera_launch(sqlm_ctx *c) {
  if (!c->cam_inline) {
    SQLM_HIP_OK(hipEventRecord(c->ev_spec_fork, c->stream));
    SQLM_HIP_OK(hipStreamWaitEvent(c->side, c->ev_spec_fork, 0));
  }
  if (int s = spec_camera_pass(c, c->cam_inline ? c->stream : c->side)) return s;
  if (!c->cam_inline) {
    SQLM_HIP_OK(hipEventRecord(c->ev_spec_join, c->side));
    c->spec_outstanding = true;
  }
  return SQLM_OK;
}

// cam_after: the speculative camera pass goes right behind k_reduce (it runs
// while the host waits for the scalars and decides)
int reduce_and_fetch(sqlm_ctx *c, TrialOut &o, bool cam_after = false) {
  DevProblem &d = c->d;
  const bool mb = c->mbox && !c->timing && !c->comm.enabled();
  const unsigned long long seq = mb ? ++c->mbox_seq : 0;
  launch_reduce(d, c->plan.n_lm_parts, c->plan.n_lm_parts, (c->n_pose + 255) / 256, (int)((d.nLid + 255) / 256), c->stream,
                mb ? c->mbox_dev : nullptr, seq);
  if (cam_after) {
    if (int e = spec_camera_launch(c)) return e;
  }
  int s = comm_allreduce_scalars(c->comm, d.scalars, c->need_maxdiag, c->stream);
  if (s) return s;
  const double *h = nullptr;
  if (mb) {
    h = mbox_wait(c, seq, s);
    if (s) return s;
  }
  if (!h) {
    SQLM_HIP_OK(hipMemcpyAsync(c->h_scalars, d.scalars, sizeof(double) * kNScalars, hipMemcpyDeviceToHost, c->stream));
    SQLM_HIP_OK(hipStreamSynchronize(c->stream));
    h = c->h_scalars;
  }
  o.chi_cur = h[kChiCur];
  o.chi_new = h[kChiNew];
  o.scale = h[kScale];
  o.maxdiag = h[kMaxDiag];
  o.ok = h[kSolveOk] > 0.5;
  o.dev_err = h[kDevErr] != 0.0;
  return SQLM_OK;
}

// host trace point i of the current trial: time since the previous point
inline void hmark(sqlm_ctx *c, int i) {
  if (!c->htrace) return;
  const auto now = std::chrono::steady_clock::now();
  if (i > 0 || c->ht_n > 0) c->ht_acc[i] += std::chrono::duration<double, std::micro>(now - c->ht_prev).count();
  c->ht_prev = now;
}

// setLambda + BlockSolver::solve + update + restoreDiagonal + computeActiveErrors,
// enqueued up to (not including) the trial scalars' reduction. cam_after: the
// speculative camera pass is still to go behind k_reduce.
int trial_launch(sqlm_ctx *c, double lambda, bool &cam_after) {
  DevProblem &d = c->d;
  hmark(c, 0);  // since the previous trial's scalars arrived: the host's decision
  c->step_valid = true;
  tmark(c, 2, false);
  launch_damp(d, lambda, c->stream);
  tmark(c, 2, true);
  tmark(c, 3, false);
  if (c->use_tiles) launch_rcs_tiles(d, lambda, c->stream, &c->tiles);
  else launch_rcs(d, lambda, c->plan.max_row_blocks, c->stream);
  tmark(c, 3, true);
  hmark(c, 1);  // damp + tile launches
  tmark(c, 8, false);
  if (c->spec_outstanding) {  // H_pp / b_p (if swapped in) and the trial state buffers it reads
    SQLM_HIP_OK(hipStreamWaitEvent(c->stream, c->ev_spec_join, 0));
    c->spec_outstanding = false;
  }
  if (c->use_tiles) {
    // cr_direct: the reduce assembles the CR superblocks itself; the RCS tile
    // kernel cleared them (no memset launches) unless there were no tiles
    if (d.cr_direct && d.n_tiles == 0) {
      const size_t blkbytes = (size_t)c->plan.cr.p * c->plan.cr.n * c->plan.cr.n * sizeof(double);
      SQLM_HIP_OK(hipMemsetAsync(d.cr_D, 0, blkbytes, c->stream));
      SQLM_HIP_OK(hipMemsetAsync(d.cr_E, 0, blkbytes, c->stream));
    }
    if (d.cr_direct && c->plan.cr.R) launch_arrow_clear(d, c->plan.cr, c->stream);
    launch_rcs_reduce(d, lambda, c->stream);
  }
  tmark(c, 8, true);
  hmark(c, 2);  // RCS reduce
  int s = 0;
  const bool sharded = c->comm.enabled(), root = !sharded || c->comm.rank == 0;
  if (sharded) {  // gather every rank's S / g rows on rank 0
    std::vector<P2POp> ops;
    if (root) {
      const GatherTab &t = c->gather;
      for (int k = 0; k < t.n; ++k) {
        ops.push_back(P2POp{k + 1, false, d.xstage + t.s_src[k], t.s_hi[k] - t.s_lo[k], SQLM_DT_F64});
        ops.push_back(P2POp{k + 1, false, d.xstage + t.g_src[k], t.g_hi[k] - t.g_lo[k], SQLM_DT_F64});
      }
    } else {
      const int me = c->comm.rank, a = c->sh_lo[me], b = c->sh_hi[me];
      const int64_t s0 = 36 * (int64_t)c->s_row_host[a], s1 = 36 * (int64_t)c->s_row_host[b];
      ops.push_back(P2POp{0, true, d.S + s0, s1 - s0, SQLM_DT_F64});
      ops.push_back(P2POp{0, true, d.g + 6 * (int64_t)a, 6 * (int64_t)(b - a), SQLM_DT_F64});
    }
    if (comm_group_p2p(c->comm, ops, c->stream)) return SQLM_ERR_COMM;
    if (root) launch_gather_add(d, c->gather, c->stream);
  }
  tmark(c, 4, false);
  // unsharded CR: the pose update reads dx off the CR solution (no gather launch)
  const bool pose_from_cr = !sharded && c->plan.cr.enabled;
  if (root) {
    s = c->plan.cr.enabled ? launch_cr_solve(d, c->plan.cr, c->stream, !pose_from_cr, &c->crs)
                      : launch_dense_solve(d, c->stream);
    if (s) return s == -2 ? SQLM_ERR_HIP : SQLM_ERR_UNSUPPORTED;
  }
  if (sharded) {  // dx and the solve flag from rank 0
    if (root) launch_flag_pack(d, false, c->stream);
    if (comm_bcast_dev(c->comm, d.dx, 6 * (int64_t)d.nP + 1, SQLM_DT_F64, 0, c->stream)) return SQLM_ERR_COMM;
    if (!root) launch_flag_pack(d, true, c->stream);
  }
  tmark(c, 4, true);
  hmark(c, 3);  // solve launches
  // the pose update folded into the first landmark-update launch (one launch
  // less per trial; SQLM_NO_POSE_FUSE=1 keeps it separate, A/B and tests)
  const bool no_fuse = c->no_pose_fuse;
  // (small problems only: the fused variant runs at lower occupancy, which the
  // latency-bound config-4 update pays for more than one launch saves)
  // (the fused variant is instantiated for the speculative schedule only)
  const bool fuse = pose_from_cr && c->spec && c->cam_inline && !no_fuse && !c->plan.buckets.empty() && !c->plan.buckets[0].wide;
  tmark(c, 5, false);
  if (!fuse) launch_pose_update(d, lambda, c->stream, pose_from_cr);
  tmark(c, 5, true);
  tmark(c, 6, false);
  // (the buckets on three streams, like the tile classes, measured slower:
  // 686 -> 647 it/s, the CR solve after them 0.54 -> 0.61 ms; profiles/r03/ab_upd_streams.log)
  // every bucket in one launch (the fused first bucket of a small problem
  // keeps its own launch: the fused form of the merged kernel measured slower)
  c->err_state = 1;  // (also when the solve failed: the update then evaluates the state with dx = 0)
  if (!fuse && c->plan.upd.nb > 0) {
    launch_landmark_update_all(d, c->plan.upd, lambda, c->stream, c->spec);
  } else {
    for (size_t b = 0; b < c->plan.buckets.size(); ++b)
      launch_landmark_update(d, c->plan.buckets[b], lambda, c->plan.bucket_part_off[b], c->stream, c->spec, fuse && b == 0);
  }
  launch_lidar_chi2(d, c->stream);
  tmark(c, 6, true);
  hmark(c, 4);  // pose + landmark updates
  // camera pass at the trial state: on the side stream, overlapped with the
  // host's decision and the next trial; small problems (cam_inline) keep it on
  // the context stream behind k_reduce instead -- the fork / join costs the
  // host more than the overlap saves there
  // (config 4 with the fork after k_reduce too, so that the host's scalars
  // come ~4 us sooner: within noise, profiles/r05/ab_stream_order_rejected.log)
  cam_after = c->spec && c->cam_inline && !c->timing;
  if (c->spec && !cam_after) return spec_camera_launch(c);
  return SQLM_OK;
}

int trial(sqlm_ctx *c, double lambda, TrialOut &o) {
  bool cam_after = false;
  int s = trial_launch(c, lambda, cam_after);
  if (s) return s;
  tmark(c, 7, false);
  hmark(c, 5);  // speculative camera pass
  s = reduce_and_fetch(c, o, cam_after);
  tmark(c, 7, true);
  hmark(c, 6);  // reduce launch + wait for the scalars
  if (c->htrace) ++c->ht_n;
  acc_events(c, 2, SQLM_NKERNEL_TIMERS);
  return s;
}

void swap_state(sqlm_ctx *c) {
  DevProblem &d = c->d;
  std::swap(d.pose_qt[0], d.pose_qt[1]);
  std::swap(d.pose_rt[0], d.pose_rt[1]);
  std::swap(d.X[0], d.X[1]);
  if (c->err_state >= 0) c->err_state ^= 1;
  c->lin_valid = c->spec;
  if (c->spec) {  // the speculative linearization at the accepted state becomes current
    std::swap(d.lm_R, d.lm_R_nx);
    std::swap(d.lm_b, d.lm_b_nx);
    std::swap(d.obs_s, d.obs_s_nx);
    std::swap(d.Hpp, d.Hpp_nx);
    std::swap(d.bp, d.bp_nx);
    std::swap(d.pc_lm, d.px_lm);
    std::swap(d.pc_lid, d.px_lid);
  }
}

// Timing of speculative camera passes not yet added (end of an LM run).
void flush_cam_timers(sqlm_ctx *c) {
  for (int p = 0; p < 2; ++p) acc_cam_timer(c, p);
}

// Host loop: every trial's scalars come back before the next trial is
// enqueued, and the host applies lm_decide. (A device-side loop -- k_reduce
// deciding, trials enqueued two ahead -- measured slower on MI355X: every
// per-trial kernel then starts with a dependent load of the control block,
// which costs more than the host turnaround it hides, config 4 703 -> 649-675
// it/s, config 2 5.58-5.61k -> 5.40k it/s, profiles/r04/ab_dlm_fuse_r4.log;
// removed in round 5.)
int lm_host(sqlm_ctx *c, LMCtl &L, const volatile uint8_t *stop) {
  while (!L.done) {
    if (L.qmax == 0 && L.its > 0) {  // the next iteration (sparse_optimizer.cpp:376-414)
      if (stopped(stop)) break;
      c->need_maxdiag = false;
      if (int s = linearize(c)) return s;
    }
    TrialOut o{};
    if (int s = trial(c, L.lambda, o)) return s;
    if (o.dev_err) return SQLM_ERR_HIP;  // a solve gave up a bounded wait (the step was rejected on the device too)
    if (L.qmax == 0) acc_events(c, 0, c->lin_timers);
    if (lm_decide(L, o.chi_cur, o.chi_new, o.scale, o.ok, stopped(stop))) swap_state(c);
    if (L.qmax == 0) c->kernel_ms_n++;  // an iteration ended
  }
  return SQLM_OK;
}

}  // namespace

// The Levenberg–Marquardt loop of g2o (levenberg.cpp:61-164 inside
// sparse_optimizer.cpp:376-414). `bench` keeps iterating after Terminate so a
// fixed number of iterations can be timed.
int run_lm(sqlm_ctx *c, int iterations, double user_lambda, const volatile uint8_t *stop, sqlm_stats *st,
           int *n_iter, bool bench) {
  sqlm_stats local;
  if (!st) st = &local;
  std::memset(st, 0, sizeof(*st));
  st->n_active_edges = c->n_active_edges;
  c->lin_valid = false;  // iteration 0 linearizes in full (lambda_0 needs max diag H)
  Timer tt;
  LMCtl L;
  std::memset(&L, 0, sizeof(LMCtl));
  L.iterations = iterations;
  L.bench = bench ? 1 : 0;
  L.done = iterations <= 0 || stopped(stop);
  if (!L.done) {
    Timer tl;
    c->need_maxdiag = true;
    int s = linearize(c);
    if (s) return s;
    TrialOut o0{};
    s = reduce_and_fetch(c, o0);
    c->need_maxdiag = false;
    if (s) return s;
    L.currentChi = L.iniChi = o0.chi_cur;  // computeActiveErrors at iteration 0 (levenberg.cpp:66-97)
    st->chi2_begin = o0.chi_cur;
    L.lambda = user_lambda > 0 ? user_lambda : 1e-5 * o0.maxdiag;  // computeLambdaInit
    L.ni = 2;
    st->ms_linearize += tl.ms();
    Timer tr;
    s = lm_host(c, L, stop);
    if (s) return s;
    st->ms_trials += tr.ms();
  }
  if (c->spec_outstanding) {  // nothing of a speculative pass outlives the run
    SQLM_HIP_OK(hipStreamWaitEvent(c->stream, c->ev_spec_join, 0));
    c->spec_outstanding = false;
  }
  flush_cam_timers(c);
  if (c->htrace && c->ht_n > 0) {
    static const char *nm[7] = {"decide", "tiles", "reduce", "solve", "updates", "campass", "wait"};
    std::fprintf(stderr, "host trace (%d trials, us/trial):", c->ht_n);
    for (int i = 0; i < 7; ++i) std::fprintf(stderr, " %s %.1f", nm[i], c->ht_acc[i] / c->ht_n);
    std::fprintf(stderr, "\n");
    std::memset(c->ht_acc, 0, sizeof(c->ht_acc));
    c->ht_n = 0;
  }
  st->iterations = L.its;
  st->trials = L.trials;
  st->result = L.result;
  st->chi2_end = L.chi2_end;
  st->lambda_end = L.lambda_end;
  st->trace_len = std::min(L.its, SQLM_TRACE_MAX);
  for (int k = 0; k < st->trace_len; ++k) {
    st->trace_chi2[k] = L.trace_chi2[k];
    st->trace_lambda[k] = L.trace_lambda[k];
    st->trace_trials[k] = L.trace_trials[k];
  }
  st->ms_total = tt.ms();
  if (n_iter) *n_iter = L.its;
  return SQLM_OK;
}

int optimize_impl(sqlm_ctx *c, int level, int iterations, double user_lambda, const volatile uint8_t *stop,
                  sqlm_stats *st, int *n_iter) {
  if (!c->has_problem) return SQLM_ERR_STATE;
  Timer ts;
  int s = prepare(c, level);
  if (s == SQLM_ERR_STATE) {  // nothing to optimize: optimize() returns -1
    if (st) std::memset(st, 0, sizeof(*st));
    if (n_iter) *n_iter = -1;
    return SQLM_OK;
  }
  if (s) return s;
  const double setup = ts.ms();
  s = run_lm(c, iterations, user_lambda, stop, st, n_iter, false);
  if (s) return s;
  s = finish(c);
  if (s) return s;
  if (st) st->ms_setup = setup;
  return SQLM_OK;
}

}  // namespace sqlm
