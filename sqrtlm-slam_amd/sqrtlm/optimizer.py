"""Host-side mirror of the reference's BA entry points, over the C ABI.

``Optimizer`` reproduces the static façade of include/backend/Optimizer.h:42-71
for the bundle-adjustment calls; each method takes the graph the reference's
``g2oOptimizer`` would have assembled (a :class:`BAProblem`) and runs the same
schedule on the MI355X through libsqrtlm.so:

* ``LocalBundleAdjustment``  -> g2oOptimizer.cc:704-1191 (3 passes, outlier tags)
* ``GlobalBundleAdjustemnt`` -> g2oOptimizer.cc:80-89 (the reference's spelling)
* ``BundleAdjustment``       -> g2oOptimizer.cc:110-362
* ``OptimizeSim3``           -> g2oOptimizer.cc:1560-1793 (batched: ``Context.sim3_optimize``)
* ``PoseOptimization``       -> g2oOptimizer.cc:385-679 (batched: ``Context.pose_optimize`` /
  ``Context.pose_refine_lidar``)

The RANSAC in front of ``OptimizeSim3`` (src/algorithm/Sim3Solver.cc) is
``sim3.Sim3Solver`` over ``Context.sim3_ransac``.

Results are written back into the problem (poses, points) like the
reference's ``SetPose`` / ``SetWorldPos`` write-back (g2oOptimizer.cc:1167-1189).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import check, lib, ptr
from .problem import HUBER_STEREO, HUBER_MONO_GBA, BAProblem


class Context:
    """One ``sqlm_ctx``: a HIP stream + device memory on one GPU. Create one per
    calling thread (the reference runs LBA, loop closing and GBA concurrently)."""

    def __init__(self, device: int = -1):
        self._h = C.c_void_p()
        check(lib().sqlm_ctx_create(int(device), C.byref(self._h)), "sqlm_ctx_create")
        self.problem: BAProblem | None = None

    def close(self) -> None:
        if self._h:
            lib().sqlm_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ------------------------------------------------------------- graph
    def set_problem(self, p: BAProblem) -> None:
        check(lib().sqlm_set_problem(
            self._h, p.n_pose, ptr(p.pose_q), ptr(p.pose_t), ptr(p.pose_fixed), ptr(p.intr), p.n_pt, ptr(p.pt),
            C.c_int64(p.n_obs), ptr(p.obs_pose), ptr(p.obs_pt), ptr(p.obs_uv), ptr(p.obs_info), ptr(p.obs_delta),
            ptr(p.obs_level)), "sqlm_set_problem")
        if p.n_lid:
            check(lib().sqlm_set_lidar(self._h, C.c_int64(p.n_lid), ptr(p.lid_pose), ptr(p.lid_pc), ptr(p.lid_pw),
                                       ptr(p.lid_n), ptr(p.lid_info)), "sqlm_set_lidar")
            if np.any(p.lid_kind):  # a problem without corner edges makes the calls it always made
                self.set_lidar_kind(p.lid_kind)
        if p.obs_ur is not None:
            check(lib().sqlm_set_stereo(self._h, ptr(p.obs_ur), ptr(p.pose_bf)), "sqlm_set_stereo")
        self.problem = p

    def set_edge_level(self, level: np.ndarray) -> None:
        level = np.ascontiguousarray(level, np.uint8)
        check(lib().sqlm_set_edge_level(self._h, ptr(level)), "sqlm_set_edge_level")

    def set_robust(self, delta: np.ndarray | None) -> None:
        d = None if delta is None else np.ascontiguousarray(delta, np.float64)
        check(lib().sqlm_set_robust(self._h, ptr(d)), "sqlm_set_robust")

    def set_lidar_level(self, level: np.ndarray) -> None:
        level = np.ascontiguousarray(level, np.uint8)
        check(lib().sqlm_set_lidar_level(self._h, ptr(level)), "sqlm_set_lidar_level")

    def set_lidar_kind(self, kind: np.ndarray | None) -> None:
        """sqlm_set_lidar_kind: 0 flat, 1 corner per LiDAR edge; None = every edge flat."""
        kind = None if kind is None else np.ascontiguousarray(kind, np.uint8)
        check(lib().sqlm_set_lidar_kind(self._h, ptr(kind)), "sqlm_set_lidar_kind")

    # ------------------------------------------------------------- solve
    def optimize(self, level: int = 0, iterations: int = 10, user_lambda: float = 0.0, stop=None):
        st = _lib.Stats()
        n = C.c_int(0)
        check(lib().sqlm_optimize(self._h, int(level), int(iterations), C.c_double(user_lambda), ptr(stop),
                                  C.byref(st), C.byref(n)), "sqlm_optimize")
        return n.value, st.as_dict()

    def local_ba(self, stop=None):
        st = (_lib.Stats * 3)()
        ran = C.c_int(0)
        outl = np.zeros(self.problem.n_obs if self.problem else 0, np.uint8)
        check(lib().sqlm_local_ba(self._h, ptr(stop), ptr(outl), st, C.byref(ran)), "sqlm_local_ba")
        return ran.value, outl, [s.as_dict() for s in st]

    def global_ba(self, iterations: int, stop=None):
        st = _lib.Stats()
        n = C.c_int(0)
        check(lib().sqlm_global_ba(self._h, int(iterations), ptr(stop), C.byref(st), C.byref(n)), "sqlm_global_ba")
        return n.value, st.as_dict()

    def rcs_layout(self) -> dict:
        """The reduced-camera-system layout of the last optimize() (sqlm_get_rcs_layout)."""
        out = (C.c_int * 8)()
        check(lib().sqlm_get_rcs_layout(self._h, out), "sqlm_get_rcs_layout")
        kind = {0: "none", 1: "band", 2: "band+border", 3: "dense"}[out[0]]
        return dict(kind=kind, B=out[1], p=out[2], n=out[3], border_cams=out[4], R=out[5], n_free=out[6],
                    coupled_superblocks=out[7])

    def exec_info(self) -> dict:
        """Device paths of the last optimize() (sqlm_get_exec_info)."""
        out = (C.c_int * 8)()
        check(lib().sqlm_get_exec_info(self._h, out), "sqlm_get_exec_info")
        solve = {0: "none", 1: "cr_levels", 3: "band+border", 4: "dense"}[out[1]]
        tile_kernel = {0: "none", 1: "rows", 2: "tile_mono", 3: "tile_stereo", 4: "tile_producer"}[out[2]]
        return dict(obs_f32=bool(out[0]), solve=solve, tile_kernel=tile_kernel, tile_kernel_id=out[2],
                    tile_classes={nt for nt in range(32) if out[3] >> nt & 1}, n_long_s=out[4], n_long_g=out[5],
                    tile_dups=out[6], tile_maxk=out[7])

    def last_step(self):
        """(g, dx) of the most recent LM trial (sqlm_get_last_step): the reduced
        camera system's right-hand side and the camera step, each (n_free, 6) in
        free-camera order, g2o's sign convention (H dx = b, b = -J^T W r).
        On a sharded context rank 0 (and the self-loop) returns the system it
        solved, g summed over the ranks; a rank >= 1 returns the broadcast dx
        and, in g, its own share as it was sent: zero outside the free cameras
        its own edges touch, not the full right-hand side inside them."""
        n = self.rcs_layout()["n_free"]
        g, dx = np.zeros((n, 6)), np.zeros((n, 6))
        check(lib().sqlm_get_last_step(self._h, ptr(g), ptr(dx)), "sqlm_get_last_step")
        return g, dx

    def bench(self, warmup: int, n: int, timers: bool = True):
        """(ms per LM iteration, per-phase ms from HIP events or {} without
        timers, stats). timers=False runs without the phase events."""
        ms = C.c_double(0)
        kms = np.zeros(_lib.NKERNEL_TIMERS)
        st = _lib.Stats()
        check(lib().sqlm_bench_iterations(self._h, int(warmup), int(n), C.byref(ms), ptr(kms) if timers else None,
                                          C.byref(st)), "sqlm_bench_iterations")
        if not timers:
            return ms.value, {}, st.as_dict()
        names = [lib().sqlm_kernel_timer_name(i).decode() for i in range(_lib.NKERNEL_TIMERS)]
        return ms.value, dict(zip(names, kms.tolist())), st.as_dict()

    def set_comm(self, unique_id: bytes, rank: int, nranks: int) -> None:
        buf = C.create_string_buffer(unique_id, len(unique_id))
        check(lib().sqlm_ctx_set_comm(self._h, buf, int(rank), int(nranks)), "sqlm_ctx_set_comm")

    def comm_info(self) -> dict:
        """The transport the exchange runs on and the rank / rank count as
        the communicator reports them (RCCL: ncclCommUserRank / ncclCommCount)."""
        tr, r, n = C.c_int(), C.c_int(), C.c_int()
        check(lib().sqlm_ctx_comm_info(self._h, C.byref(tr), C.byref(r), C.byref(n)), "sqlm_ctx_comm_info")
        names = {0: "none", 1: "rccl", 2: "rccl-selfloop", 3: "host"}
        return {"transport": names.get(tr.value, str(tr.value)), "rank": r.value, "nranks": n.value}

    def set_comm_selfloop(self, unique_id: bytes) -> None:
        """A one-rank RCCL communicator: the sharded code path with every
        exchange through real RCCL on one GPU (sqlm_ctx_set_comm_selfloop)."""
        buf = C.create_string_buffer(unique_id, len(unique_id))
        check(lib().sqlm_ctx_set_comm_selfloop(self._h, buf), "sqlm_ctx_set_comm_selfloop")

    def set_host_comm(self, rank: int, nranks: int, allreduce, p2p) -> None:
        """Shard over host collectives: ``allreduce(arr, op)`` must reduce the
        numpy array ``arr`` in place across ranks (op "sum" or "max");
        ``p2p(arr, peer, op)`` sends ``arr`` to / receives it from ``peer``
        (op "send" / "recv") or broadcasts it in place from root ``peer``
        (op "bcast"), e.g. with torch.distributed gloo. Runs several ranks on
        one GPU (tests)."""
        ops = {0: "send", 1: "recv", 2: "bcast"}

        def _p2p(_user, buf, count, dtype, peer, op):
            try:
                dt = _lib.DTYPES[dtype]
                arr = np.ctypeslib.as_array((C.c_char * (int(count) * np.dtype(dt).itemsize)).from_address(buf))
                p2p(arr.view(dt), int(peer), ops[int(op)])
                return 0
            except Exception:  # noqa: BLE001 — never unwind through the C ABI
                import traceback
                traceback.print_exc()
                return -1
        self._host_p2p = _lib.P2P_FN(_p2p)
        check(lib().sqlm_ctx_set_host_p2p(self._h, self._host_p2p, None), "sqlm_ctx_set_host_p2p")

        def _cb(_user, buf, count, dtype, op):
            try:
                dt = _lib.DTYPES[dtype]
                arr = np.ctypeslib.as_array((C.c_char * (int(count) * np.dtype(dt).itemsize)).from_address(buf))
                allreduce(arr.view(dt), "max" if op == 1 else "sum")
                return 0
            except Exception:  # noqa: BLE001 — never unwind through the C ABI
                import traceback
                traceback.print_exc()
                return -1
        self._host_cb = _lib.ALLREDUCE_FN(_cb)  # keep alive while the context lives
        check(lib().sqlm_ctx_set_host_comm(self._h, int(rank), int(nranks), self._host_cb, None),
              "sqlm_ctx_set_host_comm")

    # ------------------------------------------------------------- results
    def poses(self):
        n = self.problem.n_pose
        q, t = np.zeros((n, 4)), np.zeros((n, 3))
        check(lib().sqlm_get_poses(self._h, ptr(q), ptr(t)), "sqlm_get_poses")
        return q, t

    def points(self):
        X = np.zeros((self.problem.n_pt, 3))
        check(lib().sqlm_get_points(self._h, ptr(X)), "sqlm_get_points")
        return X

    def edge_chi2(self):
        out = np.zeros(self.problem.n_obs)
        check(lib().sqlm_get_edge_chi2(self._h, ptr(out)), "sqlm_get_edge_chi2")
        return out

    def lidar_error(self, n_lid: int | None = None):
        """(n_lid,) the last computed error of every LiDAR edge in the caller's
        edge order (sqlm_get_lidar_error); ``n_lid`` defaults to the problem's
        (pass the pair count after ``set_lidar_from_clouds``)."""
        n = self.problem.n_lid if n_lid is None else int(n_lid)
        out = np.zeros(max(n, 1))
        check(lib().sqlm_get_lidar_error(self._h, ptr(out)), "sqlm_get_lidar_error")
        return out[:n]

    def depth_positive(self):
        out = np.zeros(self.problem.n_obs, np.uint8)
        check(lib().sqlm_get_edge_depth_positive(self._h, ptr(out)), "sqlm_get_edge_depth_positive")
        return out

    def edge_level(self):
        out = np.zeros(self.problem.n_obs, np.uint8)
        check(lib().sqlm_get_edge_level(self._h, ptr(out)), "sqlm_get_edge_level")
        return out

    # ------------------------------------------------------------- essential graph
    def eg_set_problem(self, pg) -> None:
        """A synth.PoseGraph (Sim3 vertices, EdgeSim3 edges) -> sqlm_eg_set_problem."""
        info = None if pg.info is None else np.ascontiguousarray(pg.info.reshape(-1, 49), np.float64)
        check(lib().sqlm_eg_set_problem(self._h, pg.n_kf, ptr(pg.Siw), ptr(pg.fixed), int(pg.fix_scale),
                                        C.c_int64(pg.n_edge), ptr(pg.ei), ptr(pg.ej), ptr(pg.Sji), ptr(info)),
              "sqlm_eg_set_problem")
        self.pose_graph = pg

    def eg_optimize(self, iterations: int = 20, user_lambda: float = 1e-16, stop=None):
        st = _lib.Stats()
        n = C.c_int(0)
        check(lib().sqlm_eg_optimize(self._h, int(iterations), C.c_double(user_lambda), ptr(stop), C.byref(st),
                                     C.byref(n)), "sqlm_eg_optimize")
        return n.value, st.as_dict()

    def eg_poses(self):
        S = np.zeros((self.pose_graph.n_kf, 8))
        check(lib().sqlm_eg_get_poses(self._h, ptr(S)), "sqlm_eg_get_poses")
        return S

    def eg_edge_chi2(self):
        out = np.zeros(self.pose_graph.n_edge)
        check(lib().sqlm_eg_get_edge_chi2(self._h, ptr(out)), "sqlm_eg_get_edge_chi2")
        return out

    def eg_jacobians(self):
        """(n_edge, 2, 7, 7): d e / d S_i and d e / d S_j at the current estimates
        (sqlm_eg_get_jacobians, the optimizer's numeric Jacobians)."""
        out = np.zeros((self.pose_graph.n_edge, 2, 7, 7))
        check(lib().sqlm_eg_get_jacobians(self._h, ptr(out)), "sqlm_eg_get_jacobians")
        return out

    def eg_exec_info(self) -> dict:
        """What the last eg_optimize() ran (sqlm_eg_get_exec_info)."""
        out = (C.c_int * 8)()
        check(lib().sqlm_eg_get_exec_info(self._h, out), "sqlm_eg_get_exec_info")
        solve = {1: "cr", 2: "arrow_cholesky", 3: "dense"}[out[0]]
        return dict(solve=solve, n_free=out[1], p=out[2], border=out[3], nc=out[4], R=out[5], n_last=out[6],
                    info=bool(out[7]))

    def eg_last_step(self):
        """(b, dx) of the most recent LM trial of the last eg_optimize()
        (sqlm_eg_get_last_step): right-hand side and solution of
        (H + lambda I) dx = b, each (n_free, 7) in free-vertex (id) order."""
        n = self.eg_exec_info()["n_free"]
        b, dx = np.zeros((n, 7)), np.zeros((n, 7))
        check(lib().sqlm_eg_get_last_step(self._h, ptr(b), ptr(dx)), "sqlm_eg_get_last_step")
        return b, dx

    # ------------------------------------------------------------- Sim3 alignment
    def sim3_optimize(self, problems, iters=None, user_lambda: float = 0.0):
        """sqlm_sim3_optimize on a list of sim3.Sim3Problem, all in one launch.
        Returns (S12_out (P,8), n_inliers (P,), pair_state (n_pair,) in batch
        order, [stats dict per problem]); ``self.sim3_pair_off`` keeps the
        batch's CSR offsets for the introspection calls."""
        from . import sim3 as _s3
        a = _s3.pack(problems)
        P, n = len(problems), int(a["pair_off"][-1])
        S_out, n_in = np.zeros((P, 8)), np.zeros(P, np.int32)
        state = np.zeros(n, np.uint8)
        st = (_lib.Sim3Stats * max(P, 1))()
        it = None if iters is None else np.ascontiguousarray(iters, np.int32).reshape(3)
        check(lib().sqlm_sim3_optimize(
            self._h, P, ptr(a["S12"]), ptr(a["intr1"]), ptr(a["intr2"]), ptr(a["fix_scale"]), ptr(a["th2"]),
            ptr(a["pair_off"]), ptr(a["X1c"]), ptr(a["X2c"]), ptr(a["obs1"]), ptr(a["obs2"]), ptr(a["info1"]),
            ptr(a["info2"]), ptr(it), C.c_double(user_lambda), ptr(S_out), ptr(n_in), ptr(state), st),
            "sqlm_sim3_optimize")
        self.sim3_pair_off = a["pair_off"]
        return S_out, n_in, state, [st[k].as_dict() for k in range(P)]

    def sim3_pair_chi2(self):
        """(n_pair, 2 checks, 2 edges): the chi2 values the two threshold tests read."""
        out = np.zeros((int(self.sim3_pair_off[-1]), 2, 2))
        check(lib().sqlm_sim3_get_pair_chi2(self._h, ptr(out)), "sqlm_sim3_get_pair_chi2")
        return out

    def sim3_linearization(self):
        """e (n_pair, 2 edges, 2), J (n_pair, 2 edges, 2, 7) at the input S12 of the last call."""
        n = int(self.sim3_pair_off[-1])
        e, J = np.zeros((n, 2, 2)), np.zeros((n, 2, 2, 7))
        check(lib().sqlm_sim3_get_linearization(self._h, ptr(e), ptr(J)), "sqlm_sim3_get_linearization")
        return e, J

    def sim3_last_step(self, prob: int = 0):
        """H (7,7), b (7,), dx (7,) of problem ``prob``'s last LM trial: (H + lambda I) dx = b."""
        H, b, dx = np.zeros((7, 7)), np.zeros(7), np.zeros(7)
        check(lib().sqlm_sim3_get_last_step(self._h, int(prob), ptr(H), ptr(b), ptr(dx)), "sqlm_sim3_get_last_step")
        return H, b, dx

    # ------------------------------------------------------------- Sim3 RANSAC
    def sim3_ransac(self, problems, draws, max_err, min_inliers=6):
        """sqlm_sim3_ransac on a list of sim3.Sim3Problem: every hypothesis of
        every problem in one launch. ``draws``: one (n_hyp, 3) array of raw
        RandomInt values per problem; ``max_err``: one (max_err1, max_err2)
        per problem, as stored (truncated); ``min_inliers``: an int or one per
        problem. Returns one dict per problem: n_inliers (H,), flags (H,),
        R12 (H,3,3), t12 (H,3), s12 (H,) float32, first_return, best."""
        from . import sim3 as _s3
        a = _s3.pack_ransac(problems, max_err, draws, min_inliers)
        P, H = len(problems), int(a["hyp_off"][-1])
        n_in, flags = np.zeros(H, np.int32), np.zeros(H, np.uint8)
        R, t, s = np.zeros((H, 3, 3), np.float32), np.zeros((H, 3), np.float32), np.zeros(H, np.float32)
        first, best = np.zeros(P, np.int32), np.zeros(P, np.int32)
        check(lib().sqlm_sim3_ransac(
            self._h, P, ptr(a["intr1"]), ptr(a["intr2"]), ptr(a["fix_scale"]), ptr(a["min_inliers"]),
            ptr(a["pair_off"]), ptr(a["X1c"]), ptr(a["X2c"]), ptr(a["max_err1"]), ptr(a["max_err2"]),
            ptr(a["hyp_off"]), ptr(a["draws"]), ptr(n_in), ptr(flags), ptr(R), ptr(t), ptr(s), ptr(first), ptr(best)),
            "sqlm_sim3_ransac")
        self.sim3_ransac_pairs = np.diff(a["pair_off"])
        o = a["hyp_off"]
        return [dict(n_inliers=n_in[o[k]:o[k + 1]], flags=flags[o[k]:o[k + 1]], R12=R[o[k]:o[k + 1]],
                     t12=t[o[k]:o[k + 1]], s12=s[o[k]:o[k + 1]], first_return=int(first[k]), best=int(best[k]))
                for k in range(P)]

    def sim3_ransac_inliers(self, prob: int, hyp: int):
        """mvbInliersi (N,) uint8 of hypothesis ``hyp`` of problem ``prob`` of the last sim3_ransac."""
        mask = np.zeros(max(int(self.sim3_ransac_pairs[prob]), 1), np.uint8)
        check(lib().sqlm_sim3_ransac_get_inliers(self._h, int(prob), int(hyp), ptr(mask)),
              "sqlm_sim3_ransac_get_inliers")
        return mask[:int(self.sim3_ransac_pairs[prob])]

    def sim3_ransac_hypothesis(self, prob: int, hyp: int):
        """(idx (3,), T12 (4,4), T21 (4,4) float32): the pairs hypothesis ``hyp`` drew and the transforms CheckInliers used."""
        idx, T12, T21 = np.zeros(3, np.int32), np.zeros((4, 4), np.float32), np.zeros((4, 4), np.float32)
        check(lib().sqlm_sim3_ransac_get_hypothesis(self._h, int(prob), int(hyp), ptr(idx), ptr(T12), ptr(T21)),
              "sqlm_sim3_ransac_get_hypothesis")
        return idx, T12, T21

    # ------------------------------------------------------------- PnP RANSAC
    def pnp_ransac(self, problems, draws, min_inliers, max_err=None):
        """sqlm_pnp_ransac on a list of pnp.PnPProblem: every hypothesis of
        every problem in one launch, the refines of the record-breaking ones in
        a second. ``draws``: one (n_hyp, 4) array of raw RandomInt values per
        problem; ``min_inliers``: mRansacMinInliers, an int or one per problem;
        ``max_err``: one (N,) float32 array per problem (default: the
        problem's sigma2 * 5.991). Returns one dict per problem: n_inliers
        (H,), flags (H,), R (H,3,3), t (H,3) float64, first_return, best, Tcw
        (4,4) float32, n_refined."""
        from . import pnp as _pnp
        a = _pnp.pack(problems, draws, min_inliers, max_err)
        P, H = len(problems), int(a["hyp_off"][-1])
        n_in, flags = np.zeros(H, np.int32), np.zeros(H, np.uint8)
        R, t = np.zeros((H, 3, 3)), np.zeros((H, 3))
        first, best, n_ref = np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros(P, np.int32)
        Tcw = np.zeros((P, 4, 4), np.float32)
        check(lib().sqlm_pnp_ransac(
            self._h, P, ptr(a["intr"]), ptr(a["min_inliers"]), ptr(a["pair_off"]), ptr(a["Xw"]), ptr(a["uv"]),
            ptr(a["max_err"]), ptr(a["hyp_off"]), ptr(a["draws"]), ptr(n_in), ptr(flags), ptr(R), ptr(t), ptr(first),
            ptr(best), ptr(Tcw), ptr(n_ref)), "sqlm_pnp_ransac")
        self.pnp_ransac_pairs = np.diff(a["pair_off"])
        o = a["hyp_off"]
        return [dict(n_inliers=n_in[o[k]:o[k + 1]], flags=flags[o[k]:o[k + 1]], R=R[o[k]:o[k + 1]],
                     t=t[o[k]:o[k + 1]], first_return=int(first[k]), best=int(best[k]), Tcw=Tcw[k],
                     n_refined=int(n_ref[k])) for k in range(P)]

    def pnp_ransac_inliers(self, prob: int, hyp: int):
        """mvbInliersi (N,) uint8 of hypothesis ``hyp`` of problem ``prob`` of the last pnp_ransac."""
        n = int(self.pnp_ransac_pairs[prob])
        mask = np.zeros(max(n, 1), np.uint8)
        check(lib().sqlm_pnp_ransac_get_inliers(self._h, int(prob), int(hyp), ptr(mask)), "sqlm_pnp_ransac_get_inliers")
        return mask[:n]

    @staticmethod
    def _pnp_diag():
        return dict(ut=np.zeros((12, 12)), eig=np.zeros(12), betas=np.zeros((3, 4)), rep_err=np.zeros(3),
                    chosen=np.zeros(1, np.int32))

    def pnp_ransac_refined(self, prob: int, hyp: int):
        """Refine() of the mask of the record-breaking hypothesis ``hyp``: a dict of R (3,3), t (3,), mask (N,)
        uint8, n_inliers and the diagnostics of pnp_ransac_hypothesis. SqlmError (STATE) if ``hyp`` is no record."""
        n = int(self.pnp_ransac_pairs[prob])
        d = self._pnp_diag()
        R, t, mask, cnt = np.zeros((3, 3)), np.zeros(3), np.zeros(max(n, 1), np.uint8), np.zeros(1, np.int32)
        check(lib().sqlm_pnp_ransac_get_refined(self._h, int(prob), int(hyp), ptr(R), ptr(t), ptr(mask), ptr(cnt),
                                                ptr(d["ut"]), ptr(d["eig"]), ptr(d["betas"]), ptr(d["rep_err"]),
                                                ptr(d["chosen"])), "sqlm_pnp_ransac_get_refined")
        d.update(R=R, t=t, mask=mask[:n], n_inliers=int(cnt[0]), chosen=int(d["chosen"][0]))
        return d

    def pnp_ransac_hypothesis(self, prob: int, hyp: int):
        """Diagnostics of hypothesis ``hyp``: a dict of idx (4,), ut (12,12) rows by descending eigenvalue, eig
        (12,), betas (3,4) after Gauss-Newton, rep_err (3,), chosen."""
        d = self._pnp_diag()
        idx = np.zeros(4, np.int32)
        check(lib().sqlm_pnp_ransac_get_hypothesis(self._h, int(prob), int(hyp), ptr(idx), ptr(d["ut"]), ptr(d["eig"]),
                                                   ptr(d["betas"]), ptr(d["rep_err"]), ptr(d["chosen"])),
              "sqlm_pnp_ransac_get_hypothesis")
        d.update(idx=idx, chosen=int(d["chosen"][0]))
        return d

    # ------------------------------------------------------------- LocalMapping's map points
    def triangulate_pairs(self, pairs):
        """sqlm_triangulate_pairs on a list of mappoint.TriPair: the match loop
        of CreateNewMapPoints for every pair in one launch. Returns a dict of
        x3d (n,3) float32, reason (n,) uint8, n_new (n_pair,) and the CSR
        offsets ``off`` over the concatenated matches."""
        from . import mappoint as _mp
        return _mp.triangulate_pairs(self, pairs)

    def map_points_update(self, batch):
        """sqlm_map_points_update on a mappoint.MapPointBatch:
        ComputeDistinctiveDescriptors and UpdateNormalAndDepth of every point.
        Returns a dict of best_idx, best_median, normal, max_dist, min_dist
        (the keys of a half that is switched off are absent)."""
        from . import mappoint as _mp
        return _mp.map_points_update(self, batch)

    def map_points_update_info(self):
        """dict(lds_max, n_lds, n_global, n_launch) of the last map_points_update."""
        from . import mappoint as _mp
        return _mp.map_points_update_info(self)

    # ------------------------------------------------------------- motion-only BA
    def _pose_out(self, a, P):
        n = int(a["obs_off"][-1])
        return (np.zeros((P, 4)), np.zeros((P, 3)), np.zeros(P, np.int32), np.zeros(n, np.uint8),
                (_lib.PoseStats * max(P, 1))())

    def pose_optimize(self, problems, iters=None, user_lambda: float = 0.0, th2: float | None = None):
        """sqlm_pose_optimize on a list of pose.PoseProblem, all in one launch
        (``th2``: the problems' own, which must agree). Returns (pose_q (P,4),
        pose_t (P,3), n_inliers (P,), outlier (n_obs,) in batch order, [stats
        dict per problem]); ``self.pose_obs_off`` / ``self.pose_lid_off`` keep
        the batch's CSR offsets for the introspection calls."""
        from . import pose as _p
        a = _p.pack(problems)
        P = len(problems)
        th2 = self._pose_th2(problems, th2)
        q, t, n_in, flag, st = self._pose_out(a, P)
        it = None if iters is None else np.ascontiguousarray(iters, np.int32).reshape(4)
        check(lib().sqlm_pose_optimize(
            self._h, P, ptr(a["pose_q"]), ptr(a["pose_t"]), ptr(a["intr"]), ptr(a["obs_off"]), ptr(a["Xw"]),
            ptr(a["uv"]), ptr(a["info"]), ptr(it), C.c_double(th2), C.c_double(user_lambda), ptr(q), ptr(t),
            ptr(n_in), ptr(flag), st), "sqlm_pose_optimize")
        self.pose_obs_off, self.pose_lid_off = a["obs_off"], np.zeros(P + 1, np.int64)
        return q, t, n_in, flag, [st[k].as_dict() for k in range(P)]

    @staticmethod
    def _pose_th2(problems, th2):
        if th2 is not None:
            return float(th2)
        ths = {float(p.th2) for p in problems}
        if len(ths) > 1:
            raise ValueError("the problems of one call share th2")
        return ths.pop() if ths else 5.991

    def pose_refine_lidar(self, problems, lidar, outlier_in, robust_on=None, iters: int | None = None,
                          user_lambda: float = 0.0, th2: float | None = None):
        """sqlm_pose_refine_lidar: the LiDAR stage and the final classification
        on a list of pose.PoseProblem (their poses are the stage's start: pass
        them after the float round trip) with one pose.LidarPairs each.
        ``outlier_in`` (n_obs,) in batch order are the level-1 edges;
        ``robust_on`` defaults to "fewer than 10 edges". Returns as
        ``pose_optimize``."""
        from . import pose as _p
        a, l = _p.pack(problems), _p.pack_lidar(lidar)
        P = len(problems)
        if len(lidar) != P:
            raise ValueError("one LidarPairs per problem")
        th2 = self._pose_th2(problems, th2)
        oin = np.ascontiguousarray(outlier_in, np.uint8).reshape(int(a["obs_off"][-1]))
        rob = (np.array([p.n_obs < 10 for p in problems], np.uint8) if robust_on is None
               else np.ascontiguousarray(robust_on, np.uint8).reshape(P))
        q, t, n_in, flag, st = self._pose_out(a, P)
        it = None if iters is None else np.array([iters], np.int32)
        check(lib().sqlm_pose_refine_lidar(
            self._h, P, ptr(a["pose_q"]), ptr(a["pose_t"]), ptr(a["intr"]), ptr(a["obs_off"]), ptr(a["Xw"]),
            ptr(a["uv"]), ptr(a["info"]), ptr(oin), ptr(rob), ptr(l["lid_off"]), ptr(l["lid_kind"]), ptr(l["lid_pc"]),
            ptr(l["lid_pw"]), ptr(l["lid_n"]), ptr(l["lid_info"]), ptr(it), C.c_double(th2), C.c_double(user_lambda),
            ptr(q), ptr(t), ptr(n_in), ptr(flag), st), "sqlm_pose_refine_lidar")
        self.pose_obs_off, self.pose_lid_off = a["obs_off"], l["lid_off"]
        return q, t, n_in, flag, [st[k].as_dict() for k in range(P)]

    def pose_edge_chi2(self):
        """(n_obs, 5): the chi2 each check (after rounds 0-3, final) read."""
        out = np.zeros((int(self.pose_obs_off[-1]), _lib.POSE_CHECKS))
        check(lib().sqlm_pose_get_edge_chi2(self._h, ptr(out)), "sqlm_pose_get_edge_chi2")
        return out

    def pose_linearization(self):
        """e (n_obs,2), J (n_obs,2,6), lid_e (n_lid,), lid_J (n_lid,6) at the input pose of the last call."""
        n, m = int(self.pose_obs_off[-1]), int(self.pose_lid_off[-1])
        e, J, le, lJ = np.zeros((n, 2)), np.zeros((n, 2, 6)), np.zeros(m), np.zeros((m, 6))
        check(lib().sqlm_pose_get_linearization(self._h, ptr(e), ptr(J), ptr(le), ptr(lJ)),
              "sqlm_pose_get_linearization")
        return e, J, le, lJ

    def pose_last_step(self, prob: int = 0):
        """H (6,6), b (6,), dx (6,) of problem ``prob``'s last LM trial: (H + lambda I) dx = b."""
        H, b, dx = np.zeros((6, 6)), np.zeros(6), np.zeros(6)
        check(lib().sqlm_pose_get_last_step(self._h, int(prob), ptr(H), ptr(b), ptr(dx)), "sqlm_pose_get_last_step")
        return H, b, dx


    # ------------------------------------------------------------- LiDAR association
    @staticmethod
    def _lidar_in(map_clouds, map_Twc, query_xyz, query_Twc):
        from . import lidar as _l
        off, mxyz = _l.pack_clouds(map_clouds)
        K = off.size - 1
        mT = None if map_Twc is None else np.ascontiguousarray(map_Twc, np.float32).reshape(K, 16)
        qxyz = np.ascontiguousarray(query_xyz, np.float32).reshape(-1, 3)
        qT = np.ascontiguousarray(query_Twc, np.float32).reshape(16)
        return K, off, mxyz, mT, qxyz, qT

    def lidar_associate(self, map_clouds, map_Twc, query_xyz, query_Twc, dist_sq_threshold: float):
        """sqlm_lidar_associate: ``map_clouds`` a list of (n_k, 3) float32 clouds,
        each in its own sensor frame with its float T_wc ``map_Twc[k]`` (None:
        the clouds are in the world already); the queries likewise. Returns
        (nn_index (n,), nn_sq_dist (n,), nn_xyz (n, 3), accepted (n,));
        ``self.lidar_n_pairs`` keeps the number of accepted queries."""
        K, off, mxyz, mT, qxyz, qT = self._lidar_in(map_clouds, map_Twc, query_xyz, query_Twc)
        n = qxyz.shape[0]
        idx, d2 = np.zeros(n, np.int32), np.zeros(n, np.float32)
        xyz, acc = np.zeros((n, 3), np.float32), np.zeros(n, np.uint8)
        npairs = C.c_int64(0)
        check(lib().sqlm_lidar_associate(self._h, K, ptr(off), ptr(mxyz), ptr(mT), n, ptr(qxyz), ptr(qT),
                                         float(dist_sq_threshold), ptr(idx), ptr(d2), ptr(xyz), ptr(acc),
                                         C.addressof(npairs)), "sqlm_lidar_associate")
        self.lidar_n_pairs = npairs.value
        return idx, d2, xyz, acc

    def set_lidar_from_clouds(self, pose_index: int, map_clouds, map_Twc, query_xyz, query_Twc, query_normal,
                              info: float, dist_sq_threshold: float) -> int:
        """sqlm_set_lidar_from_clouds: the search of ``lidar_associate``, then the
        accepted pairs become the EdgeLidarFlatPoint edges of pose
        ``pose_index``; returns their number."""
        K, off, mxyz, mT, qxyz, qT = self._lidar_in(map_clouds, map_Twc, query_xyz, query_Twc)
        nrm = np.ascontiguousarray(query_normal, np.float32).reshape(qxyz.shape)
        npairs = C.c_int64(0)
        check(lib().sqlm_set_lidar_from_clouds(self._h, int(pose_index), K, ptr(off), ptr(mxyz), ptr(mT),
                                               qxyz.shape[0], ptr(qxyz), ptr(qT), ptr(nrm), float(info),
                                               float(dist_sq_threshold), C.addressof(npairs)),
              "sqlm_set_lidar_from_clouds")
        self.lidar_n_pairs = npairs.value
        return npairs.value

    def set_lidar_from_cloud_sets(self, pose_index: int, sets) -> list:
        """sqlm_set_lidar_from_cloud_sets: ``sets`` a list of dicts with the keys
        kind, map_clouds, map_Twc, query_xyz, query_Twc, query_normal (None
        allowed for a corner set), info, dist_sq_threshold. The edges of pose
        ``pose_index`` become the accepted pairs set by set, each in query
        order; returns the pair count of every set."""
        arr = (_lib.LidarSet * max(len(sets), 1))()
        keep = []  # the arrays the struct points into
        for s, d in zip(arr, sets):
            K, off, mxyz, mT, qxyz, qT = self._lidar_in(d["map_clouds"], d["map_Twc"], d["query_xyz"], d["query_Twc"])
            nrm = d.get("query_normal")
            nrm = None if nrm is None else np.ascontiguousarray(nrm, np.float32).reshape(qxyz.shape)
            keep.append((off, mxyz, mT, qxyz, qT, nrm))
            s.kind, s.n_map_clouds, s.n_query = int(d["kind"]), K, qxyz.shape[0]
            s.map_off, s.map_xyz, s.map_Twc = (a if a is None else a.ctypes.data for a in (off, mxyz, mT))
            s.query_xyz, s.query_Twc = qxyz.ctypes.data, qT.ctypes.data
            s.query_normal = None if nrm is None else nrm.ctypes.data
            s.info, s.dist_sq_threshold = float(d["info"]), float(d["dist_sq_threshold"])
        npairs = np.zeros(max(len(sets), 1), np.int64)
        check(lib().sqlm_set_lidar_from_cloud_sets(self._h, int(pose_index), len(sets), C.addressof(arr), ptr(npairs)),
              "sqlm_set_lidar_from_cloud_sets")
        out = [int(n) for n in npairs[:len(sets)]]
        self.lidar_n_pairs = sum(out)
        return out

    def lidar_exec_info(self) -> dict:
        """What the last association ran (sqlm_lidar_get_exec_info)."""
        out = (C.c_int * 8)()
        check(lib().sqlm_lidar_get_exec_info(self._h, out), "sqlm_lidar_get_exec_info")
        return dict(n_map=out[0], n_query=out[1], segments=out[2], map_tile=out[3], n_pairs=out[4],
                    query_tile=out[5])


def comm_unique_id() -> bytes:
    n = lib().sqlm_comm_id_size()
    buf = C.create_string_buffer(n)
    check(lib().sqlm_comm_get_unique_id(buf), "sqlm_comm_get_unique_id")
    return buf.raw


def comm_selftest(device: int = 0, count: int = 1 << 16) -> float:
    """sqlm_comm_selftest: the RCCL exchange primitives on a one-rank
    communicator; returns the largest deviation from the expected buffers."""
    err = C.c_double(-1.0)
    buf = C.create_string_buffer(comm_unique_id(), lib().sqlm_comm_id_size())
    check(lib().sqlm_comm_selftest(int(device), buf, C.c_int64(count), C.byref(err)), "sqlm_comm_selftest")
    return err.value


def pose_from_Tcw_f32(T):
    """Converter::toSE3Quat (src/utils/Converter.cc:55-68)."""
    q, t = np.zeros(4), np.zeros(3)
    lib().sqlm_pose_from_Tcw_f32(ptr(np.ascontiguousarray(T, np.float32).reshape(16)), ptr(q), ptr(t))
    return q, t


def pose_to_Tcw_f32(q, t):
    """Converter::toCvMat(SE3Quat) (src/utils/Converter.cc:73-79,98-109)."""
    T = np.zeros(16, np.float32)
    lib().sqlm_pose_to_Tcw_f32(ptr(np.ascontiguousarray(q, np.float64)), ptr(np.ascontiguousarray(t, np.float64)),
                               ptr(T))
    return T.reshape(4, 4)


@dataclass
class LBAResult:
    ran: bool
    outlier: np.ndarray
    stats: list


class Optimizer:
    """Static façade mirroring include/backend/Optimizer.h:42-71 (BA calls)."""

    _ctx: Context | None = None

    @classmethod
    def _context(cls, ctx):
        if ctx is not None:
            return ctx
        if cls._ctx is None:
            cls._ctx = Context()
        return cls._ctx

    @staticmethod
    def _write_back(ctx: Context, prob: BAProblem) -> None:
        q, t = ctx.poses()
        prob.pose_q[:] = q
        prob.pose_t[:] = t
        prob.pt[:] = ctx.points()

    @classmethod
    def LocalBundleAdjustment(cls, prob: BAProblem, stop_flag=None, ctx: Context | None = None,
                              lidar=None) -> LBAResult:
        """Local BA on an assembled local window (g2oOptimizer.cc:704-1191).
        ``prob.obs_delta`` carries the pass-1 Huber deltas ((float)sqrt(5.991));
        LiDAR flat edges in ``prob`` join in pass 3. Outlier tags returned are
        the edges the reference erases (chi2 > 5.991 or depth <= 0).
        With ``lidar`` (a lidar.LidarClouds) the pass-3 edges come from the
        association at the pass-2 poses instead (:978-1073), on the device."""
        c = cls._context(ctx)
        c.set_problem(prob)
        if lidar is not None:
            return cls._local_ba_lidar(c, prob, stop_flag, lidar)
        ran, outl, st = c.local_ba(stop_flag)
        if ran:
            cls._write_back(c, prob)
        return LBAResult(bool(ran), outl, st)

    @staticmethod
    def _tagged(c: Context, prob: BAProblem) -> np.ndarray:
        """chi2 > 5.991 (7.815 for a stereo edge) or depth <= 0 (:955-970, :1127-1140)."""
        th = np.full(prob.n_obs, 5.991)
        if prob.obs_ur is not None:
            th[prob.obs_ur >= 0] = 7.815
        return (c.edge_chi2() > th) | (c.depth_positive() == 0)

    @classmethod
    def _local_ba_lidar(cls, c: Context, prob: BAProblem, stop, clouds) -> LBAResult:
        """The schedule of sqlm_local_ba driven pass by pass, as an adapter does
        (INTEGRATION.md section 4), with the association between passes 2 and 3."""
        from . import lidar as _l

        def stopped():
            return stop is not None and bool(np.asarray(stop).reshape(-1)[0])
        zero = _lib.Stats().as_dict()
        if stopped():  # :923-928
            return LBAResult(False, np.zeros(prob.n_obs, np.uint8), [zero, zero, zero])
        if prob.n_lid:  # edges the problem brought are replaced by the association
            check(lib().sqlm_set_lidar(c._h, C.c_int64(0), None, None, None, None, None), "sqlm_set_lidar")
        st = [zero, zero, zero]
        _, st[0] = c.optimize(0, 5, 0.0, stop)
        if not stopped():  # :939-975
            level = c.edge_level()
            level[cls._tagged(c, prob)] = 1
            c.set_edge_level(level)
            c.set_robust(None)
            _, st[1] = c.optimize(0, 10, 0.0, stop)
        q, t = c.poses()  # :978-1073 at the pass-2 estimates
        Twc = [_l.Twc_f32(q[p], t[p]) for p in clouds.pose_index]
        oth = clouds.others
        if clouds.corner_xyz is not None:  # flat then corner edges (:1034-1107), one call
            c.set_lidar_from_cloud_sets(int(clouds.pose_index[clouds.current]), clouds.cloud_sets(Twc))
        else:
            c.set_lidar_from_clouds(int(clouds.pose_index[clouds.current]), [clouds.xyz[k] for k in oth],
                                    np.stack([Twc[k] for k in oth]) if oth else np.zeros((0, 16), np.float32),
                                    clouds.query_xyz, Twc[clouds.current], clouds.query_normal, clouds.weight,
                                    clouds.dist_sq_threshold)
        _, st[2] = c.optimize(0, 20, 0.0, stop)  # :1113-1114
        outl = cls._tagged(c, prob).astype(np.uint8)  # :1119-1136
        cls._write_back(c, prob)
        return LBAResult(True, outl, st)

    @classmethod
    def BundleAdjustment(cls, prob: BAProblem, nIterations: int = 5, stop_flag=None, nLoopKF: int = 0,
                         bRobust: bool = True, ctx: Context | None = None):
        """g2oOptimizer::BundleAdjustment (g2oOptimizer.cc:110-362): KF 0 fixed
        (caller sets pose_fixed), Huber (float)sqrt(5.99) if bRobust."""
        c = cls._context(ctx)
        stereo = prob.obs_ur >= 0 if prob.obs_ur is not None else np.zeros(prob.n_obs, bool)
        prob.obs_delta[:] = np.where(stereo, HUBER_STEREO, HUBER_MONO_GBA) if bRobust else 0.0
        c.set_problem(prob)
        n, st = c.global_ba(nIterations, stop_flag)
        cls._write_back(c, prob)
        return n, st

    @classmethod
    def GlobalBundleAdjustemnt(cls, prob: BAProblem, nIterations: int = 5, stop_flag=None, nLoopKF: int = 0,
                               bRobust: bool = True, ctx: Context | None = None):
        """g2oOptimizer::GlobalBundleAdjustemnt (g2oOptimizer.cc:80-89)."""
        return cls.BundleAdjustment(prob, nIterations, stop_flag, nLoopKF, bRobust, ctx)

    @classmethod
    def OptimizeEssentialGraph(cls, pg, ctx: Context | None = None, stop_flag=None):
        """g2oOptimizer::OptimizeEssentialGraph (g2oOptimizer.cc:1212-1534) on an
        assembled pose graph: setUserLambdaInit(1e-16), optimize(20); the
        corrected Sim3 estimates are written back into ``pg.Siw``."""
        c = cls._context(ctx)
        c.eg_set_problem(pg)
        n, st = c.eg_optimize(20, 1e-16, stop_flag)
        pg.Siw[:] = c.eg_poses()
        return n, st

    @classmethod
    def OptimizeSim3(cls, prob, th2: float | None = None, bFixScale: bool | None = None, ctx: Context | None = None):
        """g2oOptimizer::OptimizeSim3 (g2oOptimizer.cc:1560-1793) on an assembled
        sim3.Sim3Problem: the pairs still ``matched`` are aligned, ``prob.S12``
        receives the optimised Sim3 (unchanged when fewer than 10 pairs survive
        the first stage), rejected pairs are cleared from ``prob.matched`` like
        ``vpMatches1[idx] = NULL``, and the inlier count nIn is returned."""
        c = cls._context(ctx)
        idx = np.nonzero(prob.matched)[0]
        sub = prob.copy()
        for k in ("X1c", "X2c", "obs1", "obs2", "info1", "info2"):
            setattr(sub, k, np.ascontiguousarray(getattr(prob, k)[idx]))
        sub.matched = np.ones(idx.size, bool)
        if th2 is not None:
            sub.th2 = float(np.float32(th2))
        if bFixScale is not None:
            sub.fix_scale = bool(bFixScale)
        S, n_in, state, _ = c.sim3_optimize([sub])
        prob.S12[:] = S[0]
        prob.matched[idx[state != 0]] = False
        return int(n_in[0])

    @classmethod
    def PoseOptimization(cls, prob, lidar_assoc=None, ctx: Context | None = None):
        """g2oOptimizer::PoseOptimization (g2oOptimizer.cc:385-679) on an assembled
        pose.PoseProblem: the four vision rounds; then, if ``lidar_assoc`` is
        given (it stands in for the kd-tree search: called with the pose
        ``(q, t)`` after ``SetPose``'s float round trip, it returns the
        pose.LidarPairs), the LiDAR stage. ``prob.pose_q`` / ``prob.pose_t``
        receive the optimised pose after the float round trip of ``SetPose``
        (unchanged with fewer than 3 edges), ``prob.outlier`` the final
        ``mvbOutlier`` flags, and the inlier count is returned."""
        c = cls._context(ctx)
        q, t, n_in, flag, _ = c.pose_optimize([prob])
        if prob.n_obs < 3:
            return 0
        q, t = pose_from_Tcw_f32(pose_to_Tcw_f32(q[0], t[0]))  # pFrame->SetPose(toCvMat(estimate))
        if lidar_assoc is not None:
            sub = prob.copy()
            sub.pose_q[:], sub.pose_t[:] = q, t  # setEstimate(toSE3Quat(pFrame->mTcw))
            q, t, n_in, flag, _ = c.pose_refine_lidar([sub], [lidar_assoc((q.copy(), t.copy()))], flag)
            q, t = pose_from_Tcw_f32(pose_to_Tcw_f32(q[0], t[0]))
        prob.pose_q[:], prob.pose_t[:] = q, t
        prob.outlier[:] = flag != 0
        return int(n_in[0])
