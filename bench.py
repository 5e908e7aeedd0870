#!/usr/bin/env python3
"""Benchmark: LM iterations/sec of the MI355X square-root LM bundle adjustment.

Workload (BASELINE.json `configs`): by default config 4, the synthetic global BA
(5k poses x 500k landmarks, k ~ U{2..18}, ~5M observations, KF0 fixed, no robust
kernel), the KITTI-00-scale BA of the metric. `--config lba` runs config 2 (the
synthetic local BA, 50 KF x 5k landmarks x 200 obs/KF) instead.

A "step" is one Levenberg–Marquardt outer iteration exactly as g2o runs it
(relinearise, then damped trials until one is accepted), with every array
already resident in HBM. Multi-GPU: landmarks are sharded over ranks (one
process per GPU); every rank assembles the S / g rows of its landmarks, rank 0
gathers them over RCCL point-to-point, solves, and broadcasts the step; total
work is fixed => strong scaling.

A plain run sets up, warms up, times `--steps` steps and prints the line with
the headline figure. `--full` adds everything else the line used to carry: the
event-timed phase table and rooflines (a second run of the same steps), the
drop-in end-to-end calls, the CPU baselines, and for the default workload the
loop-closed GBA and config-2 LBA figures. `--dump-outputs DIR` writes what the
timed steps left (the arrays a caller reads back) as DIR/<name>.npy.

Prints ONE JSON line on rank 0.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.join(ROOT, "sqrtlm-slam_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md, chip-level parameters)
# Dense FP64 matrix peak: 1024 SIMDs x 2.4 GHz x 32 FLOP/clk (v_mfma_f64_16x16x4f64 =
# 2048 FLOP per 64-cycle issue, the SQ_VALU_MFMA_BUSY_CYCLES we measure per MFMA)
# = 78.6 TFLOP/s, AMD's MI355X FP64-matrix figure. The guide has no f64 row.
MFMA_F64_PEAK_TFLOPS = 78.6
# committed PMC summaries, newest round first (pmc_traffic takes the first on the same workload)
PROFILE_DIRS = [os.path.join(ROOT, "profiles", r) for r in ("r06", "r05", "r04", "r03", "r02", "r01")]


def make_workload(name: str, scale: float):
    from sqrtlm import synth
    if name == "gba":
        prob = synth.config4(seed=4, scale=scale)
        desc = {"workload": "synthetic global BA (BASELINE config 4)", "n_pose": prob.n_pose,
                "n_landmark": prob.n_pt, "n_obs": prob.n_obs, "track_len": "U{2..18}", "robust": False,
                "seed": 4, "scale": scale}
    elif name == "gba_loop":
        # the shape the reference's GBA always has: it only runs after a loop
        # closure (LoopClosing.cc:877, :987-991), so S couples the revisited
        # keyframes far off its band (band + border solve)
        prob = synth.config4_loop(seed=4, scale=scale)
        desc = {"workload": "synthetic loop-closed global BA (BASELINE config 4 + 30-KF loop closure)",
                "n_pose": prob.n_pose, "n_landmark": prob.n_pt, "n_obs": prob.n_obs, "track_len": "U{2..18}",
                "loop_kf": 30, "robust": False, "seed": 4, "scale": scale}
    else:
        prob = synth.config2(seed=2)
        desc = {"workload": "synthetic local BA (BASELINE config 2)", "n_pose": prob.n_pose,
                "n_fixed": int(prob.pose_fixed.sum()), "n_landmark": prob.n_pt, "n_obs": prob.n_obs,
                "robust": "Huber (float)sqrt(5.991)", "seed": 2}
    return prob, desc


def algorithmic_bytes_linearize(p) -> float:
    """Bytes k_linearize must move per launch: per observation
    it reads cam id, free-camera id and u v info delta as one float32 float4
    (24 B; DevProblem::obs_f32) and writes the
    error (16 B) and the weight sqrt(rho' info) (8 B) from which the consumers
    recompute the H_lp blocks; per landmark it reads X (24 B) + offset (4 B)
    and writes the QR factor R (48 B) + b_l (24 B). Pose reads (<1 MB,
    L2-resident) excluded."""
    E, L = p.n_obs, p.n_pt
    return E * (24 + 16 + 8) + L * (24 + 4 + 48 + 24)


def algorithmic_bytes_update(p) -> float:
    """Bytes k_landmark_update<SPEC> must move per trial (DESIGN.md §2 steps
    6-7): per observation it reads cam id, free-camera id, u v info delta (one
    float4: the inputs are float32 values, DevProblem::obs_f32) and the
    linearization-point weight s (32 B) and writes the trial error (16 B)
    and the trial-state weight (8 B); per landmark it reads the offset, X, R
    and b_l (100 B) and writes X' and the trial-state R, b_l (96 B). Pose and
    dx reads (<1 MB, L2-resident) excluded."""
    E, L = p.n_obs, p.n_pt
    return E * (32 + 16 + 8) + L * (100 + 96)


def algorithmic_flops_rcs(p) -> float:
    """FLOPs k_rcs_tile must do per launch: for a landmark seen
    by m free cameras, stage Y = R'^-T H_lp (m blocks of 3x6, 54 FLOP each),
    form the upper triangle of Y^T Y (m(m+1)/2 blocks of 6x6 with inner dim 3,
    216 FLOP each) and Y^T w (36 FLOP per camera)."""
    free = p.pose_fixed[p.obs_pose] == 0
    m = np.bincount(p.obs_pt[free], minlength=p.n_pt).astype(np.float64)
    return float(np.sum(108.0 * m * (m + 1) + 90.0 * m))


def pmc_traffic(kernel_prefix: str, workload: str, n_obs: int):
    """Per-launch HBM bytes of `kernel_prefix` (summed over its template
    instances, e.g. the three k_linearize<W> buckets) from the committed rocprofv3 PMC
    summary (scripts/gpu_pmc.sh + scripts/pmc_summary.py: separate FETCH_SIZE
    and WRITE_SIZE passes, FETCH_SIZE doubled for gfx950). None if the summary
    was not taken on this exact workload."""
    for pdir in PROFILE_DIRS:
        path = os.path.join(pdir, f"pmc_{workload}.json")
        if os.path.exists(path):
            summ = json.load(open(path))
            if int(summ.get("meta", {}).get("n_obs", -1)) == n_obs:
                break
    else:
        return None, None
    hits = [e["traffic_bytes"] for k, e in summ["kernels"].items()
            if k.startswith(kernel_prefix) and "traffic_bytes" in e]  # all template instances (buckets)
    return (float(sum(hits)), os.path.relpath(path, ROOT)) if hits else (None, None)


def survey_bytes_linearize(p) -> float:
    """SURVEY.md §8(d) B(l) = 28k + 28 + 16k(6m+4) (writes a dense 2k x (6m+4)
    Q-applied block per landmark; this design never materialises it)."""
    k = np.bincount(p.obs_pt, minlength=p.n_pt).astype(np.float64)
    m = np.bincount(p.obs_pt, weights=(p.pose_fixed[p.obs_pose] == 0).astype(np.float64), minlength=p.n_pt)
    return float(np.sum(28 * k + 28 + 16 * k * (6 * m + 4)))


def _gloo_allreduce(arr, op):
    """Host collective for --comm host (sqlm_ctx_set_host_comm)."""
    import torch
    import torch.distributed as dist
    rop = dist.ReduceOp.MAX if op == "max" else dist.ReduceOp.SUM
    t = torch.from_numpy(arr.astype(np.int32) if arr.dtype == np.uint8 else arr)
    dist.all_reduce(t, op=rop)
    if arr.dtype == np.uint8:
        arr[:] = t.numpy().astype(np.uint8)


def _gloo_p2p(arr, peer, op):
    """Host point-to-point for --comm host (sqlm_ctx_set_host_p2p)."""
    import torch
    import torch.distributed as dist
    t = torch.from_numpy(arr.view(np.uint8))
    if op == "send":
        dist.send(t, dst=peer)
    elif op == "recv":
        dist.recv(t, src=peer)
    else:
        dist.broadcast(t, src=peer)


def reprojection_sse(p, q, t, X):
    """(sum ||obs - proj||^2, number of edges) at the given state; the RMSE
    over all shards is sqrt(sum sse / sum n)."""
    from sqrtlm.synth import quat_to_mat
    R = quat_to_mat(q)
    Xc = np.einsum("nij,nj->ni", R[p.obs_pose], X[p.obs_pt]) + t[p.obs_pose]
    fx, fy, cx, cy = (p.intr[p.obs_pose, k] for k in range(4))
    e = p.obs_uv - np.stack([Xc[:, 0] / Xc[:, 2] * fx + cx, Xc[:, 1] / Xc[:, 2] * fy + cy], axis=1)
    return float(np.sum(e * e)), float(p.n_obs)


DUMP_MAX_BYTES = 64 << 20  # bound of one --dump-outputs directory


def dump_outputs(dirname: str, arrays: dict) -> None:
    """--dump-outputs: write each array as DIRNAME/<name>.npy in float64
    (float32 arrays stay float32, anything else becomes float32). When the
    arrays together exceed DUMP_MAX_BYTES, the leading axis of the larger ones
    is cut to a fixed seeded sample of rows (the same rows on every run)."""
    os.makedirs(dirname, exist_ok=True)
    arrs = {}
    for name, a in arrays.items():
        a = np.ascontiguousarray(a)
        arrs[name] = a if a.dtype in (np.float32, np.float64) else a.astype(np.float32)
    budget = DUMP_MAX_BYTES // max(1, len(arrs))
    if sum(a.nbytes for a in arrs.values()) > DUMP_MAX_BYTES:
        rng = np.random.default_rng(0)
        for name, a in arrs.items():
            if a.nbytes > budget and a.ndim >= 1:
                rows = max(1, budget // max(1, a.nbytes // len(a)))
                arrs[name] = a[np.sort(rng.choice(len(a), size=rows, replace=False))]
    for name, a in arrs.items():
        np.save(os.path.join(dirname, name + ".npy"), a)


def host_cpu() -> dict:
    """CPU model and core counts of the host the baseline ran on (lscpu's
    model name from /proc/cpuinfo; nproc = the cores this process may use)."""
    model = None
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    try:
        usable = len(os.sched_getaffinity(0))
    except AttributeError:
        usable = os.cpu_count()
    return {"cpu_model": model, "nproc": usable, "machine_cpus": os.cpu_count()}


def cpu_baseline(prob, name: str, omp: bool = False, gba_iters: int = 10, min_s: float = 10.0):
    """The oracle (g2o-semantics port) on a bounded sample of the same
    workload: the whole optimize(10) of the full config-4 problem (the
    reference's GlobalBundleAdjustemnt call, ~17 s on one core), or repeated
    10-iteration solves of config 2 until >= 10 s. Only the optimize()
    calls are timed. Single thread by default, matching the reference build
    (G2O_USE_OPENMP=OFF, Thirdparty/g2o/build/CMakeCache.txt:175); omp=True is
    the labelled all-cores variant (g2o's OpenMP loops on OMP_NUM_THREADS
    threads, bit-identical results). Both are -O2 C, not g2o + Eigen built
    -O3 -march=native, which cannot be built here."""
    from oracle import oracle as O
    O.build()
    total_n, total_dt, runs = 0, 0.0, 0
    while True:
        g = O.OracleGraph(prob, omp=omp)
        t0 = time.perf_counter()
        n, st = g.optimize(0, gba_iters if name.startswith("gba") else 10)
        total_dt += time.perf_counter() - t0
        total_n += max(n, 1)
        runs += 1
        del g
        if name.startswith("gba") or total_dt >= min_s:
            break
    host = host_cpu()
    threads = O.omp_threads() if omp else 1
    out = dict({"value": total_n / total_dt, "unit": "LM iterations/s", "cores": threads, "kind": "port",
                "sample": f"{total_n} LM iterations ({runs} x optimize()) on the full {name} workload, "
                          f"{threads} thread(s), {total_dt:.1f} s of optimize() time",
                "build": "oracle/g2o_ref.c gcc -O2" + (" -fopenmp (ORC_OMP)" if omp else "")}, **host)
    if omp:
        out["threads_note"] = (f"{threads} OpenMP threads = the job's CPU share (OMP_NUM_THREADS); the host shows "
                               f"{host['nproc']} usable of {host['machine_cpus']} CPUs, most of them other jobs'")
    return out


EG_N_KF = 1500  # KITTI-00 keyframe count of ORB-SLAM2-style mapping (SURVEY.md §8 sizes, config 5: EG 7*#KF)


def eg_arrow_layout(pg):
    """Band / border split of the essential graph as sqlm_eg.hip makes it
    (free vertices in id order; a greedy cover of the edges longer than 16
    vertices goes to the border): (band vertices, border vertices)."""
    free = pg.fixed == 0
    hid = np.full(pg.n_kf, -1)
    act = ~(~free[pg.ei] & ~free[pg.ej])
    vact = np.zeros(pg.n_kf, bool)
    vact[pg.ei[act]] = vact[pg.ej[act]] = True
    sel = vact & free
    hid[sel] = np.arange(int(sel.sum()))
    n_p = int(sel.sum())
    longe = [(hid[i], hid[j]) for i, j in zip(pg.ei[act], pg.ej[act])
             if hid[i] >= 0 and hid[j] >= 0 and abs(hid[i] - hid[j]) > 16]
    nlong = np.zeros(n_p, int)
    for a, b in longe:
        nlong[a] += 1
        nlong[b] += 1
    border = np.zeros(n_p, bool)
    for a, b in longe:
        if not border[a] and not border[b]:
            border[a if (nlong[a] > nlong[b] or (nlong[a] == nlong[b] and a > b)) else b] = True
    nb = int(border.sum())
    return (n_p - nb, nb) if 3 * nb <= n_p else (0, n_p)


def eg_solve_flops(pg) -> float:
    """FLOPs of one damped solve of the block-arrow system: the
    block-tridiagonal band of p blocks of 112 rows factored (Cholesky, the
    off-diagonal solve and the Schur update per block: (1/3 + 1 + 1) 112^3),
    nb + 1 right-hand sides carried through it (2 triangular solves and 2
    off-diagonal products per block: 4 * 112^2 each), the border Schur
    complement F Y (2 n_band nb^2) and its Cholesky (nb^3 / 3)."""
    band_v, border_v = eg_arrow_layout(pg)
    n_band, nb = 7 * band_v, 7 * border_v
    p = -(-n_band // 112)
    return p * (7.0 / 3.0) * 112 ** 3 + p * 4.0 * 112 ** 2 * (nb + 1) + 2.0 * n_band * nb ** 2 + nb ** 3 / 3.0


def bench_eg(args, world):
    """Essential graph (g2oOptimizer.cc:1212-1534) on a
    KITTI-00-scale loop: 1500 Sim3 keyframes, spanning tree + 8 covisibility
    edges per keyframe + 20 loop edges, fix-scale (stereo). A step is one LM
    iteration of optimize(20) with lambda_init 1e-16, as the reference runs it;
    replicas only (one pose graph per GPU)."""
    from sqrtlm import synth
    from sqrtlm.optimizer import Context
    pg = synth.make_pose_graph(EG_N_KF, window=8, n_loops=20, seed=5, fix_scale=True)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("gloo", init_method="env://")
    with Context(local_rank) as ctx:
        for _ in range(max(1, args.warmup)):
            ctx.eg_set_problem(pg)
            ctx.eg_optimize(20, 1e-16)
        if world > 1:
            dist.barrier()
        n_it, t_tot, st = 0, 0.0, None
        for _ in range(max(1, args.steps // 20)):
            ctx.eg_set_problem(pg)
            t0 = time.perf_counter()
            n, st = ctx.eg_optimize(20, 1e-16)
            t_tot += time.perf_counter() - t0
            n_it += n
        ms = 1000.0 * t_tot / max(1, n_it)
        if args.dump_outputs and rank == 0:
            dump_outputs(args.dump_outputs, {"sim3": ctx.eg_poses(), "chi2_end": np.array([st["chi2_end"]])})
    if world > 1:
        import torch
        tt = torch.tensor([ms], dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        ms = float(tt.item())
    if rank == 0:
        n = 7 * int((pg.fixed == 0).sum())
        flops = eg_solve_flops(pg)
        out = {"metric": "LM iterations/sec (essential graph, KITTI-00 scale)", "value": world * 1000.0 / ms,
               "unit": "LM iterations/s", "n_gpus": world, "steps": n_it, "warmup": args.warmup,
               "ms_per_step": ms, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
               "dtype": "f64", "data": "synthetic (repo pose-graph generator, seed 5)",
               "config": {"workload": "essential graph (Sim3, fix-scale)", "n_kf": pg.n_kf, "n_edge": pg.n_edge,
                          "dims": n, "parallelism": f"replicas x{world}"},
               "trials_per_step": st["trials"] / max(1, st["iterations"]) if st else None,
               "chi2_last": st["chi2_end"] if st else None,
               "roofline": {"bound": "mfma", "kernel": "block-arrow solve (per trial)", "algorithmic_flops": flops,
                            "peak": MFMA_F64_PEAK_TFLOPS, "unit": "TFLOP/s",
                            "achieved": flops * (st["trials"] / max(1, st["iterations"])) / (ms * 1e-3) / 1e12,
                            "note": "FLOPs of the band + border factorization and solve (eg_solve_flops) over the "
                                    "whole LM iteration time; the solve is latency-bound (log2 p cyclic-reduction "
                                    "levels of 112-row block factorizations)"}}
        out["roofline"]["frac"] = out["roofline"]["achieved"] / MFMA_F64_PEAK_TFLOPS
        if args.full and not args.no_cpu_baseline and world == 1:
            from oracle import oracle as O
            O.build()
            ref = O.OracleEG(pg)
            t0 = time.perf_counter()
            nr, _ = ref.optimize(3, 1e-16)
            dt = time.perf_counter() - t0
            out["cpu_baseline"] = dict({"value": nr / dt, "unit": "LM iterations/s", "cores": 1, "kind": "port",
                                        "sample": f"{nr} LM iterations of the same graph, single thread, {dt:.1f} s"},
                                       **host_cpu())
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


def bench_matchers(ctx, ex, reps, cpu):
    """ORBmatcher's searches on a KITTI-size scene (sqrtlm.orb_scene, two
    2000-feature frames 9 px apart): ms per call through the C ABI (host
    arrays in and out, windows / node runs and Hamming distances on the GPU,
    acceptance on the host), and the single-thread oracle beside it."""
    from sqrtlm import orb_scene as S
    from sqrtlm import synth
    from sqrtlm.orb import BowFrame, Frame, KeyFrameSlots, LastFrameSlots, ORBmatcher
    a, b = synth.make_image_pair(1241, 376, seed=17, shift=(9.0, 2.0))
    k1, d1 = ex(a)
    k2, d2 = ex(b)
    bounds, cam, sf = (0.0, 1241.0, 0.0, 376.0), S.camera(1241, 376), S.scale_factors()
    mps, md = S.local_points(k1, d1, (9.0, 2.0), seed=3, stereo=True)
    ur, sm, so = S.current_slots(k2, 3, True)
    Tcw, Tlw, lp, ld = S.last_frame(k1, d1, (9.0, 2.0), 1241, 376, seed=4, tz=1.0)
    kmp, kmd = S.map_points(k1, d1, 1241, 376, seed=5)
    Tk = S.keyframe_pose((9.0, 2.0), 1241, 376, (0.0, 0.01, 0.05))
    n1, n2 = S.bow_nodes(d1, 1), S.bow_nodes(d2, 2)
    mp1, bad1 = S.bow_points(len(k1), 1)
    mp2, bad2 = S.bow_points(len(k2), 2, base=10000)
    m = ORBmatcher(0.8, True, ctx=ctx)

    def frame(Tc=None):
        return Frame(k2, d2, bounds, sf, *cam, mvuRight=ur, mTcw=Tc, mvpMapPoints=sm.copy(), slot_obs=so.copy())
    gpu = {
        "SearchByProjection_local": lambda: m.SearchByProjection(frame(), mps, md, 1.0),
        "SearchByProjection_last": lambda: m.SearchByProjection(frame(Tcw), LastFrameSlots(Tlw, lp, ld), 7.0, False),
        "SearchByProjection_kf": lambda: m.SearchByProjection(frame(Tk), KeyFrameSlots(kmp, kmd, k1["angle"]), 10.0,
                                                              100),
        "Fuse": lambda: m.Fuse(frame(Tk), kmp, kmd, 3.0),
        "SearchByBoW_kf_frame": lambda: m.SearchByBoW(BowFrame(k1, d1, n1, mp1, bad1),
                                                      BowFrame(k2, d2, n2, keyframe=False)),
    }
    out = {}
    for name, fn in gpu.items():
        fn()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        out[name] = {"gpu_ms": (time.perf_counter() - t0) * 1e3 / reps}
    if cpu:
        from oracle import orb as OB
        oracle = {
            "SearchByProjection_local": lambda: OB.search_by_projection_local(k2, d2, bounds, sf, ur, sm, so, mps, md,
                                                                              1.0, 0.8),
            "SearchByProjection_last": lambda: OB.search_by_projection_last(k2, d2, bounds, sf, cam, ur, sm, so, Tcw,
                                                                            Tlw, lp, ld, 7.0, False),
            "SearchByProjection_kf": lambda: OB.search_by_projection_kf(k2, d2, bounds, sf, cam, sm, Tk, kmp, kmd,
                                                                        k1["angle"], 10.0, 100),
            "Fuse": lambda: OB.fuse(k2, d2, bounds, sf, cam, ur, Tk, False, kmp, kmd, 3.0),
            "SearchByBoW_kf_frame": lambda: OB.search_by_bow_kf_frame((k1, d1, n1, mp1, bad1), (k2, d2, n2, mp2),
                                                                      0.8),
        }
        for name, fn in oracle.items():
            fn()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            out[name]["cpu_port_ms"] = (time.perf_counter() - t0) * 1e3 / reps
    return out


def orb_extras(args, ctx, ex, img, reps, local_rank, world):
    """The --full legs of bench_orb on the warmed-up extractor: the stereo pair
    of extractors, the byte count behind k_orb_fast's roofline, the matchers."""
    from sqrtlm.optimizer import Context
    from sqrtlm.orb import ORBextractor
    # a stereo Frame extracts left and right on two threads with two
    # ORBextractor objects (Frame.cc stereo constructor): two contexts (own
    # HIP stream each) driven concurrently, one overlapping the other's host
    # quadtree and synchronisations
    import threading
    with Context(local_rank) as ctx2:
        ex2 = ORBextractor(2000, 1.2, 8, 20, 7, ctx=ctx2)
        ex2(img)
        th = [threading.Thread(target=e.bench, args=(img, reps)) for e in (ex, ex2)]
        t0 = time.perf_counter()
        for t in th:
            t.start()
        for t in th:
            t.join()
        stereo_fps = 2 * reps / (time.perf_counter() - t0)
    # algorithmic bytes of k_orb_fast per launch: every cell view it stages
    # (overlapping 30-px cells + 6-px overlap) + 4 B per candidate + 4 B count
    from oracle import orb as OB  # geometry only: the same cell loop as the reference
    lw, lh, _, _ = OB.levels(OB.params(), 1241, 376)
    view_bytes = 0
    ncell = 0
    for w, h in zip(lw.tolist(), lh.tolist()):
        width, height = float(w - 32), float(h - 32)
        nc, nr = int(width / 30), int(height / 30)
        wc, hc = int(np.ceil(np.float32(width) / nc)), int(np.ceil(np.float32(height) / nr))
        for i in range(nr):
            y0 = 16 + i * hc
            if y0 >= h - 16 - 3:
                continue
            for j in range(nc):
                x0 = 16 + j * wc
                if x0 >= w - 16 - 3:
                    continue
                view_bytes += (min(x0 + wc + 6, w - 16) - x0) * (min(y0 + hc + 6, h - 16) - y0)
                ncell += 1
    OB.build()
    _k, _d, pyr = OB.extract(OB.params(), img, with_levels=True)
    ncand = sum(len(OB.level_candidates(OB.params(), lev)) for lev in pyr)
    matchers = bench_matchers(ctx, ex, reps=max(20, args.steps * 4), cpu=not args.no_cpu_baseline and world == 1)
    return stereo_fps, view_bytes, ncell, ncand, matchers, OB


def bench_orb(args, world):
    """ORB front end: ORBextractor::operator() on a
    KITTI-00-size synthetic grey frame (1241x376, cfg/KITTI00-02.yaml: 2000
    features, 1.2, 8 levels, FAST 20/7). A step is one frame, image already in
    HBM, including the host quadtree step and the keypoint / descriptor D2H.
    Replicas only (one camera stream per GPU)."""
    from sqrtlm import synth
    from sqrtlm.optimizer import Context
    from sqrtlm.orb import ORBextractor
    img, _ = synth.make_image_pair(1241, 376, seed=3)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("gloo", init_method="env://")
    with Context(local_rank) as ctx:
        ex = ORBextractor(2000, 1.2, 8, 20, 7, ctx=ctx)
        for _ in range(max(1, args.warmup)):
            kps, _d = ex(img)
        if world > 1:
            dist.barrier()
        reps = max(50, args.steps * 10)
        ms, stages = ex.bench(img, reps)
        if args.dump_outputs and rank == 0:
            kd, dd = ex(img)  # what the timed call returns for this frame
            dump_outputs(args.dump_outputs, dict({f: kd[f] for f in kd.dtype.names}, descriptors=dd))
        extras = orb_extras(args, ctx, ex, img, reps, local_rank, world) if args.full else None
    if world > 1:
        import torch
        tt = torch.tensor([ms], dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        ms = float(tt.item())
    if rank == 0:
        out = {"metric": "frames/sec (ORB extraction, KITTI-00 frame)", "value": world * 1000.0 / ms,
               "unit": "frames/s", "n_gpus": world, "steps": reps, "warmup": args.warmup, "ms_per_step": ms,
               "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u8",
               "data": "synthetic grey frame (repo scene generator, seed 3)",
               "config": {"workload": "ORBextractor 1241x376, 2000 features, 8 levels", "keypoints": int(len(kps)),
                          "parallelism": f"replicas x{world}"},
               "stage_ms": dict(zip(["pyramid", "fast", "compact", "blur", "describe", "host_quadtree"], stages))}
        if extras is not None:
            stereo_fps, view_bytes, ncell, ncand, matchers, OB = extras
            alg = int(view_bytes) + 4 * int(ncand) + 4 * int(ncell)
            t_fast = stages[1]
            out["stereo_two_extractors_frames_per_s"] = stereo_fps
            out["matchers_ms_per_call"] = matchers
            out["roofline"] = {"bound": "hbm", "kernel": "k_orb_fast", "algorithmic_bytes": alg,
                               "achieved": alg / (t_fast * 1e-3) / 1e9 if t_fast > 0 else 0.0, "peak": HBM_PEAK_GBPS,
                               "unit": "GB/s", "traffic": None, "launch_ms": t_fast,
                               "note": "one launch per frame over all 30-px cells of all levels; latency-bound"}
            out["roofline"]["frac"] = out["roofline"]["achieved"] / HBM_PEAK_GBPS
        if extras is not None and not args.no_cpu_baseline and world == 1:
            OB.build()
            p = OB.params()
            t0 = time.perf_counter()
            nf = 0
            while time.perf_counter() - t0 < 5.0:
                OB.extract(p, img)
                nf += 1
            dt = time.perf_counter() - t0
            out["cpu_baseline"] = dict({"value": nf / dt, "unit": "frames/s", "cores": 1, "kind": "port",
                                        "sample": f"{nf} extractions of the same frame, single thread, {dt:.1f} s"},
                                       **host_cpu())
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


class CommInitFailed(SystemExit):
    """Every rank leaves with this status when the RCCL communicator cannot be
    built: a multi-GPU line is an RCCL measurement or no line at all."""
    STATUS = 3


def connect_rccl(ctx, rank, world, dist, make_uid):
    """Build the context's RCCL communicator over `world` ranks (rank 0 makes
    the id, the gloo group broadcasts it). Collective: every rank learns
    whether every other one succeeded and whether the communicator reports
    `world` ranks (ncclCommCount). On any failure every rank exits with
    CommInitFailed.STATUS -- there is no silent fallback to the host transport.
    Returns the description recorded in the line's config.comm and the rank
    count the communicator reports."""
    import torch
    from sqrtlm._lib import SqlmError
    uid = make_uid() if rank == 0 else b""
    t = torch.tensor([len(uid)], dtype=torch.int64)
    dist.broadcast(t, 0)
    if rank != 0:
        uid = bytes(int(t[0]))
    tu = torch.tensor(list(uid), dtype=torch.uint8)
    dist.broadcast(tu, 0)
    ok = torch.tensor([1], dtype=torch.int32)
    why = ""
    try:
        ctx.set_comm(bytes(tu.tolist()), rank, world)
        info = ctx.comm_info()
        if info["transport"] != "rccl" or info["nranks"] != world or info["rank"] != rank:
            why = f"communicator reports {info}, expected rccl rank {rank} of {world}"
            ok[0] = 0
    except SqlmError as err:
        why = str(err)
        ok[0] = 0
    dist.all_reduce(ok, op=dist.ReduceOp.MIN)
    if int(ok[0]) == 0:
        print(f"bench.py rank {rank}: RCCL communicator init failed on "
              f"{'this rank' if why else 'another rank'}{': ' + why if why else ''}; no line is written",
              file=sys.stderr)
        raise CommInitFailed(CommInitFailed.STATUS)
    return f"rccl ({info['nranks']} ranks reported by ncclCommCount)", info["nranks"]


def run_ba(args, world, rank, local_rank, dist, config, cpu_iters=10, cpu_min_s=10.0, dump=None):
    """One BA workload (config 4, the loop-closed config 4, or config 2) on this
    rank's context; returns the bench dict on rank 0 (None elsewhere). `dump`
    names the directory the state after the timed steps is written to."""
    from sqrtlm.optimizer import Context
    from sqrtlm.shard import shard
    prob, desc = make_workload(config, args.scale)
    local = shard(prob, rank, world)
    # SQLM_BENCH_ONE_GPU=1 puts every rank on GPU 0 (1-GPU rehearsal of the RCCL transport)
    one_gpu = args.comm == "host" or os.environ.get("SQLM_BENCH_ONE_GPU") == "1"
    ctx = Context(0 if one_gpu else local_rank)
    comm_used, comm_ranks = "none", 1
    if world > 1 and args.comm == "rccl":
        from sqrtlm.optimizer import comm_unique_id
        comm_used, comm_ranks = connect_rccl(ctx, rank, world, dist, comm_unique_id)
    elif world > 1:
        ctx.set_host_comm(rank, world, _gloo_allreduce, _gloo_p2p)
        comm_used, comm_ranks = "host (gloo, %d ranks on GPU 0)" % world, world
    ctx.set_problem(local)
    # the timed run without the per-phase HIP events (they cost ≈2 %), then
    # (--full) the same run from the same initial state with them, for the
    # phase breakdown and the roofline's kernel times
    ms, _none, st = ctx.bench(args.warmup, args.steps, timers=False)
    if dump:
        # the state the timed steps left, as sqlm_get_poses / sqlm_get_points hand it
        # to a caller; the cameras are replicated, the landmarks are this rank's shard
        sfx = f"_rank{rank}" if world > 1 else ""
        q_out, t_out = ctx.poses()
        dump_outputs(dump, {"pose_q" + sfx: q_out, "pose_t" + sfx: t_out, "points" + sfx: ctx.points(),
                            "chi2_end" + sfx: np.array([st["chi2_end"]])})
    kms, sse, nres = {}, 0.0, 0.0
    if args.full:
        ctx.set_problem(local)
        _ms_timed, kms, _st = ctx.bench(args.warmup, args.steps)
        sse, nres = reprojection_sse(local, *ctx.poses(), ctx.points())
    e2e = None
    if args.full and world == 1 and config == "lba":
        # the drop-in LocalBundleAdjustment call: host arrays in, the three-pass
        # schedule (5 Huber iterations, outlier tags, 10 more, + LiDAR 20), out
        reps = []
        for _ in range(3):  # the median of three calls by wall time, as for the global BA below
            t0 = time.perf_counter()
            ctx.set_problem(local)
            ran, _tags, sts = ctx.local_ba()
            ctx.poses(), ctx.points()
            reps.append((time.perf_counter() - t0, int(ran), int(sum(x["iterations"] for x in sts)),
                         float(sum(x["ms_setup"] for x in sts)), float(sum(x["ms_total"] for x in sts))))
        sec, ran, its, setup, opt = sorted(reps)[1]
        e2e = {"seconds": sec, "passes": ran, "lm_iterations": its, "setup_ms": setup, "optimize_ms": opt,
               "seconds_all": [r[0] for r in reps],
               "what": "sqlm_set_problem + sqlm_local_ba (3-pass schedule) + sqlm_get_poses/points, host buffers; "
                       "median of 3 calls by wall time"}
    if args.full and world == 1 and config in ("gba", "gba_loop"):
        # the drop-in call as the reference makes it (GlobalBundleAdjustemnt, 10
        # iterations): host arrays in, setup (sorting, tiles, H2D), the solve,
        # results out (D2H) — reported beside the metric, never as `value`
        # three calls, the median one reported (the host setup part moves by
        # several ms with the box's load from call to call)
        reps = []
        for _ in range(3):
            t0 = time.perf_counter()
            ctx.set_problem(local)
            n_e2e, _st = ctx.global_ba(10)
            ctx.poses(), ctx.points()
            reps.append((time.perf_counter() - t0, n_e2e, _st["ms_setup"], _st["ms_total"]))
        sec, n_e2e, setup, opt = sorted(reps)[1]
        e2e = {"seconds": sec, "lm_iterations": n_e2e, "setup_ms": setup, "optimize_ms": opt,
               "seconds_all": [r[0] for r in reps], "setup_ms_all": [r[2] for r in reps],
               "what": "sqlm_set_problem + sqlm_global_ba(10) + sqlm_get_poses/points, host buffers; "
                       "median of 3 calls by wall time"}
    if dist is not None:
        import torch
        tt = torch.tensor([ms], dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        ms = float(tt.item())
    if dist is not None and args.full:
        tt = torch.tensor([sse, nres], dtype=torch.float64)
        dist.all_reduce(tt)
        sse, nres = float(tt[0]), float(tt[1])
    out = None
    if rank == 0:
        out = {
            "metric": "LM iterations/sec (synthetic KITTI-00-scale BA)",
            "value": 1000.0 / ms,
            "unit": "LM iterations/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms,
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic (repo generator, SplitMix64 seed; inputs rounded through float32 like the reference)",
            "config": dict(desc, parallelism=f"landmark-shard x{world}", comm=comm_used, comm_ranks=comm_ranks),
            "trials_per_step": st["trials"] / max(1, st["iterations"]),
            "chi2_first": st["trace_chi2"][0] if st["trace_chi2"] else None,
            "chi2_last": st["chi2_end"],
        }
    if out is not None and args.full:
        launches = max(1.0, st["trials"] / max(1, st["iterations"]))  # k_rcs_tile runs once per trial
        t_rcs = kms["k_rcs_tile"] / launches
        flops = algorithmic_flops_rcs(local)
        ach_tf = flops / (t_rcs * 1e-3) / 1e12 if t_rcs > 0 else 0.0
        traffic, tsrc = pmc_traffic("k_rcs_tile", config, local.n_obs) if world == 1 else (None, None)
        # the landmark linearization runs inside k_landmark_update (speculative,
        # DESIGN.md §2 step 7) unless SQLM_NO_SPEC=1 puts it back in k_linearize
        spec = os.environ.get("SQLM_NO_SPEC", "0") in ("", "0")
        lin_kernel = "k_landmark_update" if spec else "k_linearize"
        t_lin = kms[lin_kernel] / (launches if spec else 1.0)
        alg = algorithmic_bytes_update(local) if spec else algorithmic_bytes_linearize(local)
        achieved = alg / (t_lin * 1e-3) / 1e9 if t_lin > 0 else 0.0
        lin_traffic, _ = pmc_traffic(lin_kernel, config, local.n_obs) if world == 1 else (None, None)
        out.update({
            "final_rmse_px": float(np.sqrt(sse / max(1.0, nres))),
            "kernel_ms_per_step": kms,
            "kernel_timers": "a second run of the same steps from the same initial state with HIP events per phase "
                             "(ms_per_step and value come from the run without them)",
            "roofline": {"bound": "mfma", "kernel": "k_rcs_tile", "achieved": ach_tf,
                         "peak": MFMA_F64_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": ach_tf / MFMA_F64_PEAK_TFLOPS,
                         "traffic": traffic, "traffic_source": tsrc, "algorithmic_flops": flops,
                         "launch_ms": t_rcs,
                         "note": "one RCS tile phase per trial = the width-class launches k_rcs_tile_p<8>, <6>, "
                                 "<9>, <4> (producer / consumer kernel; k_rcs_tile for stereo or repeated cameras) "
                                 "on three streams; launch_ms is the phase's wall time (HIP events on the "
                                 "context stream around the fork and join), rocprof lists the class kernels "
                                 "separately with overlapping durations"},
            "roofline_secondary": {"bound": "hbm", "kernel": f"{lin_kernel} (all buckets)", "achieved": achieved,
                                   "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBPS,
                                   "traffic": lin_traffic, "algorithmic_bytes": alg, "launch_ms": t_lin,
                                   "survey_basis_GBps": survey_bytes_linearize(local) / (t_lin * 1e-3) / 1e9
                                   if t_lin and not spec else None},
        })
        if e2e is not None:
            out["end_to_end"] = e2e
        if not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline(prob, config, gba_iters=cpu_iters, min_s=cpu_min_s)
            out["cpu_baseline_multithread"] = cpu_baseline(prob, config, omp=True, gba_iters=cpu_iters,
                                                           min_s=cpu_min_s)
    ctx.close()
    return out


def summary(out) -> dict:
    """The keys of a workload's line that the default line repeats for it."""
    keep = ("metric", "value", "unit", "ms_per_step", "trials_per_step", "final_rmse_px", "config", "end_to_end")
    s = {k: out[k] for k in keep if k in out}
    s["roofline"] = {k: out["roofline"][k] for k in ("kernel", "achieved", "peak", "unit", "frac")}
    s["kernel_ms_per_step"] = out["kernel_ms_per_step"]
    for k in ("cpu_baseline", "cpu_baseline_multithread"):
        if k in out:
            s[k] = {kk: out[k][kk] for kk in ("value", "unit", "cores", "kind", "sample")}
    return s


def free_port() -> int:
    """A TCP port on 127.0.0.1 nothing listens on right now (rendezvous of the
    self-launched ranks)."""
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def spawn_ranks(n: int, child_argv: list, timeout_s: float = 3000.0) -> int:
    """Start n copies of child_argv as ranks 0..n-1 of one job on this node
    (RANK / LOCAL_RANK / WORLD_SIZE / LOCAL_WORLD_SIZE / MASTER_ADDR /
    MASTER_PORT, as torch.distributed.run sets them) and wait for all of them.
    The parent touches no GPU: every rank is a fresh process. The first rank
    that fails ends the others (the exact processes started here); returns
    the worst exit status (0 when every rank succeeded)."""
    port = free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   GROUP_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen(child_argv, env=env))
    t0, rc = time.time(), 0
    live = list(procs)
    while live:
        for p in list(live):
            code = p.poll()
            if code is None:
                continue
            live.remove(p)
            if code != 0:
                rc = rc or code
                for q in live:  # one rank failed: the collective job cannot finish
                    q.terminate()
        if live and time.time() - t0 > timeout_s:
            for q in live:
                q.kill()
            rc = rc or 124
        time.sleep(0.05)
    for p in procs:
        p.wait()
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", choices=["gba", "gba_loop", "lba", "eg", "orb"], default="gba")
    ap.add_argument("--scale", type=float, default=1.0, help="shrink config 4 (parity / debugging only)")
    ap.add_argument("--full", action="store_true",
                    help="beyond the timed steps: phase table and rooflines (a second run), end-to-end calls, CPU "
                         "baselines, and for the default workload the loop-closed GBA and config-2 LBA figures")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed steps computed (poses, points, final chi2) as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baselines")
    ap.add_argument("--no-extras", action="store_true",
                    help="--full line without the loop-closed GBA and config-2 LBA figures")
    ap.add_argument("--comm", choices=["rccl", "host"], default="rccl",
                    help="host = exchange through gloo on the host, all ranks on GPU 0 (1-GPU rehearsal of N>1)")
    args = ap.parse_args()

    if args.gpus < 1:
        print(f"bench.py: --gpus {args.gpus} must be >= 1", file=sys.stderr)
        sys.exit(2)
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and args.gpus > 1:
        # no launcher: start the N ranks here (before anything touches a GPU in
        # this process) and exit with their status
        sys.exit(spawn_ranks(args.gpus, [sys.executable, os.path.abspath(__file__)] + sys.argv[1:]))
    world = int(env_world or "1")
    if world != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks", file=sys.stderr)
        sys.exit(2)
    if args.config == "eg":
        return bench_eg(args, world)
    if args.config == "orb":
        return bench_orb(args, world)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    if world > 1:
        import torch.distributed as dist  # rendezvous + scalar reductions only
        dist.init_process_group("gloo", init_method="env://")
    out = run_ba(args, world, rank, local_rank, dist, args.config, dump=args.dump_outputs)
    if (out is not None and args.full and args.config == "gba" and world == 1 and not args.no_extras
            and args.scale == 1.0):
        # the workloads the reference's own BA calls have, beside the metric's:
        # GBA only ever runs after a loop closure (LoopClosing.cc:877, :987-991),
        # and LocalMapping's local BA (LocalMapping.cc:131) is config 2's shape;
        # bounded CPU samples (3 LM iterations / 5 s) keep the default run short
        out["extra_workloads"] = {
            "gba_loop": summary(run_ba(args, world, rank, local_rank, dist, "gba_loop", cpu_iters=3, cpu_min_s=5.0)),
            "lba": summary(run_ba(args, world, rank, local_rank, dist, "lba", cpu_iters=3, cpu_min_s=5.0)),
        }
    if out is not None:
        print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
