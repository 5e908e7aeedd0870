#!/usr/bin/env python3
"""Time local-BA pass 3 with LiDAR clouds (association + optimize(0, 20)) on config 2, flat only and flat + corner.

Pass 3 of LocalBundleAdjustment (g2oOptimizer.cc:978-1114) on BASELINE config
2 (50 KF, 10 fixed, 5k landmarks): the association of the current keyframe's
LiDAR points against the clouds of 20 other free keyframes, then optimize(0,
20). Two configurations:

  flat         sqlm_set_lidar_from_clouds, the call made without corner points
  flat+corner  sqlm_set_lidar_from_cloud_sets with a flat and a corner set

A run is host-to-host: set_problem (not timed), then the timed association
call and the timed optimize(0, 20), each run from the same initial state, so
every run does the same work. After ``--warmup`` runs, ``--reps`` timed runs;
the line reports their median with the smallest and largest as the spread.

``--libs A.so B.so`` is the interleaved A/B: for each of ``--rounds`` rounds,
every (library, configuration) runs in a fresh child process in turn
(SQLM_LIB_PATH selects the build); a library without
sqlm_set_lidar_from_cloud_sets runs the flat configuration only. Every line
names the commit, the library, the pair counts and the per-run times.

Prints one JSON line per (round, library, configuration); needs a GPU (there is
no fallback).
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sqrtlm-slam_amd"), ROOT]

N_MAP_KF, N_PTS, N_QUERY = 20, 2000, 2000
CONFIGS = ("flat", "flat+corner")


def commit() -> str:
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:  # noqa: BLE001  (an exported tree has no .git)
        return os.environ.get("SQLM_COMMIT", "unknown")


def child(a) -> int:
    import numpy as np
    from sqrtlm import lidar, synth
    from sqrtlm._lib import lib
    from sqrtlm.optimizer import Context

    prob = synth.config2()
    free = np.nonzero(prob.pose_fixed == 0)[0]
    kfs = np.r_[free[-1], free[-1 - N_MAP_KF:-1]].astype(np.int32)     # the newest keyframe is the current one
    counts = [N_QUERY] + [N_PTS] * N_MAP_KF
    clouds = synth.make_lidar_clouds(prob.pose_q[kfs], prob.pose_t[kfs], kfs, n_points=counts, current=0, seed=2,
                                     noise=0.02, extent=6.0, dist_sq_threshold=0.04)
    have_sets = hasattr(lib(), "sqlm_set_lidar_from_cloud_sets")
    if a.config == "flat+corner":
        if not have_sets:
            return 0
        clouds.corner_xyz = lidar.make_corner_clouds(prob.pose_q[kfs], prob.pose_t[kfs], n_points=counts, seed=3,
                                                     noise=0.05, extent=6.0)
        clouds.__post_init__()
    cur = int(clouds.pose_index[clouds.current])
    Twc = [lidar.Twc_f32(prob.pose_q[p], prob.pose_t[p]) for p in clouds.pose_index]
    oth = clouds.others
    mT = np.stack([Twc[k] for k in oth])
    t_assoc, t_opt, pairs, iters = [], [], None, None
    with Context(0) as ctx:
        for r in range(a.warmup + a.reps):
            ctx.set_problem(prob)
            t0 = time.perf_counter()
            if a.config == "flat":
                n = [ctx.set_lidar_from_clouds(cur, [clouds.xyz[k] for k in oth], mT, clouds.query_xyz, Twc[0],
                                               clouds.query_normal, clouds.weight, clouds.dist_sq_threshold), 0]
            else:
                n = ctx.set_lidar_from_cloud_sets(cur, clouds.cloud_sets(Twc))
            t1 = time.perf_counter()
            n_it, st = ctx.optimize(0, 20)
            t2 = time.perf_counter()
            if r >= a.warmup:
                t_assoc.append((t1 - t0) * 1e3)
                t_opt.append((t2 - t1) * 1e3)
            assert pairs in (None, n), (pairs, n)
            pairs, iters = n, n_it
    tot = np.array(t_assoc) + np.array(t_opt)
    rec = dict(commit=a.commit, lib=os.path.basename(os.environ.get("SQLM_LIB_PATH", "libsqrtlm.so")), config=a.config,
               round=a.round, workload="config 2, pass 3", map=f"{N_MAP_KF}x{N_PTS}", queries=N_QUERY,
               flat_pairs=int(pairs[0]), corner_pairs=int(pairs[1]), iterations=int(iters),
               n_active_edges=int(st["n_active_edges"]), ms_median=round(float(np.median(tot)), 4),
               ms_min=round(float(tot.min()), 4), ms_max=round(float(tot.max()), 4),
               ms_assoc=[round(x, 4) for x in t_assoc], ms_optimize=[round(x, 4) for x in t_opt],
               includes="association call (staging, H2D, launches, D2H, sync) + optimize(0, 20) incl. setup")
    print(json.dumps(rec), flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--libs", nargs="*", default=["libsqrtlm.so"], help="library builds under sqrtlm-slam_amd/sqrtlm/")
    ap.add_argument("--rounds", type=int, default=3, help="interleaved rounds over (library, configuration)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10, help="timed runs per child")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--config", choices=CONFIGS, default=None, help=argparse.SUPPRESS)   # set for a child
    ap.add_argument("--round", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--commit", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.config is not None:
        return child(a)
    sha, lines = commit(), []
    for rnd in range(a.rounds):
        for lib_name in a.libs:
            for cfg in CONFIGS:
                env = dict(os.environ, SQLM_LIB_PATH=os.path.join(ROOT, "sqrtlm-slam_amd", "sqrtlm", lib_name))
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--config", cfg, "--round", str(rnd),
                                      "--commit", sha, "--warmup", str(a.warmup), "--reps", str(a.reps)], env=env,
                                     capture_output=True, text=True, timeout=300)
                if out.returncode != 0:   # a failed child ends the run: nothing more is started on the GPU
                    sys.stderr.write(out.stdout + out.stderr)
                    return 1
                for ln in out.stdout.splitlines():
                    if ln.startswith("{"):
                        lines.append(ln)
                        print(ln, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
