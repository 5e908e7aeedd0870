#!/usr/bin/env python3
"""Time sqlm_pose_optimize / sqlm_pose_refine_lidar (the batched GPU PoseOptimization) on an MI355X.

A call is host-to-host: staging, upload, the single k_pose launch, download and
the stream synchronisation inside the entry point, timed with the host clock
around it (the call returns only after the synchronise). For each shape the
shape is warmed up, then timed in ``--reps`` windows of ``--calls`` calls each;
the report is the median window (us per call and per problem) with the
smallest and largest window as the spread. Shapes: Tracking's call (1x100,
1x300, 1x1500 edges: latency-bound on one CU, one workgroup per problem), a
batch of relocalization candidates (64x300) and the LiDAR stage (1 x 300 edges
+ 1000 LiDAR pairs, from the vision call's pose and flags).

Prints one JSON line per shape; needs a GPU (there is no fallback).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sqrtlm-slam_amd"), ROOT]

import numpy as np  # noqa: E402

import ctypes as C  # noqa: E402

from sqrtlm import pose, synth  # noqa: E402
from sqrtlm._lib import check, lib, ptr  # noqa: E402
from sqrtlm.optimizer import Context, pose_from_Tcw_f32, pose_to_Tcw_f32  # noqa: E402

SHAPES = [(1, 100, 0), (1, 300, 0), (1, 1500, 0), (64, 300, 0), (1, 300, 1000)]  # problems, edges, LiDAR pairs


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--calls", type=int, default=200, help="calls per timed window")
    ap.add_argument("--reps", type=int, default=9, help="timed windows per shape")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    lines = []
    with Context(0) as ctx:
        for n_prob, n_obs, n_lid in SHAPES:
            probs = [synth.make_pose_problem(n_obs, seed=100 + k) for k in range(n_prob)]
            q, t, n_in, flag, st = ctx.pose_optimize(probs)
            stage = "vision"
            if n_lid:  # the LiDAR stage, from the vision call's result after the float round trip
                stage = "lidar"
                subs, pairs = [], []
                for k, p in enumerate(probs):
                    s = p.copy()
                    s.pose_q[:], s.pose_t[:] = pose_from_Tcw_f32(pose_to_Tcw_f32(q[k], t[k]))
                    subs.append(s)
                    pairs.append(pose.make_lidar_pairs(p, n_lid, seed=200 + k))
                oin = flag.copy()
                rob = np.array([p.n_obs < 10 for p in probs], np.uint8)
                q, t, n_in, flag, st = ctx.pose_refine_lidar(subs, pairs, oin, rob)
                b, l = pose.pack(subs), pose.pack_lidar(pairs)
            else:
                b = pose.pack(probs)
            # the timed loop calls the C entry point on arrays packed once
            q2, t2, n2, flag2 = np.zeros_like(q), np.zeros_like(t), np.zeros_like(n_in), np.zeros_like(flag)
            head = (ctx._h, n_prob, ptr(b["pose_q"]), ptr(b["pose_t"]), ptr(b["intr"]), ptr(b["obs_off"]), ptr(b["Xw"]),
                    ptr(b["uv"]), ptr(b["info"]))
            tail = (C.c_double(probs[0].th2), C.c_double(0.0), ptr(q2), ptr(t2), ptr(n2), ptr(flag2), None)
            if n_lid:
                fn, name = lib().sqlm_pose_refine_lidar, "sqlm_pose_refine_lidar"
                args = head + (ptr(oin), ptr(rob), ptr(l["lid_off"]), ptr(l["lid_kind"]), ptr(l["lid_pc"]),
                               ptr(l["lid_pw"]), ptr(l["lid_n"]), ptr(l["lid_info"]), None) + tail
            else:
                fn, name = lib().sqlm_pose_optimize, "sqlm_pose_optimize"
                args = head + (None,) + tail
            for _ in range(a.warmup):
                check(fn(*args), name)
            assert np.array_equal(q, q2) and np.array_equal(t, t2) and np.array_equal(flag, flag2)
            win = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    fn(*args)
                win.append((time.perf_counter() - t0) / a.calls * 1e6)
            win = np.sort(np.array(win))
            med = float(np.median(win))
            trials = float(np.mean([sum(s["trials"]) for s in st]))
            # edge evaluations: every trial evaluates the stage's active edges once (the linearizations add as many)
            rec = dict(shape=f"{n_prob}x{n_obs}" + (f"+{n_lid}" if n_lid else ""), stage=stage, n_prob=n_prob,
                       edges=n_obs, lidar=n_lid, us_per_call=round(med, 2), us_per_problem=round(med / n_prob, 2),
                       us_min=round(float(win[0]), 2), us_max=round(float(win[-1]), 2), calls=a.calls, reps=a.reps,
                       trials_per_problem=round(trials, 2),
                       iterations_per_problem=round(float(np.mean([sum(s["iterations"]) for s in st])), 2),
                       us_per_trial=round(med / n_prob / max(trials, 1.0), 2),
                       inliers_mean=round(float(np.mean(n_in)), 1), includes="host staging, H2D, kernel, D2H, sync")
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
