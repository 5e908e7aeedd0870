#!/usr/bin/env python3
"""Time sqlm_lidar_associate (the LiDAR association of local-BA pass 3 as a brute-force 1-NN) on an MI355X.

A call is host-to-host: staging, upload, the transform / search / emit
launches, download and the stream synchronisation inside the entry point,
timed with the host clock around it (the method of scripts/pose_bench.py:
warm-up, then ``--reps`` windows of ``--calls`` calls; the report is the median
window with the smallest and largest as the spread). Shapes are (map clouds x
points each, queries); the two largest also run with SQLM_LIDAR_SPLIT=1 (one
map segment). The sizes are estimates of a LOAM-style local window: no capture
holds clouds.

Beside each, the same box's CPU time for scipy.spatial.cKDTree build + query
on the transformed float clouds: a STAND-IN for the PCL / FLANN kd-tree the
reference builds on every call, which is not installed here. Every shape's
result is also compared bit for bit with the numpy reference tests/lidar_ref.py.

Prints one JSON line per shape; needs a GPU (there is no fallback).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sqrtlm-slam_amd"), ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import lidar_ref  # noqa: E402
from sqrtlm import lidar  # noqa: E402
from sqrtlm._lib import check, lib, ptr  # noqa: E402
from sqrtlm.optimizer import Context  # noqa: E402

# map clouds, points per cloud, queries, SQLM_LIDAR_SPLIT (None = default)
SHAPES = [(4, 300, 200, None), (20, 2000, 2000, None), (20, 5000, 5000, None), (20, 5000, 5000, 1),
          (50, 5000, 5000, None), (50, 5000, 5000, 1)]
THR = 0.04


def scene(n_clouds, n_pts, n_query, seed):
    """A planar scene seen from keyframes 0.2 m apart along z; the last one is the current keyframe."""
    K = n_clouds + 1
    q = np.tile([0.0, 0.0, 0.0, 1.0], (K, 1))
    t = np.zeros((K, 3))
    t[:, 2] = -0.2 * np.arange(K)
    c = lidar.make_planar_clouds(q, t, np.arange(K), n_points=[n_pts] * n_clouds + [n_query], current=K - 1, seed=seed,
                                 extent=15.0, dist_sq_threshold=THR)
    Twc = [lidar.Twc_f32(q[k], t[k]) for k in range(K)]
    return c, Twc


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    ap.add_argument("--reps", type=int, default=7, help="timed windows per shape")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    from scipy.spatial import cKDTree
    lines, refs = [], {}
    with Context(0) as ctx:
        for n_clouds, n_pts, n_query, split in SHAPES:
            os.environ.pop("SQLM_LIDAR_SPLIT", None)  # the library reads the knob at every call
            if split is not None:
                os.environ["SQLM_LIDAR_SPLIT"] = str(split)
            c, Twc = scene(n_clouds, n_pts, n_query, seed=n_clouds + n_pts)
            clouds = [c.xyz[k] for k in c.others]
            mT = np.stack([Twc[k] for k in c.others])
            key = (n_clouds, n_pts, n_query)
            if key not in refs:
                refs.clear()  # one at a time: the largest holds a quarter of a million points
                refs[key] = lidar_ref.associate(clouds, mT, c.query_xyz, Twc[c.current], THR)
            ref = refs[key]
            got = ctx.lidar_associate(clouds, mT, c.query_xyz, Twc[c.current], THR)
            same = all(np.array_equal(g, ref[k]) for g, k in zip(got, ("nn_index", "nn_sq_dist", "nn_xyz", "accepted")))
            info = ctx.lidar_exec_info()
            # the timed loop calls the C entry point on arrays packed once
            off, mxyz = lidar.pack_clouds(clouds)
            mTf = np.ascontiguousarray(mT, np.float32).reshape(-1, 16)
            qxyz, qT = c.query_xyz, np.ascontiguousarray(Twc[c.current], np.float32).reshape(16)
            idx, d2 = np.zeros(n_query, np.int32), np.zeros(n_query, np.float32)
            xyz, acc, npairs = np.zeros((n_query, 3), np.float32), np.zeros(n_query, np.uint8), C.c_int64(0)
            args = (ctx._h, n_clouds, ptr(off), ptr(mxyz), ptr(mTf), n_query, ptr(qxyz), ptr(qT), THR, ptr(idx), ptr(d2),
                    ptr(xyz), ptr(acc), C.addressof(npairs))
            fn = lib().sqlm_lidar_associate
            for _ in range(a.warmup):
                check(fn(*args), "sqlm_lidar_associate")
            same = same and np.array_equal(idx, ref["nn_index"]) and npairs.value == ref["n_pairs"]
            win = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    fn(*args)
                win.append((time.perf_counter() - t0) / a.calls * 1e3)
            win = np.sort(np.array(win))
            # the stand-in for PCL / FLANN: tree build + one query per flat point, on the float world clouds
            mw, qw = ref["map_w"], ref["query_w"]
            cpu = []
            for _ in range(5):
                t0 = time.perf_counter()
                d_tree, _ = cKDTree(mw).query(qw, k=1)
                cpu.append((time.perf_counter() - t0) * 1e3)
            rec = dict(shape=f"{n_clouds}x{n_pts}+{n_query}", n_map=n_clouds * n_pts, n_query=n_query,
                       split="default" if split is None else split, segments=info["segments"],
                       map_tile=info["map_tile"], query_tile=info["query_tile"], n_pairs=int(npairs.value),
                       bit_equal_to_reference=bool(same), ms_per_call=round(float(np.median(win)), 4),
                       ms_min=round(float(win[0]), 4), ms_max=round(float(win[-1]), 4), calls=a.calls, reps=a.reps,
                       includes="host staging, H2D, 3 launches, D2H, sync",
                       cpu_ckdtree_build_query_ms=round(float(np.median(cpu)), 3),
                       cpu_ckdtree_min_ms=round(float(min(cpu)), 3), cpu_ckdtree_max_ms=round(float(max(cpu)), 3),
                       cpu_note="scipy.spatial.cKDTree, a stand-in for PCL KdTreeFLANN (absent here); sizes are estimates")
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    os.environ.pop("SQLM_LIDAR_SPLIT", None)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
