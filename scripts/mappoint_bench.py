#!/usr/bin/env python3
"""Time sqlm_triangulate_pairs and sqlm_map_points_update on an MI355X.

A call is host-to-host: argument checks, the gather / staging, the upload, the
kernels (k_triangulate; k_mp_descriptor and k_mp_normal), the download and the
synchronisation, timed with the host clock around it on arrays packed once.
The method is scripts/pnp_bench.py's: each shape is warmed up, then timed in
``--reps`` windows of ``--calls`` calls each; the report is the median window
with the smallest and largest window as the spread. Shapes: LocalMapping's
per-keyframe work, 20 neighbours x 300 matches in one call and 1 x 300 (the
reference's call per neighbour); 1500 map points with 2 to 60 observations,
and the same with one track of 400 (the global-memory path).

Beside each figure the host twin (the same text on one CPU thread) is timed
once. That is the library's own text compiled for the host, not the
reference's OpenCV code, which was not measured; neither was the adapter's
gathering of KeyFrame / MapPoint fields, nor any end-to-end LocalMapping run.

Prints one JSON line per shape and writes them to
profiles/mappoint/mappoint_bench.jsonl (``--out``); needs a GPU.
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

from sqrtlm import mappoint as M  # noqa: E402
from sqrtlm._lib import check, lib, ptr  # noqa: E402
from sqrtlm.optimizer import Context  # noqa: E402


def _windows(fn, args, what, a):
    for _ in range(a.warmup):
        check(fn(*args), what)
    win = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        for _ in range(a.calls):
            fn(*args)
        win.append((time.perf_counter() - t0) / a.calls * 1e6)
    return np.sort(np.array(win))


def _once(fn, args, what):
    t0 = time.perf_counter()
    check(fn(*args), what)
    return (time.perf_counter() - t0) * 1e6


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--calls", type=int, default=100, help="calls per timed window")
    ap.add_argument("--reps", type=int, default=9, help="timed windows per shape")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mappoint", "mappoint_bench.jsonl"),
                    help="also write the JSON lines to this file")
    a = ap.parse_args()
    lines = []
    L = lib()
    with Context(0) as ctx:
        for n_pair, n_match in ((20, 300), (1, 300)):
            pairs = [M.make_two_view(n_match, seed=10 + k) for k in range(n_pair)]
            arr, off, m = M._pack_pairs(pairs)
            n = int(off[-1])
            x, r, nn = np.zeros((n, 3), np.float32), np.zeros(n, np.uint8), np.zeros(n_pair, np.int32)
            out = (ptr(x), ptr(r), ptr(nn))
            win = _windows(L.sqlm_triangulate_pairs, (ctx._h, n_pair, arr, ptr(off), ptr(m)) + out,
                           "sqlm_triangulate_pairs", a)
            gpu = (x.copy(), r.copy())
            cpu = _once(L.sqlm_triangulate_pairs_host, (n_pair, arr, ptr(off), ptr(m), 0) + out,
                        "sqlm_triangulate_pairs_host")
            assert np.array_equal(gpu[0], x) and np.array_equal(gpu[1], r)
            med = float(np.median(win))
            rec = dict(call="sqlm_triangulate_pairs", shape=f"{n_pair}x{n_match}", pairs=n_pair, matches=n,
                       created=int(nn.sum()), us_per_call=round(med, 2), ns_per_match=round(1e3 * med / n, 1),
                       us_min=round(float(win[0]), 2), us_max=round(float(win[-1]), 2), calls=a.calls, reps=a.reps,
                       cpu_host_text_us=round(cpu, 1),
                       cpu_note="one run, one thread, the library's own text; not the reference",
                       includes="argument checks, gather, H2D, k_triangulate, D2H, sync, per-pair counts")
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
        rng = np.random.default_rng(3)
        for what, counts in (("1500 x N in 2..60", rng.integers(2, 61, 1500).tolist()),
                             ("1499 x N in 2..60 + 1 x 400", rng.integers(2, 61, 1499).tolist() + [400])):
            b = M.make_tracks(counts, seed=4)
            n = b.n_pt
            o = [np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, 3), np.float32), np.zeros(n, np.float32),
                 np.zeros(n, np.float32)]
            ins = (n, ptr(b.obs_off), ptr(b.obs_desc), ptr(b.obs_center), ptr(b.pos), ptr(b.ref_center),
                   ptr(b.level_scale), ptr(b.max_scale)) + tuple(ptr(v) for v in o)
            win = _windows(L.sqlm_map_points_update, (ctx._h,) + ins, "sqlm_map_points_update", a)
            gpu = [v.copy() for v in o]
            info = M.map_points_update_info(ctx)
            cpu = _once(L.sqlm_map_points_update_host, ins, "sqlm_map_points_update_host")
            assert all(np.array_equal(g, v, equal_nan=(v.dtype.kind == "f")) for g, v in zip(gpu, o))
            med = float(np.median(win))
            rec = dict(call="sqlm_map_points_update", shape=what, points=n, observations=int(b.obs_off[-1]),
                       lds_points=info["n_lds"], global_points=info["n_global"], us_per_call=round(med, 2),
                       ns_per_point=round(1e3 * med / n, 1), us_min=round(float(win[0]), 2),
                       us_max=round(float(win[-1]), 2), calls=a.calls, reps=a.reps, cpu_host_text_us=round(cpu, 1),
                       cpu_note="one run, one thread, the library's own text; not the reference",
                       includes="argument checks, staging, H2D, k_mp_descriptor, k_mp_normal, D2H, sync")
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
