#!/usr/bin/env python3
"""Time sqlm_lidar_features_all on an MI355X, corner branch off and on, beside its host twin.

A call is host-to-host: argument checks, staging, the upload of the sweep, the
kernels (7 without the corner stage, 13 with it), the read-back of the offsets,
then of the packed clouds, timed with the host clock around it on arrays packed
once. Shapes: one generated 64 x 1800 sweep with poles (the scenery that yields
corner points), and a batch of 8 such sweeps in one call, at the shipped
parameters.

The sides are interleaved as in scripts/lidar_feat_bench.py: each of ``--reps``
rounds times a window of ``--calls`` GPU calls with the corner branch off, a
window with it on, and then one call of sqlm_lidar_features_all_host with it on
(the library's own text on one CPU thread). The report is the median round of
each with the smallest and largest as the spread. The host twin is not the
reference's code, which was not measured. What the walk kernel costs next to the
parallel stages is not in these lines: that is a kernel trace of this script.

Prints one JSON line per shape and writes them to
profiles/lidar/lidar_corner_bench.jsonl (``--out``); needs a GPU.
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

from sqrtlm import lidar_feat as LF  # noqa: E402
from sqrtlm._lib import check, lib  # noqa: E402
from sqrtlm.optimizer import Context  # noqa: E402


def _same(a, b):
    return np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                          b.view(np.uint32) if b.dtype == np.float32 else b)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10, help="GPU calls per timed window")
    ap.add_argument("--reps", type=int, default=7, help="interleaved rounds per shape")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lidar", "lidar_corner_bench.jsonl"),
                    help="also write the JSON lines to this file")
    a = ap.parse_args()
    L = lib()
    P, CP = LF.Params(), LF.CornerParams()
    lines = []
    with Context(0) as ctx:
        for n_sweep in (1, 8):
            sweeps = [LF.make_sweep(100 + k, n_az=1800, order="azimuth", start_deg=17.0 * k, n_poles=12)
                      for k in range(n_sweep)]
            _, _, n, o_off, args_off, keep_off = LF._all_args(sweeps, P, None, None, True)
            _, _, _, o_on, args_on, keep_on = LF._all_args(sweeps, P, CP, None, True)
            _, _, _, o_host, args_host, keep_host = LF._all_args(sweeps, P, CP, None, True)
            for _ in range(a.warmup):
                check(L.sqlm_lidar_features_all(ctx._h, *args_off), "sqlm_lidar_features_all")
                check(L.sqlm_lidar_features_all(ctx._h, *args_on), "sqlm_lidar_features_all")
            off_us, on_us, cpu_us = [], [], []
            for _ in range(a.reps):
                for args, acc in ((args_off, off_us), (args_on, on_us)):
                    t0 = time.perf_counter()
                    for _ in range(a.calls):
                        L.sqlm_lidar_features_all(ctx._h, *args)
                    acc.append((time.perf_counter() - t0) / a.calls * 1e6)
                t0 = time.perf_counter()
                check(L.sqlm_lidar_features_all_host(*args_host, None, None), "sqlm_lidar_features_all_host")
                cpu_us.append((time.perf_counter() - t0) * 1e6)
            assert all(_same(o_on[k], o_host[k]) for k in o_on), "the device and the host twin differ"
            assert all(_same(o_on[k], o_off[k]) for k in o_off), "the flat outputs depend on the corner branch"
            info = LF.features_all_info(ctx)
            off_us, on_us, cpu_us = np.sort(off_us), np.sort(on_us), np.sort(cpu_us)
            g0, g1, c = float(np.median(off_us)), float(np.median(on_us)), float(np.median(cpu_us))
            rec = dict(call="sqlm_lidar_features_all", shape=f"{n_sweep} x (64 x 1800)", sweeps=n_sweep, points=n,
                       sharp=info["sharp"], less_sharp=info["less_sharp"], seeds_grown=info["seeds_grown"],
                       cells_labelled=info["cells_labelled"], cells_unstable=info["cells_unstable"],
                       largest_segment=info["largest_segment"], most_levels=info["most_levels"],
                       launches=info["launches"],
                       corner_off_us=round(g0, 1), corner_off_us_min=round(float(off_us[0]), 1),
                       corner_off_us_max=round(float(off_us[-1]), 1),
                       corner_on_us=round(g1, 1), corner_on_us_min=round(float(on_us[0]), 1),
                       corner_on_us_max=round(float(on_us[-1]), 1), corner_on_us_per_sweep=round(g1 / n_sweep, 1),
                       calls=a.calls, reps=a.reps,
                       cpu_host_text_us=round(c, 1), cpu_us_min=round(float(cpu_us[0]), 1),
                       cpu_us_max=round(float(cpu_us[-1]), 1), gpu_over_cpu=round(g1 / c, 3),
                       cpu_note="one thread, the library's own text with the corner branch on, interleaved; not the reference",
                       includes="argument checks, staging, H2D, 7 / 13 kernels, D2H of offsets then clouds, 2 syncs")
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
