#!/usr/bin/env python3
"""Time sqlm_lidar_features on an MI355X beside its single-thread host twin.

A call is host-to-host: argument checks, staging, the upload of the sweep, the
seven kernels, the read-back of the offsets, then of the packed clouds, timed
with the host clock around it on arrays packed once. Shapes: one generated
64 x 1800 sweep of about 113k points, and a batch of 8 such sweeps in one call.

The two sides are interleaved: each of ``--reps`` rounds times a window of
``--calls`` GPU calls and then one call of sqlm_lidar_features_host (the
library's own text on one CPU thread), so that both see the same machine state.
The report is the median round of each with the smallest and largest as the
spread. The host twin is not the reference's code (PCL, Eigen), which was not
measured; neither was the adapter's packing of the PCL cloud.

Prints one JSON line per shape and writes them to
profiles/lidar/lidar_feat_bench.jsonl (``--out``); needs a GPU.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sqrtlm-slam_amd"), ROOT]

import numpy as np  # noqa: E402

from sqrtlm import lidar_feat as LF  # noqa: E402
from sqrtlm._lib import check, lib, ptr  # noqa: E402
from sqrtlm.optimizer import Context  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="GPU calls per timed window")
    ap.add_argument("--reps", type=int, default=7, help="interleaved rounds per shape")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lidar", "lidar_feat_bench.jsonl"),
                    help="also write the JSON lines to this file")
    a = ap.parse_args()
    L = lib()
    P = LF.Params()
    pc = P.as_c()
    lines = []
    with Context(0) as ctx:
        for n_sweep in (1, 8):
            sweeps = [LF.make_sweep(100 + k, n_az=1800, order="azimuth", start_deg=17.0 * k) for k in range(n_sweep)]
            off, xyz = LF._pack(sweeps)
            n = int(off[-1])
            dev, host = LF._outputs(n_sweep, n), LF._outputs(n_sweep, n)
            keys = ("flat_off", "flat_xyz", "flat_normal", "less_off", "less_xyz", "less_normal", "less_rc")
            head = (n_sweep, ptr(off), ptr(xyz), C.addressof(pc), None)
            gpu_args = (ctx._h,) + head + tuple(ptr(dev[k]) for k in keys)
            cpu_args = head + tuple(ptr(host[k]) for k in keys) + (None,)
            for _ in range(a.warmup):
                check(L.sqlm_lidar_features(*gpu_args), "sqlm_lidar_features")
            gpu_us, cpu_us = [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    L.sqlm_lidar_features(*gpu_args)
                gpu_us.append((time.perf_counter() - t0) / a.calls * 1e6)
                t0 = time.perf_counter()
                check(L.sqlm_lidar_features_host(*cpu_args), "sqlm_lidar_features_host")
                cpu_us.append((time.perf_counter() - t0) * 1e6)
            assert all(np.array_equal(dev[k].view(np.uint32) if dev[k].dtype == np.float32 else dev[k],
                                      host[k].view(np.uint32) if host[k].dtype == np.float32 else host[k])
                       for k in keys), "the device and the host twin differ"
            info = LF.features_info(ctx)
            gpu_us, cpu_us = np.sort(gpu_us), np.sort(cpu_us)
            g, c = float(np.median(gpu_us)), float(np.median(cpu_us))
            rec = dict(call="sqlm_lidar_features", shape=f"{n_sweep} x (64 x 1800)", sweeps=n_sweep, points=n,
                       less_flat=int(dev["less_off"][-1]), flat=int(dev["flat_off"][-1]),
                       candidates=info["candidates"], evaluated=info["evaluated"], launches=info["launches"],
                       us_per_call=round(g, 1), us_per_sweep=round(g / n_sweep, 1), us_min=round(float(gpu_us[0]), 1),
                       us_max=round(float(gpu_us[-1]), 1), calls=a.calls, reps=a.reps,
                       cpu_host_text_us=round(c, 1), cpu_us_min=round(float(cpu_us[0]), 1),
                       cpu_us_max=round(float(cpu_us[-1]), 1), gpu_over_cpu=round(g / c, 3),
                       cpu_note="one thread, the library's own text, interleaved with the GPU windows; not the reference",
                       includes="argument checks, staging, H2D, 7 kernels, D2H of offsets then clouds, 2 syncs")
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
