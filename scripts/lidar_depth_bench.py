#!/usr/bin/env python3
"""Time sqlm_lidar_depth on an MI355X beside its single-thread host twin.

A call is host-to-host: argument checks, staging, the upload of the sweep and
the keypoints, the three kernels, the read-back of the packed outputs and (in
the ``image`` rows) of the double depth image, timed with the host clock around
it on arrays packed once. Shapes: one 376 x 1241 frame with one generated
64 x 1800 sweep of about 113k points and 2000 keypoints, and a batch of 8 such
frames in one call; each with and without the download of the depth image.

The two sides are interleaved: each of ``--reps`` rounds times a window of
``--calls`` GPU calls and then one call of sqlm_lidar_depth_host (the library's
own text on one CPU thread), so that both see the same machine state. The report
is the median round of each with the smallest and largest as the spread. The
host twin is not the reference's code (Eigen, OpenCV), which was not measured;
neither were the kernels one by one, the transfers' share of a call, or the
adapter's packing of the PCL cloud and the keypoints.

Prints one JSON line per shape and writes them to
profiles/lidar/lidar_depth_bench.jsonl (``--out``); needs a GPU.
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

from sqrtlm import lidar_depth as LD  # noqa: E402
from sqrtlm import lidar_feat as LF  # noqa: E402
from sqrtlm._lib import check, lib  # noqa: E402
from sqrtlm.optimizer import Context  # noqa: E402

KEYS = ("class_id", "depth", "nearest_uv", "xyz_cam", "stats", "image")


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else (a.view(np.uint64) if a.dtype == np.float64 else a)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="GPU calls per timed window")
    ap.add_argument("--reps", type=int, default=7, help="interleaved rounds per shape")
    ap.add_argument("--keypoints", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lidar", "lidar_depth_bench.jsonl"),
                    help="also write the JSON lines to this file")
    a = ap.parse_args()
    L = lib()
    rows, cols = LD.KITTI_ROWS, LD.KITTI_COLS
    lines = []
    with Context(0) as ctx:
        for n_frame in (1, 8):
            sweeps = [LF.make_sweep(100 + k, n_az=1800, order="azimuth", start_deg=17.0 * k) for k in range(n_frame)]
            keys = [LD.make_keypoints(200 + k, a.keypoints) for k in range(n_frame)]
            un = [(k + np.float32(0.25)).astype(np.float32) for k in keys]
            for image in (False, True):
                dev = LD._args(sweeps, keys, un, rows, cols, LD.KITTI_INTRINSIC, LD.VELO_TO_CAM, LD.KITTI_CAM, image)
                host = LD._args(sweeps, keys, un, rows, cols, LD.KITTI_INTRINSIC, LD.VELO_TO_CAM, LD.KITTI_CAM, image)
                gpu_args = (ctx._h,) + tuple(LD._call_args(dev))
                cpu_args = tuple(LD._call_args(host)) + (None, None)
                for _ in range(a.warmup):
                    check(L.sqlm_lidar_depth(*gpu_args), "sqlm_lidar_depth")
                gpu_us, cpu_us = [], []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    for _ in range(a.calls):
                        L.sqlm_lidar_depth(*gpu_args)
                    gpu_us.append((time.perf_counter() - t0) / a.calls * 1e6)
                    t0 = time.perf_counter()
                    check(L.sqlm_lidar_depth_host(*cpu_args), "sqlm_lidar_depth_host")
                    cpu_us.append((time.perf_counter() - t0) * 1e6)
                assert all(np.array_equal(_bits(dev[k]), _bits(host[k])) for k in KEYS if dev[k] is not None), \
                    "the device and the host twin differ"
                info = LD.depth_info(ctx)
                gpu_us, cpu_us = np.sort(gpu_us), np.sort(cpu_us)
                g, c = float(np.median(gpu_us)), float(np.median(cpu_us))
                st = dev["stats"]
                rec = dict(call="sqlm_lidar_depth", shape=f"{n_frame} x ({rows} x {cols}), {a.keypoints} keypoints each",
                           frames=n_frame, points=dev["n"], keypoints=dev["m"], image_download=image,
                           written=int(st[:, 1].sum()), occupied=int(st[:, 2].sum()), with_depth=int(st[:, 3].sum()),
                           launches=info["launches"], us_per_call=round(g, 1), us_per_frame=round(g / n_frame, 1),
                           us_min=round(float(gpu_us[0]), 1), us_max=round(float(gpu_us[-1]), 1), calls=a.calls,
                           reps=a.reps, cpu_host_text_us=round(c, 1), cpu_us_min=round(float(cpu_us[0]), 1),
                           cpu_us_max=round(float(cpu_us[-1]), 1), gpu_over_cpu=round(g / c, 3),
                           cpu_note="one thread, the library's own text, interleaved with the GPU windows; not the "
                                    "reference; it always fills an image",
                           includes="argument checks, staging, H2D, 3 kernels, D2H of outputs" +
                                    (" and of the double image" if image else "") + ", 1 sync")
                lines.append(json.dumps(rec))
                print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
