#!/usr/bin/env python3
"""Time sqlm_sim3_optimize (the batched GPU OptimizeSim3) on an MI355X.

A call is host-to-host: staging, upload, the single k_sim3 launch, download and
the stream synchronisation inside sqlm_sim3_optimize, timed with the host clock
around it (the call returns only after the synchronise). For each shape
(problems x pairs per problem) the shape is warmed up, then timed in ``--reps``
windows of ``--calls`` calls each; the report is the median window (us per call
and per problem) with the smallest and largest window as the spread. Shapes:
one alignment (1x100, 1x300: latency-bound on one CU, one workgroup per
problem) and batches (16x150, 64x150) that show what the batch buys.

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

from sqrtlm import sim3, synth  # noqa: E402
from sqrtlm._lib import check, lib, ptr  # noqa: E402
from sqrtlm.optimizer import Context  # noqa: E402

SHAPES = [(1, 100), (1, 300), (16, 150), (64, 150)]


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--calls", type=int, default=200, help="calls per timed window")
    ap.add_argument("--reps", type=int, default=9, help="timed windows per shape")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    lines = []
    with Context(0) as ctx:
        for n_prob, n_pair in SHAPES:
            probs = [synth.make_sim3_problem(n_pair, seed=100 + k) for k in range(n_prob)]
            S, n_in, state, st = ctx.sim3_optimize(probs)
            # the timed loop calls the C entry point on arrays packed once
            b = sim3.pack(probs)
            S2, n2, state2 = np.zeros_like(S), np.zeros_like(n_in), np.zeros_like(state)
            args = (ctx._h, n_prob, ptr(b["S12"]), ptr(b["intr1"]), ptr(b["intr2"]), ptr(b["fix_scale"]), ptr(b["th2"]),
                    ptr(b["pair_off"]), ptr(b["X1c"]), ptr(b["X2c"]), ptr(b["obs1"]), ptr(b["obs2"]), ptr(b["info1"]),
                    ptr(b["info2"]), None, C.c_double(0.0), ptr(S2), ptr(n2), ptr(state2), None)
            fn = lib().sqlm_sim3_optimize
            for _ in range(a.warmup):
                check(fn(*args), "sqlm_sim3_optimize")
            assert np.array_equal(S, S2) and np.array_equal(state, state2)
            win = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    fn(*args)
                win.append((time.perf_counter() - t0) / a.calls * 1e6)
            win = np.sort(np.array(win))
            med = float(np.median(win))
            rec = dict(shape=f"{n_prob}x{n_pair}", n_prob=n_prob, pairs=n_pair, us_per_call=round(med, 2),
                       us_per_problem=round(med / n_prob, 2), us_min=round(float(win[0]), 2),
                       us_max=round(float(win[-1]), 2), calls=a.calls, reps=a.reps,
                       trials_per_problem=round(float(np.mean([sum(s["trials"]) for s in st])), 2),
                       inliers_mean=round(float(np.mean(n_in)), 1), includes="host staging, H2D, kernel, D2H, sync")
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
