#!/usr/bin/env python3
"""Time sqlm_sim3_ransac (the batched GPU Sim3Solver) on an MI355X.

A call is host-to-host: argument checks, staging, upload, the single
k_sim3_ransac launch, download, the stream synchronisation and the host scan
inside sqlm_sim3_ransac, timed with the host clock around it (the call returns
only after the synchronise). For each shape (problems x pairs x hypotheses per
problem) the shape is warmed up, then timed in ``--reps`` windows of
``--calls`` calls each; the report is the median window (us per call, per
problem and per hypothesis) with the smallest and largest window as the
spread. Shapes: one candidate (1x100x300) and LoopClosing's several candidates
at once (8x150x300), every hypothesis the reference's
SetRansacParameters(0.99, 20, 300) allows.

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

from sqrtlm import sim3  # noqa: E402
from sqrtlm._lib import check, lib, ptr  # noqa: E402
from sqrtlm.optimizer import Context  # noqa: E402

SHAPES = [(1, 100, 300), (8, 150, 300)]
MIN_INLIERS = 20
ORDER = ("intr1", "intr2", "fix_scale", "min_inliers", "pair_off", "X1c", "X2c", "max_err1", "max_err2", "hyp_off",
         "draws")


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--calls", type=int, default=200, help="calls per timed window")
    ap.add_argument("--reps", type=int, default=9, help="timed windows per shape")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    lines = []
    with Context(0) as ctx:
        for n_prob, n_pair, n_hyp in SHAPES:
            gen = [sim3.make_sim3_ransac_problem(n_pair, seed=100 + k, point_noise=0.005) for k in range(n_prob)]
            probs, errs = [g[0] for g in gen], [(g[1], g[2]) for g in gen]
            assert sim3.ransac_max_its(n_pair, 0.99, MIN_INLIERS, 300) == n_hyp
            rng = np.random.default_rng(n_prob)
            draws = [np.stack([rng.integers(0, n_pair - i, n_hyp) for i in range(3)], axis=1) for _ in range(n_prob)]
            res = ctx.sim3_ransac(probs, draws, errs, MIN_INLIERS)
            # the timed loop calls the C entry point on arrays packed once
            b = sim3.pack_ransac(probs, errs, draws, MIN_INLIERS)
            H = n_prob * n_hyp
            n_in, flags = np.zeros(H, np.int32), np.zeros(H, np.uint8)
            R, t, s = np.zeros((H, 9), np.float32), np.zeros((H, 3), np.float32), np.zeros(H, np.float32)
            first, best = np.zeros(n_prob, np.int32), np.zeros(n_prob, np.int32)
            args = (ctx._h, n_prob, *[ptr(b[k]) for k in ORDER], ptr(n_in), ptr(flags), ptr(R), ptr(t), ptr(s),
                    ptr(first), ptr(best))
            fn = lib().sqlm_sim3_ransac
            for _ in range(a.warmup):
                check(fn(*args), "sqlm_sim3_ransac")
            assert np.array_equal(n_in, np.concatenate([r["n_inliers"] for r in res]))
            assert first.tolist() == [r["first_return"] for r in res]
            win = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    fn(*args)
                win.append((time.perf_counter() - t0) / a.calls * 1e6)
            win = np.sort(np.array(win))
            med = float(np.median(win))
            rec = dict(shape=f"{n_prob}x{n_pair}x{n_hyp}", n_prob=n_prob, pairs=n_pair, hypotheses=n_hyp,
                       us_per_call=round(med, 2), us_per_problem=round(med / n_prob, 2),
                       ns_per_hypothesis=round(1e3 * med / H, 1), us_min=round(float(win[0]), 2),
                       us_max=round(float(win[-1]), 2), calls=a.calls, reps=a.reps,
                       first_return_mean=round(float(np.mean(first)), 1),
                       returning=int(np.sum(first >= 0)),
                       includes="argument checks, host staging, H2D, kernel, D2H, sync, host scan")
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
