#!/usr/bin/env python3
"""Time sqlm_pnp_ransac (the batched GPU PnPsolver) on an MI355X.

A call is host-to-host: argument checks, staging, upload, k_pnp_hyp, the
download of the counts, the host scan for the record-breaking hypotheses, the
upload of their table, k_pnp_refine, the download, the second synchronisation
and the final scan, timed with the host clock around it. For each shape
(problems x pairs x hypotheses per problem) the shape is warmed up, then timed
in ``--reps`` windows of ``--calls`` calls each; the report is the median window
with the smallest and largest window as the spread. Shapes: one candidate
(1x100x300) and Relocalization's several candidates at once (8x150x300).

Beside each shape the same work is timed once on one CPU thread through
sqlm_pnp_ransac_hypothesis_host / _refine_host: every hypothesis, and the refine
of every record-breaking one. That CPU figure is the library's own text compiled
for the host, not the reference's PnPsolver, which needs OpenCV.

Prints one JSON line per shape and writes them to profiles/pnp/pnp_bench.jsonl
(``--out``); needs a GPU (there is no fallback).
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

from sqrtlm import pnp  # noqa: E402
from sqrtlm._lib import check, lib, ptr  # noqa: E402
from sqrtlm.optimizer import Context  # noqa: E402

SHAPES = [(1, 100, 300), (8, 150, 300)]
MIN_INLIERS = 20
ORDER = ("intr", "min_inliers", "pair_off", "Xw", "uv", "max_err", "hyp_off", "draws")


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--calls", type=int, default=100, help="calls per timed window")
    ap.add_argument("--reps", type=int, default=9, help="timed windows per shape")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pnp", "pnp_bench.jsonl"),
                    help="also write the JSON lines to this file")
    a = ap.parse_args()
    lines = []
    with Context(0) as ctx:
        for n_prob, n_pair, n_hyp in SHAPES:
            probs = [pnp.make_pnp_problem(n_pair, seed=100 + k) for k in range(n_prob)]
            rng = np.random.default_rng(n_prob)
            draws = [pnp.draw(rng, n_pair, n_hyp) for _ in range(n_prob)]
            res = ctx.pnp_ransac(probs, draws, MIN_INLIERS)
            # the timed loop calls the C entry point on arrays packed once
            b = pnp.pack(probs, draws, MIN_INLIERS)
            H = n_prob * n_hyp
            n_in, flags = np.zeros(H, np.int32), np.zeros(H, np.uint8)
            R, t = np.zeros((H, 9)), np.zeros((H, 3))
            first, best, n_ref = np.zeros(n_prob, np.int32), np.zeros(n_prob, np.int32), np.zeros(n_prob, np.int32)
            Tcw = np.zeros((n_prob, 16), np.float32)
            args = (ctx._h, n_prob, *[ptr(b[k]) for k in ORDER], ptr(n_in), ptr(flags), ptr(R), ptr(t), ptr(first),
                    ptr(best), ptr(Tcw), ptr(n_ref))
            fn = lib().sqlm_pnp_ransac
            for _ in range(a.warmup):
                check(fn(*args), "sqlm_pnp_ransac")
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
            # the same work on one CPU thread, from the same source text
            records = 0
            t0 = time.perf_counter()
            for p, d, r in zip(probs, draws, res):
                masks = {}
                for h in range(n_hyp):
                    o = pnp.hypothesis_host(p, d[h])
                    if r["flags"][h] & 2:
                        masks[h] = o["mask"]
                for m in masks.values():
                    pnp.refine_host(p, m)
                records += len(masks)
            cpu_us = (time.perf_counter() - t0) * 1e6
            rec = dict(shape=f"{n_prob}x{n_pair}x{n_hyp}", n_prob=n_prob, pairs=n_pair, hypotheses=n_hyp,
                       us_per_call=round(med, 2), us_per_problem=round(med / n_prob, 2),
                       ns_per_hypothesis=round(1e3 * med / H, 1), us_min=round(float(win[0]), 2),
                       us_max=round(float(win[-1]), 2), calls=a.calls, reps=a.reps, records=records,
                       returning=int(np.sum(first >= 0)),
                       cpu_host_text_us=round(cpu_us, 1),
                       cpu_note="one run, one thread, the library's own text through ctypes; not the reference",
                       includes="argument checks, staging, H2D, k_pnp_hyp, D2H counts, sync, host scan, H2D records, "
                                "k_pnp_refine, D2H, sync, final scan")
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
