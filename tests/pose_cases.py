"""The motion-only-BA cases shared by tests/test_pose_ref.py (CPU: conditions on
the inputs, asserted on the numpy reference alone) and tests/test_gpu_pose.py
(GPU against that reference). Shapes are edges per problem: the fewer-than-3
rule (0, 2, 3), the fewer-than-10 break (9, 10, 11), the wavefront (63, 64, 65),
the 256-thread workgroup (255, 256, 257) and several strides (600).

The seeds were chosen so that every chi2 a check reads lies outside
[th2 / 2, 2 th2] on the main cases and outside [th2 / 1.05, 1.05 th2] on the
re-entry cases (far start, one iteration in round 0: the outlier set changes
between the rounds); test_pose_ref.py asserts it. That margin is what lets the
GPU test demand identical flags.
"""
from __future__ import annotations

import numpy as np

import pose_ref as R
from sqrtlm import pose as P
from sqrtlm import synth

K2 = (700.0, 705.0, 600.0, 180.0)  # a second intrinsics set
FAR = dict(rot_pert=0.03, trans_pert=0.3)  # a far start

# name: (edges, seed, generator arguments, iters, user_lambda)
SPECS = {
    "n0": (0, 1, dict(), (10, 10, 10, 10), 0.0),
    "n2": (2, 1, dict(outlier_frac=0.0), (10, 10, 10, 10), 0.0),
    "n3": (3, 1, dict(outlier_frac=0.0), (10, 10, 10, 10), 0.0),
    "n9": (9, 1, dict(outlier_frac=0.0), (10, 10, 10, 10), 0.0),
    "n10_clean": (10, 1, dict(outlier_frac=0.0), (10, 10, 10, 10), 0.0),
    "n11_out": (11, 1, dict(outlier_frac=0.2), (10, 10, 10, 10), 0.0),
    "n63": (63, 1, dict(outlier_frac=0.2), (10, 10, 10, 10), 0.0),
    "n64_k2": (64, 1, dict(outlier_frac=0.2, intr=K2), (10, 10, 10, 10), 0.0),
    "n65_clean": (65, 1, dict(outlier_frac=0.0), (10, 10, 10, 10), 0.0),
    "n255_o35": (255, 2, dict(outlier_frac=0.35, pixel_noise=0.4), (10, 10, 10, 10), 0.0),
    "n256_k2": (256, 1, dict(outlier_frac=0.2, intr=K2), (10, 10, 10, 10), 0.0),
    "n257": (257, 1, dict(outlier_frac=0.2), (10, 10, 10, 10), 0.0),
    "n600_o35": (600, 1, dict(outlier_frac=0.35, pixel_noise=0.4), (10, 10, 10, 10), 0.0),
    # re-entry: the outlier set differs between rounds
    "n65_re": (65, 6, dict(outlier_frac=0.2, **FAR), (1, 10, 10, 10), 0.0),
    "n257_re": (257, 8, dict(outlier_frac=0.2, **FAR), (1, 10, 10, 10), 0.0),
    # a damping so large that round 0 does not move: every edge goes to level 1
    # and rounds 1-3 have no level-0 edge
    "n12_stuck": (12, 1, dict(outlier_frac=0.0, **FAR), (10, 10, 10, 10), 1e14),
}
NAMES = list(SPECS)
REENTRY = ["n65_re", "n257_re"]
MAIN = [n for n in NAMES if n not in REENTRY]

# LiDAR stage: name: (vision case, pairs, kinds, seed, outlier_in: "vision" | "all")
LIDAR_SPECS = {
    "l0": ("n63", 0, "mixed", 1, "vision"),
    "l1_flat": ("n64_k2", 1, "flat", 1, "vision"),
    "l64_corner": ("n65_clean", 64, "corner", 1, "vision"),
    "l257_mixed": ("n257", 257, "mixed", 1, "vision"),
    "l700_mixed": ("n600_o35", 700, "mixed", 1, "vision"),
    "l64_flat_robust": ("n9", 64, "flat", 1, "vision"),   # 9 mono edges: the Huber kernels stayed on
    "l64_mixed_allout": ("n11_out", 64, "mixed", 1, "all"),  # every mono edge on level 1
}
LIDAR_NAMES = list(LIDAR_SPECS)

_problems: dict = {}
_refs: dict = {}


def problem(name: str):
    """The case's problem (built once; callers must not modify it)."""
    if name not in _problems:
        n, seed, kw, _, _ = SPECS[name]
        _problems[name] = synth.make_pose_problem(n, seed=seed, **kw)
    return _problems[name]


def args(name: str):
    return SPECS[name][3], SPECS[name][4]


def reference(O, name: str, iters=None, user_lambda=None, T=np.float64):
    """pose_ref.optimize on the case (computed once, shared, left unchanged)."""
    it, lam = args(name)
    it = it if iters is None else tuple(iters)
    lam = lam if user_lambda is None else float(user_lambda)
    key = (name, it, lam, T)
    if key not in _refs:
        _refs[key] = R.optimize(O, problem(name), it, lam, T)
    return _refs[key]


def _bump(p):
    p = p.copy()
    p.pose_t[:] = np.nextafter(p.pose_t, np.inf)
    return p


def ulp_spread(O, name: str):
    """How far the reference's own result moves when the input translation is
    perturbed by one ulp: (|d pose| max, [|d chi2_end| per stage], decisions
    unchanged, [|d chi2_begin| per stage])."""
    key = (name, "ulp")
    if key not in _refs:
        ref = reference(O, name)
        r = R.optimize(O, _bump(problem(name)), *args(name))
        _refs[key] = _spread(r, ref)
    return _refs[key]


def _spread(r, ref):
    dS = float(max(np.abs(r["pose_q"] - ref["pose_q"]).max(), np.abs(r["pose_t"] - ref["pose_t"]).max()))
    dchi = [0.0 if a is None else abs(float(a["chi2_end"]) - float(b["chi2_end"]))
            for a, b in zip(r["stats"], ref["stats"])]
    same = (np.array_equal(r["outlier"], ref["outlier"]) and r["n_inliers"] == ref["n_inliers"]
            and r["n_bad"] == ref["n_bad"] and r["rounds"] == ref["rounds"]
            and all(np.array_equal(a, b) for a, b in zip(r["levels"], ref["levels"])))
    dbeg = [0.0 if a is None else abs(float(a["chi2_begin"]) - float(b["chi2_begin"]))
            for a, b in zip(r["stats"], ref["stats"])]
    return dS, dchi, same, dbeg


def lidar_problem(O, name: str):
    """(problem with the stage's start pose, LidarPairs, outlier_in, robust_on)
    of a LiDAR case: the start is the vision reference's pose after SetPose's
    float round trip, the level-1 edges are the vision reference's flags."""
    key = ("lidar", name)
    if key not in _problems:
        base, m, kinds, seed, which = LIDAR_SPECS[name]
        p, ref = problem(base), reference(O, base)
        sub = p.copy()
        q, t = O.se3_from_Tcw_f32(O.se3_to_Tcw_f32(ref["pose_q"], ref["pose_t"]))
        sub.pose_q[:], sub.pose_t[:] = q, t
        L = P.make_lidar_pairs(p, m, seed=seed, kinds=kinds)
        oin = ref["outlier"].copy() if which == "vision" else np.ones(p.n_obs, bool)
        _problems[key] = (sub, L, oin, p.n_obs < 10)
    return _problems[key]


def lidar_reference(O, name: str, iters=10, user_lambda=0.0, T=np.float64):
    key = ("lidar", name, int(iters), float(user_lambda), T)
    if key not in _refs:
        sub, L, oin, rob = lidar_problem(O, name)
        _refs[key] = R.refine(O, sub, L, oin, rob, iters, user_lambda, T)
    return _refs[key]


def lidar_ulp_spread(O, name: str):
    key = ("lidar", name, "ulp")
    if key not in _refs:
        sub, L, oin, rob = lidar_problem(O, name)
        _refs[key] = _spread(R.refine(O, _bump(sub), L, oin, rob), lidar_reference(O, name))
    return _refs[key]
