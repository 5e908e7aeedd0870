"""The Sim3-alignment cases shared by tests/test_sim3_ref.py (CPU: conditions on
the inputs, asserted on the numpy reference alone) and tests/test_gpu_sim3.py
(GPU against that reference). Shapes are pairs per problem: 0 and 1, the
>= 10 rule of the schedule (9, 10, 11), the wavefront (63, 64, 65), the
256-thread workgroup (255, 256, 257) and several strides (600).

The seeds were chosen so that every chi2 either threshold test reads lies
outside [th2 / 2, 2 th2] (test_sim3_ref.py asserts it); that margin is what
lets the GPU test demand identical pair states.
"""
from __future__ import annotations

import numpy as np

import sim3_ref as R
from sqrtlm import synth

K2 = (700.0, 705.0, 600.0, 180.0)  # a second camera: K1 != K2

# name: (pairs, seed, generator arguments)
SPECS = {
    "n0": (0, 3, dict()),
    "n1": (1, 3, dict(outlier_frac=0.0)),
    "n9": (9, 3, dict(outlier_frac=0.0)),
    "n10_clean": (10, 2, dict(outlier_frac=0.0)),
    "n11_out": (11, 3, dict(outlier_frac=0.3)),
    "n63_fix": (63, 3, dict(fix_scale=True)),
    "n64_k2": (64, 3, dict(intr2=K2)),
    "n65_clean": (65, 1, dict(outlier_frac=0.0, pixel_noise=0.3)),
    "n255_fix_k2": (255, 3, dict(fix_scale=True, intr2=K2)),
    "n256": (256, 3, dict()),
    "n257": (257, 3, dict(outlier_frac=0.1)),
    "n600": (600, 3, dict(pixel_noise=0.4)),
}
NAMES = list(SPECS)

_problems: dict = {}
_refs: dict = {}


def problem(name: str):
    """The case's problem (built once; callers must not modify it)."""
    if name not in _problems:
        n, seed, kw = SPECS[name]
        _problems[name] = synth.make_sim3_problem(n, seed=seed, **kw)
    return _problems[name]


def reference(O, name: str, iters=(5, 10, 5), user_lambda: float = 0.0):
    """sim3_ref.optimize in float64 on the case (computed once, shared, left unchanged)."""
    key = (name, tuple(iters), float(user_lambda))
    if key not in _refs:
        _refs[key] = R.optimize(O, problem(name), iters, user_lambda, np.float64)
    return _refs[key]


def ulp_spread(O, name: str):
    """How far the reference's own result moves when the initial translation is
    perturbed by one ulp: (|dS12_out| max, [|d chi2_end| per stage])."""
    key = (name, "ulp")
    if key not in _refs:
        ref = reference(O, name)
        p = problem(name).copy()
        p.S12[4:7] = np.nextafter(p.S12[4:7], np.inf)
        r = R.optimize(O, p, (5, 10, 5), 0.0, np.float64)
        dS = float(np.abs(r["S12_out"] - ref["S12_out"]).max())
        dchi = [abs(float(a["chi2_end"]) - float(b["chi2_end"])) for a, b in zip(r["stats"], ref["stats"])]
        same = (np.array_equal(r["pair_state"], ref["pair_state"]) and r["n_inliers"] == ref["n_inliers"]
                and len(r["stats"]) == len(ref["stats"]))
        _refs[key] = (dS, dchi, same)
    return _refs[key]
