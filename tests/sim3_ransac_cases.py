"""The Sim3 RANSAC cases shared by tests/test_sim3_ransac_ref.py (CPU: what the
numpy definition tests/sim3_ransac_ref.py does on them) and
tests/test_gpu_sim3_ransac.py (GPU against that definition). The smallest
shapes at which the kernel can still go wrong: pair counts at the wavefront
(63, 64, 65), two and three ballot words (129, 300), the minimum (3);
hypothesis counts 1, 4, 5, 8, 13 and 300 (a workgroup takes 8, a wavefront 2);
free and fixed scale; two different cameras; a problem without hypotheses
(N < minInliers); minInliers == N; an exact pure translation; three coinciding
points (den = 0) with free and with fixed scale.

A case fixes its draws: seeded ones, with some hypotheses overridden by chosen
pair triples so that the sequential bookkeeping is exercised on purpose
("good" = three planted inliers far apart, "bad" = a triple with a mismatched
pair). test_sim3_ransac_ref.py asserts what each override is there for.
"""
from __future__ import annotations

import numpy as np

import sim3_ransac_ref as R
from sqrtlm import sim3

K2 = (700.0, 705.0, 600.0, 180.0)  # a second camera: K1 != K2

# name: pairs, seed, minInliers, maxIterations, generator arguments, {hypothesis: "good" | "bad" | "same"}
SPECS = {
    "n3_h1": (3, 1, 3, 300, dict(outlier_frac=0.0), {}),
    "n20_h4_fix": (20, 2, 6, 4, dict(fix_scale=True), {0: "good"}),
    "n63_h5": (63, 3, 10, 5, dict(), {0: "bad", 1: "bad", 2: "bad", 3: "bad", 4: "good"}),
    "n64_h300_k2": (64, 4, 10, 300, dict(intr2=K2), {0: "bad", 1: "bad", 2: "bad", 3: "bad", 4: "bad", 5: "bad", 6: "good"}),
    "n5_lt_min": (5, 5, 6, 300, dict(outlier_frac=0.0), {}),
    "n65_h13_fix_k2": (65, 6, 10, 13, dict(fix_scale=True, intr2=K2), {12: "good"}),
    "n129_h8_never": (129, 7, 100, 300, dict(outlier_frac=0.3), {}),
    "n20_min_eq_n": (20, 8, 20, 300, dict(outlier_frac=0.0), {}),
    "n300_h300": (300, 9, 20, 300, dict(point_noise=0.002), {}),
    "n20_translation": (20, 10, 6, 5, dict(translation_only=True, outlier_frac=0.0), {}),
    "n20_same_free": (20, 11, 6, 5, dict(), {0: "same", 3: "good"}),
    "n20_same_fix": (20, 11, 6, 5, dict(fix_scale=True), {0: "same", 3: "good"}),
}
NAMES = list(SPECS)
CHAIN = dict(n_pair=150, seed=21, outlier_frac=0.3, point_noise=0.005, pixel_noise=0.5, min_inliers=20)

_cases: dict = {}
_refs: dict = {}


def _raw(idx):
    """Raw draws that the swap-remove maps to the distinct pair indices idx (each within its draw's range)."""
    return np.asarray(idx, np.int32)


def _spread_triple(X, who):
    """Three of the pairs `who` spanning a large triangle: the extremes along x and the farthest from their line."""
    P = X[who]
    a, b = who[np.argmin(P[:, 0])], who[np.argmax(P[:, 0])]
    d = np.linalg.norm(np.cross(X[who] - X[a], X[b] - X[a]), axis=1)
    c = who[np.argmax(d)]
    return [int(a), int(b), int(c)]


def case(name: str):
    """dict(problem, max_err, draws (H,3), min_inliers, n_hyp) of the case (built once; callers must not modify it)."""
    if name not in _cases:
        n, seed, min_in, max_it, kw, over = SPECS[name]
        p, e1, e2 = sim3.make_sim3_ransac_problem(n, seed=seed, **kw)
        if "same" in over.values():   # pairs 0, 1, 2 become one and the same pair
            for a in (p.X1c, p.X2c):       # few bits: x + x + x and a third of it are exact, the centroid is x
                a[0] = np.round(a[0] * 64.0) / 64.0
            for a in (p.X1c, p.X2c, p.obs1, p.obs2):
                a[1] = a[2] = a[0]
            p.info1[1:3], p.info2[1:3], e1[1:3], e2[1:3] = p.info1[0], p.info2[0], e1[0], e2[0]
            p.meta["outlier"][:3] = p.meta["outlier"][0]
            p.meta["levels"][:3] = p.meta["levels"][0]
        H = R.max_its(n, 0.99, min_in, max_it)
        rng = np.random.default_rng([seed, 0xD4A3])
        draws = (np.stack([rng.integers(0, n - i, H) for i in range(3)], axis=1).astype(np.int32)
                 if H else np.zeros((0, 3), np.int32))
        inl = np.flatnonzero(~p.meta["outlier"])
        inl = inl[inl < n - 2]            # usable as any of the three raw draws
        for h, kind in over.items():
            if kind == "same":
                t = [0, 1, 2]
            else:
                t = _spread_triple(p.X1c, inl[inl > 2] if "same" in over.values() else inl)
                if kind == "bad":
                    out = np.flatnonzero(p.meta["outlier"])
                    out = out[(out < n - 2) & ~np.isin(out, t)]
                    t[2] = int(out[h % len(out)])
            draws[h] = _raw(t)
        _cases[name] = dict(problem=p, max_err=(e1, e2), draws=draws, min_inliers=min_in, n_hyp=H)
    return _cases[name]


def reference(name: str):
    """The float32 definition of every hypothesis of the case, and the scan over its counts (computed once, shared)."""
    if name not in _refs:
        c = case(name)
        p = c["problem"]
        r = R.hypotheses(p.X1c, p.X2c, p.intr1, p.intr2, p.fix_scale, c["max_err"][0], c["max_err"][1], c["draws"])
        r["flags"], r["first_return"], r["best"] = R.scan(r["count"], c["min_inliers"])
        _refs[name] = r
    return _refs[name]


def literal(name: str, hyp=None):
    """A fresh literal solver (sim3_ransac_ref.LiteralSolver) on the case, fed `hyp` or the definition's results."""
    c = case(name)
    return R.LiteralSolver(reference(name) if hyp is None else hyp, c["problem"].n_pair, c["min_inliers"], c["n_hyp"])


def chain_case():
    """The planted candidate of the chain test: point noise, keypoint noise and mismatches."""
    if "chain" not in _cases:
        kw = dict(CHAIN)
        n, min_in = kw.pop("n_pair"), kw.pop("min_inliers")
        p, e1, e2 = sim3.make_sim3_ransac_problem(n, **kw)
        H = R.max_its(n, 0.99, min_in, 300)
        rng = np.random.default_rng([kw["seed"], 0xD4A3])
        draws = np.stack([rng.integers(0, n - i, H) for i in range(3)], axis=1).astype(np.int32)
        _cases["chain"] = dict(problem=p, max_err=(e1, e2), draws=draws, min_inliers=min_in, n_hyp=H)
    return _cases["chain"]


def chain_subproblem(c, R12, t12, s12, mask):
    """What LoopClosing.cc:509-513 hands to OptimizeSim3 after a RANSAC return:
    gScm from (R, t, s) of the solver and the inlier matches only."""
    from sqrtlm import synth
    p = c["problem"]
    m = np.asarray(mask, bool)
    q = synth.quat_from_mat(np.asarray(R12, np.float64).reshape(1, 3, 3))[0]
    S = np.concatenate([q, np.asarray(t12, np.float64).reshape(3), [float(s12)]])
    return sim3.Sim3Problem(S12=S, intr1=p.intr1, intr2=p.intr2, X1c=p.X1c[m], X2c=p.X2c[m], obs1=p.obs1[m],
                            obs2=p.obs2[m], info1=p.info1[m], info2=p.info2[m], th2=sim3.TH2_LOOP,
                            fix_scale=p.fix_scale)
