"""The PnP RANSAC cases shared by tests/test_pnp_ransac_ref.py and
tests/test_pnp_ransac_abi.py (CPU) and tests/test_gpu_pnp_ransac.py (GPU
against the numpy definition tests/pnp_ransac_ref.py). The smallest shapes at
which the kernels can still go wrong: pair counts 4, 15, 63, 64, 65, 129, 300
(the minimum, one ballot word and its edges, two and five words); hypothesis
counts 1, 3, 4, 5 (a workgroup takes 4) and 300; two cameras; octaves mixed
over ORB's 8 levels; a problem without hypotheses (N < minInliers) in the middle
of the batch; minInliers == N; four coplanar points; four points of which two
coincide; a point behind the camera; refines on 4, 10, 63, 64, 65 and 129+
inliers; a record-breaking hypothesis whose refine fails followed by one whose
refine succeeds; no qualifying hypothesis at all; mRansacMaxIts = 4 with 12
hypotheses, so that iterate(5) runs past it.

A case fixes its draws: seeded ones, with some hypotheses overridden by chosen
quadruples ("good" = four planted inliers far apart, "bad" = three of them and a
mismatch, "same" = pairs 0 and 1, which coincide, and two more, "behind" = a
point behind the camera first). test_pnp_ransac_ref.py asserts what each
override is there for.
"""
from __future__ import annotations

import numpy as np

import pnp_ransac_ref as R
from sqrtlm import pnp

K2 = (700.0, 705.0, 600.0, 180.0)  # a second camera

# name: pairs, seed, mRansacMinInliers, hypotheses, generator arguments, {hypothesis: kind}
SPECS = {
    "n4_h1_min_eq_n": (4, 6, 4, 1, dict(outlier_frac=0.0, pixel_noise=0.0), {}),
    "n15_h5_refine10": (15, 2, 10, 5, dict(outlier_frac=1 / 3, pixel_noise=0.0), {1: "bad", 3: "good"}),
    "n63_h3_k2": (63, 3, 20, 3, dict(outlier_frac=0.0, pixel_noise=0.1, intr=K2), {2: "good"}),
    "n8_lt_min": (8, 4, 10, 0, dict(outlier_frac=0.0), {}),
    "n64_h4": (64, 5, 20, 4, dict(outlier_frac=0.0, pixel_noise=0.1), {0: "good"}),
    "n65_h5": (65, 6, 20, 5, dict(outlier_frac=0.0, pixel_noise=0.1), {4: "good"}),
    "n129_h300": (129, 7, 20, 300, dict(outlier_frac=0.3, pixel_noise=0.5), {}),
    "n129_never": (129, 7, 120, 5, dict(outlier_frac=0.3, pixel_noise=0.5), {0: "good"}),
    "n300_h5": (300, 8, 50, 5, dict(outlier_frac=0.3, pixel_noise=0.5), {0: "bad", 2: "good"}),
    "n20_coplanar": (20, 9, 10, 5, dict(outlier_frac=0.0, pixel_noise=0.1, coplanar=True), {0: "good"}),
    "n20_same": (20, 10, 10, 5, dict(outlier_frac=0.0, pixel_noise=0.1), {0: "same", 3: "good"}),
    "n20_behind": (20, 11, 10, 5, dict(outlier_frac=0.0, pixel_noise=0.1, behind=2), {0: "behind", 1: "good"}),
    "n30_fail_then_ok": (30, 12, 10, 4, dict(), {0: "bad", 1: "goodA", 2: "goodB"}),
    # SetRansacParameters(0.99, 18, 300, 4, 0.5) on 20 pairs: mRansacMaxIts = 4 < 5, iterate(5) runs past it
    "n20_its4": (20, 13, 18, 12, dict(outlier_frac=0.1, pixel_noise=0.1), {1: "good", 6: "good"}),
}
MAX_ITS = {"n20_its4": 4}   # mRansacMaxIts of the replay tests where it is not the case's hypothesis count less 5
NAMES = list(SPECS)

_cases: dict = {}
_refs: dict = {}


def _good(p, who, rng, must=()):
    """An all-inlier quadruple that works: EPnP on four points is ambiguous for many quadruples, so this is the
    first of the spread one and 31 seeded ones (each starting with `must`) whose hypothesis, by the numpy
    definition, has the most inliers."""
    who = np.asarray([w for w in who if w not in must])
    k = 4 - len(must)
    cand = [list(must) + _spread(p.Xw, who, k)] + [list(must) + [int(v) for v in rng.permutation(who)[:k]]
                                                    for _ in range(31)]
    r = R.hypotheses(p, np.stack([raw_draws(p.n_pair, q) for q in cand]))
    return cand[int(np.argmax(r["count"]))]


def _spread(X, who, k=4):
    """k of the pairs `who` far apart: the extremes along x, then greedily the farthest from those chosen."""
    who = np.asarray(who)
    P = X[who].astype(np.float64)
    pick = [int(np.argmin(P[:, 0])), int(np.argmax(P[:, 0]))]
    while len(pick) < k:
        d = np.min(np.linalg.norm(P[:, None] - P[pick][None], axis=2), axis=1)
        pick.append(int(np.argmax(d)))
    return [int(who[i]) for i in pick]


def raw_draws(n, idx):
    """Raw draws that the swap-remove maps to the distinct pair indices idx."""
    avail, out = list(range(n)), []
    for j in idx:
        r = avail.index(int(j))
        out.append(r)
        avail[r] = avail[-1]
        avail.pop()
    return np.asarray(out, np.int32)


def _two_structures(seed):
    """10 pairs consistent with one pose (no noise) and 20 consistent with another: a hypothesis from the first
    group qualifies at minInliers = 10 but its refine cannot exceed 10."""
    a = pnp.make_pnp_problem(10, seed=seed, outlier_frac=0.0, pixel_noise=0.0, levels=np.zeros(10, int))
    b = pnp.make_pnp_problem(20, seed=seed + 100, outlier_frac=0.0, pixel_noise=0.0, levels=np.zeros(20, int))
    grp = np.array([0] * 10 + [1] * 20)
    return pnp.PnPProblem(intr=a.intr, Xw=np.concatenate([a.Xw, b.Xw]), uv=np.concatenate([a.uv, b.uv]),
                          sigma2=np.concatenate([a.sigma2, b.sigma2]),
                          meta=dict(group=grp, outlier=np.zeros(30, bool), Rcw=b.meta["Rcw"], tcw=b.meta["tcw"]))


def case(name: str):
    """dict(problem, draws (H,4), min_inliers, n_hyp, quads) of the case (built once; callers must not modify it)."""
    if name not in _cases:
        n, seed, min_in, H, kw, over = SPECS[name]
        p = _two_structures(seed) if name == "n30_fail_then_ok" else pnp.make_pnp_problem(n, seed=seed, **kw)
        n = p.n_pair
        if "same" in over.values():
            p.Xw[1], p.uv[1], p.sigma2[1] = p.Xw[0], p.uv[0], p.sigma2[0]
        draws = pnp.draw(np.random.default_rng([seed, 0xE9A3]), n, H)
        inl = np.flatnonzero(~p.meta["outlier"])
        if kw.get("behind"):
            inl = inl[inl < n - kw["behind"]]
        quads = {}
        qrng = np.random.default_rng([seed, 0x600D])
        for h, kind in over.items():
            if kind == "same":
                q = _good(p, inl[inl > 1], qrng, must=(0, 1))
            elif kind == "behind":
                q = [n - 1] + _spread(p.Xw, inl, 3)
            elif kind in ("goodA", "goodB"):
                q = _good(p, np.flatnonzero(p.meta["group"] == (kind == "goodB")), qrng)
            elif name == "n30_fail_then_ok":   # "bad": two pairs of either structure
                q = [0, 5, 12, 25]
            else:
                q = _good(p, inl[inl > 1] if "same" in over.values() else inl, qrng)
                if kind == "bad":
                    out = np.flatnonzero(p.meta["outlier"])
                    q[3] = int(out[h % len(out)])
            quads[h] = q
            draws[h] = raw_draws(n, q)
        _cases[name] = dict(problem=p, draws=draws, min_inliers=min_in, n_hyp=H, quads=quads)
    return _cases[name]


def reference(name: str):
    """The numpy definition of every hypothesis of the case, of the refine of every record-breaking one
    (``refined``: {hypothesis: result}) and the scan over the counts (computed once, shared)."""
    if name not in _refs:
        c = case(name)
        p = c["problem"]
        if c["n_hyp"]:
            r = R.hypotheses(p, c["draws"])
        else:
            r = dict(count=np.zeros(0, np.int32), mask=np.zeros((0, p.n_pair), bool))
        best, r["refined"] = 0, {}
        for h, cnt in enumerate(r["count"]):
            if cnt >= c["min_inliers"] and cnt > best:
                best = int(cnt)
                r["refined"][h] = R.refine(p, r["mask"][h])
        r["flags"], r["first_return"], r["best"] = scan_literal(r["count"], {h: int(v["count"][0]) for h, v in r["refined"].items()},
                                                                 c["min_inliers"])
        _refs[name] = r
    return _refs[name]


def scan_literal(counts, refined_of, min_inliers):
    """flags, first_return, best from a LiteralSolver stepped one hypothesis at a time."""
    H = len(counts)
    s = R.LiteralSolver(counts, lambda h: refined_of[h], 1 << 30, min_inliers, H)
    flags, first = np.zeros(H, np.uint8), -1
    for h in range(H):
        before = s.best
        kind, _, _ = _step(s)
        f = 1 if counts[h] >= min_inliers else 0
        if s.best != before:
            f |= 2
        if kind == "refined":
            f |= 4
            first = h if first < 0 else first
        flags[h] = f
    return flags, first, s.best


def _step(s):
    """One pass of iterate's loop body."""
    s.mRansacMaxIts = s.mnIterations + 1
    k = s.iterate(0)
    return k if k[0] == "refined" else (None, -1, False)
