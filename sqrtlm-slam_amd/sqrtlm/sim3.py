"""Sim3 alignment of a loop candidate: the problem ``g2oOptimizer::OptimizeSim3``
(g2oOptimizer.cc:1560-1793) assembles, as plain arrays for
``sqlm_sim3_optimize``, and a synthetic generator for it.

A *pair* is one surviving correspondence of ``vpMatches1``: the reference adds
an EdgeSim3ProjectXYZ (pMP2 into keyframe 1) and an EdgeInverseSim3ProjectXYZ
(pMP1 into keyframe 2) for it (:1641-1668).

The RANSAC that produces the initial S12 (``Sim3Solver``,
src/algorithm/Sim3Solver.cc) works on the same pairs: ``Sim3Solver`` below
mirrors its interface over ``sqlm_sim3_ransac``, and
``make_sim3_ransac_problem`` plants mismatched pairs for it.
"""
from __future__ import annotations

import copy
from dataclasses import dataclass, field

import numpy as np

from .synth import _sim3_compose, _sim3_inv, _so3_exp, orb_inv_level_sigma2, quat_from_mat, quat_to_mat

TH2_LOOP = 10.0  # LoopClosing.cc:513: OptimizeSim3(..., 10, mbFixScale)


@dataclass
class Sim3Problem:
    S12: np.ndarray        # (8,) qx qy qz qw tx ty tz s: camera 2 -> camera 1
    intr1: np.ndarray      # (4,) fx fy cx cy of keyframe 1
    intr2: np.ndarray      # (4,)
    X1c: np.ndarray        # (n,3) pMP1 in camera 1
    X2c: np.ndarray        # (n,3) pMP2 in camera 2
    obs1: np.ndarray       # (n,2) kpUn1.pt
    obs2: np.ndarray       # (n,2) kpUn2.pt
    info1: np.ndarray      # (n,) mvInvLevelSigma2[kpUn1.octave]
    info2: np.ndarray      # (n,)
    th2: float = TH2_LOOP
    fix_scale: bool = False
    matched: np.ndarray | None = None  # (n,) bool: vpMatches1[idx] still set; OptimizeSim3 clears rejected ones
    meta: dict = field(default_factory=dict)

    def __post_init__(self):
        f = lambda a, *s: np.ascontiguousarray(a, np.float64).reshape(*s)
        self.S12 = f(self.S12, 8)
        self.intr1, self.intr2 = f(self.intr1, 4), f(self.intr2, 4)
        self.X1c, self.X2c = f(self.X1c, -1, 3), f(self.X2c, -1, 3)
        self.obs1, self.obs2 = f(self.obs1, -1, 2), f(self.obs2, -1, 2)
        self.info1, self.info2 = f(self.info1, -1), f(self.info2, -1)
        n = self.X1c.shape[0]
        if any(a.shape[0] != n for a in (self.X2c, self.obs1, self.obs2, self.info1, self.info2)):
            raise ValueError("pair arrays disagree in length")
        self.th2 = float(np.float32(self.th2))  # the reference's th2 is a float
        self.matched = np.ones(n, bool) if self.matched is None else np.asarray(self.matched, bool).reshape(n).copy()

    @property
    def n_pair(self) -> int:
        return self.X1c.shape[0]

    def copy(self) -> "Sim3Problem":
        return copy.deepcopy(self)


def _map(S, X):
    return S[7] * (quat_to_mat(S[:4])[0] @ X.T).T + S[4:7]


def make_sim3_problem(n_pair: int = 150, *, seed: int = 0, pixel_noise: float = 0.5, outlier_frac: float = 0.2,
                      outlier_px=(20.0, 60.0), point_noise: float = 0.0, scale: float = 1.1, fix_scale: bool = False,
                      rot_pert: float = 0.01, trans_pert: float = 0.05, scale_pert: float = 0.02,
                      intr1=(718.856, 718.856, 607.1928, 185.2157), intr2=None, th2: float = TH2_LOOP,
                      n_levels: int = 8) -> Sim3Problem:
    """Two views of ``n_pair`` points related by a known S12 (``meta['S12_true']``).

    The points lie 4-25 m in front of camera 1; camera 2 sees them through
    S12^-1. Keypoints are the projections plus Gaussian ``pixel_noise`` px,
    rounded to float like ``cv::KeyPoint::pt``; a fraction ``outlier_frac`` of
    the pairs (``meta['outlier']``) has one keypoint displaced by
    ``outlier_px`` px. Each keypoint gets an octave and the matching ORB
    ``mvInvLevelSigma2`` weight. ``point_noise`` (m) perturbs the two map
    points independently, as two separately triangulated landmarks differ. The
    initial S12 is the true one perturbed by a rotation (rad), translation (m)
    and log-scale of the given sizes; with ``fix_scale`` the true scale is 1
    and stays unperturbed."""
    rng = np.random.default_rng([seed, 0x51A3])
    intr1 = np.array(intr1, np.float32).astype(np.float64)
    intr2 = intr1.copy() if intr2 is None else np.array(intr2, np.float32).astype(np.float64)
    s_true = 1.0 if fix_scale else float(scale)
    w = np.array([0.05, -0.12, 0.03]) + 0.02 * rng.normal(size=3)
    S_true = np.concatenate([quat_from_mat(_so3_exp(w[None]))[0], np.array([0.6, -0.1, 0.4]) + 0.1 * rng.normal(size=3),
                             [s_true]])
    n = int(n_pair)
    z = rng.uniform(4.0, 25.0, n)
    X1 = np.stack([rng.uniform(-0.8, 0.8, n) * z, rng.uniform(-0.25, 0.25, n) * z, z], axis=1)
    X2 = _map(_sim3_inv(S_true[None])[0], X1) if n else np.zeros((0, 3))

    def proj(K, X):
        return np.stack([K[0] * X[:, 0] / X[:, 2] + K[2], K[1] * X[:, 1] / X[:, 2] + K[3]], axis=1)

    obs1 = proj(intr1, X1) + pixel_noise * rng.normal(size=(n, 2))
    obs2 = proj(intr2, X2) + pixel_noise * rng.normal(size=(n, 2))
    outlier = rng.uniform(size=n) < outlier_frac
    ang = rng.uniform(0, 2 * np.pi, n)
    mag = rng.uniform(outlier_px[0], outlier_px[1], n)
    side = rng.uniform(size=n) < 0.5
    d = np.stack([np.cos(ang), np.sin(ang)], axis=1) * mag[:, None]
    obs1 = obs1 + d * (outlier & side)[:, None]
    obs2 = obs2 + d * (outlier & ~side)[:, None]
    X1c = X1 + point_noise * rng.normal(size=(n, 3))
    X2c = X2 + point_noise * rng.normal(size=(n, 3))
    lv = orb_inv_level_sigma2(n_levels).astype(np.float64)
    info1, info2 = lv[rng.integers(0, n_levels, n)], lv[rng.integers(0, n_levels, n)]
    pert = np.concatenate([quat_from_mat(_so3_exp((rot_pert * rng.normal(size=3))[None]))[0],
                           trans_pert * rng.normal(size=3),
                           [1.0 if fix_scale else float(np.exp(scale_pert * rng.normal()))]])
    S0 = _sim3_compose(pert[None], S_true[None])[0]
    return Sim3Problem(S12=S0, intr1=intr1, intr2=intr2, X1c=X1c, X2c=X2c,
                       obs1=obs1.astype(np.float32), obs2=obs2.astype(np.float32), info1=info1, info2=info2, th2=th2,
                       fix_scale=fix_scale, meta=dict(S12_true=S_true, outlier=outlier, seed=seed))


def orb_level_sigma2(n_levels: int = 8, scale: float = 1.2) -> np.ndarray:
    """mvLevelSigma2 computed in float as ORBextractor.cc:485-505."""
    s = [np.float32(1.0)]
    for _ in range(1, n_levels):
        s.append(np.float32(s[-1] * np.float32(scale)))
    return np.array([np.float32(v * v) for v in s], np.float32)


def ransac_max_err(sigma2) -> np.ndarray:
    """mvnMaxError as stored (Sim3Solver.cc:109-110): ``9.210 * sigma2`` is a
    double, the vector's element type is size_t, so the value is truncated."""
    return np.floor(9.210 * np.asarray(sigma2, np.float32).astype(np.float64)).astype(np.int32)


def make_sim3_ransac_problem(n_pair: int = 100, *, seed: int = 0, outlier_frac: float = 0.3, point_noise: float = 0.0,
                             pixel_noise: float = 0.0, scale: float = 1.1, fix_scale: bool = False,
                             intr1=(718.856, 718.856, 607.1928, 185.2157), intr2=None, n_levels: int = 8,
                             levels=None, translation_only: bool = False):
    """A loop candidate for the Sim3 RANSAC: ``(problem, max_err1, max_err2)``.

    ``n_pair`` points 4-25 m in front of camera 1, seen by camera 2 through the
    known S12^-1 (``meta['S12_true']``; ``translation_only``: identity rotation
    and a translation of exact float values, so that the planted rotation is
    exactly I). RANSAC reads the map points only, never the keypoints, so the
    outliers are mismatched pairs: ``round(outlier_frac * n_pair)`` pairs
    (``meta['outlier']``) have their camera-2 side (point, keypoint, octave)
    permuted cyclically among themselves. ``point_noise`` (m) perturbs the two
    map points independently. Each keypoint gets an octave (``levels``: an
    ``(n_pair, 2)`` array, else random below ``n_levels``); the thresholds are
    ``floor(9.210 * sigma2[level])``, as the reference's size_t vectors hold
    them. Keypoints (projection plus ``pixel_noise`` px, float) and their
    information come along so that the problem can go on to
    ``sqlm_sim3_optimize``; its initial ``S12`` is the true one."""
    rng = np.random.default_rng([seed, 0x5A3C])
    intr1 = np.array(intr1, np.float32).astype(np.float64)
    intr2 = intr1.copy() if intr2 is None else np.array(intr2, np.float32).astype(np.float64)
    s_true = 1.0 if fix_scale else float(scale)
    if translation_only:
        q = np.array([0.0, 0.0, 0.0, 1.0])
        t = np.array([0.75, -0.375, 0.1875])
        s_true = 1.0 if fix_scale else 2.0
    else:
        w = np.array([0.05, -0.12, 0.03]) + 0.02 * rng.normal(size=3)
        q = quat_from_mat(_so3_exp(w[None]))[0]
        t = np.array([0.6, -0.1, 0.4]) + 0.1 * rng.normal(size=3)
    S_true = np.concatenate([q, t, [s_true]])
    n = int(n_pair)
    z = rng.uniform(4.0, 25.0, n)
    X1 = np.stack([rng.uniform(-0.8, 0.8, n) * z, rng.uniform(-0.25, 0.25, n) * z, z], axis=1)
    if translation_only:
        # multiples of 3/256, like t: (X1 - t) / s, the sum of any three points and a third of it are
        # exact in float, so the relative coordinates of the two sides differ by the factor s exactly
        X1 = np.round(X1 * (256.0 / 3.0)) * (3.0 / 256.0)
    X2 = _map(_sim3_inv(S_true[None])[0], X1) if n else np.zeros((0, 3))

    def proj(K, X):
        return np.stack([K[0] * X[:, 0] / X[:, 2] + K[2], K[1] * X[:, 1] / X[:, 2] + K[3]], axis=1)

    obs1 = proj(intr1, X1) + pixel_noise * rng.normal(size=(n, 2))
    obs2 = proj(intr2, X2) + pixel_noise * rng.normal(size=(n, 2))
    lv = (rng.integers(0, n_levels, (n, 2)) if levels is None else np.asarray(levels, np.int64).reshape(n, 2))
    X1c = (X1 + point_noise * rng.normal(size=(n, 3))).astype(np.float32).astype(np.float64)
    X2c = (X2 + point_noise * rng.normal(size=(n, 3))).astype(np.float32).astype(np.float64)
    n_out = int(round(outlier_frac * n))
    outlier = np.zeros(n, bool)
    lv2 = lv[:, 1].copy()
    if n_out >= 2:
        who = np.sort(rng.permutation(n)[:n_out])
        outlier[who] = True
        src = np.roll(who, 1)   # a cyclic shift: every chosen pair gets another pair's camera-2 side
        X2c[who], obs2[who], lv2[who] = X2c[src], obs2[src], lv2[src]
    sig2 = orb_level_sigma2(n_levels)
    inv = orb_inv_level_sigma2(n_levels).astype(np.float64)
    prob = Sim3Problem(S12=S_true, intr1=intr1, intr2=intr2, X1c=X1c, X2c=X2c, obs1=obs1.astype(np.float32),
                       obs2=obs2.astype(np.float32), info1=inv[lv[:, 0]], info2=inv[lv2], fix_scale=fix_scale,
                       meta=dict(S12_true=S_true, outlier=outlier, seed=seed,
                                 levels=np.stack([lv[:, 0], lv2], axis=1)))
    return prob, ransac_max_err(sig2[lv[:, 0]]), ransac_max_err(sig2[lv2])


def pack_ransac(problems, max_err, draws, min_inliers):
    """The batch arrays of ``sqlm_sim3_ransac``: ``max_err`` a list of
    (max_err1, max_err2) per problem, ``draws`` a list of (n_hyp, 3) arrays,
    ``min_inliers`` an int or one per problem."""
    P = len(problems)
    c = lambda xs, w, t: (np.concatenate([np.asarray(x, t).reshape(-1, w) for x in xs], axis=0)
                          if xs else np.zeros((0, w), t))
    poff, hoff = np.zeros(P + 1, np.int64), np.zeros(P + 1, np.int64)
    poff[1:] = np.cumsum([p.n_pair for p in problems])
    draws = [np.asarray(d, np.int32).reshape(-1, 3) for d in draws]
    hoff[1:] = np.cumsum([d.shape[0] for d in draws])
    if len(max_err) != P or len(draws) != P:
        raise ValueError("one (max_err1, max_err2) and one draws array per problem")
    mi = np.broadcast_to(np.asarray(min_inliers, np.int32), (P,)).copy()
    return dict(intr1=c([p.intr1 for p in problems], 4, np.float64), intr2=c([p.intr2 for p in problems], 4, np.float64),
                fix_scale=np.array([p.fix_scale for p in problems], np.uint8), min_inliers=mi, pair_off=poff,
                X1c=c([p.X1c for p in problems], 3, np.float64), X2c=c([p.X2c for p in problems], 3, np.float64),
                max_err1=c([m[0] for m in max_err], 1, np.int32).reshape(-1),
                max_err2=c([m[1] for m in max_err], 1, np.int32).reshape(-1),
                hyp_off=hoff, draws=c(draws, 3, np.int32))


def ransac_max_its(n_pair: int, probability: float = 0.99, min_inliers: int = 6, max_iterations: int = 300) -> int:
    """sqlm_sim3_ransac_max_its: the hypothesis count SetRansacParameters leaves (host only, no GPU)."""
    from ._lib import lib
    return int(lib().sqlm_sim3_ransac_max_its(int(n_pair), float(probability), int(min_inliers), int(max_iterations)))


class Sim3Solver:
    """The reference's Sim3Solver (src/algorithm/Sim3Solver.cc) on the GPU.

    Constructed from a Sim3Problem (the pairs the reference's constructor
    keeps) and the stored thresholds; the random draws come from a numpy
    ``Generator`` (``rng``) or are given (``draws``, ``(>= max_its, 3)`` raw
    RandomInt values). All hypotheses are evaluated in one GPU call, made
    lazily by the first ``iterate`` / ``find`` (or by ``solve_batch`` for
    several solvers at once); every later call is served from those results.
    ``indices1`` / ``n1`` are mvnIndices1 / mN1: ``vbInliers`` has ``n1``
    entries and pair k sets entry ``indices1[k]``."""

    def __init__(self, problem: Sim3Problem, max_err1, max_err2, rng=None, draws=None, indices1=None, n1=None,
                 ctx=None):
        self.problem = problem
        self.N = problem.n_pair
        self.max_err = (np.asarray(max_err1, np.int32).reshape(self.N), np.asarray(max_err2, np.int32).reshape(self.N))
        self.indices1 = np.arange(self.N) if indices1 is None else np.asarray(indices1, np.int64).reshape(self.N)
        self.n1 = self.N if n1 is None else int(n1)
        self._rng, self._given, self._ctx = rng, draws, ctx
        if rng is None and draws is None:
            raise ValueError("give a numpy Generator (rng) or explicit draws")
        self.SetRansacParameters()

    def SetRansacParameters(self, probability: float = 0.99, minInliers: int = 6, maxIterations: int = 300):
        self.mRansacMinInliers = int(minInliers)
        self.mRansacMaxIts = ransac_max_its(self.N, probability, minInliers, maxIterations)
        self.mnIterations = 0
        self.mnBestInliers = 0
        self._best = -1
        self._res = None
        self._draws = None

    @property
    def draws(self):
        """(mRansacMaxIts, 3) raw RandomInt values: draw i of a hypothesis is in [0, N-1-i]."""
        if self._draws is None:
            H = self.mRansacMaxIts
            if self._given is not None:
                d = np.asarray(self._given, np.int32).reshape(-1, 3)
                if d.shape[0] < H:
                    raise ValueError(f"{H} hypotheses need {H} draw triples, {d.shape[0]} given")
                self._draws = d[:H].copy()
            elif H:
                self._draws = np.stack([self._rng.integers(0, self.N - i, H) for i in range(3)], axis=1).astype(np.int32)
            else:
                self._draws = np.zeros((0, 3), np.int32)
        return self._draws

    # -- the GPU call ---------------------------------------------------------
    @classmethod
    def solve_batch(cls, solvers, ctx=None):
        """Evaluate every hypothesis of every solver in one sqlm_sim3_ransac call."""
        solvers = list(solvers)
        if not solvers:
            return
        own = None
        if ctx is None:
            ctx = next((s._ctx for s in solvers if s._ctx is not None), None)
        if ctx is None:
            from .optimizer import Context
            ctx = own = Context(0)
        try:
            res = ctx.sim3_ransac([s.problem for s in solvers], [s.draws for s in solvers],
                                  [s.max_err for s in solvers], [s.mRansacMinInliers for s in solvers])
            for k, s in enumerate(solvers):
                r = res[k]
                H = r["n_inliers"].shape[0]
                r["mask"] = np.array([ctx.sim3_ransac_inliers(k, h) for h in range(H) if r["flags"][h] & 2]
                                     ).reshape(-1, s.N).astype(bool)
                r["mask_of"] = {int(h): i for i, h in enumerate(np.flatnonzero(r["flags"] & 2))}
                r["T12"] = {h: ctx.sim3_ransac_hypothesis(k, h)[1] for h in r["mask_of"]}
                s._res = r
        finally:
            if own is not None:
                own.close()

    def _results(self):
        if self._res is None:
            type(self).solve_batch([self])
        return self._res

    # -- the reference's interface ----------------------------------------------
    def iterate(self, nIterations: int):
        """(T12 (4,4) float32 or None, bNoMore, vbInliers (n1,) bool, nInliers): Sim3Solver.cc:207-292."""
        vb = np.zeros(self.n1, bool)
        if self.N < self.mRansacMinInliers:
            return None, True, vb, 0
        r = self._results()
        cur = 0
        while self.mnIterations < self.mRansacMaxIts and cur < nIterations:
            cur += 1
            h = self.mnIterations
            self.mnIterations += 1
            f = int(r["flags"][h])
            if f & 1:
                self._best, self.mnBestInliers = h, int(r["n_inliers"][h])
                if f & 2:
                    vb[self.indices1[r["mask"][r["mask_of"][h]]]] = True
                    return self._T12(h), False, vb, self.mnBestInliers
        return None, self.mnIterations >= self.mRansacMaxIts, vb, 0

    def find(self):
        """(T12 or None, vbInliers12, nInliers): iterate(mRansacMaxIts) without its flag (:296-300)."""
        T, _, vb, n = self.iterate(self.mRansacMaxIts)
        return T, vb, n

    def _T12(self, h):
        return self._res["T12"][h].copy()

    def _best_or_raise(self):
        if self._best < 0:
            raise RuntimeError("no hypothesis has been evaluated yet")
        return self._best

    def GetEstimatedRotation(self):
        return self._res["R12"][self._best_or_raise()].copy()

    def GetEstimatedTranslation(self):
        return self._res["t12"][self._best_or_raise()].copy()

    def GetEstimatedScale(self):
        return float(self._res["s12"][self._best_or_raise()])


def pack(problems):
    """The batch arrays of ``sqlm_sim3_optimize`` for a list of problems."""
    c = lambda xs, w: (np.concatenate([np.asarray(x, np.float64).reshape(-1, w) for x in xs], axis=0)
                       if xs else np.zeros((0, w)))
    off = np.zeros(len(problems) + 1, np.int64)
    off[1:] = np.cumsum([p.n_pair for p in problems])
    return dict(S12=c([p.S12 for p in problems], 8), intr1=c([p.intr1 for p in problems], 4),
                intr2=c([p.intr2 for p in problems], 4),
                fix_scale=np.array([p.fix_scale for p in problems], np.uint8),
                th2=np.array([p.th2 for p in problems], np.float64), pair_off=off,
                X1c=c([p.X1c for p in problems], 3), X2c=c([p.X2c for p in problems], 3),
                obs1=c([p.obs1 for p in problems], 2), obs2=c([p.obs2 for p in problems], 2),
                info1=c([p.info1 for p in problems], 1).reshape(-1), info2=c([p.info2 for p in problems], 1).reshape(-1))
