"""Sim3 alignment of a loop candidate: the problem ``g2oOptimizer::OptimizeSim3``
(g2oOptimizer.cc:1560-1793) assembles, as plain arrays for
``sqlm_sim3_optimize``, and a synthetic generator for it.

A *pair* is one surviving correspondence of ``vpMatches1``: the reference adds
an EdgeSim3ProjectXYZ (pMP2 into keyframe 1) and an EdgeInverseSim3ProjectXYZ
(pMP1 into keyframe 2) for it (:1641-1668).
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
