"""Motion-only bundle adjustment of one frame: the problem
``g2oOptimizer::PoseOptimization`` (g2oOptimizer.cc:385-679) assembles, as plain
arrays for ``sqlm_pose_optimize`` / ``sqlm_pose_refine_lidar``, and synthetic
generators for it.

An *edge* is one monocular correspondence (``mvuRight < 0``) of the frame: the
reference adds an EdgeSE3ProjectXYZOnlyPose for it (:443-480). A *LiDAR pair* is
one kd-tree association of the optional LiDAR stage (:560-630): a flat point
(EdgeLidarFlatPoint) or a corner point (EdgeLidarCornerPoint).
"""
from __future__ import annotations

import copy
from dataclasses import dataclass, field

import numpy as np

from .synth import KITTI_INTR, _so3_exp, orb_inv_level_sigma2, quat_from_mat, quat_to_mat

TH2_MONO = 5.991  # chi-square, 2 degrees of freedom, 5 %


@dataclass
class PoseProblem:
    pose_q: np.ndarray     # (4,) qx qy qz qw of T_cw (pFrame->mTcw)
    pose_t: np.ndarray     # (3,)
    intr: np.ndarray       # (4,) fx fy cx cy
    Xw: np.ndarray         # (n,3) pMP->GetWorldPos() (float values)
    uv: np.ndarray         # (n,2) kpUn.pt (float values)
    info: np.ndarray       # (n,) mvInvLevelSigma2[kpUn.octave] (float values)
    th2: float = TH2_MONO
    outlier: np.ndarray | None = None  # (n,) bool: mvbOutlier of the counted keypoints
    meta: dict = field(default_factory=dict)

    def __post_init__(self):
        f = lambda a, *s: np.ascontiguousarray(a, np.float64).reshape(*s)
        self.pose_q, self.pose_t, self.intr = f(self.pose_q, 4), f(self.pose_t, 3), f(self.intr, 4)
        self.Xw, self.uv, self.info = f(self.Xw, -1, 3), f(self.uv, -1, 2), f(self.info, -1)
        n = self.Xw.shape[0]
        if self.uv.shape[0] != n or self.info.shape[0] != n:
            raise ValueError("edge arrays disagree in length")
        self.th2 = float(self.th2)
        self.outlier = np.zeros(n, bool) if self.outlier is None else np.asarray(self.outlier, bool).reshape(n).copy()

    @property
    def n_obs(self) -> int:
        return self.Xw.shape[0]

    def copy(self) -> "PoseProblem":
        return copy.deepcopy(self)


@dataclass
class LidarPairs:
    kind: np.ndarray       # (m,) uint8: 0 flat, 1 corner
    pc: np.ndarray         # (m,3) the frame's point, camera frame
    pw: np.ndarray         # (m,3) its nearest local-map point, world frame
    n: np.ndarray          # (m,3) the flat point's normal (ignored for corners)
    info: np.ndarray       # (m,) flat_optimized_weight / corner_optimized_weight

    def __post_init__(self):
        f = lambda a, *s: np.ascontiguousarray(a, np.float64).reshape(*s)
        self.kind = np.ascontiguousarray(self.kind, np.uint8).reshape(-1)
        self.pc, self.pw, self.n, self.info = f(self.pc, -1, 3), f(self.pw, -1, 3), f(self.n, -1, 3), f(self.info, -1)
        m = self.kind.shape[0]
        if any(a.shape[0] != m for a in (self.pc, self.pw, self.n, self.info)):
            raise ValueError("LiDAR arrays disagree in length")

    @property
    def n_lid(self) -> int:
        return self.kind.shape[0]


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def make_pose_problem(n: int = 300, *, seed: int = 0, pixel_noise: float = 0.3, outlier_frac: float = 0.2,
                      outlier_px=(8.0, 40.0), rot_pert: float = 0.01, trans_pert: float = 0.05,
                      intr=KITTI_INTR, th2: float = TH2_MONO, n_levels: int = 8) -> PoseProblem:
    """``n`` map points seen by a frame with a known pose (``meta['q_true']``,
    ``meta['t_true']``).

    The points lie 4-25 m in front of the camera. ``Xw``, ``uv`` and ``info``
    are float32 values widened to double, as the adapter passes them
    (``GetWorldPos`` is a float matrix, ``kpUn.pt`` a float pair,
    ``mvInvLevelSigma2`` a float vector indexed by the keypoint's octave).
    Keypoints are the projections plus Gaussian ``pixel_noise`` px, scaled by
    the octave's sigma; a fraction ``outlier_frac`` (``meta['outlier']``) is
    displaced by ``outlier_px`` px times that sigma. The initial pose is the
    true one perturbed by a rotation (rad) and a translation (m) of the given
    sizes: a large perturbation ("far start") makes the outlier set change
    between the rounds."""
    rng = np.random.default_rng([seed, 0x905E])
    intr = _f32(intr)
    w = np.array([0.03, -0.2, 0.05]) + 0.02 * rng.normal(size=3)
    R_true = _so3_exp(w[None])[0]
    t_true = np.array([0.4, -0.1, 1.5]) + 0.2 * rng.normal(size=3)
    n = int(n)
    z = rng.uniform(4.0, 25.0, n)
    Xc = np.stack([rng.uniform(-0.8, 0.8, n) * z, rng.uniform(-0.25, 0.25, n) * z, z], axis=1)
    Xw = _f32((Xc - t_true) @ R_true)  # R^T (Xc - t)
    Xc = Xw @ R_true.T + t_true
    lv = orb_inv_level_sigma2(n_levels).astype(np.float64)
    octave = rng.integers(0, n_levels, n)
    info = lv[octave]
    sigma = 1.0 / np.sqrt(info)
    uv = np.stack([intr[0] * Xc[:, 0] / Xc[:, 2] + intr[2], intr[1] * Xc[:, 1] / Xc[:, 2] + intr[3]], axis=1)
    uv = uv + pixel_noise * sigma[:, None] * rng.normal(size=(n, 2))
    outlier = rng.uniform(size=n) < outlier_frac
    ang = rng.uniform(0, 2 * np.pi, n)
    mag = rng.uniform(outlier_px[0], outlier_px[1], n) * sigma
    uv = uv + (np.stack([np.cos(ang), np.sin(ang)], axis=1) * mag[:, None]) * outlier[:, None]
    dR = _so3_exp((rot_pert * rng.normal(size=3))[None])[0]
    dt = trans_pert * rng.normal(size=3)
    q0 = quat_from_mat((dR @ R_true)[None])[0]
    t0 = dR @ t_true + dt
    return PoseProblem(pose_q=q0, pose_t=t0, intr=intr, Xw=Xw, uv=_f32(uv), info=info, th2=th2,
                       meta=dict(q_true=quat_from_mat(R_true[None])[0], t_true=t_true, outlier=outlier, octave=octave,
                                 seed=seed))


def make_lidar_pairs(prob: PoseProblem, m: int = 200, *, seed: int = 0, kinds: str = "mixed", noise: float = 0.02,
                     flat_weight: float = 1.0, corner_weight: float = 0.5) -> LidarPairs:
    """``m`` LiDAR associations consistent with ``prob``'s true pose: map points
    3-30 m in front of the camera, the frame's points displaced by ``noise`` m
    (float32 values, as PCL points are). ``kinds``: ``flat``, ``corner`` or
    ``mixed``."""
    rng = np.random.default_rng([seed, 0x11DA])
    R = quat_to_mat(prob.meta["q_true"])[0]
    t = prob.meta["t_true"]
    m = int(m)
    z = rng.uniform(3.0, 30.0, m)
    pc_true = np.stack([rng.uniform(-1.0, 1.0, m) * z, rng.uniform(-0.3, 0.3, m) * z, z], axis=1)
    pw = _f32((pc_true - t) @ R)
    pc = _f32(pw @ R.T + t + noise * rng.normal(size=(m, 3)))
    nrm = rng.normal(size=(m, 3))
    nrm = _f32(nrm / np.linalg.norm(nrm, axis=1, keepdims=True)) if m else nrm
    kind = {"flat": np.zeros(m, np.uint8), "corner": np.ones(m, np.uint8),
            "mixed": (rng.uniform(size=m) < 0.4).astype(np.uint8)}[kinds]
    info = np.where(kind == 0, float(np.float32(flat_weight)), float(np.float32(corner_weight)))
    return LidarPairs(kind=kind, pc=pc, pw=pw, n=nrm, info=info)


def _cat(xs, w):
    return (np.concatenate([np.asarray(x, np.float64).reshape(-1, w) for x in xs], axis=0) if xs
            else np.zeros((0, w)))


def pack(problems):
    """The batch arrays of ``sqlm_pose_optimize`` for a list of problems."""
    off = np.zeros(len(problems) + 1, np.int64)
    off[1:] = np.cumsum([p.n_obs for p in problems])
    return dict(pose_q=_cat([p.pose_q for p in problems], 4), pose_t=_cat([p.pose_t for p in problems], 3),
                intr=_cat([p.intr for p in problems], 4), obs_off=off, Xw=_cat([p.Xw for p in problems], 3),
                uv=_cat([p.uv for p in problems], 2), info=_cat([p.info for p in problems], 1).reshape(-1))


def pack_lidar(pairs):
    """The LiDAR arrays of ``sqlm_pose_refine_lidar`` for a list of LidarPairs (one per problem)."""
    off = np.zeros(len(pairs) + 1, np.int64)
    off[1:] = np.cumsum([l.n_lid for l in pairs])
    kind = np.concatenate([l.kind for l in pairs]) if pairs else np.zeros(0, np.uint8)
    return dict(lid_off=off, lid_kind=np.ascontiguousarray(kind, np.uint8), lid_pc=_cat([l.pc for l in pairs], 3),
                lid_pw=_cat([l.pw for l in pairs], 3), lid_n=_cat([l.n for l in pairs], 3),
                lid_info=_cat([l.info for l in pairs], 1).reshape(-1))
