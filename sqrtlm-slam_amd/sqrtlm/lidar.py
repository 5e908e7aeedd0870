"""LiDAR flat- and corner-point association of local-BA pass 3 (g2oOptimizer.cc:978-1107).

The reference moves the ``surface_points_less_flat_`` clouds of the other local
keyframes to the world with their pass-2 poses, builds a kd-tree over them and
gives every flat point of the current keyframe its nearest neighbour; a
neighbour closer than ``distance_sq_threshold`` becomes an EdgeLidarFlatPoint.
The library does the search as an exact brute-force 1-NN on the device
(``sqlm_lidar_associate`` / ``sqlm_set_lidar_from_clouds``); this module holds
the clouds of one local window and a seeded generator of planar scenes.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np


@dataclass
class LidarClouds:
    """The flat clouds of a local window, each in its keyframe's sensor frame.

    ``xyz[k]`` / ``normal[k]`` are (n_k, 3) float32 (surface_points_less_flat_ and
    surface_points_less_flat_normal_ of keyframe k), ``pose_index[k]`` the pose of
    the BA problem keyframe k is; ``current`` names the entry of the keyframe
    being optimised (the reference's pKF): its points are the queries, all other
    entries form the map, in list order. ``dist_sq_threshold`` and ``weight`` are
    lidarConfig's distance_sq_threshold and flat_optimized_weight.
    ``corner_xyz`` (optional, one (m_k, 3) float32 cloud per keyframe) holds the
    corner_points_less_sharp_ clouds of using_sharp_point (:1075-1107), searched
    the same way among themselves; ``corner_weight`` is corner_optimized_weight."""
    xyz: list
    normal: list
    pose_index: np.ndarray
    current: int = 0
    dist_sq_threshold: float = 1.0
    weight: float = 50.0
    corner_xyz: list | None = None
    corner_weight: float = 30.0

    def __post_init__(self):
        self.xyz = [np.ascontiguousarray(a, np.float32).reshape(-1, 3) for a in self.xyz]
        self.normal = [np.ascontiguousarray(a, np.float32).reshape(-1, 3) for a in self.normal]
        self.pose_index = np.ascontiguousarray(self.pose_index, np.int32).reshape(-1)
        if not (len(self.xyz) == len(self.normal) == self.pose_index.size):
            raise ValueError("one cloud, one normal cloud and one pose index per keyframe")
        for a, b in zip(self.xyz, self.normal):
            if a.shape != b.shape:
                raise ValueError("a normal per point")
        if not 0 <= self.current < len(self.xyz):
            raise ValueError("current out of range")
        if self.corner_xyz is not None:
            self.corner_xyz = [np.ascontiguousarray(a, np.float32).reshape(-1, 3) for a in self.corner_xyz]
            if len(self.corner_xyz) != len(self.xyz):
                raise ValueError("one corner cloud per keyframe")

    @property
    def others(self) -> list:
        """The map keyframes: every entry but the current one, in list order."""
        return [k for k in range(len(self.xyz)) if k != self.current]

    @property
    def query_xyz(self) -> np.ndarray:
        return self.xyz[self.current]

    @property
    def query_normal(self) -> np.ndarray:
        return self.normal[self.current]

    def cloud_sets(self, Twc) -> list:
        """The sets of ``Context.set_lidar_from_cloud_sets`` at the float T_wc
        ``Twc[k]`` of every keyframe: the flat set, then the corner set."""
        oth = self.others
        mT = np.stack([Twc[k] for k in oth]) if oth else np.zeros((0, 16), np.float32)
        common = dict(map_Twc=mT, query_Twc=Twc[self.current], dist_sq_threshold=self.dist_sq_threshold)
        sets = [dict(kind=0, map_clouds=[self.xyz[k] for k in oth], query_xyz=self.query_xyz,
                     query_normal=self.query_normal, info=self.weight, **common)]
        if self.corner_xyz is not None:
            sets.append(dict(kind=1, map_clouds=[self.corner_xyz[k] for k in oth],
                             query_xyz=self.corner_xyz[self.current], query_normal=None, info=self.corner_weight,
                             **common))
        return sets


def pack_clouds(clouds):
    """[(n_k, 3) float32, ...] -> (map_off int64 [K+1], map_xyz float32 (n, 3))."""
    clouds = [np.ascontiguousarray(a, np.float32).reshape(-1, 3) for a in clouds]
    off = np.zeros(len(clouds) + 1, np.int64)
    if clouds:
        off[1:] = np.cumsum([a.shape[0] for a in clouds])
    xyz = np.concatenate(clouds, axis=0) if clouds else np.zeros((0, 3), np.float32)
    return off, np.ascontiguousarray(xyz, np.float32)


def Twc_f32(q, t) -> np.ndarray:
    """The float 4x4 T_wc of the pose (q, t) = T_cw: Converter::toCvMat(estimate)
    (``pose_to_Tcw_f32``) followed by a **float32** ``np.linalg.inv``. The
    inversion stands in for ``cv::Mat::inv()``, whose 4x4 float LU the library
    does not restate: façade and tests only; an adapter calls OpenCV."""
    from .optimizer import pose_to_Tcw_f32
    T = pose_to_Tcw_f32(q, t)
    return np.ascontiguousarray(np.linalg.inv(T.astype(np.float32)), np.float32)


def associate(ctx, map_clouds, map_Twc, query_xyz, query_Twc, dist_sq_threshold: float):
    """``Context.lidar_associate``: (nn_index, nn_sq_dist, nn_xyz, accepted)."""
    return ctx.lidar_associate(map_clouds, map_Twc, query_xyz, query_Twc, dist_sq_threshold)


def make_planar_clouds(pose_q, pose_t, pose_index, *, n_points=300, current: int = 0, seed: int = 0,
                       noise: float = 0.02, extent: float = 3.0, dist_sq_threshold: float = 0.04,
                       weight: float = 50.0) -> LidarClouds:
    """A seeded planar scene seen from K poses: a ground plane 1.5 m under the
    first camera centre and two walls 4 m to either side of it, sampled
    uniformly within ``extent`` metres of each keyframe's centre with Gaussian
    noise ``noise`` along the plane normal. Every point is expressed in its
    keyframe's sensor frame (p_c = R_cw p_w + t_cw from the given T_cw = (q, t)),
    with the plane normal rotated into that frame. ``n_points`` is one count or
    one per keyframe; ``pose_index[k]`` is the BA pose of keyframe k."""
    from .synth import quat_to_mat
    q = np.asarray(pose_q, np.float64).reshape(-1, 4)
    t = np.asarray(pose_t, np.float64).reshape(-1, 3)
    K = q.shape[0]
    counts = np.broadcast_to(np.asarray(n_points, np.int64), (K,))
    rng = np.random.default_rng(seed)
    R = quat_to_mat(q)                                   # R_cw
    C = -np.einsum("nji,nj->ni", R, t)                   # camera centres
    # plane: (axis the plane fixes, its coordinate, world normal)
    planes = [(1, C[0, 1] + 1.5, np.array([0.0, -1.0, 0.0])),
              (0, C[0, 0] - 4.0, np.array([1.0, 0.0, 0.0])),
              (0, C[0, 0] + 4.0, np.array([-1.0, 0.0, 0.0]))]
    xyz, nrm = [], []
    for k in range(K):
        n = int(counts[k])
        which = rng.integers(0, len(planes), n)
        pw = C[k] + rng.uniform(-extent, extent, (n, 3))
        nw = np.zeros((n, 3))
        for p, (ax, val, nv) in enumerate(planes):
            m = which == p
            pw[m, ax] = val
            nw[m] = nv
        pw += nw * rng.normal(0.0, noise, (n, 1))
        xyz.append((pw @ R[k].T + t[k]).astype(np.float32))
        nrm.append((nw @ R[k].T).astype(np.float32))
    return LidarClouds(xyz, nrm, np.asarray(pose_index, np.int32), current, dist_sq_threshold, weight)


def make_corner_clouds(pose_q, pose_t, *, n_points=200, seed: int = 0, noise: float = 0.02, extent: float = 3.0) -> list:
    """Corner clouds of a seeded scene of line segments seen from K poses: four
    vertical edges (where the walls of ``make_planar_clouds`` would meet a cross
    wall, 4 m to either side of the first camera centre and 2 m / 6 m ahead of
    it) and two horizontal ones along the foot of the walls. Every keyframe
    samples ``n_points`` points (one count or one per keyframe) on the parts of
    the lines within ``extent`` metres of its centre along the line, with
    isotropic Gaussian noise ``noise``, expressed in its sensor frame. Returns
    the list of (n_k, 3) float32 clouds for ``LidarClouds.corner_xyz``."""
    from .synth import quat_to_mat
    q = np.asarray(pose_q, np.float64).reshape(-1, 4)
    t = np.asarray(pose_t, np.float64).reshape(-1, 3)
    K = q.shape[0]
    counts = np.broadcast_to(np.asarray(n_points, np.int64), (K,))
    rng = np.random.default_rng(seed)
    R = quat_to_mat(q)                                   # R_cw
    C = -np.einsum("nji,nj->ni", R, t)                   # camera centres
    c0 = C[0]
    # line: (a point on it, the axis it runs along)
    lines = [(c0 + np.array([sx * 4.0, 0.0, dz]), 1) for sx in (-1.0, 1.0) for dz in (2.0, 6.0)]
    lines += [(c0 + np.array([sx * 4.0, 1.5, 0.0]), 2) for sx in (-1.0, 1.0)]
    out = []
    for k in range(K):
        n = int(counts[k])
        which = rng.integers(0, len(lines), n)
        s = rng.uniform(-extent, extent, n)
        pw = np.zeros((n, 3))
        for l, (p0, ax) in enumerate(lines):
            m = which == l
            pw[m] = p0
            pw[m, ax] = C[k, ax] + s[m]
        pw += rng.normal(0.0, noise, (n, 3))
        out.append((pw @ R[k].T + t[k]).astype(np.float32))
    return out
