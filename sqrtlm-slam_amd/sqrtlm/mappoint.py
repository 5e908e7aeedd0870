"""Host-side mirror of LocalMapping's map-point steps over the C ABI
(include/sqrtlm_orb.h): the match loop of ``LocalMapping::CreateNewMapPoints``
(src/backend/LocalMapping.cc:436-624 of the reference) as
``sqlm_triangulate_pairs`` and ``MapPoint::ComputeDistinctiveDescriptors`` /
``UpdateNormalAndDepth`` (src/data_structure/MapPoint.cc:382-481, :531-578) as
``sqlm_map_points_update``. The array packing, the host-only twins, synthetic
two-view / many-view scenes with planted points and the small mirrors
``CreateNewMapPoints`` / ``UpdateMapPoints``. The work runs on the GPU
(libsqrtlm.so); the ``*_host`` functions run the same text on the CPU and need
no context.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from ._lib import check, lib, ptr
from .orb import KP_DTYPE

REASONS = ("created", "parallax", "w_zero", "z1", "z2", "reproj1", "reproj2", "zero_dist", "scale")


class _TriFrame(C.Structure):
    _fields_ = [("kps", C.c_void_p), ("uright", C.c_void_p), ("scale_factors", C.c_void_p),
                ("level_sigma2", C.c_void_p), ("n", C.c_int32), ("n_levels", C.c_int32), ("Tcw", C.c_float * 12),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("invfx", C.c_float),
                ("invfy", C.c_float)]


class _TriPair(C.Structure):
    _fields_ = [("kf1", _TriFrame), ("kf2", _TriFrame), ("ratio_factor", C.c_float), ("pad", C.c_int32)]


class TriKeyFrame:
    """The KeyFrame fields CreateNewMapPoints reads: mvKeysUn, mvuRight (None:
    monocular), mvScaleFactors, mvLevelSigma2 (None: the squares of the scale
    factors, as ORBextractor fills it), the 3x4 Tcw, fx fy cx cy (invfx, invfy
    = 1.0f / fx, 1.0f / fy as Frame computes them unless given)."""

    def __init__(self, mvKeysUn, mvScaleFactors, Tcw, fx, fy, cx, cy, mvLevelSigma2=None, mvuRight=None,
                 invfx=None, invfy=None):
        self.mvKeysUn = np.array(mvKeysUn, KP_DTYPE, order="C")  # copies: a keyframe owns its arrays
        self.N = len(self.mvKeysUn)
        self.mvScaleFactors = np.ascontiguousarray(mvScaleFactors, np.float32)
        self.mvLevelSigma2 = (self.mvScaleFactors * self.mvScaleFactors if mvLevelSigma2 is None
                              else np.ascontiguousarray(mvLevelSigma2, np.float32))
        if self.mvLevelSigma2.shape != self.mvScaleFactors.shape:
            raise ValueError("mvLevelSigma2 must hold one entry per level")
        self.Tcw = np.array(np.asarray(Tcw, np.float32)[:3, :4], order="C")
        f32 = np.float32
        self.fx, self.fy, self.cx, self.cy = f32(fx), f32(fy), f32(cx), f32(cy)
        with np.errstate(all="ignore"):
            self.invfx = f32(1.0) / self.fx if invfx is None else f32(invfx)
            self.invfy = f32(1.0) / self.fy if invfy is None else f32(invfy)
        self.mvuRight = None if mvuRight is None else np.ascontiguousarray(mvuRight, np.float32)
        if self.mvuRight is not None and self.mvuRight.shape != (self.N,):
            raise ValueError("mvuRight must hold one entry per keypoint")

    @property
    def cam(self):
        return np.array([self.fx, self.fy, self.cx, self.cy, self.invfx, self.invfy], np.float32)

    def _fill(self, f: _TriFrame) -> None:
        f.kps = self.mvKeysUn.ctypes.data if self.N else None
        f.uright = None if self.mvuRight is None else self.mvuRight.ctypes.data
        f.scale_factors, f.level_sigma2 = self.mvScaleFactors.ctypes.data, self.mvLevelSigma2.ctypes.data
        f.n, f.n_levels = self.N, len(self.mvScaleFactors)
        f.Tcw = (C.c_float * 12)(*self.Tcw.reshape(12).tolist())
        f.fx, f.fy, f.cx, f.cy, f.invfx, f.invfy = (float(v) for v in self.cam)


@dataclass
class TriPair:
    """One (mpCurrentKeyFrame, pKF2) pair with its vMatchedIndices [m][2] and
    ratioFactor = 1.5f * mfScaleFactor."""
    kf1: TriKeyFrame
    kf2: TriKeyFrame
    matches: np.ndarray
    ratio_factor: float = float(np.float32(1.5) * np.float32(1.2))
    meta: dict = field(default_factory=dict)

    def __post_init__(self):
        self.matches = np.ascontiguousarray(self.matches, np.int32).reshape(-1, 2)


def _pack_pairs(pairs):
    arr = (_TriPair * max(len(pairs), 1))()
    off = np.zeros(len(pairs) + 1, np.int64)
    for k, p in enumerate(pairs):
        p.kf1._fill(arr[k].kf1)
        p.kf2._fill(arr[k].kf2)
        arr[k].ratio_factor = float(p.ratio_factor)
        off[k + 1] = off[k] + len(p.matches)
    m = (np.concatenate([p.matches for p in pairs]) if pairs else np.zeros((0, 2), np.int32))
    return arr, off, np.ascontiguousarray(m, np.int32)


def _tri_call(pairs, fn, what):
    arr, off, m = _pack_pairs(pairs)
    n = int(off[-1])
    x3d, reason = np.zeros((n, 3), np.float32), np.zeros(n, np.uint8)
    n_new = np.zeros(len(pairs), np.int32)
    check(fn(arr, off, m, x3d, reason, n_new), what)
    return dict(x3d=x3d, reason=reason, n_new=n_new, off=off)


def triangulate_pairs(ctx, pairs):
    """sqlm_triangulate_pairs: dict(x3d [n][3], reason [n], n_new [n_pair], off) over the concatenated matches."""
    return _tri_call(pairs, lambda a, off, m, x, r, nn: lib().sqlm_triangulate_pairs(
        ctx._h, len(pairs), a, ptr(off), ptr(m), ptr(x), ptr(r), ptr(nn)), "sqlm_triangulate_pairs")


def triangulate_pairs_host(pairs, sweeps=0):
    """The same text on the CPU (sqlm_triangulate_pairs_host); sweeps = 0: the library's Jacobi sweep count."""
    return _tri_call(pairs, lambda a, off, m, x, r, nn: lib().sqlm_triangulate_pairs_host(
        len(pairs), a, ptr(off), ptr(m), int(sweeps), ptr(x), ptr(r), ptr(nn)), "sqlm_triangulate_pairs_host")


def triangulate_info():
    """dict(sweeps, block, wave): the Jacobi sweeps and the kernel's workgroup and wavefront sizes in matches."""
    out = (C.c_int32 * 4)()
    check(lib().sqlm_triangulate_info(out), "sqlm_triangulate_info")
    return dict(sweeps=out[0], block=out[1], wave=out[2])


@dataclass
class MapPointBatch:
    """A batch of map points for sqlm_map_points_update: per point its
    observations in the caller's order (obs_off CSR), their descriptors
    [n_obs][32] and camera centres [n_obs][3] (either may be None), mWorldPos,
    the reference keyframe's centre and the two scale factors."""
    obs_off: np.ndarray
    obs_desc: np.ndarray | None
    obs_center: np.ndarray | None
    pos: np.ndarray | None = None
    ref_center: np.ndarray | None = None
    level_scale: np.ndarray | None = None
    max_scale: np.ndarray | None = None
    meta: dict = field(default_factory=dict)

    def __post_init__(self):
        self.obs_off = np.ascontiguousarray(self.obs_off, np.int64)
        n_obs = int(self.obs_off[-1])
        if self.obs_desc is not None:
            self.obs_desc = np.ascontiguousarray(self.obs_desc, np.uint8).reshape(n_obs, 32)
        if self.obs_center is not None:
            self.obs_center = np.ascontiguousarray(self.obs_center, np.float32).reshape(n_obs, 3)
            self.pos = np.ascontiguousarray(self.pos, np.float32).reshape(self.n_pt, 3)
            self.ref_center = np.ascontiguousarray(self.ref_center, np.float32).reshape(self.n_pt, 3)
            self.level_scale = np.ascontiguousarray(self.level_scale, np.float32).reshape(self.n_pt)
            self.max_scale = np.ascontiguousarray(self.max_scale, np.float32).reshape(self.n_pt)

    @property
    def n_pt(self):
        return len(self.obs_off) - 1

    def halves(self, desc=True, normal=True):
        """The same batch with one half switched off."""
        return MapPointBatch(self.obs_off, self.obs_desc if desc else None, self.obs_center if normal else None,
                             self.pos, self.ref_center, self.level_scale, self.max_scale, self.meta)

    def select(self, idx):
        """The batch of the points idx, in that order."""
        idx = [int(i) for i in idx]
        cnt = [int(self.obs_off[i + 1] - self.obs_off[i]) for i in idx]
        off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        rows = (np.concatenate([np.arange(self.obs_off[i], self.obs_off[i + 1]) for i in idx]).astype(np.int64)
                if idx else np.zeros(0, np.int64))
        take = lambda a: None if a is None else a[rows]
        per = lambda a: None if a is None else a[idx]
        return MapPointBatch(off, take(self.obs_desc), take(self.obs_center), per(self.pos), per(self.ref_center),
                             per(self.level_scale), per(self.max_scale))


def _mp_call(b: MapPointBatch, fn, what):
    n = b.n_pt
    out = dict(best_idx=np.zeros(n, np.int32), best_median=np.zeros(n, np.int32), normal=np.zeros((n, 3), np.float32),
               max_dist=np.zeros(n, np.float32), min_dist=np.zeros(n, np.float32))
    check(fn(n, ptr(b.obs_off), ptr(b.obs_desc), ptr(b.obs_center), ptr(b.pos), ptr(b.ref_center), ptr(b.level_scale),
             ptr(b.max_scale), ptr(out["best_idx"]), ptr(out["best_median"]), ptr(out["normal"]),
             ptr(out["max_dist"]), ptr(out["min_dist"])), what)
    if b.obs_desc is None:
        del out["best_idx"], out["best_median"]
    if b.obs_center is None:
        del out["normal"], out["max_dist"], out["min_dist"]
    return out


def map_points_update(ctx, batch: MapPointBatch):
    """sqlm_map_points_update: dict(best_idx, best_median, normal, max_dist, min_dist), a half's keys only if it ran."""
    return _mp_call(batch, lambda *a: lib().sqlm_map_points_update(ctx._h, *a), "sqlm_map_points_update")


def map_points_update_host(batch: MapPointBatch):
    return _mp_call(batch, lambda *a: lib().sqlm_map_points_update_host(*a), "sqlm_map_points_update_host")


def map_points_update_info(ctx=None):
    """dict(lds_max, n_lds, n_global, n_launch): the longest track whose descriptors the kernel keeps in LDS and,
    of the context's last call, the points on each descriptor path and the kernels launched."""
    out = (C.c_int32 * 4)()
    check(lib().sqlm_map_points_update_info(None if ctx is None else ctx._h, out), "sqlm_map_points_update_info")
    return dict(lds_max=out[0], n_lds=out[1], n_global=out[2], n_launch=out[3])


# ---- synthetic scenes ----

def orb_scale_factors(n_levels=8, scale_factor=1.2):
    """mvScaleFactors as ORBextractor fills it: float products (ORBextractor.cc:484-494)."""
    sf = np.ones(n_levels, np.float32)
    for i in range(1, n_levels):
        sf[i] = sf[i - 1] * np.float32(scale_factor)
    return sf


def _rot(w):
    th = float(np.linalg.norm(w))
    if th == 0:
        return np.eye(3)
    k = np.asarray(w, float) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def make_pose(rvec, center):
    """Tcw (3x4 float32) of a camera at `center` with rotation exp(rvec)."""
    R = _rot(rvec)
    T = np.zeros((3, 4))
    T[:, :3] = R
    T[:, 3] = -R @ np.asarray(center, float)
    return T.astype(np.float32)


def project(T, cam, X):
    Xc = np.asarray(X, float) @ np.asarray(T, float)[:, :3].T + np.asarray(T, float)[:, 3]
    return np.stack([cam[0] * Xc[:, 0] / Xc[:, 2] + cam[2], cam[1] * Xc[:, 1] / Xc[:, 2] + cam[3]], 1), Xc[:, 2]


def make_two_view(n, seed=0, pixel_noise=0.5, baseline=1.0, depth=(4.0, 12.0), cam=(718.856, 718.856, 607.1928, 185.2157),
                  n_levels=8):
    """A keyframe pair with n planted points seen by both: TriPair with meta['X'] (the planted points) and matches
    (i, perm[i]); both keypoints of a match share an octave, so the scale test agrees with the geometry."""
    rng = np.random.default_rng(seed)
    sf = orb_scale_factors(n_levels)
    T1 = make_pose(rng.normal(size=3) * 0.02, rng.normal(size=3) * 0.05)
    T2 = make_pose(rng.normal(size=3) * 0.03, np.array([baseline, 0.1 * baseline, 0.15 * baseline]))
    X = np.stack([rng.uniform(-3, 3, n), rng.uniform(-1, 1, n), rng.uniform(*depth, n)], 1)
    octave = rng.integers(0, n_levels, n).astype(np.int32)
    perm = rng.permutation(n)
    kps = []
    for T, order in ((T1, np.arange(n)), (T2, perm)):
        uv, _ = project(T, cam, X)
        uv = uv + rng.normal(size=uv.shape) * pixel_noise
        k = np.zeros(n, KP_DTYPE)
        k["x"][order], k["y"][order] = uv[:, 0], uv[:, 1]
        k["octave"][order] = octave
        k["size"] = 31.0
        kps.append(k)
    kf1 = TriKeyFrame(kps[0], sf, T1, *cam)
    kf2 = TriKeyFrame(kps[1], sf, T2, *cam)
    matches = np.stack([np.arange(n), perm], 1).astype(np.int32)
    return TriPair(kf1, kf2, matches, meta=dict(X=X, perm=perm))


def make_tracks(counts, seed=0, n_levels=8, flip_bits=40):
    """A batch of map points with the given observation counts: every point has a base descriptor, each
    observation's is that with up to `flip_bits` random bits flipped; camera centres on an arc around the point."""
    rng = np.random.default_rng(seed)
    counts = [int(c) for c in counts]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    n_obs, n_pt = int(off[-1]), len(counts)
    desc = np.zeros((n_obs, 32), np.uint8)
    center = np.zeros((n_obs, 3), np.float32)
    pos = rng.uniform(-5, 5, (n_pt, 3)).astype(np.float32)
    pos[:, 2] += 10
    sf = orb_scale_factors(n_levels)
    for j, c in enumerate(counts):
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        for i in range(c):
            bits = np.unpackbits(base)
            flip = rng.choice(256, int(rng.integers(0, flip_bits + 1)), replace=False)
            bits[flip] ^= 1
            desc[off[j] + i] = np.packbits(bits)
        center[off[j]:off[j + 1]] = rng.normal(size=(c, 3)) * 2.0
    ref_center = np.stack([center[off[j]] if c else np.zeros(3, np.float32) for j, c in enumerate(counts)]
                          ).astype(np.float32).reshape(n_pt, 3)
    level_scale = sf[rng.integers(0, n_levels, n_pt)]
    max_scale = np.full(n_pt, sf[-1], np.float32)
    return MapPointBatch(off, desc, center, pos, ref_center, level_scale, max_scale)


# ---- small mirrors of the reference's loops ----

def CreateNewMapPoints(ctx, pairs):
    """The match loops of CreateNewMapPoints for the given pairs: per pair the list of (idx1, idx2, x3D) of the map
    points the reference would create, in match order, and nnew."""
    o = triangulate_pairs(ctx, pairs)
    created = []
    for k, p in enumerate(pairs):
        lo, hi = int(o["off"][k]), int(o["off"][k + 1])
        created.append([(int(p.matches[i - lo, 0]), int(p.matches[i - lo, 1]), o["x3d"][i].copy())
                        for i in range(lo, hi) if o["reason"][i] == 0])
    return created, int(o["n_new"].sum())


def UpdateMapPoints(ctx, batch: MapPointBatch, mDescriptor=None):
    """ComputeDistinctiveDescriptors + UpdateNormalAndDepth of every point: (mDescriptor [n_pt][32], normal,
    max_dist, min_dist). A point without observations keeps its row of `mDescriptor` (zeros if none is given)."""
    o = map_points_update(ctx, batch)
    d = np.zeros((batch.n_pt, 32), np.uint8) if mDescriptor is None else np.array(mDescriptor, np.uint8)
    for j in range(batch.n_pt):
        if o["best_idx"][j] >= 0:
            d[j] = batch.obs_desc[batch.obs_off[j] + o["best_idx"][j]]
    return d, o["normal"], o["max_dist"], o["min_dist"]
