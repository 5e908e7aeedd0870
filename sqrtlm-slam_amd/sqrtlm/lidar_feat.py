"""LiDAR flat-feature extraction of a fusion frame: the flat-point path of the
reference's ``Frame::lidarProcess`` (sqlm_lidar_features, include/sqrtlm.h).

``Params`` carries the reference's lidarConfig settings with the defaults
``cfg/lidar_slam.yaml`` ships; ``features`` runs a batch of sweeps on the GPU,
``features_host`` the same text on the CPU; ``lidarProcess`` mirrors the
reference interface for one frame; ``make_sweep`` generates a seeded synthetic
sweep; ``set_lidar_edges`` hands the less-flat clouds of several sweeps to the
existing cloud path of local BA pass 3."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._lib import check, lib, ptr

REASONS = {0: "none", 1: "masked", 2: "curvature", 3: "few_search", 4: "degenerate", 5: "plane_invalid",
           6: "over_cap", 7: "picked"}
NONE, MASKED, CURVATURE, FEW_SEARCH, DEGENERATE, PLANE_INVALID, OVER_CAP, PICKED = range(8)
N_SCANS = 64


@dataclass
class Params:
    """lidarConfig as plain numbers. The four ring ranges are 1-based and
    inclusive, as the reference's settings are."""
    row_num: int = 64
    col_num: int = 1800  # int(360.0 / deg_diff)
    num_scan_subregions: int = 8
    num_curvature_regions_flat: int = 5
    num_curvature_regions_corner: int = 3
    surf_curv_th: float = 0.001
    max_surf_flat: int = 2
    max_surf_less_flat: int = 6
    max_sq_dis: float = 1.0
    deg_diff: float = 0.2
    using_sharp_point: int = 0
    ring_x_rot: tuple = (5, 50)
    ring_y_rot: tuple = (5, 50)
    ring_z_trans: tuple = (5, 50)
    ring_z_rot_xy_trans: tuple = (5, 50)
    ring_enabled: np.ndarray | None = field(default=None, repr=False)  # overrides the ranges

    def enabled(self) -> np.ndarray:
        """ring_enabled[128] from the ranges of Frame.cc:1042-1045; the fourth
        test there compares both ends against the lower bound."""
        if self.ring_enabled is not None:
            e = np.zeros(_lib.LF_MAX_ROWS, np.uint8)
            src = np.asarray(self.ring_enabled, np.uint8)
            e[:len(src)] = src
            return e
        i1 = np.arange(_lib.LF_MAX_ROWS) + 1
        ok = np.zeros(_lib.LF_MAX_ROWS, bool)
        for lo, hi in (self.ring_x_rot, self.ring_y_rot, self.ring_z_trans):
            ok |= (lo <= i1) & (i1 <= hi)
        lo = self.ring_z_rot_xy_trans[0]
        ok |= (lo <= i1) & (i1 <= lo)
        return ok.astype(np.uint8)

    def as_c(self) -> _lib.LidarFeatParams:
        p = _lib.LidarFeatParams()
        for k in ("row_num", "col_num", "num_scan_subregions", "num_curvature_regions_flat",
                  "num_curvature_regions_corner", "max_surf_flat", "max_surf_less_flat", "using_sharp_point"):
            setattr(p, k, int(getattr(self, k)))
        p.surf_curv_th, p.max_sq_dis, p.deg_diff = float(self.surf_curv_th), float(self.max_sq_dis), float(self.deg_diff)
        p.ring_enabled[:] = self.enabled().tolist()
        return p


def _pack(sweeps):
    sweeps = [np.ascontiguousarray(s, np.float32).reshape(-1, 3) for s in sweeps]
    off = np.zeros(len(sweeps) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in sweeps])
    xyz = np.concatenate(sweeps) if sweeps else np.zeros((0, 3), np.float32)
    return off, np.ascontiguousarray(xyz, np.float32)


def _outputs(n_sweep, n):
    m = max(n, 1)
    return dict(flat_off=np.zeros(n_sweep + 1, np.int64), flat_xyz=np.zeros((m, 3), np.float32),
                flat_normal=np.zeros((m, 3), np.float32), less_off=np.zeros(n_sweep + 1, np.int64),
                less_xyz=np.zeros((m, 3), np.float32), less_normal=np.zeros((m, 3), np.float32),
                less_rc=np.zeros((m, 2), np.int32))


def _trim(o):
    kf, kl = int(o["flat_off"][-1]), int(o["less_off"][-1])
    for k in ("flat_xyz", "flat_normal"):
        o[k] = o[k][:kf].copy()
    for k in ("less_xyz", "less_normal", "less_rc"):
        o[k] = o[k][:kl].copy()
    return o


def _state_arrays(n_sweep, n, p: Params):
    m, S = max(n, 1), n_sweep * p.row_num
    a = dict(ring=np.zeros(m, np.int32), scan_off=np.zeros(S + 1, np.int64), scan_src=np.zeros(m, np.int32),
             scan_col=np.zeros(m, np.int32), image_index=np.zeros((max(S, 1), p.col_num), np.int32),
             mask=np.zeros(m, np.uint8), curvature=np.zeros(m, np.float32), neighbours=np.zeros(m, np.int32),
             sorted=np.zeros(m, np.int32), reason=np.zeros(m, np.uint8))
    st = _lib.LidarFeatState()
    for k, v in a.items():
        setattr(st, k, v.ctypes.data)
    return a, st


def _trim_state(a, n_sweep, n, p: Params):
    ns = int(a["scan_off"][-1])
    a["ring"] = a["ring"][:n].copy()
    a["image_index"] = a["image_index"][:n_sweep * p.row_num].copy()
    for k in ("scan_src", "scan_col", "mask", "curvature", "neighbours", "sorted", "reason"):
        a[k] = a[k][:ns].copy()
    return a


def _ext(extrinsic):
    return None if extrinsic is None else np.ascontiguousarray(extrinsic, np.float64).reshape(16)


def features_host(sweeps, params: Params, extrinsic=None, state: bool = False) -> dict:
    """sqlm_lidar_features_host on a list of (n, 3) float32 sweeps. Returns a
    dict of flat_off, flat_xyz, flat_normal, less_off, less_xyz, less_normal,
    less_rc and, with ``state``, the intermediate arrays under "state"."""
    off, xyz = _pack(sweeps)
    n_sweep, n = len(off) - 1, int(off[-1])
    o = _outputs(n_sweep, n)
    pc, e = params.as_c(), _ext(extrinsic)
    a, st = _state_arrays(n_sweep, n, params) if state else (None, None)
    check(lib().sqlm_lidar_features_host(
        n_sweep, ptr(off), ptr(xyz), C.addressof(pc), ptr(e), ptr(o["flat_off"]), ptr(o["flat_xyz"]),
        ptr(o["flat_normal"]), ptr(o["less_off"]), ptr(o["less_xyz"]), ptr(o["less_normal"]), ptr(o["less_rc"]),
        C.addressof(st) if state else None), "sqlm_lidar_features_host")
    o = _trim(o)
    if state:
        o["state"] = _trim_state(a, n_sweep, n, params)
    return o


def features(ctx, sweeps, params: Params, extrinsic=None) -> dict:
    """sqlm_lidar_features: every sweep of the batch in one set of launches."""
    off, xyz = _pack(sweeps)
    n_sweep, n = len(off) - 1, int(off[-1])
    o = _outputs(n_sweep, n)
    pc, e = params.as_c(), _ext(extrinsic)
    check(lib().sqlm_lidar_features(
        ctx._h, n_sweep, ptr(off), ptr(xyz), C.addressof(pc), ptr(e), ptr(o["flat_off"]), ptr(o["flat_xyz"]),
        ptr(o["flat_normal"]), ptr(o["less_off"]), ptr(o["less_xyz"]), ptr(o["less_normal"]), ptr(o["less_rc"])),
        "sqlm_lidar_features")
    ctx._lidar_feat_shape = (n_sweep, n, params)
    return _trim(o)


def features_state(ctx) -> dict:
    """The intermediate state of the context's last ``features`` call."""
    n_sweep, n, params = ctx._lidar_feat_shape
    a, st = _state_arrays(n_sweep, n, params)
    check(lib().sqlm_lidar_features_get_state(ctx._h, C.addressof(st)), "sqlm_lidar_features_get_state")
    return _trim_state(a, n_sweep, n, params)


def features_info(ctx=None) -> dict:
    out = (C.c_int32 * 8)()
    check(lib().sqlm_lidar_features_info(ctx._h if ctx is not None else None, out), "sqlm_lidar_features_info")
    return dict(max_rows=out[0], max_cols=out[1], launches=out[2], largest_subregion=out[3], candidates=out[4],
                evaluated=out[5], picked=out[6], max_half_width=out[7])


def trig_probe(y, x=None) -> np.ndarray:
    """sqlm_atan2(y, x) (sqlm_atan(y) without x) as the library compiled them."""
    y = np.ascontiguousarray(y, np.float64)
    x = None if x is None else np.ascontiguousarray(x, np.float64)
    out = np.zeros_like(y)
    check(lib().sqlm_lidar_feat_trig_probe(y.size, ptr(y), ptr(x), ptr(out)), "sqlm_lidar_feat_trig_probe")
    return out


def lidarProcess(ctx, cloud, params: Params, extrinsic=None):
    """One frame as the reference's Frame constructor leaves it: returns
    (surface_points_flat, surface_points_less_flat,
    surface_points_less_flat_normal, surface_points_less_flat_index), the
    clouds in the extrinsic's target frame."""
    o = features(ctx, [cloud], params, extrinsic)
    return o["flat_xyz"], o["less_xyz"], o["less_normal"], o["less_rc"]


def set_lidar_edges(ctx, pose_index: int, feats: dict, Twc, query: int, info: float, dist_sq_threshold: float) -> int:
    """Local BA pass 3 from extracted features: sweep ``query``'s less-flat
    points and normals are the queries, every other sweep's less-flat cloud a
    map cloud (g2oOptimizer.cc:1045-1068), through Context.set_lidar_from_clouds.
    ``feats`` is a ``features`` result, ``Twc`` one float 4x4 per sweep."""
    off = feats["less_off"]
    others = [k for k in range(len(off) - 1) if k != query]
    maps = [feats["less_xyz"][off[k]:off[k + 1]] for k in others]
    lo, hi = int(off[query]), int(off[query + 1])
    return ctx.set_lidar_from_clouds(pose_index, maps, [Twc[k] for k in others], feats["less_xyz"][lo:hi],
                                     Twc[query], feats["less_normal"][lo:hi], info, dist_sq_threshold)


def ring_elevation_deg(ring):
    """The elevation at the centre of a virtual ring (CalculateRingAndTime inverted)."""
    ring = np.asarray(ring, np.float64)
    return np.where(ring < 32, 2.0 - ring / 3.0, -8.83 - (ring - 32) / 2.0)


def make_sweep(seed: int, n_az: int = 1800, order: str = "ring", noise: float = 0.01, dropout: float = 0.02,
               start_deg: float = 0.0, n_boxes: int = 6, room: float = 25.0, ground_z: float = -1.73,
               max_range: float = 80.0, pose=None, rings=None) -> np.ndarray:
    """A seeded synthetic sweep: a ground plane, four vertical walls and
    ``n_boxes`` boxes, sampled along 64 elevation rays x ``n_az`` azimuths
    (clockwise, as the sensor turns), with range noise and dropouts. ``order``
    is "ring" (ring-major) or "azimuth" (azimuth-major input order). ``pose``
    (R, t) places the sensor in the scene; the points are in the sensor frame. ``rings`` restricts the rays to those
    virtual rings (all 64 by default)."""
    rng = np.random.default_rng(seed)
    rings = np.arange(N_SCANS) if rings is None else np.asarray(list(rings), np.int64)
    n_el = len(rings)
    el = np.deg2rad(ring_elevation_deg(rings))
    az = np.deg2rad(start_deg) - 2.0 * np.pi * (np.arange(n_az) + 0.5) / n_az
    E, A = np.meshgrid(el, az, indexing="ij")
    d = np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], -1).reshape(-1, 3)
    R, t = (np.eye(3), np.zeros(3)) if pose is None else (np.asarray(pose[0], float), np.asarray(pose[1], float))
    dw, ow = d @ R.T, t  # rays in the scene
    boxes = [(np.array([-room, -room, ground_z - 1.0]), np.array([room, room, ground_z]), False),  # the ground slab
             (np.array([-room, -room, ground_z]), np.array([room, room, 30.0]), True)]            # the room, from inside
    brng = np.random.default_rng(1000 + n_boxes)  # the scene does not depend on the sweep's seed
    for _ in range(n_boxes):
        c = np.array([brng.uniform(-room + 4, room - 4), brng.uniform(-room + 4, room - 4), ground_z])
        if np.hypot(c[0], c[1]) < 5.0:
            c[:2] += 6.0
        h = np.array([brng.uniform(0.8, 3.0), brng.uniform(0.8, 3.0), brng.uniform(1.0, 4.0)])
        boxes.append((c - [h[0], h[1], 0.0], c + [h[0], h[1], h[2]], False))
    best = np.full(len(dw), np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / dw
        for lo, hi, inside in boxes:
            t0, t1 = (lo - ow) * inv, (hi - ow) * inv
            tn, tf = np.minimum(t0, t1).max(1), np.maximum(t0, t1).min(1)
            hit = tf if inside else tn
            ok = (tn <= tf) & (hit > 0.5)
            best = np.where(ok & (hit < best), hit, best)
    r = best + rng.normal(0.0, noise, len(best))
    keep = np.isfinite(r) & (r < max_range) & (r > 1.0) & (rng.random(len(r)) >= dropout)
    pts = (d * np.where(keep, r, 0.0)[:, None]).astype(np.float32).reshape(n_el, n_az, 3)
    keep = keep.reshape(n_el, n_az)
    if order == "azimuth":
        pts, keep = pts.transpose(1, 0, 2), keep.T
    elif order != "ring":
        raise ValueError(order)
    return np.ascontiguousarray(pts[keep], np.float32)
