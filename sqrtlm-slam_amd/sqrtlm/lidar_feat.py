"""LiDAR flat-feature extraction of a fusion frame: the flat-point path of the
reference's ``Frame::lidarProcess`` (sqlm_lidar_features, include/sqrtlm.h).

``Params`` carries the reference's lidarConfig settings with the defaults
``cfg/lidar_slam.yaml`` ships; ``features`` runs a batch of sweeps on the GPU,
``features_host`` the same text on the CPU; ``lidarProcess`` mirrors the
reference interface for one frame; ``make_sweep`` generates a seeded synthetic
sweep; ``set_lidar_edges`` hands the less-flat clouds of several sweeps to the
existing cloud path of local BA pass 3.

``CornerParams`` adds the settings of the corner branch; ``features_all`` /
``features_all_host`` run both branches on one range image
(sqlm_lidar_features_all), ``features_all_state`` / ``features_all_info`` read
back what the last call did, and ``set_lidar_edge_sets`` hands the less-flat and
the less-sharp clouds to local BA pass 3 as a flat and a corner set."""
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


CORNER_REASONS = {0: "none", 1: "ground", 2: "masked", 3: "curvature", 4: "unstable", 5: "over_cap", 6: "picked"}
LC_NONE, LC_GROUND, LC_MASKED, LC_CURVATURE, LC_UNSTABLE, LC_OVER_CAP, LC_PICKED = range(7)
# the six distinct (row, column) offsets of Frame.cc:929-938, bit k of a cell's edge mask
CORNER_OFFSETS = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1))


@dataclass
class CornerParams:
    """The corner settings of lidarConfig with the defaults cfg/lidar_slam.yaml
    ships. The ring range is the reference's: ring i (0-based) takes part when
    lower <= i + 1 and i < upper."""
    max_corner_sharp: int = 3
    max_corner_less_sharp: int = 30
    sharp_curv_th: float = 20.0
    ground_z_bound: float = -1.5
    lower_ring_num_sharp_point: int = 1
    upper_ring_num_sharp_point: int = 40
    ring_enabled: np.ndarray | None = field(default=None, repr=False)  # overrides the range

    def enabled(self) -> np.ndarray:
        """corner_ring_enabled[128] from the two bounds of Frame.cc:862."""
        if self.ring_enabled is not None:
            e = np.zeros(_lib.LF_MAX_ROWS, np.uint8)
            src = np.asarray(self.ring_enabled, np.uint8)
            e[:len(src)] = src
            return e
        i = np.arange(_lib.LF_MAX_ROWS)
        return ((self.lower_ring_num_sharp_point <= i + 1) & (i < self.upper_ring_num_sharp_point)).astype(np.uint8)

    def as_c(self) -> _lib.LidarCornerParams:
        p = _lib.LidarCornerParams()
        p.max_corner_sharp, p.max_corner_less_sharp = int(self.max_corner_sharp), int(self.max_corner_less_sharp)
        p.sharp_curv_th, p.ground_z_bound = float(self.sharp_curv_th), float(self.ground_z_bound)
        p.corner_ring_enabled[:] = self.enabled().tolist()
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


def _corner_outputs(n_sweep, n):
    m = max(n, 1)
    return dict(sharp_off=np.zeros(n_sweep + 1, np.int64), sharp_xyz=np.zeros((m, 3), np.float32),
                less_sharp_off=np.zeros(n_sweep + 1, np.int64), less_sharp_xyz=np.zeros((m, 3), np.float32),
                less_sharp_label=np.zeros(m, np.int32), less_sharp_rc=np.zeros((m, 2), np.int32))


_CORNER_ORDER = ("sharp_off", "sharp_xyz", "less_sharp_off", "less_sharp_xyz", "less_sharp_label", "less_sharp_rc")
_FLAT_ORDER = ("flat_off", "flat_xyz", "flat_normal", "less_off", "less_xyz", "less_normal", "less_rc")


def _trim_corner(o):
    ks, kl = int(o["sharp_off"][-1]), int(o["less_sharp_off"][-1])
    o["sharp_xyz"] = o["sharp_xyz"][:ks].copy()
    for k in ("less_sharp_xyz", "less_sharp_label", "less_sharp_rc"):
        o[k] = o[k][:kl].copy()
    return o


def _corner_state_arrays(n_sweep, n, p: Params):
    m, S = max(n, 1), max(n_sweep * p.row_num, 1)
    a = dict(cell_state=np.zeros((S, p.col_num), np.int32), mask=np.zeros(m, np.uint8), curvature=np.zeros(m, np.float32),
             sorted=np.zeros(m, np.int32), reason=np.zeros(m, np.uint8), edge=np.zeros((S, p.col_num), np.uint8),
             angle=np.zeros((S, p.col_num, 6), np.float32))
    st = _lib.LidarCornerState()
    for k, v in a.items():
        setattr(st, k, v.ctypes.data)
    return a, st


def _trim_corner_state(a, n_sweep, ns, p: Params):
    S = n_sweep * p.row_num
    for k in ("cell_state", "edge", "angle"):
        a[k] = a[k][:S].copy()
    for k in ("mask", "curvature", "sorted", "reason"):
        a[k] = a[k][:ns].copy()
    return a


def _all_args(sweeps, params, corner, extrinsic, flat):
    off, xyz = _pack(sweeps)
    n_sweep, n = len(off) - 1, int(off[-1])
    o = _outputs(n_sweep, n) if flat else {}
    if corner is not None:
        o.update(_corner_outputs(n_sweep, n))
    pc, cc, e = params.as_c(), None if corner is None else corner.as_c(), _ext(extrinsic)
    args = [n_sweep, ptr(off), ptr(xyz), C.addressof(pc), None if cc is None else C.addressof(cc), ptr(e)]
    args += [ptr(o[k]) if flat else None for k in _FLAT_ORDER]
    args += [ptr(o[k]) if corner is not None else None for k in _CORNER_ORDER]
    return off, n_sweep, n, o, args, (pc, cc, e, xyz)


def _finish_all(o, flat, corner):
    if flat:
        o = _trim(o)
    if corner is not None:
        o = _trim_corner(o)
    return o


def features_all_host(sweeps, params: Params, corner: CornerParams | None = None, extrinsic=None, state: bool = False,
                      flat: bool = True) -> dict:
    """sqlm_lidar_features_all_host: the flat outputs of ``features_host``
    (unless ``flat`` is False) and, with ``corner``, sharp_off, sharp_xyz,
    less_sharp_off, less_sharp_xyz, less_sharp_label, less_sharp_rc; with
    ``state`` the flat state under "state" and the corner state under
    "corner_state"."""
    off, n_sweep, n, o, args, keep = _all_args(sweeps, params, corner, extrinsic, flat)
    a, st = _state_arrays(n_sweep, n, params) if state else (None, None)
    ca, cst = _corner_state_arrays(n_sweep, n, params) if state and corner is not None else (None, None)
    check(lib().sqlm_lidar_features_all_host(*args, C.addressof(st) if st is not None else None,
                                             C.addressof(cst) if cst is not None else None),
          "sqlm_lidar_features_all_host")
    o = _finish_all(o, flat, corner)
    if state:
        o["state"] = _trim_state(a, n_sweep, n, params)
        if ca is not None:
            o["corner_state"] = _trim_corner_state(ca, n_sweep, len(o["state"]["mask"]), params)
    return o


def features_all(ctx, sweeps, params: Params, corner: CornerParams | None = None, extrinsic=None,
                 flat: bool = True) -> dict:
    """sqlm_lidar_features_all: both branches of every sweep of the batch on
    one upload and one range image. ``corner`` None runs the flat branch alone
    and equals ``features``."""
    off, n_sweep, n, o, args, keep = _all_args(sweeps, params, corner, extrinsic, flat)
    check(lib().sqlm_lidar_features_all(ctx._h, *args), "sqlm_lidar_features_all")
    ctx._lidar_feat_shape = (n_sweep, n, params)
    ctx._lidar_corner = corner is not None
    return _finish_all(o, flat, corner)


def features_all_state(ctx) -> dict:
    """{"state": flat state, "corner_state": corner state} of the context's
    last ``features_all`` (the corner state only if it ran a corner stage)."""
    n_sweep, n, params = ctx._lidar_feat_shape
    a, st = _state_arrays(n_sweep, n, params)
    ca, cst = _corner_state_arrays(n_sweep, n, params) if ctx._lidar_corner else (None, None)
    check(lib().sqlm_lidar_features_all_get_state(ctx._h, C.addressof(st), C.addressof(cst) if cst is not None else None),
          "sqlm_lidar_features_all_get_state")
    out = dict(state=_trim_state(a, n_sweep, n, params))
    if ca is not None:
        out["corner_state"] = _trim_corner_state(ca, n_sweep, len(out["state"]["mask"]), params)
    return out


def features_all_info(ctx=None) -> dict:
    out = (C.c_int32 * 8)()
    check(lib().sqlm_lidar_features_all_info(ctx._h if ctx is not None else None, out), "sqlm_lidar_features_all_info")
    return dict(launches=out[0], seeds_grown=out[1], cells_labelled=out[2], cells_unstable=out[3],
                largest_segment=out[4], most_levels=out[5], less_sharp=out[6], sharp=out[7])


def corner_trig_probe(which: str, x) -> np.ndarray:
    """sqlm_acos / sqlm_sin / sqlm_cos as the library compiled them."""
    x = np.ascontiguousarray(x, np.float64)
    out = np.zeros_like(x)
    check(lib().sqlm_lidar_corner_trig_probe(x.size, {"acos": 0, "sin": 1, "cos": 2}[which], ptr(x), ptr(out)),
          "sqlm_lidar_corner_trig_probe")
    return out


def corner_angle_probe(p1, p2) -> np.ndarray:
    """The float angle of the corner branch's edge predicate for point pairs, on the host."""
    p1 = np.ascontiguousarray(p1, np.float32).reshape(-1, 3)
    p2 = np.ascontiguousarray(p2, np.float32).reshape(-1, 3)
    out = np.zeros(len(p1), np.float32)
    check(lib().sqlm_lidar_corner_angle_probe(len(p1), ptr(p1), ptr(p2), ptr(out)), "sqlm_lidar_corner_angle_probe")
    return out


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


def lidarProcess(ctx, cloud, params: Params, extrinsic=None, corner: CornerParams | None = None):
    """One frame as the reference's Frame constructor leaves it: returns
    (surface_points_flat, surface_points_less_flat,
    surface_points_less_flat_normal, surface_points_less_flat_index), the
    clouds in the extrinsic's target frame. With ``corner`` both branches run
    (``features_all``) and the tuple continues with (corner_points_sharp,
    corner_points_less_sharp, the less-sharp labels)."""
    if corner is None:
        o = features(ctx, [cloud], params, extrinsic)
        return o["flat_xyz"], o["less_xyz"], o["less_normal"], o["less_rc"]
    o = features_all(ctx, [cloud], params, corner, extrinsic)
    return (o["flat_xyz"], o["less_xyz"], o["less_normal"], o["less_rc"], o["sharp_xyz"], o["less_sharp_xyz"],
            o["less_sharp_label"])


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


def set_lidar_edge_sets(ctx, pose_index: int, feats: dict, Twc, query: int, info: float, dist_sq_threshold: float,
                        corner_info: float | None = None, corner_dist_sq_threshold: float | None = None) -> list:
    """Local BA pass 3 from a ``features_all`` result: a flat set (sweep
    ``query``'s less-flat points and normals against every other sweep's
    less-flat cloud) and a corner set (its less-sharp points against the other
    sweeps' less-sharp clouds) through Context.set_lidar_from_cloud_sets;
    returns the pair count of each."""
    others = [k for k in range(len(feats["less_off"]) - 1) if k != query]
    sets = []
    for kind, off, xyz, nrm, w, th in (
            (0, feats["less_off"], feats["less_xyz"], feats["less_normal"], info, dist_sq_threshold),
            (1, feats["less_sharp_off"], feats["less_sharp_xyz"], None,
             info if corner_info is None else corner_info,
             dist_sq_threshold if corner_dist_sq_threshold is None else corner_dist_sq_threshold)):
        lo, hi = int(off[query]), int(off[query + 1])
        sets.append(dict(kind=kind, map_clouds=[xyz[off[k]:off[k + 1]] for k in others], map_Twc=[Twc[k] for k in others],
                         query_xyz=xyz[lo:hi], query_Twc=Twc[query], query_normal=None if nrm is None else nrm[lo:hi],
                         info=w, dist_sq_threshold=th))
    return ctx.set_lidar_from_cloud_sets(pose_index, sets)


def ring_elevation_deg(ring):
    """The elevation at the centre of a virtual ring (CalculateRingAndTime inverted)."""
    ring = np.asarray(ring, np.float64)
    return np.where(ring < 32, 2.0 - ring / 3.0, -8.83 - (ring - 32) / 2.0)


def make_sweep(seed: int, n_az: int = 1800, order: str = "ring", noise: float = 0.01, dropout: float = 0.02,
               start_deg: float = 0.0, n_boxes: int = 6, room: float = 25.0, ground_z: float = -1.73,
               max_range: float = 80.0, pose=None, rings=None, n_poles: int = 0) -> np.ndarray:
    """A seeded synthetic sweep: a ground plane, four vertical walls and
    ``n_boxes`` boxes, sampled along 64 elevation rays x ``n_az`` azimuths
    (clockwise, as the sensor turns), with range noise and dropouts. ``order``
    is "ring" (ring-major) or "azimuth" (azimuth-major input order). ``pose``
    (R, t) places the sensor in the scene; the points are in the sensor frame. ``rings`` restricts the rays to those
    virtual rings (all 64 by default). ``n_poles`` adds that many thin free-standing
    poles (0.3 m square, 6 m tall), the scenery that yields corner points; the
    default of 0 leaves every existing seed's sweep as it was."""
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
    prng = np.random.default_rng([2000 + n_poles, seed])  # the poles move with the sweep's seed; the boxes above do not
    for _ in range(n_poles):
        a, rad = prng.uniform(0.0, 2.0 * np.pi), prng.uniform(5.0, room - 6.0)
        c = np.array([rad * np.cos(a), rad * np.sin(a), ground_z])
        boxes.append((c - [0.15, 0.15, 0.0], c + [0.15, 0.15, 6.0], False))
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
