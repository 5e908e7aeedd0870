"""LiDAR depth image and keypoint depth association of a fusion frame: the part
of the reference's ``Frame`` constructor that projects the sweep into
``Depthimg_`` and gives every ORB keypoint a ``class_id`` and an ``mvDepth``
(sqlm_lidar_depth, include/sqrtlm.h).

``depth`` runs a batch of frames on the GPU, ``depth_host`` the same text on
the CPU; ``depth_state`` reads back the intermediate state of the context's last
call, ``depth_info`` the limits and the launches; ``frame_depth`` mirrors what
the constructor leaves behind for one frame; ``make_keypoints`` generates seeded
keypoints (the sweep comes from ``lidar_feat.make_sweep``)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import check, lib, ptr
from .synth import KITTI_INTR

HALF_W, HALF_H = 4, 7
MIN_X, MAX_RANGE = 1.0, 2.0
MAX_DIM, MAX_CELLS = 4096, 1 << 25
KITTI_ROWS, KITTI_COLS = 376, 1241
# cfg/KITTI00-02.yaml:8-19 as the 3x4 intrinsicMatrix of the fusion frame
KITTI_INTRINSIC = np.array([[KITTI_INTR[0], 0.0, KITTI_INTR[2], 0.0],
                            [0.0, KITTI_INTR[1], KITTI_INTR[3], 0.0],
                            [0.0, 0.0, 1.0, 0.0]])
KITTI_CAM = np.asarray(KITTI_INTR, np.float32)
# velodyne to camera, written by hand: sensor x (forward) -> camera z, y (left) -> -x, z (up) -> -y,
# with a small lever arm
VELO_TO_CAM = np.array([[0.0, -1.0, 0.0, 0.02],
                        [0.0, 0.0, -1.0, -0.08],
                        [1.0, 0.0, 0.0, -0.27],
                        [0.0, 0.0, 0.0, 1.0]])
STATS = ("min_v", "n_written", "n_occupied", "n_with_depth")


def _pack(items, width):
    items = [np.ascontiguousarray(s, np.float32).reshape(-1, width) for s in items]
    off = np.zeros(len(items) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in items])
    a = np.concatenate(items) if items else np.zeros((0, width), np.float32)
    return off, np.ascontiguousarray(a, np.float32)


def _args(sweeps, keys, keys_un, rows, cols, intrinsic, extrinsic, cam, image):
    if len(sweeps) != len(keys) or (keys_un is not None and len(keys_un) != len(keys)):
        raise ValueError("one sweep, one keypoint list (and one undistorted list) per frame")
    soff, xyz = _pack(sweeps, 3)
    koff, kxy = _pack(keys, 2)
    kun = None
    if keys_un is not None:
        uoff, kun = _pack(keys_un, 2)
        if not np.array_equal(uoff, koff):
            raise ValueError("keys_un does not match keys")
    nf, m = len(soff) - 1, int(koff[-1])
    unproject = keys_un is not None and cam is not None
    a = dict(n_frame=nf, n=int(soff[-1]), m=m, rows=int(rows), cols=int(cols), sweep_off=soff, key_off=koff, xyz=xyz,
             key_xy=kxy, key_un_xy=kun if unproject else None,
             intrinsic=np.ascontiguousarray(intrinsic, np.float64).reshape(12),
             extrinsic=np.ascontiguousarray(extrinsic, np.float64).reshape(16),
             cam=np.ascontiguousarray(cam, np.float32).reshape(4) if unproject else None,
             class_id=np.zeros(m, np.int32), depth=np.zeros(m, np.float32), nearest_uv=np.zeros((m, 2), np.int32),
             xyz_cam=np.zeros((m, 3), np.float32) if unproject else None, stats=np.zeros((nf, 4), np.int32),
             image=np.zeros((nf, int(rows), int(cols)), np.float64) if image else None)
    return a


def _call_args(a):
    return [a["n_frame"], ptr(a["sweep_off"]), ptr(a["xyz"]), ptr(a["key_off"]), ptr(a["key_xy"]), ptr(a["key_un_xy"]),
            a["rows"], a["cols"], ptr(a["intrinsic"]), ptr(a["extrinsic"]), ptr(a["cam"]), ptr(a["class_id"]),
            ptr(a["depth"]), ptr(a["nearest_uv"]), ptr(a["xyz_cam"]), ptr(a["stats"]), ptr(a["image"])]


def _result(a):
    o = {k: a[k] for k in ("class_id", "depth", "nearest_uv", "stats", "sweep_off", "key_off")}
    if a["xyz_cam"] is not None:
        o["xyz_cam"] = a["xyz_cam"]
    if a["image"] is not None:
        o["image"] = a["image"]
    return o


def depth_host(sweeps, keys, rows, cols, intrinsic=KITTI_INTRINSIC, extrinsic=VELO_TO_CAM, keys_un=None, cam=None,
               image: bool = True, state: bool = False) -> dict:
    """sqlm_lidar_depth_host on a list of (n, 3) float32 sweeps and a list of
    (m, 2) float32 keypoint arrays, one of each per frame. Returns class_id,
    depth, nearest_uv, stats [n_frame][4], with ``keys_un`` and ``cam`` xyz_cam,
    with ``image`` the depth images, with ``state`` pixel and winner under
    "state"."""
    a = _args(sweeps, keys, keys_un, rows, cols, intrinsic, extrinsic, cam, image)
    pixel = np.zeros(a["n"], np.int32) if state else None
    winner = np.zeros((a["n_frame"], a["rows"], a["cols"]), np.int32) if state else None
    check(lib().sqlm_lidar_depth_host(*_call_args(a), ptr(pixel), ptr(winner)), "sqlm_lidar_depth_host")
    o = _result(a)
    if state:
        o["state"] = dict(pixel=pixel, winner=winner)
    return o


def depth(ctx, sweeps, keys, rows, cols, intrinsic=KITTI_INTRINSIC, extrinsic=VELO_TO_CAM, keys_un=None, cam=None,
          image: bool = False) -> dict:
    """sqlm_lidar_depth: every frame of the batch in one set of launches. The
    depth images are read back only with ``image``."""
    a = _args(sweeps, keys, keys_un, rows, cols, intrinsic, extrinsic, cam, image)
    check(lib().sqlm_lidar_depth(ctx._h, *_call_args(a)), "sqlm_lidar_depth")
    ctx._lidar_depth_shape = (a["n_frame"], a["n"], a["rows"], a["cols"])
    return _result(a)


def depth_state(ctx) -> dict:
    """pixel, winner and image of the context's last ``depth`` call."""
    nf, n, rows, cols = ctx._lidar_depth_shape
    pixel, winner = np.zeros(n, np.int32), np.zeros((nf, rows, cols), np.int32)
    image = np.zeros((nf, rows, cols), np.float64)
    check(lib().sqlm_lidar_depth_get_state(ctx._h, ptr(pixel), ptr(winner), ptr(image)), "sqlm_lidar_depth_get_state")
    return dict(pixel=pixel, winner=winner, image=image)


def depth_info(ctx=None) -> dict:
    out = (C.c_int32 * 8)()
    check(lib().sqlm_lidar_depth_info(ctx._h if ctx is not None else None, out), "sqlm_lidar_depth_info")
    return dict(max_dim=out[0], max_cells=out[1], launches=out[2], half_w=out[3], half_h=out[4], lanes_per_keypoint=out[5],
                points=out[6], keypoints=out[7])


def frame_depth(ctx, sweep, keys, rows=KITTI_ROWS, cols=KITTI_COLS, intrinsic=KITTI_INTRINSIC, extrinsic=VELO_TO_CAM):
    """One frame as the reference's Frame constructor leaves it: returns
    (class_id of every mvKeys entry, mvDepth, Depthimg_)."""
    o = depth(ctx, [sweep], [keys], rows, cols, intrinsic, extrinsic, image=True)
    return o["class_id"], o["depth"], o["image"][0]


def make_keypoints(seed: int, n: int, rows: int = KITTI_ROWS, cols: int = KITTI_COLS, border: int = 16) -> np.ndarray:
    """``n`` seeded keypoints, uniform float coordinates at least ``border`` px
    inside the image, as the reference's extractor keeps them."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(border, cols - 1 - border, n)
    y = rng.uniform(border, rows - 1 - border, n)
    return np.stack([x, y], 1).astype(np.float32)
