"""The definition of sqlm_lidar_depth (include/sqrtlm.h) in numpy: the LiDAR
depth image of a fusion frame and the class / depth of every keypoint, as
order-free rules over whole arrays. numpy evaluates every elementwise operation
as one IEEE operation in the order written, nothing fused, which is what the
library's -ffp-contract=off text does. tests/lidar_depth_naive.py transcribes
the reference's loops; tests/test_lidar_depth_ref.py compares the two."""
import numpy as np

f32, f64 = np.float32, np.float64
HALF_W, HALF_H = 4, 7
MIN_X, MAX_RANGE = f32(1.0), 2.0
NO_KEY = 0x7fffffff
DX = np.arange(-HALF_W, HALF_W)
DY = np.arange(-HALF_H, HALF_H)
# (dx dx + dy dy, scan position), dx-major
KEY = ((DX[:, None] ** 2 + DY[None, :] ** 2) * 128 + (DX[:, None] + HALF_W) * (2 * HALF_H) + (DY[None, :] + HALF_H))


def product(intrinsic, extrinsic):
    """M = intrinsic (3x4) extrinsic (4x4), each entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3."""
    a, b = np.asarray(intrinsic, f64).reshape(3, 4), np.asarray(extrinsic, f64).reshape(4, 4)
    M = np.zeros((3, 4))
    for r in range(3):
        for c in range(4):
            M[r, c] = ((a[r, 0] * b[0, c] + a[r, 1] * b[1, c]) + a[r, 2] * b[2, c]) + a[r, 3] * b[3, c]
    return M


def _row(m, x, y, z):
    return ((m[0] * x + m[1] * y) + m[2] * z) + m[3]


def cell(q, n):
    """int(q) as a cell of [0, n): -1 outside, NaN included; (-1, 0) lands on 0."""
    q = np.asarray(q)
    with np.errstate(invalid="ignore"):
        ok = (q > -1) & (q < n)
    return np.where(ok, np.trunc(np.where(ok, q, 0)), -1).astype(np.int32)


def project(xyz, M, extrinsic, rows, cols):
    """(pixel v cols + u or -1, depth) of every point."""
    xyz = np.ascontiguousarray(xyz, f32).reshape(-1, 3)
    E2 = np.asarray(extrinsic, f64).reshape(4, 4)[2]
    x, y, z = (xyz[:, k].astype(f64) for k in range(3))
    with np.errstate(all="ignore"):
        zu, zv, zw, dep = _row(M[0], x, y, z), _row(M[1], x, y, z), _row(M[2], x, y, z), _row(E2, x, y, z)
        u, v = cell(zu / zw, cols), cell(zv / zw, rows)
        ok = np.isfinite(xyz).all(1) & (xyz[:, 0] > MIN_X) & (u >= 0) & (v >= 0)
    return np.where(ok, v * cols + u, -1).astype(np.int32), dep


def seen(d):
    """The uchar read of :366-367: the low byte of the truncated int32, INT_MIN beyond int32."""
    d = np.asarray(d, f64)
    with np.errstate(invalid="ignore"):
        ok = np.abs(d) < 2147483648.0
    t = np.trunc(np.where(ok, d, -2147483648.0)).astype(np.int64)
    return (t & 255) != 0


def process(xyz, keys, rows, cols, intrinsic, extrinsic, keys_un=None, cam=None):
    """One frame. Returns class_id, depth, nearest_uv, stats, image, pixel,
    winner and, with keys_un and cam, xyz_cam."""
    xyz = np.ascontiguousarray(xyz, f32).reshape(-1, 3)
    keys = np.ascontiguousarray(keys, f32).reshape(-1, 2)
    M = product(intrinsic, extrinsic)
    pixel, dep = project(xyz, M, extrinsic, rows, cols)
    writers = np.flatnonzero(pixel >= 0)
    winner = np.zeros(rows * cols, np.int32)
    np.maximum.at(winner, pixel[writers], (writers + 1).astype(np.int32))  # the greatest index: the last write
    image = np.where(winner > 0, dep[np.maximum(winner, 1) - 1] if len(xyz) else 0.0, 0.0).reshape(rows, cols)
    with np.errstate(invalid="ignore"):
        positive_rows = np.flatnonzero((image > 0.0).any(1))
    min_v = int(positive_rows[0]) if len(positive_rows) else 0

    m = len(keys)
    px, py = keys[:, 0], keys[:, 1]
    with np.errstate(invalid="ignore"):
        below = py < f32(min_v)
        col = cell(px[:, None] + DX.astype(f32)[None, :], cols)  # [m][8], the add in float
        row = cell(py[:, None] + DY.astype(f32)[None, :], rows)  # [m][14]
    inside = (col[:, :, None] >= 0) & (row[:, None, :] >= 0)
    val = image[np.maximum(row, 0)[:, None, :], np.maximum(col, 0)[:, :, None]]  # [m][dx][dy]
    vis = inside & seen(val) & ~below[:, None, None]
    lo = np.where(vis, val, np.inf).reshape(m, -1).min(1) if m else np.zeros(0)
    hi = np.where(vis, val, -np.inf).reshape(m, -1).max(1) if m else np.zeros(0)
    key = np.where(vis, KEY[None], NO_KEY).reshape(m, -1).min(1) if m else np.zeros(0, np.int64)
    any_seen = key != NO_KEY
    slot = key & 127
    idx = np.arange(m)
    u = np.where(any_seen, col[idx, np.minimum(slot // (2 * HALF_H), 2 * HALF_W - 1)], -1).astype(np.int32)
    v = np.where(any_seen, row[idx, slot % (2 * HALF_H)], -1).astype(np.int32)
    with np.errstate(invalid="ignore"):
        wide = (hi - lo) > MAX_RANGE
    cls = np.where(~any_seen, 0, np.where(wide, 2, 1)).astype(np.int32)
    depth = np.where(cls == 1, image[np.maximum(v, 0), np.maximum(u, 0)].astype(f32), f32(-1.0)).astype(f32)
    out = dict(class_id=cls, depth=depth, nearest_uv=np.stack([u, v], 1).astype(np.int32).reshape(m, 2),
               stats=np.array([min_v, len(writers), int((winner > 0).sum()), int((depth > 0).sum())], np.int32),
               image=image, pixel=pixel, winner=winner.reshape(rows, cols))
    if keys_un is not None and cam is not None:
        un = np.ascontiguousarray(keys_un, f32).reshape(-1, 2)
        fx, fy, cx, cy = (f32(c) for c in np.asarray(cam, f32))
        pos = depth > 0
        z = np.where(pos, depth, f32(0.0)).astype(f32)
        X = ((un[:, 0] - cx) * z) * (f32(1.0) / fx)
        Y = ((un[:, 1] - cy) * z) * (f32(1.0) / fy)
        out["xyz_cam"] = np.where(pos[:, None], np.stack([X, Y, z], 1), f32(0.0)).astype(f32).reshape(m, 3)
    return out
