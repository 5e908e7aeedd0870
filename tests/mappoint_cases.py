"""The cases shared by tests/test_mappoint_ref.py, test_mappoint_abi.py,
test_mappoint_accuracy.py (CPU) and test_gpu_mappoint.py (GPU against the numpy
definition tests/mappoint_ref.py). The smallest shapes at which the kernels can
still go wrong.

Triangulation, one batch of pairs (tri_pairs()): planted two-view scenes with
0.5 px noise and 1, 63, 64, 65, 257 matches (the edges of a wavefront and of a
256-lane workgroup), a pair without matches in the middle, and pairs whose
matches are made for one reason code each (REASON_PAIRS names them; tests/
test_mappoint_ref.py asserts that each does what it is there for):
a distant point (parallax), a point behind either camera, a keypoint shifted
across the epipolar line for either reprojection test, octaves that break the
ratio test on either side, a NaN keypoint, an Inf pose entry, two identical
poses. Two pairs are degenerate on purpose and their "poses" are no rigid
motions, which the arithmetic does not ask for: "w_zero" shears the second
camera so that A has an exactly zero third column while the rays still show
parallax, and "zero_dist" halves the first camera's depth axis so that the point
triangulated at its centre has z1 > 0.

Refresh, one batch of points (mp_batch()): N = 0, 1, 2, 3, 4, 5, 63, 64, 65,
one point of LDS_MAX + 1 observations (the smallest that reads global memory),
a point whose descriptors are all equal, a point with two rows tied for the
least median, the same point with its observations permuted, a point with a
camera centre equal to the point.
"""
from __future__ import annotations

import numpy as np

import mappoint_ref as R
from sqrtlm import mappoint as M
from sqrtlm.orb import KP_DTYPE

CAM = (718.856, 718.856, 607.1928, 185.2157)
SIZES = (1, 63, 64, 65, 257)
MP_COUNTS = (0, 1, 2, 3, 4, 5, 63, 64, 65, R.LDS_MAX + 1)

_cache: dict = {}


def _kps(uv, octave):
    k = np.zeros(len(uv), KP_DTYPE)
    k["x"], k["y"] = np.asarray(uv, np.float64)[:, 0], np.asarray(uv, np.float64)[:, 1]
    k["octave"] = octave
    k["size"] = 31.0
    return k


def _pair(T1, T2, X, oct1, oct2, shift1=None, shift2=None, cam=CAM, meta=None):
    """A pair whose match i is the projection of X[i] into both views (behind a camera: the mirrored pixel),
    with per-match octaves and pixel shifts."""
    X = np.asarray(X, float).reshape(-1, 3)
    n = len(X)
    sf = M.orb_scale_factors()
    uv1, _ = M.project(T1, cam, X)
    uv2, _ = M.project(T2, cam, X)
    if shift1 is not None:
        uv1 = uv1 + np.asarray(shift1, float)
    if shift2 is not None:
        uv2 = uv2 + np.asarray(shift2, float)
    kf1 = M.TriKeyFrame(_kps(uv1, oct1), sf, T1, *cam)
    kf2 = M.TriKeyFrame(_kps(uv2, oct2), sf, T2, *cam)
    m = np.stack([np.arange(n), np.arange(n)], 1)
    return M.TriPair(kf1, kf2, m, meta=dict(meta or {}, X=X))


def _I(center):
    return M.make_pose(np.zeros(3), center)


def _reason_pairs():
    """name -> (pair, the reason its matches are made for, or None where only equality is asked)."""
    out = {}
    T1, T2 = _I([0, 0, 0]), _I([1.0, 0.1, 0.15])
    X = np.array([[0.3, -0.2, 6.0], [-1.0, 0.4, 9.0]])
    out["created"] = (_pair(T1, T2, X, [2, 3], [2, 3]), 0)
    out["parallax"] = (_pair(T1, T2, [[0.3, -0.2, 6.0e4], [10.0, 4.0, 9.0e4]], [0, 1], [0, 1]), 1)
    # behind camera 1: camera 2 sits further back, so the rays still agree in direction
    out["z1"] = (_pair(T1, _I([0.5, 0, -5.0]), [[0.2, 0, -1.0], [-0.1, 0.05, -2.0]], [0, 0], [0, 0]), 3)
    out["z2"] = (_pair(T1, _I([0.5, 0, 5.0]), [[0.2, 0, 4.0], [-0.1, 0.05, 3.0]], [0, 0], [0, 0]), 4)
    # 8 px across the epipolar lines: about 4 px of error in either view
    out["reproj1"] = (_pair(T1, T2, X, [0, 0], [0, 0], shift1=[[0, 8.0], [0, -8.0]]), 5)
    out["reproj2"] = (_pair(T1, T2, X, [7, 7], [0, 0], shift2=[[0, 8.0], [0, -8.0]]), 6)
    out["scale"] = (_pair(T1, T2, X, [7, 0], [0, 7]), 8)   # ratioOctave 3.58 and 0.279 against ratioDist ~ 1
    # a sheared second camera: R2 = [[1,0,.5],[0,1,0],[0,0,1]], keypoint 1 at the principal point, xn2 = (.5, 0, 1):
    # column 2 of A is exactly zero, its null vector e3 has w = 0, and ray2 = R2^T xn2 still shows parallax
    sf = M.orb_scale_factors()
    Ts = np.array([[1, 0, 0.5, 1.0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)
    cam = (512.0, 512.0, 320.0, 240.0)
    k1 = M.TriKeyFrame(_kps([[320.0, 240.0]], [0]), sf, _I([0, 0, 0]), *cam)
    k2 = M.TriKeyFrame(_kps([[320.0 + 256.0, 240.0]], [0]), sf, Ts, *cam)
    out["w_zero"] = (M.TriPair(k1, k2, [[0, 0]]), 2)
    # camera 1 with its depth axis halved, Ow1 = (0, 0, -1) and z1 = 1.5 there; camera 2 sees that point at
    # xn2 = (.5, 0, 1); every level's sigma2 is huge so that only the distance test is left
    Th = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0.5, 2.0]], np.float32)
    Tz = np.array([[1, 0, 0, 1.0], [0, 1, 0, 0], [0, 0, 1, 3.0]], np.float32)
    big = np.full(8, 1e30, np.float32)
    k1 = M.TriKeyFrame(_kps([[320.0, 240.0]], [0]), sf, Th, *cam, mvLevelSigma2=big)
    k2 = M.TriKeyFrame(_kps([[320.0 + 256.0, 240.0]], [0]), sf, Tz, *cam, mvLevelSigma2=big)
    p = M.TriPair(k1, k2, [[0, 0]])
    # A does not depend on tcw1(2) here (xn1 = (0, 0, 1), tcw1 = (0, 0, .)): move the centre onto the point the
    # definition triangulates, which is (0, 0, -1) up to its float rounding
    z = R.triangulate_pairs([p])["x3d"][0, 2]
    p.kf1.Tcw[2, 3] = np.float32(-2.0) * z
    out["zero_dist"] = (p, 7)
    p = _pair(T1, T2, X, [1, 1], [1, 1])
    p.kf1.mvKeysUn["x"][0] = np.nan
    p.kf2.mvKeysUn["y"][1] = np.nan
    out["nan_keypoint"] = (p, 1)
    p = _pair(T1, T2, X, [1, 1], [1, 1])
    p.kf2.Tcw[0, 3] = np.inf
    out["inf_translation"] = (p, None)
    p = _pair(T1, T2, X, [1, 1], [1, 1])
    p.kf1.Tcw[1, 1] = np.inf
    out["inf_rotation"] = (p, 1)
    out["same_pose"] = (_pair(T2, T2, X, [1, 1], [1, 1], shift1=[[0.3, 0.2], [0.1, -0.4]]), 1)
    return out


def reason_pairs():
    if "reason" not in _cache:
        _cache["reason"] = _reason_pairs()
    return _cache["reason"]


REASON_NAMES = ("created", "parallax", "z1", "z2", "reproj1", "reproj2", "scale", "w_zero", "zero_dist",
                "nan_keypoint", "inf_translation", "inf_rotation", "same_pose")


def tri_names():
    return [f"n{n}" for n in SIZES[:2]] + ["empty"] + [f"n{n}" for n in SIZES[2:]] + list(REASON_NAMES)


def tri_pairs():
    """name -> TriPair, in batch order; "empty" (no match) sits in the middle of the planted pairs."""
    if "tri" not in _cache:
        d = {}
        for n in SIZES[:2]:
            d[f"n{n}"] = M.make_two_view(n, seed=100 + n)
        e = M.make_two_view(5, seed=99)
        d["empty"] = M.TriPair(e.kf1, e.kf2, np.zeros((0, 2), np.int32))
        for n in SIZES[2:]:
            d[f"n{n}"] = M.make_two_view(n, seed=100 + n)
        for k in REASON_NAMES:
            d[k] = reason_pairs()[k][0]
        _cache["tri"] = d
    return _cache["tri"]


def tri_reference():
    """The definition over the whole batch (with the A of every match past the parallax test), computed once."""
    if "tri_ref" not in _cache:
        _cache["tri_ref"] = R.triangulate_pairs(list(tri_pairs().values()), keep_A=True)
    return _cache["tri_ref"]


def tri_slice(name):
    """The reference's rows of pair `name`."""
    names = list(tri_pairs())
    k = names.index(name)
    r = tri_reference()
    lo, hi = int(r["off"][k]), int(r["off"][k + 1])
    return dict(x3d=r["x3d"][lo:hi], reason=r["reason"][lo:hi], n_new=r["n_new"][k:k + 1], A=r["A"][lo:hi])


def _bits(*ranges):
    b = np.zeros(256, np.uint8)
    for lo, hi in ranges:
        b[lo:hi] = 1
    return np.packbits(b)


MP_NAMES = tuple(f"n{c}" for c in MP_COUNTS) + ("all_equal", "tie", "tie_permuted", "at_center")
TIE_PERM = (2, 1, 0)


def mp_batch():
    """The refresh batch; the points are MP_NAMES in order."""
    if "mp" in _cache:
        return _cache["mp"]
    base = M.make_tracks(MP_COUNTS, seed=5)
    extra = M.make_tracks((6, 3, 3, 3), seed=6)
    d, c = extra.obs_desc.copy(), extra.obs_center.copy()
    o = extra.obs_off
    d[o[0]:o[1]] = d[o[0]]                                      # all equal
    tie = np.stack([_bits(), _bits((0, 10)), _bits((10, 40))])  # d(a,b) = 10, d(a,c) = 30, d(b,c) = 40
    d[o[1]:o[2]] = tie
    d[o[2]:o[3]] = tie[list(TIE_PERM)]
    c[o[2]:o[3]] = c[o[1]:o[2]][list(TIE_PERM)]
    pos, ref = extra.pos.copy(), extra.ref_center.copy()
    pos[2], ref[2] = pos[1], ref[1]
    ls, ms = extra.level_scale.copy(), extra.max_scale.copy()
    ls[2] = ls[1]
    c[o[3] + 1] = pos[3]                                        # a camera centre equal to the point
    extra = M.MapPointBatch(o, d, c, pos, ref, ls, ms)
    cat = lambda a, b: np.concatenate([a, b])
    _cache["mp"] = M.MapPointBatch(
        np.concatenate([base.obs_off, base.obs_off[-1] + extra.obs_off[1:]]), cat(base.obs_desc, extra.obs_desc),
        cat(base.obs_center, extra.obs_center), cat(base.pos, extra.pos), cat(base.ref_center, extra.ref_center),
        cat(base.level_scale, extra.level_scale), cat(base.max_scale, extra.max_scale))
    return _cache["mp"]


def mp_reference():
    if "mp_ref" not in _cache:
        _cache["mp_ref"] = R.map_points_update(mp_batch())
    return _cache["mp_ref"]


def same(a, b):
    """Bit for bit, a NaN for a NaN (its sign and payload are the processor's, not the arithmetic's)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return a.tobytes() == b.tobytes()
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all()) and np.where(na, 0, a).tobytes() == np.where(nb, 0, b).tobytes()
