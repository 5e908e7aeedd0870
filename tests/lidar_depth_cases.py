"""Cases of the LiDAR depth image and keypoint depth association, each at the
smallest shape where its rule can go wrong (tests/lidar_depth_ref.py is the
definition they are checked against). A case is a ``Case``: a sweep, keypoints
(optionally the undistorted ones) and a ``Cfg`` (image size, matrices, camera);
``expect`` holds what the case is there to show, checked against the definition
in tests/test_lidar_depth_ref.py. ``reference(name)`` evaluates the definition
once per session and is shared by the CPU and the GPU tests. ``batches()``
groups the cases that share a Cfg, the batch being a property of one call.

Most cases use a camera whose projection is exact: pixel quotients y / x' and
z / x' and depth x' = x + tz of a sensor point (x, y, z), so a return is placed
on a pixel, with a depth, by hand."""
import functools
import itertools
from dataclasses import dataclass, field

import numpy as np

import lidar_depth_ref as R
from sqrtlm import lidar_depth as LD
from sqrtlm import lidar_feat as LF

f32, f64 = np.float32, np.float64
UNIT_K = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]])


def axes(tz=0.0, eps=0.0):
    """Sensor x forward -> camera z (depth x + eps y + tz), y -> camera x, z -> camera y."""
    return np.array([[0.0, 1, 0, 0], [0, 0, 1.0, 0], [1.0, eps, 0, tz], [0, 0, 0, 1.0]])


@dataclass(frozen=True, eq=False)
class Cfg:
    rows: int
    cols: int
    extrinsic: np.ndarray = field(default_factory=axes)
    intrinsic: np.ndarray = field(default_factory=lambda: UNIT_K)
    cam: tuple = None  # (fx, fy, cx, cy): the case carries undistorted keypoints

    @property
    def tz(self):
        return float(self.extrinsic[2, 3])


@dataclass(eq=False)
class Case:
    cfg: Cfg
    xyz: np.ndarray
    keys: np.ndarray
    keys_un: np.ndarray = None
    expect: dict = field(default_factory=dict)


CAM = (20.0, 21.0, 11.5, 7.25)
S16, S37 = Cfg(16, 24), Cfg(37, 53)
S16U, S37U = Cfg(16, 24, cam=CAM), Cfg(37, 53, cam=CAM)
T16, T37 = Cfg(16, 24, axes(-10.0)), Cfg(37, 53, axes(-10.0), cam=CAM)   # depth = x - 10: any sign with x > 1
X16 = Cfg(16, 24, axes(3.0))                                             # depth = x + 3: x around 1
Z16 = Cfg(16, 24, axes(-2.0))                                            # depth = x - 2: zw at and around 0
E16 = Cfg(16, 24, axes(0.0, 2.0 ** -51))                                 # depth = x + y 2^-51
F16 = Cfg(16, 24, axes(0.1))                                             # depth = x + 0.1: not a float
ONE = Cfg(1, 1)
FULL = Cfg(LD.KITTI_ROWS, LD.KITTI_COLS, LD.VELO_TO_CAM, LD.KITTI_INTRINSIC, tuple(LD.KITTI_CAM))


def ret(cfg, qu, qv, depth):
    """The sensor point that lands on quotients (qu, qv) with this depth under an axes() camera."""
    return [depth - cfg.tz, qu * depth, qv * depth]


def at(cfg, u, v, depth):
    return ret(cfg, u + 0.5, v + 0.5, depth)


def pts(rows):
    return np.asarray(rows, f32).reshape(-1, 3)


def kps(rows):
    return np.asarray(rows, f32).reshape(-1, 2)


def shifted(keys, seed):
    """Undistorted keypoints: the keypoints moved by up to a pixel."""
    k = kps(keys)
    return (k + np.random.default_rng(seed).uniform(-1, 1, k.shape)).astype(f32)


def _collision(cfg, n):
    """n points on at most three pixels: pixel A is written by point 0 alone (its winner comes
    first), B and C alternate up to the middle (B's winner is in the middle), then C alone
    (its winner is the last point). Every point has its own depth."""
    A, B, C = (3, 2), (12, 9), (13, 9)
    rows = []
    for i in range(n):
        where = A if i == 0 else ((B if i % 2 else C) if i <= n // 2 else C)
        rows.append(at(cfg, where[0], where[1], 2.0 + (i % 1024) / 512.0))
    keys = [[12.0, 9.0], [3.0, 2.0], [12.5, 9.5], [20.0, 13.0]]
    return Case(cfg, pts(rows), kps(keys), expect=dict(n_written=n, n_occupied=min(n, 3)))


def _thresholds():
    one = f32(1.0)
    xs = [np.nextafter(one, f32(0)), one, np.nextafter(one, f32(2))]
    rows = [[x, (5.5 + 4 * k) * (float(x) + 3.0), 8.5 * (float(x) + 3.0)] for k, x in enumerate(xs)]
    return Case(X16, pts(rows), kps([[5.0, 8.0], [9.0, 8.0], [13.0, 8.0]]),
                expect=dict(pixel=[-1, -1, 8 * 24 + 13], class_id=[0, 0, 1]))


def _truncation(cfg, un=False):
    r, c = cfg.rows, cfg.cols
    d = 4.0
    rows = [ret(cfg, -0.5, 2.5, d),             # lands on column 0
            ret(cfg, c - 1, 3.5, d),            # the last column
            ret(cfg, c - 1 + 0.99, 4.5, d),     # still the last column
            ret(cfg, c, 5.5, d),                # outside
            ret(cfg, 2.5, -0.5, d),             # row 0
            ret(cfg, 3.5, r - 1, d),
            ret(cfg, 4.5, r - 1 + 0.99, d),
            ret(cfg, 5.5, r, d),                # outside
            ret(cfg, -1.0, 6.5, d),             # exactly -1: outside
            ret(cfg, -0.5, -0.5, d),            # the corner pixel
            [np.nan, 1.0, 1.0], [5.0, np.inf, 1.0], [5.0, 1.0, -np.inf], [np.inf, 1.0, 1.0], [np.nan, np.nan, np.nan]]
    want = [2 * c, 3 * c + c - 1, 4 * c + c - 1, -1, 2, (r - 1) * c + 3, (r - 1) * c + 4, -1, -1, 0, -1, -1, -1, -1, -1]
    keys = [[4.0, 7.0], [c - 5.0, 7.0], [4.0, r - 8.0], [c - 5.0, r - 8.0], [c / 2.0, r / 2.0]]
    return Case(cfg, pts(rows), kps(keys), shifted(keys, 5) if un else None, expect=dict(pixel=want))


def _zw():
    two = f32(2.0)
    tiny = np.nextafter(two, f32(3))            # zw = 2^-22: the quotient of y = 3000 is beyond int32
    rows = [[2.0, 5.0, 5.0],                    # zw = 0: quotients inf
            [2.0, 0.0, 0.0],                    # 0 / 0
            [tiny, 3000.0, 0.0], [tiny, -3000.0, 0.0], [tiny, 0.0, 3000.0],
            [1.5, -0.5 * 6.5, -0.5 * 7.5],      # zw = -0.5, quotients 6.5 and 7.5: writes a negative depth
            [1.25, -0.75 * 9.5, -0.75 * 7.5]]
    return Case(Z16, pts(rows), kps([[6.0, 7.0], [9.0, 7.0]]),
                expect=dict(pixel=[-1, -1, -1, -1, -1, 7 * 24 + 6, 7 * 24 + 9], n_written=2, min_v=0))


UCHAR_DEPTHS = [0.5, 1.0, 1.5, 255.9, 256.3, 257.0, -0.5, -3.2]
UCHAR_SEEN = [False, True, True, True, False, True, False, True]


def _uchar():
    """Each depth alone in the patch of its own keypoint (two rows of patches)."""
    spots = [(5 + 10 * (k % 5), 10 + 16 * (k // 5)) for k in range(len(UCHAR_DEPTHS))]
    rows = [at(T37, u, v, d) for (u, v), d in zip(spots, UCHAR_DEPTHS)]
    keys = [[u, v] for u, v in spots]
    return Case(T37, pts(rows), kps(keys), shifted(keys, 2),
                expect=dict(class_id=[1 if s else 0 for s in UCHAR_SEEN], n_written=8, min_v=10))


def _min_v_cases():
    C = {}
    keys = [[12.0, 7.0], [12.0, 15.0], [12.0, 0.0]]
    C["min_v_none"] = Case(T16, pts([at(T16, 12, 7, -3.0), at(T16, 3, 3, -0.5)]), kps(keys), expect=dict(min_v=0))
    C["min_v_no_return"] = Case(S16, pts([[0.5, 0.0, 0.0]]), kps(keys), expect=dict(min_v=0, n_written=0))
    C["min_v_last_row"] = Case(S16, pts([at(S16, 12, 15, 4.0)]), kps(keys + [[12.0, 14.99], [12.0, 15.5]]),
                               expect=dict(min_v=15, class_id=[0, 1, 0, 0, 1]))
    C["min_v_first_row"] = Case(S16, pts([at(S16, 12, 0, 4.0)]), kps(keys), expect=dict(min_v=0, class_id=[1, 0, 1]))  # dy = -7 reaches row 0
    C["min_v_negative_top"] = Case(T16, pts([at(T16, 20, 2, -3.0), at(T16, 12, 9, 4.0), at(T16, 5, 12, 5.0)]),
                                   kps([[12.0, 8.0], [12.0, 9.0], [12.0, 8.999999], [12.0, 9.000001], [12.0, 5.0]]),
                                   expect=dict(min_v=9, class_id=[0, 1, 0, 1, 0]))
    # a 0.5 return on top: it sets min_v and is not seen, so the keypoint beside it sees the return below alone
    C["min_v_half_top"] = Case(T16, pts([at(T16, 12, 3, 0.5), at(T16, 12, 9, 4.0)]),
                               kps([[12.0, 2.999], [12.0, 3.0], [12.0, 3.001], [12.0, 2.0], [12.0, 9.0]]),
                               expect=dict(min_v=3, class_id=[0, 1, 1, 0, 1],
                                           nearest_uv=[[-1, -1], [12, 9], [12, 9], [-1, -1], [12, 9]]))
    return C


def _offsets():
    """One return; a keypoint at every one of the 112 offsets from it, and one cell outside on each
    side. A second return on the top row, out of every patch's reach, keeps min_v at 0: the
    keypoints above the first return would be class 0 by the min_v rule otherwise."""
    u0, v0 = 26, 18
    keys, want = [], []
    for dx in range(-4, 4):
        for dy in range(-7, 7):
            keys.append([u0 - dx, v0 - dy])
            want.append([u0, v0])
    for dx, dy in ((-5, 0), (4, 0), (0, -8), (0, 7), (-5, -8), (4, 7)):
        keys.append([u0 - dx, v0 - dy])
        want.append([-1, -1])
    return Case(S37, pts([at(S37, u0, v0, 6.0), at(S37, 50, 0, 6.0)]), kps(keys), expect=dict(nearest_uv=want, min_v=0))


def _fractional():
    below4, below1 = np.nextafter(f32(4.0), f32(0)), np.nextafter(f32(1.0), f32(0))
    rows = [at(S37, 0, 20, 5.0), at(S37, 30, 0, 5.0), at(S37, 44, 30, 5.0), at(S37, 20, 30, 5.0)]
    keys = [[3.5, 20.0],            # dx = -4 and dx = -3 both reach column 0
            [4.5, 20.0],            # only dx = -4 does
            [4.999, 20.5],          # int(0.999) = 0
            [5.0, 20.0],
            [30.0, 6.5],            # dy = -7 reaches row 0 (-0.5)
            [30.0, 7.999], [30.0, 8.0],
            [below4, 20.0],         # 3.9999998 - 4 = -2.4e-7: column 0
            [40.0 + below1, 30.0],  # the float add of dx = 3 rounds up to 44
            [48.999, 30.0],         # column 44 = int(48.999 - 4)
            [49.0, 30.0],           # column 45: out of reach
            [20.0 + below1, 30.0 + below1], [16.5, 23.5], [24.999, 37.999 - 1.0]]
    return Case(S37, pts(rows), kps(keys), shifted(keys, 3),
                expect=dict(class_id=[1, 1, 1, 0, 1, 1, 0, 1, 1, 1, 0, 1, 0, 1]))


def _borders(cfg, un=False):
    r, c = cfg.rows, cfg.cols
    rows = [at(cfg, 0, 0, 3.0), at(cfg, c - 1, 0, 3.5), at(cfg, 0, r - 1, 4.0), at(cfg, c - 1, r - 1, 4.5),
            at(cfg, c // 2, r // 2, 5.0)]
    xs = [-1e9, -5.0, -4.5, -1.0, -0.5, 0.0, 3.0, c - 1.0, c - 0.5, c, c + 3.5, c + 4.0, 1e9, 3e38]
    ys = [-1e9, -8.0, -7.5, -1.0, -0.5, 0.0, 6.0, r - 1.0, r - 0.5, r, r + 6.5, r + 7.0, 1e9, 3e38]
    keys = [[x, y] for x in xs for y in ys]
    keys += [[np.nan, 3.0], [3.0, np.nan], [np.nan, np.nan], [np.inf, 3.0], [3.0, -np.inf], [-np.inf, np.inf]]
    return Case(cfg, pts(rows), kps(keys), shifted(np.nan_to_num(kps(keys), posinf=9.0, neginf=-9.0), 4) if un else None)


TIE_OFFSETS = [(-1, 0), (0, -1), (0, 1), (1, 0)]  # in scan order: dx-major, then dy


def _tie(offsets):
    u0, v0 = 12, 8
    first = min(offsets, key=lambda o: (o[0], o[1]))  # equal distances: the first in scan order
    return Case(S16, pts([at(S16, u0 + dx, v0 + dy, 4.0) for dx, dy in offsets]), kps([[u0, v0]]),
                expect=dict(class_id=[1], nearest_uv=[[u0 + first[0], v0 + first[1]]]))


def _range():
    """Returns at x = 3 and x = 5 in one patch; the depth is x + y 2^-51, so y = -1 puts the
    first at 3 - 2^-51: the range is the next double above 2.0. Class 1, then class 2."""
    def point(x, y, u, v):
        dep = x + y * 2.0 ** -51
        return [x, y, (v + 0.5) * dep]  # the column is int(y / dep)
    C = {"range_exactly_2": Case(S16, pts([at(S16, 13, 4, 3.0), at(S16, 14, 4, 5.0)]), kps([[13.0, 4.0]]),
                                 expect=dict(class_id=[1], depth=[3.0]))}
    # y = -1 lands on column int(-1 / 3) = 0, beside the second return on column 1
    C["range_next_above_2"] = Case(E16, pts([point(3.0, -1.0, 0, 4), point(5.0, 1.5 * 5.0, 1, 4)]), kps([[3.0, 4.0]]),
                                   expect=dict(class_id=[2], depth=[-1.0], nearest_uv=[[1, 4]]))
    C["depth_rounds_to_float"] = Case(F16, pts([at(F16, 8, 8, 3.3), at(F16, 9, 8, 3.7)]), kps([[8.0, 8.0], [9.0, 8.0]]),
                                      shifted([[8.0, 8.0], [9.0, 8.0]], 6), expect=dict(class_id=[1, 1]))
    return C


def _scattered(cfg, seed, n_pts, n_keys, un=True):
    """Random returns over the image (depths 2 to 12, a few negative or below 1 with the
    tz = -10 camera) and random fractional keypoints, some outside."""
    rng = np.random.default_rng(seed)
    qu, qv = rng.uniform(-1.5, cfg.cols + 0.5, n_pts), rng.uniform(-1.5, cfg.rows + 0.5, n_pts)
    dep = rng.uniform(2.0, 12.0, n_pts)
    if cfg.tz < 0:
        dep[rng.random(n_pts) < 0.1] *= -0.3
        dep[rng.random(n_pts) < 0.05] = 0.6
    xyz = pts(np.stack([dep - cfg.tz, qu * dep, qv * dep], 1))
    keys = kps(np.stack([rng.uniform(-6, cfg.cols + 6, n_keys), rng.uniform(-9, cfg.rows + 9, n_keys)], 1))
    return Case(cfg, xyz, keys, shifted(keys, seed + 1) if un else None)


@functools.lru_cache(maxsize=None)
def cases():
    C = {}
    for n in (1, 63, 64, 65, 257, 4097):
        C[f"collide_{n}"] = _collision(S16, n)
    C["collide_257_large"] = _collision(S37, 257)
    C["x_thresholds"] = _thresholds()
    C["truncation_16"] = _truncation(S16)
    C["truncation_37"] = _truncation(S37U, un=True)
    C["zw"] = _zw()
    C["uchar"] = _uchar()
    C.update(_min_v_cases())
    C["offsets"] = _offsets()
    C["fractional"] = _fractional()
    C["borders_16"] = _borders(S16)
    C["borders_37"] = _borders(S37U, un=True)
    C["one_by_one"] = Case(ONE, pts([at(ONE, 0, 0, 4.0), ret(ONE, 1.0, 0.5, 5.0)]),
                           kps([[0.0, 0.0], [3.5, 6.5], [4.0, 0.0], [-4.5, -7.5], [0.999, 0.999], [-5.0, 0.0]]),
                           expect=dict(class_id=[1, 1, 1, 0, 1, 0], n_written=1))
    C["ties_all"] = _tie(TIE_OFFSETS)
    for pair in itertools.combinations(TIE_OFFSETS, 2):
        C["ties_" + "_".join(f"{dx}{dy}" for dx, dy in pair).replace("-", "m")] = _tie(list(pair))
    C["ties_diagonal"] = _tie([(-1, -1), (1, 1)])
    C["ties_diagonal_swapped"] = _tie([(1, 1), (-1, -1)])
    C.update(_range())
    for m in (0, 1, 63, 64, 65, 2049):
        C[f"keys_{m}"] = _scattered(T37, 100 + m, 300, m)
    C["keys_65_plain"] = _scattered(S37, 7, 300, 65, un=False)
    C["scattered_16"] = _scattered(T16, 8, 2000, 40, un=False)    # far more points than pixels
    C["empty_sweep"] = Case(T37, pts([]), kps([[10.0, 10.0], [20.5, 30.5]]), shifted([[10.0, 10.0], [20.5, 30.5]], 9),
                            expect=dict(class_id=[0, 0], n_written=0, min_v=0))
    C["empty_keys"] = Case(T37, _scattered(T37, 11, 50, 0).xyz, kps([]), kps([]))
    C["empty_both"] = Case(T37, pts([]), kps([]), kps([]), expect=dict(n_written=0, n_occupied=0, n_with_depth=0))
    sweep = LF.make_sweep(3, n_az=1800, order="azimuth", start_deg=23.0)
    keys = LD.make_keypoints(5, 2000)
    C["full_size"] = Case(FULL, sweep, keys, shifted(keys, 12))
    return C


def names(full=True):
    return [n for n in cases() if full or n != "full_size"]


@functools.lru_cache(maxsize=None)
def reference(name):
    c = cases()[name]
    return R.process(c.xyz, c.keys, c.cfg.rows, c.cfg.cols, c.cfg.intrinsic, c.cfg.extrinsic, c.keys_un, c.cfg.cam)


def batches():
    """[(Cfg, [names])]: the cases that share a Cfg, in case order; "full_size" stays alone."""
    out = []
    for n, c in cases().items():
        if n == "full_size":
            continue
        for b in out:
            if b[0] is c.cfg:
                b[1].append(n)
                break
        else:
            out.append((c.cfg, [n]))
    return out


def fillers(cfg):
    """Two frames that accompany the cases of a batch: one ordinary, one with nothing in it."""
    a = _scattered(cfg, 41, 120, 30, un=cfg.cam is not None)
    return [a, Case(cfg, pts([]), kps([]), kps([]) if cfg.cam is not None else None)]


def call_args(group):
    """The arguments of LD.depth / LD.depth_host for a list of cases that share a Cfg."""
    cfg = group[0].cfg
    un = [c.keys_un for c in group] if cfg.cam is not None else None
    return dict(sweeps=[c.xyz for c in group], keys=[c.keys for c in group], rows=cfg.rows, cols=cfg.cols,
                intrinsic=cfg.intrinsic, extrinsic=cfg.extrinsic, keys_un=un, cam=cfg.cam)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else (a.view(np.uint64) if a.dtype == np.float64 else a)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


OUT_KEYS = ("class_id", "depth", "nearest_uv", "stats", "image")
STATE_KEYS = ("pixel", "winner")


def slice_of(o, k):
    """Frame k of a batched result (outputs and, if present, state and image) as a single-frame result."""
    a, b = int(o["key_off"][k]), int(o["key_off"][k + 1])
    r = dict(class_id=o["class_id"][a:b], depth=o["depth"][a:b], nearest_uv=o["nearest_uv"][a:b], stats=o["stats"][k])
    if "xyz_cam" in o:
        r["xyz_cam"] = o["xyz_cam"][a:b]
    if "image" in o:
        r["image"] = o["image"][k]
    if "state" in o:
        p, q = int(o["sweep_off"][k]), int(o["sweep_off"][k + 1])
        r["pixel"], r["winner"] = o["state"]["pixel"][p:q], o["state"]["winner"][k]
        if "image" in o["state"]:
            r["state_image"] = o["state"]["image"][k]
    return r


def differences(got, want):
    """The names of everything in which a single-frame result differs from the definition's, bit for bit."""
    bad = [k for k in OUT_KEYS + STATE_KEYS if k in got and not same(got[k], want[k])]
    bad += [k for k in OUT_KEYS if k not in got]
    if ("xyz_cam" in got) != ("xyz_cam" in want) or ("xyz_cam" in want and not same(got["xyz_cam"], want["xyz_cam"])):
        bad.append("xyz_cam")
    if "state_image" in got and not same(got["state_image"], want["image"]):
        bad.append("state_image")
    return bad
