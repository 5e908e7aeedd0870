"""ORB front-end inputs built for the paths one extracted KITTI frame pair does
not reach, shared by tests/test_orb_edge_ref.py (CPU: the conditions on the
inputs, asserted on the oracle alone, and the oracle against the Python
transliterations) and tests/test_gpu_orb_edges.py (GPU against the oracle).
Everything is built once and cached: callers must not modify what they get
(the run_* functions copy what a search updates in place).

Matcher frames are keypoint arrays written directly, no extractor in the loop:

- ``crowd``: 601 keypoints (601 % 4 == 1: the last block of four waves is
  partial) on a frame whose bounds are non-zero and non-integer on all four
  sides. Three clusters put exactly 64, 70 and 150 keypoints into single grid
  cells (one, two and three ballots of k_area_list's 64-wide loop), the
  largest into the last column and row of the 64 x 48 grid; keypoints lie
  outside the bounds on each side (outside the grid, and between the bounds
  and the first cell centre, which PosInGrid still rounds into the grid);
  octaves cover 0..7; a few frame-2 keypoints of one cell carry identical
  descriptors (best == second best, the first index wins). Frame 1 is frame 2
  shifted by SHIFT with perturbed angles and 6 flipped descriptor bits per
  feature, independently permuted.
- ``tiny``: frames of 0, 1, 3 and 5 keypoints paired as TINY_PAIRS.

The inputs of the eleven ORBmatcher searches come from these frames through
sqrtlm.orb_scene with the parameter grids of tests/test_orb_gpu.py (SEARCHES);
the camera's principal point is the centre of the bounds. The BoW node of a
side-2 feature comes from explicit run lengths (BOW_RUNS), side 1 takes the
node of its nearest side-2 descriptor.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

from sqrtlm import orb_scene as S
from sqrtlm import synth

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                     ("octave", "<i4")])
GRID_COLS, GRID_ROWS = 64, 48
BOUNDS = (-11.5, 652.25, -7.75, 489.5)  # mnMinX, mnMaxX, mnMinY, mnMaxY
SHIFT = (5.0, -3.0)                     # frame 2 = frame 1 + SHIFT
# orb_scene.camera(W, H) puts the principal point at (W / 2, H / 2): the centre of BOUNDS
W, H = BOUNDS[0] + BOUNDS[1], BOUNDS[2] + BOUNDS[3]
CAM = S.camera(W, H)
SF = S.scale_factors()
# (cell column, cell row, keypoints): one, two and three 64-wide ballots; the last one in the last column and row
CLUSTERS = ((10, 12, 64), (30, 20, 70), (GRID_COLS - 1, GRID_ROWS - 1, 150))
N_CROWD = 601
BOW_RUNS = (1, 63, 64, 65, 128, 129, 140)  # side-2 features per node; the rest are not in the vocabulary

Frames = namedtuple("Frames", "k1 d1 k2 d2 bounds src")  # src[i]: the frame-2 keypoint frame-1 keypoint i came from


def _freeze(*arrays):
    for a in arrays:
        a.flags.writeable = False


def pos_in_grid(kps, bounds=BOUNDS):
    """Frame::PosInGrid (Frame.cc:1554-1565): (column, row, inside the grid) per keypoint."""
    f32 = np.float32
    minx, maxx, miny, maxy = (f32(v) for v in bounds)
    wi, hi = f32(GRID_COLS) / (maxx - minx), f32(GRID_ROWS) / (maxy - miny)
    px = np.floor(((kps["x"] - minx) * wi).astype(np.float64) + 0.5).astype(np.int64)
    py = np.floor(((kps["y"] - miny) * hi).astype(np.float64) + 0.5).astype(np.int64)
    return px, py, (px >= 0) & (px < GRID_COLS) & (py >= 0) & (py < GRID_ROWS)


def _cell_xy(rng, cx, cy, n, bounds=BOUNDS):
    """n positions well inside grid cell (cx, cy): within 0.4 of a cell of its centre."""
    minx, maxx, miny, maxy = bounds
    x = minx + (cx + rng.uniform(-0.4, 0.4, n)) * (maxx - minx) / GRID_COLS
    y = miny + (cy + rng.uniform(-0.4, 0.4, n)) * (maxy - miny) / GRID_ROWS
    return x, y


def _keypoints(x, y, octave, rng):
    k = np.zeros(len(x), KP_DTYPE)
    k["x"], k["y"], k["octave"] = x, y, octave
    k["size"] = (31.0 * SF[octave]).astype(np.float32)
    k["angle"] = rng.uniform(0.0, 360.0, len(x))
    k["response"] = rng.integers(7, 200, len(x))
    return k


def _frame1_of(k2, d2, rng, permute):
    """Frame 1: frame 2 moved back by SHIFT, angles turned by 24 +- 6 degrees, 6 descriptor bits flipped."""
    n = len(k2)
    src = rng.permutation(n) if permute else np.arange(n)
    k1 = k2[src].copy()
    k1["x"] -= np.float32(SHIFT[0])
    k1["y"] -= np.float32(SHIFT[1])
    k1["angle"] = np.mod(k1["angle"] + 24.0 + rng.normal(0.0, 6.0, n), 360.0).astype(np.float32)
    k1["response"] = rng.integers(7, 200, n)
    bits = np.unpackbits(d2[src], axis=1)
    for i in range(n):
        bits[i, rng.choice(256, 6, replace=False)] ^= 1
    return k1, np.ascontiguousarray(np.packbits(bits, axis=1)), src


@functools.lru_cache(maxsize=None)
def crowd(seed: int = 2) -> Frames:
    rng = np.random.default_rng(seed)
    minx, maxx, miny, maxy = BOUNDS
    xs, ys = [], []
    for cx, cy, n in CLUSTERS:
        x, y = _cell_xy(rng, cx, cy, n)
        xs.append(x)
        ys.append(y)
    n_cl = sum(c[2] for c in CLUSTERS)
    # outside the bounds: two beyond the grid on each side, one beyond a corner, and one per side
    # between the bounds and the first / last cell centre (still rounded into the grid)
    ox = [minx - 7.0, minx - 9.5, maxx + 3.0, maxx + 6.5, 100.0, 400.0, 250.0, 500.0, minx - 8.0,
          minx - 2.0, maxx + 0.5, 200.0, 300.0]
    oy = [50.0, 300.0, 120.0, 410.0, miny - 7.0, miny - 8.5, maxy + 3.0, maxy + 7.0, miny - 9.0,
          150.0, 100.0, miny - 2.0, maxy + 0.25]
    n_uni = N_CROWD - n_cl - len(ox)
    ux, uy = rng.uniform(minx, maxx, n_uni), rng.uniform(miny, maxy, n_uni)
    while True:  # the uniform part stays out of the cluster cells: their occupancy is exact
        probe = np.zeros(n_uni, KP_DTYPE)
        probe["x"], probe["y"] = ux, uy
        px, py, _ = pos_in_grid(probe)
        hit = np.zeros(n_uni, bool)
        for cx, cy, _n in CLUSTERS:
            hit |= (px == cx) & (py == cy)
        if not hit.any():
            break
        ux[hit], uy[hit] = rng.uniform(minx, maxx, hit.sum()), rng.uniform(miny, maxy, hit.sum())
    x = np.concatenate(xs + [np.array(ox), ux])
    y = np.concatenate(ys + [np.array(oy), uy])
    octave = rng.choice(8, N_CROWD, p=[0.5, 0.15, 0.1, 0.08, 0.06, 0.05, 0.03, 0.03])
    d2 = rng.integers(0, 256, (N_CROWD, 32), dtype=np.uint8)
    # identical descriptors inside one cell (same octave: both pass every level filter together)
    for a, b in ((0, 1), (64, 65), (66, 130), (134, 135), (140, 283), (150, 151)):
        d2[b] = d2[a]
        octave[b] = octave[a]
    order = rng.permutation(N_CROWD)  # cluster members get scattered indices
    k2 = _keypoints(x[order], y[order], octave[order], rng)
    d2 = np.ascontiguousarray(d2[order])
    k1, d1, src = _frame1_of(k2, d2, rng, permute=True)
    _freeze(k1, d1, k2, d2, src)
    return Frames(k1, d1, k2, d2, BOUNDS, src)


TINY_PAIRS = ((1, 0), (0, 1), (1, 1), (3, 0), (0, 3), (3, 5), (5, 0), (0, 5), (5, 3))  # (n1, n2)


@functools.lru_cache(maxsize=None)
def _tiny_base(seed: int = 5):
    rng = np.random.default_rng(seed)
    minx, maxx, miny, maxy = BOUNDS
    # well inside the image, a few cells apart, all on level 0: every search can reach them
    x = rng.uniform(minx + 150.0, maxx - 150.0, 5)
    y = rng.uniform(miny + 120.0, maxy - 120.0, 5)
    k2 = _keypoints(x, y, np.zeros(5, np.int64), rng)
    d2 = rng.integers(0, 256, (5, 32), dtype=np.uint8)
    k1, d1, src = _frame1_of(k2, d2, rng, permute=False)
    _freeze(k1, d1, k2, d2, src)
    return k1, d1, k2, d2, src


@functools.lru_cache(maxsize=None)
def tiny(n1: int, n2: int) -> Frames:
    """Frame 1 / frame 2 of n1 / n2 keypoints; keypoint i of one is keypoint i of the other."""
    k1, d1, k2, d2, src = _tiny_base()
    return Frames(k1[:n1], d1[:n1], k2[:n2], d2[:n2], BOUNDS, src[:n1])


def frames(name) -> Frames:
    return crowd() if name == "crowd" else tiny(*name)


# The seed of the orb_scene helpers per frame pair. On the tiny pairs the helpers' random flags
# (in view, bad, occupied slots, NULL map points) decide whether a single keypoint can match at
# all: the seeds are the first for which every search finds a match (test_orb_edge_ref.py).
SEEDS = {(1, 1): 11, (3, 5): 0, (5, 3): 0}


def seed_of(name) -> int:
    return SEEDS.get(name, 3)


# ---- BoW nodes ------------------------------------------------------------------------
def hamming_matrix(a, b):
    return np.unpackbits(a[:, None, :] ^ b[None, :, :], axis=2).sum(axis=2)


@functools.lru_cache(maxsize=None)
def bow_nodes(name, seed):
    """(node per side-1 feature, node per side-2 feature): side 2 from BOW_RUNS
    (one node for a tiny frame), side 1 the node of its nearest side-2 descriptor."""
    F = frames(name)
    n1, n2 = len(F.k1), len(F.k2)
    rng = np.random.default_rng(seed + 57)
    runs = BOW_RUNS if n2 >= sum(BOW_RUNS) else ((n2,) if n2 else ())
    ids = 1000 + 37 * rng.permutation(len(runs))  # node order differs from the run-length order
    node2 = np.full(n2, -1, np.int32)
    perm = rng.permutation(n2)
    o = 0
    for r, nid in zip(runs, ids):
        node2[perm[o:o + r]] = nid
        o += r
    node1 = np.full(n1, -1, np.int32)
    if n1 and n2:
        node1 = node2[hamming_matrix(F.d1, F.d2).argmin(axis=1)].astype(np.int32)
    _freeze(node1, node2)
    return node1, node2


# ---- the eleven searches -----------------------------------------------------------------
# search: parameter tuples (the grids of tests/test_orb_gpu.py)
SEARCHES = {
    "init": [(True,), (False,)],                                     # check_ori; window 100, nnratio 0.9
    "local": [(False, 1.0, 0.8), (True, 1.0, 0.8), (True, 5.0, 0.9), (False, 10.0, 0.6)],  # stereo, th, nnratio
    "last": [(False, True, 0.0, 7.0, True), (True, False, 1.0, 7.0, True), (True, False, -1.0, 15.0, True),
             (True, False, 0.0, 15.0, False)],                      # stereo, mono, tz, th, check_ori
    "proj_sim3": [(1.0, 10), (1.3, 10), (0.8, 4)],                   # s, th
    "fuse": [(False, 3.0), (True, 5.0)],                             # stereo, th
    "fuse_sim3": [(4.0,)],                                           # th
    "proj_kf": [(10.0, 100, True), (3.0, 64, False)],                # th, ORBdist, check_ori
    "bow_kf_frame": [(True,), (False,)],                             # check_ori
    "bow_kf_kf": [(True,), (False,)],
    "triangulation": [(False, False, False), (True, False, True), (True, True, False)],  # stereo, only, check_ori
    "sim3": [(1.0, 7.5), (1.03, 10.0)],                              # s12, th
}
# the four searches held to >= 100 oracle matches on crowd, and the case that is held (every other: >= 30)
MEASURED = {"init": (True,), "local": (True, 5.0, 0.9), "bow_kf_frame": (True,), "bow_kf_kf": (True,)}
CASES = [(s, p) for s, grid in SEARCHES.items() for p in grid]


def _sim3_scene(F, seed):
    if len(F.k1) >= 40 and len(F.k2) >= 40:
        return S.sim3_scene(F.k1, F.d1, F.k2, F.d2, SHIFT, W, H, seed)
    # orb_scene.sim3_scene seeds vpMatches12 with 20 earlier matches; a tiny frame has none
    T1 = S.keyframe_pose((0.0, 0.0), W, H)
    T2 = S.keyframe_pose(SHIFT, W, H, (0.05, 0.0, 0.02))
    mp1, md1 = S.map_points(F.k1, F.d1, W, H, seed)
    mp2, md2 = S.keyframe_points(F.k2, F.d2, T2, W, H, seed + 1)
    mp2["id"] = np.arange(len(mp2)) + 20000
    R2, t2 = T2[:, :3].astype(np.float64), T2[:, 3].astype(np.float64)
    return (T1, T2, mp1, md1, mp2, md2, R2.T.astype(np.float32), (-R2.T @ t2).astype(np.float32),
            np.full(len(F.k1), -1, np.int32))


@functools.lru_cache(maxsize=None)
def inputs(name, search, params, seed):
    """The derived inputs of one search on one frame pair, as a dict."""
    F = frames(name)
    k1, d1, k2, d2 = F.k1, F.d1, F.k2, F.d2
    if search == "init":
        return dict(prev=np.ascontiguousarray(np.stack([k1["x"], k1["y"]], 1), np.float32))
    if search == "local":
        stereo = params[0]
        mps, md = S.local_points(k1, d1, SHIFT, seed, stereo)
        ur, sm, so = S.current_slots(k2, seed, stereo)
        return dict(mps=mps, md=md, ur=ur, sm=sm, so=so)
    if search == "last":
        stereo, _, tz = params[:3]
        Tcw, Tlw, lp, ld = S.last_frame(k1, d1, SHIFT, W, H, seed, tz=tz)
        ur, sm, so = S.current_slots(k2, seed, stereo)
        return dict(Tcw=Tcw, Tlw=Tlw, lp=lp, ld=ld, ur=ur, sm=sm, so=so)
    if search in ("proj_sim3", "fuse", "fuse_sim3", "proj_kf"):
        mps, md = S.map_points(k1, d1, W, H, seed)
        ur, sm, so = S.current_slots(k2, seed, search == "fuse" and params[0])
        t = {"proj_sim3": (0.02, 0.0, 0.1), "proj_kf": (0.01, 0.0, -0.1)}.get(search, (0.0, 0.01, 0.05))
        T = S.keyframe_pose(SHIFT, W, H, t)
        Tq = S.sim3_of(T, params[0]) if search == "proj_sim3" else S.sim3_of(T, 1.2) if search == "fuse_sim3" else T
        return dict(mps=mps, md=md, ur=ur, sm=sm, so=so, T=T, Tq=Tq)
    if search in ("bow_kf_frame", "bow_kf_kf"):
        n1, n2 = bow_nodes(name, seed)
        mp1, bad1 = S.bow_points(len(k1), seed)
        mp2, bad2 = S.bow_points(len(k2), seed + 1, base=10000)
        return dict(n1=n1, n2=n2, mp1=mp1, bad1=bad1, mp2=mp2, bad2=bad2)
    if search == "triangulation":
        stereo = params[0]
        n1, n2 = bow_nodes(name, seed + 2)
        T1 = S.keyframe_pose((0.0, 0.0), W, H)
        T2 = S.keyframe_pose(SHIFT, W, H, (0.3, 0.0, 0.05))
        mp1, _ = S.bow_points(len(k1), seed + 2, frac=0.3)
        mp2, _ = S.bow_points(len(k2), seed + 3, frac=0.3)
        ur1, _, _ = S.current_slots(k1, seed + 2, stereo)
        ur2, _, _ = S.current_slots(k2, seed + 3, stereo)
        Ow = -(T1[:, :3].T.astype(np.float64) @ T1[:, 3].astype(np.float64))  # T1 = [I | 0]: exact in any precision
        return dict(n1=n1, n2=n2, mp1=mp1, mp2=mp2, ur1=ur1, ur2=ur2, T1=T1, T2=T2, C1=Ow.astype(np.float32),
                    F12=S.fundamental_12(T1, T2, CAM, CAM))
    if search == "sim3":
        return dict(zip(("T1", "T2", "mp1", "md1", "mp2", "md2", "R12", "t12", "m12"), _sim3_scene(F, seed)))
    raise KeyError(search)


def _pairs(m12):
    i1 = np.nonzero(m12 >= 0)[0]
    return np.stack([i1, m12[i1]], 1).astype(np.int64).reshape(-1, 2)


def run_oracle(OB, name, search, params, seed=None, translit=False):
    """One search on the C oracle (or, translit=True, on the Python transliteration):
    a tuple (matches, output arrays ...), the outputs tests/test_orb_gpu.py compares."""
    import orb_translit as T
    F = frames(name)
    k1, d1, k2, d2, b = F.k1, F.d1, F.k2, F.d2, F.bounds
    I = inputs(name, search, params, seed_of(name) if seed is None else seed)
    if search == "init":
        if translit:
            return T._py_search_for_init(k1, d1, k2, d2, b, I["prev"], 100, 0.9, params[0])
        return OB.search_for_init(k1, d1, k2, d2, b, I["prev"], 100, 0.9, params[0])
    if search == "local":
        a = (k2, d2, b, SF, I["ur"], I["sm"], I["so"], I["mps"], I["md"], params[1], params[2])
        return T._py_sbp_local(*a) if translit else OB.search_by_projection_local(*a)
    if search == "last":
        a = (k2, d2, b, SF, CAM, I["ur"], I["sm"], I["so"], I["Tcw"], I["Tlw"], I["lp"], I["ld"], params[3], params[1],
             params[4])
        return T._py_sbp_last(*a) if translit else OB.search_by_projection_last(*a)
    if search == "proj_sim3":
        a = (k2, d2, b, SF, CAM, I["sm"], I["Tq"], I["mps"], I["md"], params[1])
        return T._py_sbp_sim3(*a) if translit else OB.search_by_projection_sim3(*a)
    if search in ("fuse", "fuse_sim3"):
        a = (k2, d2, b, SF, CAM, I["ur"], I["Tq"], search == "fuse_sim3", I["mps"], I["md"], params[-1])
        return T._py_fuse(*a) if translit else OB.fuse(*a)
    if search == "proj_kf":
        a = (k2, d2, b, SF, CAM, I["sm"], I["T"], I["mps"], I["md"], k1["angle"], *params)
        return T._py_sbp_kf(*a) if translit else OB.search_by_projection_kf(*a)
    if search == "bow_kf_frame":
        kf = (k1, d1, I["n1"], I["mp1"], I["bad1"])
        if translit:
            return T._py_bow_kf_frame(kf, (k2, d2, I["n2"]), 0.7, params[0])
        return OB.search_by_bow_kf_frame(kf, (k2, d2, I["n2"], I["mp2"]), 0.7, params[0])
    if search == "bow_kf_kf":
        a = ((k1, d1, I["n1"], I["mp1"], I["bad1"]), (k2, d2, I["n2"], I["mp2"], I["bad2"]), 0.75, params[0])
        return T._py_bow_kf_kf(*a) if translit else OB.search_by_bow_kf_kf(*a)
    if search == "triangulation":
        a = ((k1, d1, I["n1"], I["mp1"], None, I["ur1"]), (k2, d2, I["n2"], I["mp2"], None, I["ur2"]), I["C1"], I["T2"],
             CAM[:4], SF, I["F12"], params[1], params[2])
        n, m12 = T._py_triangulation(*a) if translit else OB.search_for_triangulation(*a)
        return n, _pairs(m12)
    if search == "sim3":
        a = (k1, d1, k2, d2, b, SF, CAM, I["T1"], I["T2"], I["mp1"], I["md1"], I["mp2"], I["md2"], params[0], I["R12"],
             I["t12"], params[1], I["m12"])
        return T._py_search_by_sim3(*a) if translit else OB.search_by_sim3(*a)
    raise KeyError(search)


def gpu_frame(F, I, Tcw=None):
    from sqrtlm.orb import Frame
    fx, fy, cx, cy, bf, mb = CAM
    return Frame(F.k2, F.d2, F.bounds, SF, fx, fy, cx, cy, bf, mb, mvuRight=I.get("ur"), mTcw=Tcw,
                 mvpMapPoints=I["sm"].copy(), slot_obs=I["so"].copy())


def run_gpu(ctx, name, search, params, seed=None):
    """The same search through sqrtlm.orb.ORBmatcher: the tuple run_oracle returns."""
    from sqrtlm.orb import BowFrame, Frame, KeyFrameSlots, LastFrameSlots, ORBmatcher
    F = frames(name)
    k1, d1, k2, d2, b = F.k1, F.d1, F.k2, F.d2, F.bounds
    I = inputs(name, search, params, seed_of(name) if seed is None else seed)
    if search == "init":
        prev = I["prev"].copy()
        n, m = ORBmatcher(0.9, params[0], ctx=ctx).SearchForInitialization(k1, d1, k2, d2, b, prev, 100)
        return n, m, prev
    if search == "local":
        G = gpu_frame(F, I)
        n = ORBmatcher(params[2], ctx=ctx).SearchByProjection(G, I["mps"], I["md"], params[1])
        return n, G.mvpMapPoints, G.slot_obs
    if search == "last":
        G = gpu_frame(F, I, I["Tcw"])
        n = ORBmatcher(0.9, params[4], ctx=ctx).SearchByProjection(G, LastFrameSlots(I["Tlw"], I["lp"], I["ld"]),
                                                                  params[3], params[1])
        return n, G.mvpMapPoints, G.slot_obs
    if search == "proj_sim3":
        G = gpu_frame(F, I)
        n = ORBmatcher(0.75, ctx=ctx).SearchByProjection(G, I["Tq"], I["mps"], I["md"], params[1])
        return n, G.mvpMapPoints
    if search in ("fuse", "fuse_sim3"):
        G = gpu_frame(F, I, I["T"])
        m = ORBmatcher(0.6, ctx=ctx)
        if search == "fuse_sim3":
            return m.Fuse(G, I["Tq"], I["mps"], I["md"], params[0])
        return m.Fuse(G, I["mps"], I["md"], params[1])
    if search == "proj_kf":
        G = gpu_frame(F, I, I["T"])
        n = ORBmatcher(0.75, params[2], ctx=ctx).SearchByProjection(G, KeyFrameSlots(I["mps"], I["md"], k1["angle"]),
                                                                   params[0], params[1])
        return n, G.mvpMapPoints
    if search == "bow_kf_frame":
        KF = BowFrame(k1, d1, I["n1"], I["mp1"], I["bad1"])
        return ORBmatcher(0.7, params[0], ctx=ctx).SearchByBoW(KF, BowFrame(k2, d2, I["n2"], keyframe=False))
    if search == "bow_kf_kf":
        KF = BowFrame(k1, d1, I["n1"], I["mp1"], I["bad1"])
        return ORBmatcher(0.75, params[0], ctx=ctx).SearchByBoW(KF, BowFrame(k2, d2, I["n2"], I["mp2"], I["bad2"]))
    if search == "triangulation":
        K1 = BowFrame(k1, d1, I["n1"], I["mp1"], None, I["ur1"], Tcw=I["T1"], cam=CAM[:4], mvScaleFactors=SF)
        K2 = BowFrame(k2, d2, I["n2"], I["mp2"], None, I["ur2"], Tcw=I["T2"], cam=CAM[:4], mvScaleFactors=SF)
        assert np.array_equal(K1.GetCameraCenter(), I["C1"])
        n, pairs = ORBmatcher(0.6, params[2], ctx=ctx).SearchForTriangulation(K1, K2, I["F12"], params[1])
        return n, np.array(pairs, np.int64).reshape(-1, 2)
    if search == "sim3":
        K1 = Frame(k1, d1, b, SF, *CAM[:4], mTcw=I["T1"])
        K2 = Frame(k2, d2, b, SF, *CAM[:4], mTcw=I["T2"])
        m = I["m12"].copy()
        n = ORBmatcher(0.75, ctx=ctx).SearchBySim3(K1, K2, I["mp1"], I["md1"], I["mp2"], I["md2"], m, params[0],
                                                    I["R12"], I["t12"], params[1])
        return n, m
    raise KeyError(search)


# ---- query counts of the local projection search (k_orb_scan: chunk = ceil(n / 1024)) ----
QUERY_COUNTS = (1, 3, 1023, 1024, 1025, 2049)
LOCAL_Q_PARAMS = (True, 5.0, 0.9)  # stereo, th, nnratio
LOCAL_Q_SEEDS = {1: 2, 3: 3}       # the first seeds for which the one and the three points match (else: m)


@functools.lru_cache(maxsize=None)
def local_queries(m):
    """m map points sampled with repetition from crowd's frame 1 (orb_scene.local_points
    appends n // 5 duplicates with fresh ids; the first m entries are kept)."""
    F = crowd()
    seed = LOCAL_Q_SEEDS.get(m, m)
    idx = np.random.default_rng(1000 + seed).integers(0, len(F.k1), m)
    mps, md = S.local_points(F.k1[idx], F.d1[idx], SHIFT, seed, True)
    ur, sm, so = S.current_slots(F.k2, seed, True)
    return dict(mps=mps[:m].copy(), md=np.ascontiguousarray(md[:m]), ur=ur, sm=sm, so=so)


# ---- area search bounds: windows beside the grid and one over all of it ----------------
def area_bound_points(F):
    """Six local map points on a tiny frame: windows entirely left of, right of, above
    and below the grid, one over all 64 x 48 cells, one over none of the keypoints
    (th 1000: the window's half side is 4000 px)."""
    minx, maxx, miny, maxy = F.bounds
    cx, cy = (minx + maxx) / 2, (miny + maxy) / 2
    mps = np.zeros(6, S.TRACK_POINT_DTYPE)
    mps["id"] = np.arange(6) + 300
    mps["proj_x"] = [minx - 1e5, maxx + 1e5, cx, cx, cx, cx + 4500.0]
    mps["proj_y"] = [cy, cy, miny - 1e5, maxy + 1e5, cy, cy]
    mps["proj_xr"] = -1.0
    mps["view_cos"] = 0.99
    mps["level"] = 0
    mps["in_view"] = 1
    mps["has_obs"] = 1
    md = np.ascontiguousarray(np.resize(F.d2, (6, 32)) if len(F.d2) else np.zeros((6, 32), np.uint8))
    return mps, md, 1000.0


# ---- brute force --------------------------------------------------------------------------
BF_CASES = ((1, 1, "random"), (1, 2, "random"), (255, 256, "random"), (256, 257, "random"), (257, 255, "random"),
            (513, 64, "random"), (256, 257, "equal"))


@functools.lru_cache(maxsize=None)
def bf_case(nq, nt, kind):
    """(query, train, [(query index, first train index, second train index)] of the planted duplicates)."""
    rng = np.random.default_rng(nq * 1000 + nt)
    if kind == "equal":
        row = rng.integers(0, 256, 32, dtype=np.uint8)
        q, t = np.tile(row, (nq, 1)), np.tile(row, (nt, 1))
        _freeze(q, t)
        return q, t, ()
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    planted = []
    if nt >= 2:
        # the same descriptor twice in train: on both sides of the 256-row tile boundary where there
        # is one, in the last two rows otherwise; the queries sit at the query-side block boundaries
        pairs = [(255, 256)] if nt > 256 else []
        pairs += [(0, nt - 1)] + ([(nt - 3, nt - 2)] if nt >= 5 else [])
        pairs = [p for i, p in enumerate(pairs) if not any(set(p) & set(o) for o in pairs[:i])]
        for qi, (a, b) in zip(sorted({0, min(255, nq - 1), nq - 1}), pairs):
            t[a] = q[qi]
            t[b] = q[qi]
            planted.append((qi, a, b))
    _freeze(q, t)
    return q, t, tuple(planted)


# ---- extractor -----------------------------------------------------------------------------
EDGE_THRESHOLD = 19


def min_size(OB):
    """The smallest (w, h) all 8 default levels accept, from the oracle's level geometry."""
    def ok(w, h):
        try:
            OB.levels(OB.params(), w, h)
            return True
        except ValueError:
            return False
    # both sides obey the same rule (the top level keeps one 30-px cell between its borders), and a
    # square passes the aspect rule of DistributeOctTree: the smallest accepted square is the answer
    v = next(v for v in range(64, 1000) if ok(v, v))
    return v, v


def block_image(w, h, seed):
    """Saturated 0 / 255 blocks of 3..5 px a side: FAST scores at the top of the uint8
    score plane and dense response ties."""
    rng = np.random.default_rng(seed)
    cols = np.repeat(np.arange(w), rng.integers(3, 6, w))[:w]
    rows = np.repeat(np.arange(h), rng.integers(3, 6, h))[:h]
    val = rng.integers(0, 2, (h, w), dtype=np.uint8) * 255
    return np.ascontiguousarray(val[rows[:, None], cols[None, :]])


def border_image(w, h, seed):
    """Weak texture inside, a 0 / 255 checkerboard of 5-px squares (counted from the nearest
    border) in a 24-px band along every border: strong corners within EDGE_THRESHOLD of each
    side, the innermost of them exactly on the first and last pixel the extractor may keep."""
    rng = np.random.default_rng(seed)
    img = np.clip(128 + rng.normal(0, 4, (h, w)), 0, 255).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    u, v = np.minimum(xx, w - 1 - xx), np.minimum(yy, h - 1 - yy)
    check = (((((u + 4) // 5) + ((v + 4) // 5)) % 2) * 255).astype(np.uint8)
    band = (u < 24) | (v < 24)
    img[band] = check[band]
    return img


def _synth(w, h, seed):
    return lambda: synth.make_image_pair(w, h, seed=seed)[0]


# name: (image builder, (nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST))
EXTRACT_CASES = {
    "w4096": (_synth(4096, 240, 2), (2000, 1.2, 8, 20, 7)),
    "one_level": (_synth(322, 243, 3), (500, 1.2, 1, 20, 7)),
    "scale2_3lv": (_synth(646, 362, 4), (1000, 2.0, 3, 20, 7)),
    "scale1.1_12lv": (_synth(421, 317, 5), (1500, 1.1, 12, 20, 7)),
    "nfeat0": (_synth(320, 240, 6), (0, 1.2, 8, 20, 7)),
    "nfeat1": (_synth(320, 240, 6), (1, 1.2, 8, 20, 7)),
    "nfeat50000": (_synth(320, 240, 6), (50000, 1.2, 8, 20, 7)),
    "blocks": (lambda: block_image(331, 246, 7), (2000, 1.2, 8, 20, 7)),
    "border": (lambda: border_image(352, 288, 8), (1000, 1.2, 8, 20, 7)),
    "synth643": (_synth(643, 361, 9), (2000, 1.2, 8, 20, 7)),
    "synth486": (_synth(486, 365, 10), (1200, 1.2, 8, 20, 7)),
}


@functools.lru_cache(maxsize=None)
def extract_image(name):
    img = np.ascontiguousarray(EXTRACT_CASES[name][0](), np.uint8)
    _freeze(img)
    return img


def strided(img, stride, fill, seed=0):
    """img as a view into a buffer of the given row stride whose padding holds `fill`
    (a byte value, or "noise")."""
    h, w = img.shape
    if fill == "noise":
        buf = np.random.default_rng(seed).integers(0, 256, (h, stride), dtype=np.uint8)
    else:
        buf = np.full((h, stride), fill, np.uint8)
    buf[:, :w] = img
    return buf[:, :w]
