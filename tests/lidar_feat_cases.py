"""Cases of the LiDAR flat-feature extraction, each at the smallest shape where
its rule can go wrong (tests/lidar_feat_ref.py is the definition they are
checked against). A case is (cloud, Params, extrinsic); ``reference(name)``
evaluates the definition once per session and is shared by the CPU and the GPU
tests. ``batches()`` groups the cases that share their parameters, the batch
being a property of one call."""
import functools
import math

import numpy as np

import lidar_feat_ref as R
from sqrtlm import lidar_feat as LF

f32 = np.float32
ALL = np.ones(128, np.uint8)


def small(rows=6, cols=256, **kw):
    """Small-shape parameters: every ring enabled, the reference's other defaults."""
    kw.setdefault("ring_enabled", ALL)
    return LF.Params(row_num=rows, col_num=cols, **kw)


def pt(el_deg, az_deg, rng):
    e, a = math.radians(el_deg), math.radians(az_deg)
    return [rng * math.cos(e) * math.cos(a), rng * math.cos(e) * math.sin(a), rng * math.sin(e)]


def room(seed, rows=6, cols=256, order="ring", start_deg=0.0, bump=True, **kw):
    """A 4 m room seen by the first ``rows`` rings: neighbours 0.1 to 0.2 m
    apart, so the walls are unmasked and flat near normal incidence. ``bump``
    pulls the points of a 17 degree window 30 % nearer: a depth jump at either
    end, one for each branch of the ring mask."""
    kw.setdefault("n_boxes", 0)
    kw.setdefault("noise", 0.002)
    kw.setdefault("dropout", 0.0)
    c = LF.make_sweep(seed, n_az=cols, order=order, start_deg=start_deg, room=4.0, rings=range(rows), **kw)
    if bump:
        az = np.arctan2(c[:, 1], c[:, 0])
        c[(az > 0.3) & (az < 0.6)] *= f32(0.7)
    return c


def lines(n_per_line, rows=(5, 6, 7), step=1.0 / 16, x=4.0):
    """Exactly planar, exactly regular: one line of points per ring in the
    plane x = 4, y = k * step, z = 0 or +-3/128 (all exact in float). Every
    interior curvature is exactly zero, so the sort is decided by the index.
    A step of 1/16 is 1.1 to 1.3 columns of 512 for up to 60 points a line,
    3/64 is 1.1 to 1.9 columns of 1024 for up to 140: no two points share a cell."""
    z = {5: 3.0 / 128, 6: 0.0, 7: -3.0 / 128}
    out = []
    for r in rows:
        k = np.arange(n_per_line) - n_per_line // 2
        out.append(np.stack([np.full(n_per_line, x), k * step, np.full(n_per_line, z[r])], 1))
    return np.concatenate(out).astype(f32)


ONLY6 = np.zeros(128, np.uint8)
ONLY6[6] = 1


def lines_params(**kw):
    kw.setdefault("ring_enabled", ONLY6)
    kw.setdefault("num_scan_subregions", 1)
    kw.setdefault("col_num", 512)
    return LF.Params(row_num=8, **kw)


def ring_limit_points():
    """Elevations 0.01 deg either side of ring boundaries: the ring-0 limit
    (2.5 deg), the -8.83 deg switch between the two formulas, the ring-63
    limit, and a few boundaries between."""
    els, want = [], []
    for e, w in ((2.51, -1), (2.49, 0), (2.0 - 0.5 / 3 + 0.01, 0), (2.0 - 0.5 / 3 - 0.01, 1),
                 (-8.82, 32), (-8.84, 32), (-8.83 + 0.25 - 0.01, 32), (-8.83 - 0.25 - 0.01, 33), (-8.83 - 0.25 + 0.01, 32),
                 (2.0 - 31.5 / 3 + 0.01, 31), (2.0 - 31.5 / 3 - 0.01, 32),
                 (-8.83 - 15.75 + 0.01, 63), (-8.83 - 15.75 - 0.01, -1), (60.0, -1), (-60.0, -1)):
        els.append(e)
        want.append(w)
    pts = [pt(e, -3.0 * k, 7.0 + 0.1 * k) for k, e in enumerate(els)]
    pts.append([0.0, 0.0, 0.0])     # angle NaN
    pts.append([0.0, 0.0, 2.0])     # straight up
    return np.asarray(pts, f32), np.asarray(want + [-1, -1], np.int32)


def _collisions():
    c = room(11)
    k = len(c) // 3
    extra = np.stack([c[k] * f32(0.9),            # nearer: takes the cell, not the index
                      c[k + 1],                   # equal distance: the earlier stays
                      c[k + 2] * f32(1.1),        # later and farther: changes nothing
                      c[k] * f32(0.8),            # a third point in one cell
                      c[k + 40] * f32(1.05)])
    return np.concatenate([c, extra]).astype(f32)


def _shuffled(seed):
    c = room(seed, cols=96, dropout=0.03, bump=False)
    return c[np.random.default_rng(seed).permutation(len(c))]


def _short_ring(m):
    """Ring 2 cut down to m scan points."""
    c = room(13)
    ring, _, src, _, _ = R.image_of(c, small())
    keep = ring != 2
    keep[src[2][:m]] = True  # the occupants of the ring's first m cells
    return c[keep]


def _outlier():
    c = lines(40)
    c[20, 0] += f32(0.3)  # one point of the first line leaves the plane, its cell and ring stay: the middle
    # line's candidates beside it keep their zero curvature and gather it
    return c


def _cap_case(k_valid, seed):
    """A sweep and a curvature threshold that lets exactly k_valid candidates
    of the one processed subregion (ring 2, one subregion) through."""
    c = room(seed, rows=5, cols=128, bump=False)
    P0 = small(rows=5, cols=128)
    ring, image_index, src, cols, scans = R.image_of(c, P0)
    cv, _ = R.curvatures(scans[2], 5)
    rules = R.mask_rules(scans[2], 5)
    mask = np.zeros(len(scans[2]), bool)
    for q in np.flatnonzero(rules):
        i = 5 + int(q)
        if rules[q] == 1:
            mask[i - 5:i + 1] = True
        else:
            mask[i + 1:i + 6] = True
    free = np.sort(cv[~mask[5:len(scans[2]) - 5]].astype(np.float64))
    th = 0.0 if k_valid == 0 else 0.5 * (free[k_valid - 1] + free[k_valid])
    only2 = np.zeros(128, np.uint8)
    only2[2] = 1
    return c, th, only2


@functools.lru_cache(maxsize=None)
def cases():
    C = {}
    rl, _ = ring_limit_points()
    C["ring_limits"] = (rl, LF.Params(row_num=64, col_num=128, ring_enabled=ALL), None)
    base = small()
    for name, start, order in (("start_0", 0.0, "azimuth"), ("start_100", 100.0, "azimuth"),
                               ("start_170", 170.0, "azimuth"), ("start_m100_ring", -100.0, "ring"),
                               ("start_179_ring", 179.0, "ring")):
        C[name] = (room(3, order=order, start_deg=start), base, None)
    c = room(5).copy()
    c[len(c) // 2] = [np.nan, 1.0, 1.0]
    c[len(c) // 2 + 7] = [1.0, np.inf, 1.0]
    C["non_finite"] = (c, base, None)
    C["empty"] = (np.zeros((0, 3), f32), base, None)
    C["dropped_only"] = (np.asarray([pt(60.0, 10.0 * k, 5.0) for k in range(9)], f32), base, None)
    C["rows_above_row_num"] = (room(6, rows=9), base, None)  # rings 6..8 are kept points without a cell
    C["collisions"] = (_collisions(), base, None)
    # arrival order is not column order; the scan order is arbitrary, so the curvature test is opened wide
    C["shuffled"] = (_shuffled(7), small(cols=96, surf_curv_th=1e9), None)
    one_sub = small(num_scan_subregions=1)
    for m in (10, 11, 12, 13):
        C[f"short_ring_{m}"] = (_short_ring(m), one_sub, None)
    C["short_ring_24_sub8"] = (_short_ring(24), base, None)  # subregions of one point (skipped) and of two
    wide = lines_params(col_num=1024)
    for size in (63, 64, 65, 129):
        C[f"region_{size}"] = (lines(size + 10, step=3.0 / 64), wide, None)
    C["three_lines_all_rings"] = (lines(60), lines_params(ring_enabled=ALL, num_scan_subregions=3), None)
    C["mask_both"] = (lines(32, step=0.375), lines_params(ring_enabled=ALL, num_scan_subregions=2), None)
    C["few_search"] = (lines(40, rows=(6,)), lines_params(deg_diff=1.0), None)
    C["few_near"] = (lines(40), lines_params(max_sq_dis=0.001), None)
    C["collinear_zero_column"] = (lines(40, rows=(6,)), lines_params(), None)
    only5 = np.zeros(128, np.uint8)
    only5[5] = 1
    C["collinear_proportional_columns"] = (lines(40, rows=(5,)), lines_params(ring_enabled=only5), None)
    C["outlier"] = (_outlier(), lines_params(ring_enabled=ALL, max_surf_less_flat=100), None)
    for k in (0, 1, 2, 3, 6, 7):
        c, th, only2 = _cap_case(k, 20 + k)
        for cf, cl in ((2, 6), (6, 6), (2, 2)):
            C[f"caps_{k}valid_{cf}_{cl}"] = (c, small(rows=5, cols=128, ring_enabled=only2, num_scan_subregions=1,
                                                      surf_curv_th=th, max_surf_flat=cf, max_surf_less_flat=cl), None)
    c, th, only2 = _cap_case(3, 31)
    C["caps_zero"] = (c, small(rows=5, cols=128, ring_enabled=only2, num_scan_subregions=1, surf_curv_th=th, max_surf_flat=0,
                               max_surf_less_flat=0), None)
    C["caps_flat_zero"] = (c, small(rows=5, cols=128, ring_enabled=only2, num_scan_subregions=1, surf_curv_th=th,
                                    max_surf_flat=0, max_surf_less_flat=6), None)
    C["corner_wider_than_flat"] = (_short_ring(16), small(num_curvature_regions_corner=7), None)
    ext = np.array([[0.0, -1.0, 0.0, 0.11], [0.0, 0.0, -1.0, -0.27], [1.0, 0.0, 0.0, 0.05], [0.0, 0.0, 0.0, 1.0]])
    th = 0.3
    ext[:3, :3] = ext[:3, :3] @ np.array([[math.cos(th), -math.sin(th), 0], [math.sin(th), math.cos(th), 0], [0, 0, 1]])
    C["extrinsic"] = (room(9), base, ext)
    C["full_size"] = (LF.make_sweep(3, n_az=1800, order="azimuth", start_deg=23.0), LF.Params(), None)
    return C


def names(full=True):
    return [n for n in cases() if full or n != "full_size"]


@functools.lru_cache(maxsize=None)
def reference(name):
    cloud, P, ext = cases()[name]
    return R.process(cloud, P, ext)


def batches():
    """[(Params, extrinsic, [names])]: the cases that share their parameters
    object and extrinsic, in case order; "full_size" stays alone."""
    out = []
    for n, (_, P, ext) in cases().items():
        if n == "full_size":
            continue
        for b in out:
            if b[0] is P and b[1] is ext:
                b[2].append(n)
                break
        else:
            out.append((P, ext, [n]))
    return out


def fillers(P):
    """Two sweeps that accompany a case whose parameters no other case shares."""
    return [room(41, rows=min(P.row_num, 6), cols=min(P.col_num, 128)), lines(30)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


OUT_KEYS = ("flat_xyz", "flat_normal", "less_xyz", "less_normal", "less_rc")
STATE_KEYS = ("ring", "scan_src", "scan_col", "image_index", "mask", "curvature", "neighbours", "sorted", "reason")


def slice_of(o, k, cloud_off=None, P=None):
    """Sweep k of a batched result (outputs and, if present, state) as a single-sweep result."""
    fl, fh = int(o["flat_off"][k]), int(o["flat_off"][k + 1])
    ll, lh = int(o["less_off"][k]), int(o["less_off"][k + 1])
    r = dict(flat_xyz=o["flat_xyz"][fl:fh], flat_normal=o["flat_normal"][fl:fh], less_xyz=o["less_xyz"][ll:lh],
             less_normal=o["less_normal"][ll:lh], less_rc=o["less_rc"][ll:lh])
    if "state" in o:
        st, R_ = o["state"], P.row_num
        so = st["scan_off"]
        a, b = int(so[k * R_]), int(so[(k + 1) * R_])
        s = {key: st[key][a:b] for key in ("scan_src", "scan_col", "mask", "curvature", "neighbours", "sorted", "reason")}
        s["ring"] = st["ring"][int(cloud_off[k]):int(cloud_off[k + 1])]
        s["image_index"] = st["image_index"][k * R_:(k + 1) * R_]
        s["scan_n"] = np.diff(so[k * R_:(k + 1) * R_ + 1])
        r["state"] = s
    return r


def differences(got, want):
    """The names of everything in which a single-sweep result differs from the definition's."""
    bad = [k for k in OUT_KEYS if not same(got[k], want[k])]
    if "state" in got:
        g, w = got["state"], want["state"]
        if not np.array_equal(g["scan_n"], w["scan_n"]):
            bad.append("scan_n")
        bad += [k for k in STATE_KEYS if not same(g[k], w[k])]
    return bad
