"""The numpy definition of the corner branch of sqlm_lidar_features_all
(include/sqrtlm.h): the range image, scans and helpers are those of
tests/lidar_feat_ref.py; the cell state, the corner mask and curvature, the edge
predicate and the growth are restated here as order-free rules. Float
expressions are numpy float32 operations, double ones float64, in the order the
header states. acos / sin / cos restate the fdlibm polynomials of
include/sqlm_libm.h on arrays.

``process(xyz, P, CP, extrinsic)`` handles one sweep and returns the corner
outputs and the corner state under the names sqrtlm.lidar_feat uses. ``angle_fn``
replaces the float angle of a point pair (the accuracy test evaluates it in
longdouble)."""
import numpy as np

import lidar_feat_ref as R

f32, f64 = np.float32, np.float64
NONE, GROUND, MASKED, CURVATURE, UNSTABLE, OVER_CAP, PICKED = range(7)
OFFSETS = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1))


def _hi(x):
    return (np.ascontiguousarray(x, f64).view(np.int64) >> 32).astype(np.int64)  # signed, as the int cast


def _make_hi(hi):
    return (np.asarray(hi, np.int64) << 32).view(f64)


def _ksin(x, y, iy):
    S1, S2, S3 = -1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04
    S4, S5, S6 = 2.75573137070700676789e-06, -2.50507602534068634195e-08, 1.58969099521155010221e-10
    z = x * x
    v = z * x
    r = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)))
    out = x + v * (S1 + z * r) if iy == 0 else x - ((z * (0.5 * y - v * r) - y) - v * S1)
    return np.where((_hi(x) & 0x7fffffff) < 0x3e400000, x, out)


def _kcos(x, y):
    C1, C2, C3 = 4.16666666666666019037e-02, -1.38888888888741095749e-03, 2.48015872894767294178e-05
    C4, C5, C6 = -2.75573143513906633035e-07, 2.08757232129817482790e-09, -1.13596475577881948265e-11
    ix = _hi(x) & 0x7fffffff
    z = x * x
    r = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))))
    small = 1.0 - (0.5 * z - (z * r - x * y))
    qx = np.where(ix > 0x3fe90000, 0.28125, _make_hi(np.maximum(ix - 0x00200000, 0)))
    hz, a = 0.5 * z - qx, 1.0 - qx
    big = a - (hz - (z * r - x * y))
    return np.where(ix < 0x3e400000, 1.0, np.where(ix < 0x3FD33333, small, big))


def _rem_pio2(x):
    """(n, y0, y1) of sqlm_lm_rem_pio2 for finite |x| in the medium range."""
    invpio2, pio2_1, pio2_1t = 6.36619772367581382433e-01, 1.57079632673412561417e+00, 6.07710050650619224932e-11
    pio2_2, pio2_2t = 6.07710050630396597660e-11, 2.02226624879595063154e-21
    pio2_3, pio2_3t = 2.02226624871116645580e-21, 8.47842766036889956997e-32
    hx = _hi(x)
    ix = hx & 0x7fffffff
    t = np.abs(x)
    n = np.trunc(t * invpio2 + 0.5).astype(np.int64)
    fn = n.astype(f64)
    r = t - fn * pio2_1
    w = fn * pio2_1t
    j = ix >> 20
    y0 = r - w
    i = j - ((_hi(y0) >> 20) & 0x7ff)
    t2 = r
    w2 = fn * pio2_2
    r2 = t2 - w2
    w2 = fn * pio2_2t - ((t2 - r2) - w2)
    y0b = r2 - w2
    i2 = j - ((_hi(y0b) >> 20) & 0x7ff)
    t3 = r2
    w3 = fn * pio2_3
    r3 = t3 - w3
    w3 = fn * pio2_3t - ((t3 - r3) - w3)
    y0c = r3 - w3
    second, third = i > 16, (i > 16) & (i2 > 49)
    r = np.where(third, r3, np.where(second, r2, r))
    w = np.where(third, w3, np.where(second, w2, w))
    y0 = np.where(third, y0c, np.where(second, y0b, y0))
    y1 = (r - y0) - w
    neg = hx < 0
    return np.where(neg, -n, n), np.where(neg, -y0, y0), np.where(neg, -y1, y1)


def _sincos(x, cos):
    x = np.asarray(x, f64)
    with np.errstate(all="ignore"):
        ix = _hi(x) & 0x7fffffff
        ok = ix <= 0x413921fb
        xs = np.where(ok, x, 0.0)
        n, y0, y1 = _rem_pio2(xs)
        ks, kc = _ksin(y0, y1, 1), _kcos(y0, y1)
        q = (n + (1 if cos else 0)) & 3  # cos(x) = sin(x + pi/2)
        red = np.select([q == 0, q == 1, q == 2], [ks, kc, -ks], -kc)
        direct = _kcos(xs, np.zeros_like(xs)) if cos else _ksin(xs, np.zeros_like(xs), 0)
        out = np.where(ix <= 0x3fe921fb, direct, red)
        return np.where(ok, out, np.nan)


def sin(x):
    """sqlm_sin on a float64 array (medium range; beyond it and for inf / NaN: NaN)."""
    return _sincos(x, False)


def cos(x):
    """sqlm_cos on a float64 array."""
    return _sincos(x, True)


def acos(x):
    """sqlm_acos on a float64 array."""
    x = np.asarray(x, f64)
    pi, pio2_hi, pio2_lo = 3.14159265358979311600e+00, 1.57079632679489655800e+00, 6.12323399573676603587e-17
    pS = (1.66666666666666657415e-01, -3.25565818622400915405e-01, 2.01212532134862925881e-01,
          -4.00555345006794114027e-02, 7.91534994289814532176e-04, 3.47933107596021167570e-05)
    qS = (-2.40339491173441421878e+00, 2.02094576023350569471e+00, -6.88283971605453293030e-01,
          7.70381505559019352791e-02)
    hx = _hi(x)
    ix = hx & 0x7fffffff

    def ratio(z):
        p = z * (pS[0] + z * (pS[1] + z * (pS[2] + z * (pS[3] + z * (pS[4] + z * pS[5])))))
        q = 1.0 + z * (qS[0] + z * (qS[1] + z * (qS[2] + z * qS[3])))
        return p / q

    with np.errstate(all="ignore"):
        z = x * x
        small = pio2_hi - (x - (pio2_lo - x * ratio(z)))
        small = np.where(ix <= 0x3c600000, pio2_hi + pio2_lo, small)
        zn = (1.0 + x) * 0.5
        sn = np.sqrt(zn)
        neg = pi - 2.0 * (sn + (ratio(zn) * sn - pio2_lo))
        zp = (1.0 - x) * 0.5
        sp = np.sqrt(zp)
        df = _make_hi(_hi(sp))
        c = (zp - df * df) / (sp + df)
        pos = 2.0 * (df + (ratio(zp) * sp + c))
        out = np.where(ix < 0x3fe00000, small, np.where(hx < 0, neg, pos))
        one = np.where(x == 1.0, 0.0, np.where(x == -1.0, pi + 2.0 * pio2_lo, np.nan))
        return np.where(ix >= 0x3ff00000, one, out)


def angle(p1, p2):
    """The float angle of the edge predicate for float32 points (..., 3); symmetric bit for bit."""
    a, b = np.asarray(p1, f32).astype(f64), np.asarray(p2, f32).astype(f64)
    with np.errstate(all="ignore"):
        n1 = np.sqrt((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2])
        n2 = np.sqrt((b[..., 0] * b[..., 0] + b[..., 1] * b[..., 1]) + b[..., 2] * b[..., 2])
        dot = (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
        d1 = np.where(n1 > n2, n1, n2).astype(f32)
        d2 = np.where(n1 > n2, n2, n1).astype(f32)
        alpha = acos(dot / (n1 * n2)).astype(f32)
        sa, ca = sin(alpha.astype(f64)).astype(f32), cos(alpha.astype(f64)).astype(f32)
        ys, xs = d2 * sa, d1 - d2 * ca
        return R.atan2(ys.astype(f64), xs.astype(f64)).astype(f32)


def target(k, row, col, rows, cols):
    """The target cell of offset k from (row, col), None outside the rows."""
    r, c = row + OFFSETS[k][0], col + OFFSETS[k][1]
    if r < 0 or r >= rows:
        return None
    if c < 0:
        c = cols - 1
    if c >= cols:
        c = 0
    return r, c


def initial_state(image_index, scans, ground_z):
    rows, cols = image_index.shape
    st = np.full((rows, cols), -3, np.int32)
    for r in range(rows):
        occ = np.flatnonzero(image_index[r] >= 0)
        if len(occ):
            z = scans[r][image_index[r, occ], 2].astype(f64)
            st[r, occ] = np.where(z < ground_z, -1, 0)
    return st


def edges(image_index, scans, state0, angle_fn=angle):
    """(edge mask [rows][cols] uint8, angle [rows][cols][6] float32) of one sweep."""
    rows, cols = image_index.shape
    pts = np.zeros((rows, cols, 3), f32)
    for r in range(rows):
        occ = np.flatnonzero(image_index[r] >= 0)
        pts[r, occ] = scans[r][image_index[r, occ]]
    live = state0 == 0
    ang = np.full((rows, cols, 6), np.nan, f32)
    rr, cc = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    for k, (dr, dc) in enumerate(OFFSETS):
        tr, tc = rr + dr, cc + dc
        tc = np.where(tc < 0, cols - 1, np.where(tc >= cols, 0, tc))
        ok = (tr >= 0) & (tr < rows)
        trc = np.clip(tr, 0, rows - 1)
        ok &= live & live[trc, tc]
        if ok.any():
            a = np.asarray(angle_fn(pts[rr[ok], cc[ok]], pts[trc[ok], tc[ok]]), f32)
            a = np.where(np.isnan(a), f32(np.nan), a)  # one NaN for every producer
            ang[rr[ok], cc[ok], k] = a
    with np.errstate(invalid="ignore"):
        bits = ((ang > f32(1.0)) * (1 << np.arange(6))).sum(-1).astype(np.uint8)
    return bits, ang


def corner_mask(pts, c):
    m = len(pts)
    mask = np.zeros(m, np.uint8)
    rules = R.mask_rules(pts, c)
    i = np.arange(c, m - c)
    pc = pts[i]
    with np.errstate(all="ignore"):
        dn, dp = R.sqdiff(pc, pts[i + 1]).astype(f64), R.sqdiff(pc, pts[i - 1]).astype(f64)
        dis2 = (pc[:, 0] * pc[:, 0] + pc[:, 1] * pc[:, 1] + pc[:, 2] * pc[:, 2]).astype(f64)
        third = (rules == 0) & (dn > 0.0002 * dis2) & (dp > 0.0002 * dis2)
    for k in np.flatnonzero(rules):
        q = c + int(k)
        if rules[k] == 1:
            mask[q - c:q + 1] = 1
        else:
            mask[q + 1:q + c + 1] = 1
    mask[i[third]] = 1
    return mask, rules, third


def corner_curvatures(pts, c):
    """The corner curvature of every i in [c, m - c)."""
    m = len(pts)
    i = np.arange(c, m - c)
    nn = 2 * c
    with np.errstate(all="ignore"):
        d = f32(-nn) * pts[i]
        for j in range(1, c + 1):
            d = d + (pts[i + j] + pts[i - j])
        return ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]) / f32(nn)).astype(f32)


def grow(state, bits, seed, label):
    """The growth from ``seed`` (state 0): labels or -2 in ``state``; returns (cells of S, lineCount, BFS levels)."""
    rows, cols = state.shape
    S = {seed}
    frontier, levels = [seed], 0
    while frontier:
        levels += 1
        nxt = set()
        for (r, c) in frontier:
            for k in range(6):
                if bits[r, c] >> k & 1:
                    t = target(k, r, c, rows, cols)
                    if t is not None and state[t] == 0 and t not in S:
                        nxt.add(t)
        S |= nxt
        frontier = sorted(nxt, reverse=True)  # any order
    lines = len({r for (r, c) in S if (r, c) != seed})
    for cell in S:
        state[cell] = label if lines >= 3 else -2
    return S, lines, levels


def process(xyz, P, CP, extrinsic=None, angle_fn=angle, image=None):
    xyz = np.ascontiguousarray(xyz, f32).reshape(-1, 3)
    ring, image_index, src, cols, scans = R.image_of(xyz, P) if image is None else image
    rows, c, n_sub = P.row_num, P.num_curvature_regions_corner, P.num_scan_subregions
    enabled = CP.enabled()
    state = initial_state(image_index, scans, CP.ground_z_bound)
    state0 = state.copy()
    bits, ang = edges(image_index, scans, state0, angle_fn)
    st = dict(mask=[], curvature=[], sorted=[], reason=[])
    sharp, less, less_label, less_rc = [], [], [], []
    stats = dict(seeds_grown=0, cells_labelled=0, cells_unstable=0, largest_segment=0, most_levels=0, ungrown_passing=0)
    label = 1
    for r in range(rows):
        pts, m = scans[r], len(scans[r])
        mask, curv = np.zeros(m, np.uint8), np.zeros(m, f32)
        srt, reason = np.full(m, -1, np.int32), np.zeros(m, np.uint8)
        if enabled[r] and m > R.min_scan(P):
            mask, _, _ = corner_mask(pts, c)
            cv_all = corner_curvatures(pts, c)
            for j in range(n_sub):
                sp, ep = R.region(m, c, n_sub, j)
                if ep <= sp:
                    continue
                i = np.arange(sp, ep + 1)
                curv[i] = cv_all[i - c]
                key = (curv[i].view(np.uint32).astype(np.uint64) << np.uint64(32)) | i.astype(np.uint64)
                order = i[np.argsort(key, kind="stable")]
                srt[sp:ep + 1] = order
                num, stopped = 0, False
                for idx in order[::-1]:
                    idx = int(idx)
                    cell = (r, int(cols[r][idx]))
                    static = GROUND if state0[cell] == -1 else MASKED if mask[idx] else \
                        CURVATURE if not f64(curv[idx]) > CP.sharp_curv_th else NONE
                    if stopped:
                        reason[idx] = OVER_CAP
                        stats["ungrown_passing"] += int(static == NONE and state[cell] == 0)
                        continue
                    if static != NONE:
                        reason[idx] = static
                        continue
                    if state[cell] == 0:
                        S, _, levels = grow(state, bits, cell, label)
                        stats["seeds_grown"] += 1
                        stats["largest_segment"] = max(stats["largest_segment"], len(S))
                        stats["most_levels"] = max(stats["most_levels"], levels)
                        if state[cell] > 0:
                            label += 1
                            stats["cells_labelled"] += len(S)
                        else:
                            stats["cells_unstable"] += len(S)
                    if state[cell] < 1:
                        reason[idx] = UNSTABLE
                        continue
                    if num < CP.max_corner_less_sharp:
                        reason[idx] = PICKED
                        less.append(pts[idx])
                        less_label.append(int(state[cell]))
                        less_rc.append(cell)
                        if num < CP.max_corner_sharp:
                            sharp.append(pts[idx])
                        num += 1
                    else:
                        reason[idx] = OVER_CAP
                    stopped = num >= CP.max_corner_less_sharp
        for k, v in (("mask", mask), ("curvature", curv), ("sorted", srt), ("reason", reason)):
            st[k].append(v)
    cat = lambda L, dt: np.concatenate(L).astype(dt) if L else np.zeros(0, dt)
    cstate = dict(cell_state=state, initial_state=state0, mask=cat(st["mask"], np.uint8), curvature=cat(st["curvature"], f32),
                  sorted=cat(st["sorted"], np.int32), reason=cat(st["reason"], np.uint8), edge=bits, angle=ang,
                  scan_n=np.array([len(s) for s in src], np.int64), scan_col=cat(cols, np.int32))
    pts3 = lambda L: R.transform(extrinsic, np.asarray(L, f32).reshape(-1, 3))
    return dict(sharp_xyz=pts3(sharp), less_sharp_xyz=pts3(less), less_sharp_label=np.asarray(less_label, np.int32),
                less_sharp_rc=np.asarray(less_rc, np.int32).reshape(-1, 2), corner_state=cstate, stats=stats)
