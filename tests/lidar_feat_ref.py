"""The numpy definition of sqlm_lidar_features (include/sqrtlm.h): the flat-point
path of the reference's Frame::lidarProcess with every sequential part restated
as an order-free rule. Float expressions are numpy float32 operations, double
ones float64 / Python floats, in the order the header states; numpy and CPython
do not contract to FMA. atan / atan2 restate the fdlibm polynomials of
include/sqlm_libm.h.

``process(xyz, P, extrinsic)`` handles one sweep and returns the outputs and the
intermediate state under the names sqrtlm.lidar_feat uses."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
PI = math.pi
MAX_HALF = 8
PIVOT_TOL2 = 1e-24
NONE, MASKED, CURVATURE, FEW_SEARCH, DEGENERATE, PLANE_INVALID, OVER_CAP, PICKED = range(8)

_HI = [0.0, 4.63647609000806093515e-01, 7.85398163397448278999e-01, 9.82793723247329054082e-01,
       1.57079632679489655800e+00]
_LO = [0.0, 2.26987774529616870924e-17, 3.06161699786838301793e-17, 1.39033110312309984516e-17,
       6.12323399573676603587e-17]
_AT = [3.33333333333329318027e-01, -1.99999999998764832476e-01, 1.42857142725034663711e-01,
       -1.11111104054623557880e-01, 9.09088713343650656196e-02, -7.69187620504482999495e-02,
       6.66107313738753120669e-02, -5.83357013379057348645e-02, 4.97687799461593236017e-02,
       -3.65315727442169155270e-02, 1.62858201153657823623e-02]


def atan(x, xlo=None):
    """sqlm_atan on a float64 array; with xlo, sqlm_lm_atan_lo: atan(x) + xlo / (1 + x x), the
    correction entering before the last rounding."""
    x = np.asarray(x, f64)
    xlo = np.zeros_like(x) if xlo is None else np.asarray(xlo, f64)
    neg, ax = np.signbit(x), np.abs(x)
    a = _AT
    with np.errstate(all="ignore"):
        idx = np.select([ax < 0.4375, ax < 0.6875, ax < 1.1875, ax < 2.4375], [0, 1, 2, 3], 4)
        t = np.select([idx == 0, idx == 1, idx == 2, idx == 3],
                      [x, (2.0 * ax - 1.0) / (2.0 + ax), (ax - 1.0) / (ax + 1.0), (ax - 1.5) / (1.0 + 1.5 * ax)],
                      -1.0 / ax)
        hi, lo = np.asarray(_HI)[idx], np.asarray(_LO)[idx]
        z = t * t
        w = z * z
        s1 = z * (a[0] + w * (a[2] + w * (a[4] + w * (a[6] + w * (a[8] + w * a[10])))))
        s2 = w * (a[1] + w * (a[3] + w * (a[5] + w * (a[7] + w * a[9]))))
        c = xlo / (1.0 + ax * ax)
        small = t - (t * (s1 + s2) - c)
        r = hi - ((t * (s1 + s2) - (lo + np.where(neg, -c, c))) - t)
        out = np.where(idx == 0, small, np.where(neg, -r, r))
        out = np.where(ax < 1.862645149230957e-09, np.where(xlo == 0.0, x, x + xlo), out)
        out = np.where(ax >= 7.3786976294838206464e19, np.where(neg, -_HI[4] - _LO[4], _HI[4] + _LO[4]), out)
        out = np.where(np.isnan(x), x + x, out)
    return out


def atan2(y, x):
    """sqlm_atan2 on float64 arrays."""
    y, x = np.broadcast_arrays(np.asarray(y, f64), np.asarray(x, f64))
    y, x = np.ascontiguousarray(y), np.ascontiguousarray(x)
    pi_o_2, pi, pi_lo = 1.5707963267948965580e+00, 3.1415926535897931160e+00, 1.2246467991473531772e-16
    hx, hy = x.view(np.int64) >> 32, y.view(np.int64) >> 32
    m = ((hy >> 31) & 1) | ((hx >> 30) & 2)
    k = ((hy & 0x7fffffff) - (hx & 0x7fffffff)) >> 20
    with np.errstate(all="ignore"):
        q = y / x
        q = np.where(q < 0.0, -q, q)
        # the quotient's rounding error, |y| - q |x| exactly by Dekker's product, over |x|
        ay, ax = np.abs(y), np.abs(x)
        t = 134217729.0 * q
        qh = t - (t - q)
        ql = q - qh
        t = 134217729.0 * ax
        xh = t - (t - ax)
        xl = ax - xh
        p = q * ax
        e = (((qh * xh - p) + qh * xl) + ql * xh) + ql * xl
        lo_b, hi_b = 3.0549363634996047e-151, 3.273390607896142e+150  # 2^-500, 2^500
        ok = (ax > lo_b) & (ax < hi_b) & (ay > lo_b) & (ay < hi_b)
        dq = np.where(ok, ((ay - p) - e) / ax, 0.0)
        z = atan(q, dq)
        z = np.where(k > 60, pi_o_2 + 0.5 * pi_lo, np.where((hx < 0) & (k < -60), 0.0, z))
        r = np.select([m == 0, m == 1, m == 2], [z, -z, pi - (z - pi_lo)], (z - pi_lo) - pi)
        r = np.where(x == 0.0, np.where(hy < 0, -pi_o_2, pi_o_2), r)
        r = np.where(y == 0.0, np.where(m < 2, y, np.where(m == 2, pi, -pi)), r)
        r = np.where(x == 1.0, atan(y), r)
        r = np.where(np.isnan(x) | np.isnan(y), x + y, r)
    return r


def sqrtf(v):
    return np.sqrt(np.asarray(v, f32).astype(f64)).astype(f32)


def atanf(v):
    return atan(np.asarray(v, f32).astype(f64)).astype(f32)


def atan2f(y, x):
    return atan2(np.asarray(y, f32).astype(f64), np.asarray(x, f32).astype(f64)).astype(f32)


def rings(xyz):
    """The virtual ring of every point, -1 for a dropped one."""
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(all="ignore"):
        fin = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        s = sqrtf(x * x + y * y)
        t = atanf(z / s) * f32(180.0)
        ang = (t.astype(f64) / PI).astype(f32)
        a64 = ang.astype(f64)
        up = np.trunc((f32(2.0) - ang).astype(f64) * 3.0 + 0.5)
        low = 32 + np.trunc((-8.83 - a64) * 2.0 + 0.5)
        rid = np.where(a64 >= -8.83, up, low)
        ok = fin & ~np.isnan(ang) & (rid >= 0) & (rid <= 63)
    return np.where(ok, rid, -1).astype(np.int32)


def oris(azi_first, azi_last):
    s = f32(f64(azi_first) + PI)
    e = f32(f64(azi_last) + 3.0 * PI)
    d = f32(e - s)
    if f64(d) > 3.0 * PI:
        e = f32(f64(e) - 2.0 * PI)
    elif f64(d) < PI:
        e = f32(f64(e) + 2.0 * PI)
    return s, e


def unpassed(azi, start):
    a64, s64 = azi.astype(f64), f64(start)
    return np.where(a64 < s64 - PI / 2.0, (a64 + 2.0 * PI).astype(f32),
                    np.where(a64 > s64 + PI * 3.0 / 2.0, (a64 - 2.0 * PI).astype(f32), azi))


def passed(azi, end):
    a = (azi.astype(f64) + 2.0 * PI).astype(f32)
    a64, e64 = a.astype(f64), f64(end)
    return np.where(a64 < e64 - PI * 3.0 / 2.0, (a64 + 2.0 * PI).astype(f32),
                    np.where(a64 > e64 + PI / 2.0, (a64 - 2.0 * PI).astype(f32), a))


def dist(p):
    return sqrtf(p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1] + p[..., 2] * p[..., 2])


def sqdiff(a, b, wb=None):
    if wb is None:
        d = a - b
    else:
        d = a - b * wb[..., None]
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


def mask_rules(pts, c):
    """The rule of every i in [c, m - c): 0 nothing, 1 masks [i - c, i], 2 masks [i + 1, i + c]."""
    m = len(pts)
    pc, pn = pts[c:m - c], pts[c + 1:m - c + 1]
    with np.errstate(all="ignore"):
        big = sqdiff(pc, pn).astype(f64) > 0.1
        depth, dn = dist(pc), dist(pn)
        deeper = depth > dn
        wd1 = sqrtf(sqdiff(pn, pc, dn / depth)) / dn
        wd2 = sqrtf(sqdiff(pc, pn, depth / dn)) / depth
    return np.where(big & deeper & (wd1.astype(f64) < 0.1), 1,
                    np.where(big & ~deeper & (wd2.astype(f64) < 0.1), 2, 0))


def curvatures(pts, ncr):
    """(curvature, half-width) of every i in [ncr, m - ncr) of a scan."""
    m = len(pts)
    i = np.arange(ncr, m - ncr)
    p = pts[i]
    with np.errstate(all="ignore"):
        q = 25.0 / dist(p).astype(f64) + 0.5
    n = np.where(q < 1073741824.0, np.trunc(np.where(q < 1073741824.0, q, 0.0)) + 1, ncr).astype(np.int64)
    n = np.where((i < n) | (i + n >= m), ncr, n)
    nn = 2 * n
    d = (-nn).astype(f32)[:, None] * p
    for j in range(1, int(n.max()) + 1 if len(n) else 0):
        use = j <= n
        a, b = pts[np.clip(i + j, 0, m - 1)], pts[np.clip(i - j, 0, m - 1)]
        with np.errstate(all="ignore"):
            d = np.where(use[:, None], d + (a + b), d)
    with np.errstate(all="ignore"):
        cv = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]) / nn.astype(f32)
    return cv.astype(f32), n.astype(np.int32)


def region(size, ncr, n_sub, j):
    sp = (ncr * (n_sub - j) + (size - ncr) * j) // n_sub
    ep = (ncr * (n_sub - 1 - j) + (size - ncr) * (j + 1)) // n_sub - 1
    return sp, ep


def qr_solve(A, b, sqrt=math.sqrt):
    """The column-pivoted Householder QR of the header on lists of Python floats; None = degenerate.
    (With np.longdouble entries and sqrt=np.sqrt: the same steps in extended precision.)"""
    m = len(A)
    A = [list(r) for r in A]
    b = list(b)
    perm = [0, 1, 2]
    max0 = 0.0
    for k in range(3):
        nrm = [0.0, 0.0, 0.0]
        for j in range(k, 3):
            s = 0.0
            for r in range(k, m):
                s += A[r][j] * A[r][j]
            nrm[j] = s
        if k == 0:
            max0 = max(nrm)
        best = k
        for j in range(k + 1, 3):
            if nrm[j] > nrm[best]:
                best = j
        if not nrm[best] > PIVOT_TOL2 * max0:
            return None
        if best != k:
            for r in range(m):
                A[r][k], A[r][best] = A[r][best], A[r][k]
            perm[k], perm[best] = perm[best], perm[k]
        alpha = A[k][k]
        nx = sqrt(nrm[best])
        beta = -nx if alpha >= 0.0 else nx
        v0, tau = alpha - beta, (beta - alpha) / beta
        for r in range(k + 1, m):
            A[r][k] = A[r][k] / v0
        for j in range(k + 1, 4):
            col = (lambda r: A[r][j]) if j < 3 else (lambda r: b[r])
            w = col(k)
            for r in range(k + 1, m):
                w += A[r][k] * col(r)
            w = tau * w
            if j < 3:
                A[k][j] -= w
                for r in range(k + 1, m):
                    A[r][j] -= A[r][k] * w
            else:
                b[k] -= w
                for r in range(k + 1, m):
                    b[r] -= A[r][k] * w
        A[k][k] = beta
    x2 = b[2] / A[2][2]
    x1 = (b[1] - A[1][2] * x2) / A[1][1]
    x0 = ((b[0] - A[0][1] * x1) - A[0][2] * x2) / A[0][0]
    x = [0.0, 0.0, 0.0]
    x[perm[0]], x[perm[1]], x[perm[2]] = x0, x1, x2
    return x


def gather(image_index, scans, row, idx, col, cw, P):
    """The search points of :1088-1138 in order, the scan point itself first."""
    row_num, col_num = image_index.shape
    out = [scans[row][idx]]

    def visit(r, c):
        k = image_index[r, c]
        if k >= 0:
            out.append(scans[r][k])

    def visit_row(r, centre):
        if centre:
            visit(r, col)
        for c in range(1, cw + 1):
            if col + c < col_num:
                visit(r, col + c)
            if col >= c:
                visit(r, col - c)

    visit_row(row, False)
    if row > 0:
        visit_row(row - 1, True)
    if row + 1 < row_num:
        visit_row(row + 1, True)
    return out


def half_width(d, P):
    with np.errstate(all="ignore"):
        q = f64(d) * 0.01 / (f64(P.deg_diff) / 180.0 * PI * f64(d)) + 0.5
    return 0 if np.isnan(q) else (MAX_HALF if q >= MAX_HALF + 1 else int(q))


def near_points(image_index, scans, cols, row, idx, P):
    """(number of search points, the near points as float32 rows in gather order)."""
    pt = scans[row][idx]
    cw = half_width(dist(pt), P)
    search = gather(image_index, scans, row, idx, int(cols[row][idx]), cw, P)
    S = np.asarray(search, f32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        near = sqdiff(pt[None, :], S).astype(f64) < P.max_sq_dis
    return len(search), S[near]


def candidate(image_index, scans, cols, row, idx, P):
    """(reason, float32 normal or None) of an unmasked, flat-enough scan point."""
    n_search, near = near_points(image_index, scans, cols, row, idx, P)
    if n_search < 5:
        return FEW_SEARCH, None
    if len(near) < 3:
        return DEGENERATE, None
    A = [[float(v) for v in r] for r in near]
    x = qr_solve(A, [-1.0] * len(A))
    if x is None:
        return DEGENERATE, None
    nrm = math.sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2])
    d0 = 1.0 / nrm
    n0, n1, n2 = x[0] / nrm, x[1] / nrm, x[2] / nrm
    for r in A:
        if abs(n0 * r[0] + n1 * r[1] + n2 * r[2] + d0) > 0.1:
            return PLANE_INVALID, None
    return PICKED, np.array([n0, n1, n2], f64).astype(f32)


def transform(ext, p):
    """pcl::transformPointCloud as the header defines it; ext None = copy."""
    p = np.asarray(p, f32).reshape(-1, 3)
    if ext is None:
        return p.copy()
    m = np.asarray(ext, f64).reshape(4, 4)
    q = p.astype(f64)
    return np.stack([((m[k, 0] * q[:, 0] + m[k, 1] * q[:, 1]) + m[k, 2] * q[:, 2]) + m[k, 3] for k in range(3)],
                    1).astype(f32)


def min_scan(P):
    return 2 * max(P.num_curvature_regions_flat, P.num_curvature_regions_corner) + 1


def image_of(xyz, P):
    """Rings, the range image and the scans of one sweep by the order-free rules."""
    n = len(xyz)
    R, Cn = P.row_num, P.col_num
    ring = rings(xyz) if n else np.zeros(0, np.int32)
    image_index = np.full((R, Cn), -1, np.int32)
    src = [np.zeros(0, np.int32) for _ in range(R)]
    cols = [np.zeros(0, np.int32) for _ in range(R)]
    kept = np.flatnonzero(ring >= 0)
    if len(kept):
        azi = np.zeros(n, f32)
        azi[kept] = -atan2f(xyz[kept, 1], xyz[kept, 0])
        start, end = oris(azi[kept[0]], azi[kept[-1]])
        A = unpassed(azi, start)
        turns = ((A - start).astype(f64) > PI) & (ring >= 0)
        half = int(np.flatnonzero(turns)[0]) if turns.any() else n
        a = np.where(np.arange(n) <= half, A, passed(azi, end))
        t = (a - start).astype(f64) / (2.0 * PI) * f64(Cn)
        col = np.fmod(np.trunc(t).astype(np.int64) + Cn, Cn)
        claim = np.flatnonzero((ring >= 0) & (ring < R) & (col >= 0) & (col < Cn))
        cell = ring[claim].astype(np.int64) * Cn + col[claim]
        with np.errstate(all="ignore"):
            key = (dist(xyz[claim]).view(np.uint32).astype(np.uint64) << np.uint64(32)) | claim.astype(np.uint64)
        none = np.uint64(0xffffffffffffffff)
        cell_key = np.full(R * Cn, none, np.uint64)
        np.minimum.at(cell_key, cell, key)
        cell_first = np.full(R * Cn, n, np.int64)
        np.minimum.at(cell_first, cell, claim)
        for r in range(R):
            occ = np.flatnonzero(cell_first[r * Cn:(r + 1) * Cn] < n)
            order = occ[np.argsort(cell_first[r * Cn + occ], kind="stable")]
            image_index[r, order] = np.arange(len(order))
            src[r] = (cell_key[r * Cn + order] & np.uint64(0xffffffff)).astype(np.int32)
            cols[r] = order.astype(np.int32)
    scans = [xyz[s] for s in src]
    return ring, image_index, src, cols, scans


def process(xyz, P, extrinsic=None):
    xyz = np.ascontiguousarray(xyz, f32).reshape(-1, 3)
    ring, image_index, src, cols, scans = image_of(xyz, P)
    R, ncr = P.row_num, P.num_curvature_regions_flat
    enabled = P.enabled()
    st = dict(mask=[], curvature=[], neighbours=[], sorted=[], reason=[])
    flat, flat_n, less, less_n, less_rc = [], [], [], [], []
    stats = dict(largest_subregion=0, candidates=0, picked=0)
    for r in range(R):
        pts, m = scans[r], len(scans[r])
        mask, curv, nbr = np.zeros(m, np.uint8), np.zeros(m, f32), np.zeros(m, np.int32)
        srt, reason = np.full(m, -1, np.int32), np.zeros(m, np.uint8)
        if enabled[r] and m > min_scan(P):
            rules = mask_rules(pts, ncr)
            for k in np.flatnonzero(rules):
                i = ncr + int(k)
                if rules[k] == 1:
                    mask[i - ncr:i + 1] = 1
                else:
                    mask[i + 1:i + ncr + 1] = 1
            cv_all, nb_all = curvatures(pts, ncr)
            for j in range(P.num_scan_subregions):
                sp, ep = region(m, ncr, P.num_scan_subregions, j)
                if ep <= sp:
                    continue
                size = ep - sp + 1
                stats["largest_subregion"] = max(stats["largest_subregion"], size)
                stats["candidates"] += size
                i = np.arange(sp, ep + 1)
                curv[i], nbr[i] = cv_all[i - ncr], nb_all[i - ncr]
                key = (curv[i].view(np.uint32).astype(np.uint64) << np.uint64(32)) | i.astype(np.uint64)
                order = i[np.argsort(key, kind="stable")]
                srt[sp:ep + 1] = order
                picked, stopped = 0, False
                for idx in order:
                    idx = int(idx)
                    if stopped:
                        reason[idx] = OVER_CAP
                    elif mask[idx]:
                        reason[idx] = MASKED
                    elif not f64(curv[idx]) < P.surf_curv_th:
                        reason[idx] = CURVATURE
                    else:
                        code, nrm = candidate(image_index, scans, cols, r, idx, P)
                        if code == PICKED:
                            if picked < P.max_surf_less_flat:
                                less.append(pts[idx])
                                less_n.append(nrm)
                                less_rc.append((r, cols[r][idx]))
                                if picked < P.max_surf_flat:
                                    flat.append(pts[idx])
                                    flat_n.append(nrm)
                                picked += 1
                            else:
                                code = OVER_CAP
                            stopped = picked >= P.max_surf_less_flat
                        reason[idx] = code
                stats["picked"] += picked
        for k, v in (("mask", mask), ("curvature", curv), ("neighbours", nbr), ("sorted", srt), ("reason", reason)):
            st[k].append(v)
    cat = lambda L, dt: np.concatenate(L).astype(dt) if L else np.zeros(0, dt)
    state = dict(ring=ring, scan_n=np.array([len(s) for s in src], np.int64), scan_src=cat(src, np.int32),
                 scan_col=cat(cols, np.int32), image_index=image_index,
                 mask=cat(st["mask"], np.uint8), curvature=cat(st["curvature"], f32),
                 neighbours=cat(st["neighbours"], np.int32), sorted=cat(st["sorted"], np.int32),
                 reason=cat(st["reason"], np.uint8))
    pts3 = lambda L: transform(extrinsic, np.asarray(L, f32).reshape(-1, 3))
    return dict(flat_xyz=pts3(flat), flat_normal=pts3(flat_n), less_xyz=pts3(less), less_normal=pts3(less_n),
                less_rc=np.asarray(less_rc, np.int32).reshape(-1, 2), state=state, stats=stats)
