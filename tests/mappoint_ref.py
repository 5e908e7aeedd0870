"""The numpy definition of sqlm_triangulate_pairs and sqlm_map_points_update,
written operation by operation: what the host twins and the kernels have to
equal bit for bit (tests/test_mappoint_abi.py, tests/test_gpu_mappoint.py).

Floats are numpy float32 scalars (every operation on two of them is one IEEE
binary32 operation), doubles are Python floats (IEEE binary64, math.sqrt
correctly rounded). `f(x)` rounds a double to float, `d(x)` widens a float.

triangulate_match is LocalMapping::CreateNewMapPoints' match loop
(src/backend/LocalMapping.cc:436-624 of the reference, monocular branch) with
OpenCV's small-matrix expressions restated as DESIGN.md 8 states them and
cv::SVD::compute replaced by the library's fixed-sweep one-sided Jacobi
(DESIGN.md 8h). distinctive / normal_depth are MapPoint::
ComputeDistinctiveDescriptors and UpdateNormalAndDepth
(src/data_structure/MapPoint.cc:382-481, :531-578).
"""
from __future__ import annotations

import math

import numpy as np

f32 = np.float32
SWEEPS = 13       # the library's Jacobi sweep count (kTriSweeps)
ORTH_TOL = 1e-15
LDS_MAX = 128     # the longest track whose descriptors the kernel keeps in LDS (kMpLdsMax)


def f(x):
    with np.errstate(all="ignore"):
        return f32(x)


def d(x):
    return float(x)


def _div(a, b):
    """IEEE double division, also by zero."""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)


def _sqrt(a):
    if a != a or a < 0:
        return math.nan
    return math.sqrt(a)


def _dot3(a, b):
    s = 0.0
    for i in range(3):
        s += d(a[i]) * d(b[i])
    return s


def _norm3(a):
    return _sqrt(_dot3(a, a))


def center(T):
    """GetCameraCenter() = -Rcw.t() * tcw: float dots left to right, negated."""
    T = np.asarray(T, f32).reshape(12)
    with np.errstate(all="ignore"):
        return np.array([-(T[i] * T[3] + T[4 + i] * T[7] + T[8 + i] * T[11]) for i in range(3)], f32)


def null_vector(A, sweeps=SWEEPS):
    """One-sided Jacobi SVD in double of the 4x4 float A (row-major, 16): the right singular vector of the
    smallest singular value as floats, and the doubles before rounding."""
    W = [d(a) for a in A]
    V = [1.0 if k % 5 == 0 else 0.0 for k in range(16)]
    for _ in range(sweeps):
        for p in range(3):
            for q in range(p + 1, 4):
                al = W[p] * W[p] + W[4 + p] * W[4 + p] + W[8 + p] * W[8 + p] + W[12 + p] * W[12 + p]
                be = W[q] * W[q] + W[4 + q] * W[4 + q] + W[8 + q] * W[8 + q] + W[12 + q] * W[12 + q]
                ga = W[p] * W[q] + W[4 + p] * W[4 + q] + W[8 + p] * W[8 + q] + W[12 + p] * W[12 + q]
                if abs(ga) <= ORTH_TOL * _sqrt(al * be):
                    continue
                zeta = _div(be - al, ga + ga)
                t = _div(1.0, abs(zeta) + _sqrt(zeta * zeta + 1.0))
                if zeta < 0:
                    t = -t
                c = _div(1.0, _sqrt(t * t + 1.0))
                s = t * c
                for r in range(4):
                    wp, wq = W[4 * r + p], W[4 * r + q]
                    W[4 * r + p] = c * wp - s * wq
                    W[4 * r + q] = s * wp + c * wq
                    vp, vq = V[4 * r + p], V[4 * r + q]
                    V[4 * r + p] = c * vp - s * vq
                    V[4 * r + q] = s * vp + c * vq
    n2 = [W[k] * W[k] + W[4 + k] * W[4 + k] + W[8 + k] * W[8 + k] + W[12 + k] * W[12 + k] for k in range(4)]
    m, best = 0, n2[0]
    for k in range(1, 4):
        if n2[k] <= best:
            best, m = n2[k], k
    v = [V[4 * r + m] for r in range(4)]
    return np.array([f(x) for x in v], f32), v


def build_A(T1, cam1, T2, cam2, kp1, kp2):
    """xn1, xn2 (:461-462) and the 4x4 A (:500-504) as float32 arrays."""
    with np.errstate(all="ignore"):
        xn1 = [(kp1[0] - cam1[2]) * cam1[4], (kp1[1] - cam1[3]) * cam1[5], f32(1.0)]
        xn2 = [(kp2[0] - cam2[2]) * cam2[4], (kp2[1] - cam2[3]) * cam2[5], f32(1.0)]
        A = np.zeros(16, f32)
        for j in range(4):
            A[j] = xn1[0] * T1[8 + j] - T1[j]
            A[4 + j] = xn1[1] * T1[8 + j] - T1[4 + j]
            A[8 + j] = xn2[0] * T2[8 + j] - T2[j]
            A[12 + j] = xn2[1] * T2[8 + j] - T2[4 + j]
    return xn1, xn2, A


def divide_w(x4):
    """x3D.rowRange(0,3) / x3D.at<float>(3): a float scale by (float)(1 / w)."""
    with np.errstate(all="ignore"):
        inv = f(_div(1.0, d(x4[3])))
        return np.array([x4[0] * inv, x4[1] * inv, x4[2] * inv], f32)


def _row_dot(T, r, X):
    return f(_dot3(T[4 * r:4 * r + 3], X) + d(T[4 * r + 3]))


def _reproj2(T, cam, X, z, kp):
    with np.errstate(all="ignore"):
        x, y = _row_dot(T, 0, X), _row_dot(T, 1, X)
        invz = f(_div(1.0, d(z)))
        u = cam[0] * x * invz + cam[2]
        v = cam[1] * y * invz + cam[3]
        ex, ey = u - kp[0], v - kp[1]
        return ex * ex + ey * ey


def triangulate_match(T1, cam1, T2, cam2, ratio_factor, kp1, kp2, sig1, sig2, sf1, sf2, sweeps=SWEEPS):
    """(reason, x3D float32 [3], passed_parallax A or None)."""
    T1, T2 = np.asarray(T1, f32).reshape(12), np.asarray(T2, f32).reshape(12)
    zero = np.zeros(3, f32)
    with np.errstate(all="ignore"):
        xn1, xn2, A = build_A(T1, cam1, T2, cam2, kp1, kp2)
        ray1 = [T1[i] * xn1[0] + T1[4 + i] * xn1[1] + T1[8 + i] * xn1[2] for i in range(3)]
        ray2 = [T2[i] * xn2[0] + T2[4 + i] * xn2[1] + T2[8 + i] * xn2[2] for i in range(3)]
        cosr = f(_div(_dot3(ray1, ray2), _norm3(ray1) * _norm3(ray2)))
        cosst = cosr + f32(1.0)
        if not (cosr < cosst and cosr > 0 and d(cosr) < 0.9998):
            return 1, zero, None
        x4, _ = null_vector(A, sweeps)
        if x4[3] == 0:
            return 2, zero, A
        X = divide_w(x4)
        z1 = _row_dot(T1, 2, X)
        if not (z1 > 0):
            return 3, X, A
        z2 = _row_dot(T2, 2, X)
        if not (z2 > 0):
            return 4, X, A
        e1 = _reproj2(T1, cam1, X, z1, kp1)
        if not (d(e1) <= 5.991 * d(sig1)):
            return 5, X, A
        e2 = _reproj2(T2, cam2, X, z2, kp2)
        if not (d(e2) <= 5.991 * d(sig2)):
            return 6, X, A
        Ow1, Ow2 = center(T1), center(T2)
        dist1, dist2 = f(_norm3(X - Ow1)), f(_norm3(X - Ow2))
        if dist1 == 0 or dist2 == 0:
            return 7, X, A
        ratio_dist = dist2 / dist1
        ratio_octave = f32(sf1) / f32(sf2)
        rf = f32(ratio_factor)
        if not (ratio_dist * rf >= ratio_octave and ratio_dist <= ratio_octave * rf):
            return 8, X, A
        return 0, X, A


def triangulate_pairs(pairs, sweeps=SWEEPS, keep_A=False):
    """The definition over a list of sqrtlm.mappoint.TriPair: x3d, reason, n_new, off (and the A of every match
    that passed the parallax test)."""
    off = np.concatenate([[0], np.cumsum([len(p.matches) for p in pairs])]).astype(np.int64)
    n = int(off[-1])
    x3d, reason, n_new = np.zeros((n, 3), f32), np.zeros(n, np.uint8), np.zeros(len(pairs), np.int32)
    As = [None] * n
    for k, p in enumerate(pairs):
        a, b = p.kf1, p.kf2
        for j, (i1, i2) in enumerate(p.matches):
            k1, k2 = a.mvKeysUn[i1], b.mvKeysUn[i2]
            r, X, A = triangulate_match(
                a.Tcw, a.cam, b.Tcw, b.cam, p.ratio_factor, (k1["x"], k1["y"]), (k2["x"], k2["y"]),
                a.mvLevelSigma2[k1["octave"]], b.mvLevelSigma2[k2["octave"]], a.mvScaleFactors[k1["octave"]],
                b.mvScaleFactors[k2["octave"]], sweeps)
            i = int(off[k]) + j
            x3d[i], reason[i], As[i] = X, r, A
            n_new[k] += r == 0
    out = dict(x3d=x3d, reason=reason, n_new=n_new, off=off)
    if keep_A:
        out["A"] = As
    return out


_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming_matrix(desc):
    """[N][N] Hamming distances over 256 bits of the N descriptors [N][32]."""
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    return _POP[desc[:, None, :] ^ desc[None, :, :]].sum(-1).astype(np.int32)


def distinctive(desc):
    """(BestIdx, BestMedian) of ComputeDistinctiveDescriptors: the median of row i is the element at index
    (size_t)(0.5 * (N - 1)) of the ascending row (the self-distance 0 included); strict <. N = 0: (-1, INT_MAX)."""
    N = len(desc)
    if N == 0:
        return -1, 2**31 - 1
    D = np.sort(hamming_matrix(desc), axis=1, kind="stable")
    med = D[:, int(0.5 * (N - 1))]
    best = int(np.argmin(med))  # the first of equals
    return best, int(med[best])


def distinctive_literal(desc):
    """A literal transcription of MapPoint.cc:437-475 with sorted()."""
    N = len(desc)
    Distances = [[0.0] * N for _ in range(N)]
    for i in range(N):
        Distances[i][i] = 0
        for j in range(i + 1, N):
            distij = int(_POP[np.asarray(desc[i], np.uint8) ^ np.asarray(desc[j], np.uint8)].sum())
            Distances[i][j] = float(distij)
            Distances[j][i] = float(distij)
    BestMedian, BestIdx = 2**31 - 1, 0
    for i in range(N):
        vDists = sorted(int(v) for v in Distances[i])
        median = vDists[int(0.5 * (N - 1))]
        if median < BestMedian:
            BestMedian, BestIdx = median, i
    return BestIdx, BestMedian


def normal_depth(pos, centers, ref_center, level_scale, max_scale):
    """(normal [3], max_dist, min_dist) of UpdateNormalAndDepth over the centres in list order; zeros for none."""
    pos, centers = np.asarray(pos, f32), np.asarray(centers, f32).reshape(-1, 3)
    n = len(centers)
    if n == 0:
        return np.zeros(3, f32), f32(0), f32(0)
    with np.errstate(all="ignore"):
        acc = np.zeros(3, f32)
        for O in centers:
            di = pos - O
            inv = f(_div(1.0, _norm3(di)))
            for i in range(3):
                acc[i] = acc[i] + di[i] * inv
        pc = pos - np.asarray(ref_center, f32)
        dist = f(_norm3(pc))
        mx = dist * f32(level_scale)
        mn = mx / f32(max_scale)
        invn = f(1.0 / float(n))
        return np.array([acc[i] * invn for i in range(3)], f32), mx, mn


def map_points_update(batch):
    """The definition over a sqrtlm.mappoint.MapPointBatch."""
    n = batch.n_pt
    out = {}
    if batch.obs_desc is not None:
        out["best_idx"], out["best_median"] = np.zeros(n, np.int32), np.zeros(n, np.int32)
    if batch.obs_center is not None:
        out["normal"], out["max_dist"], out["min_dist"] = (np.zeros((n, 3), f32), np.zeros(n, f32), np.zeros(n, f32))
    for j in range(n):
        lo, hi = int(batch.obs_off[j]), int(batch.obs_off[j + 1])
        if batch.obs_desc is not None:
            out["best_idx"][j], out["best_median"][j] = distinctive(batch.obs_desc[lo:hi])
        if batch.obs_center is not None:
            out["normal"][j], out["max_dist"][j], out["min_dist"][j] = normal_depth(
                batch.pos[j], batch.obs_center[lo:hi], batch.ref_center[j], batch.level_scale[j], batch.max_scale[j])
    return out
