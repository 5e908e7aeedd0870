"""numpy definition of the batched Sim3 RANSAC (sqlm_sim3_ransac): our own
restatement of the semantics of the reference's Sim3Solver
(src/algorithm/Sim3Solver.cc), not its text.

Three pieces:

* ``closed_form``: Horn's closed form on three pairs (ComputeSim3, :319-458),
  once under the float32 rule the library follows (``LD = False``) and once in
  longdouble from the same float inputs (``LD = True``). One code path: every
  site where the source stores a float goes through ``st`` (round to float32,
  or nothing in longdouble), every operation is done in the work type ``W``
  (float64, or longdouble). A float32 operation written out in the source is
  ``st(a op b)`` with a, b widened to float64: for + - * / a double has more
  than 2 * 24 + 2 bits, so rounding its result to float32 is the float32
  operation itself. Where the source hands arithmetic to OpenCV (reduce,
  matrix products, scaling by a scalar, dot, norm) products and sums accumulate
  in ``W`` in index order and are rounded once per stored element.
  Step 4 is the deliberate deviation: the eigenvector of the largest eigenvalue
  of the float N by cyclic Jacobi in ``W`` (SWEEPS sweeps, rotation order
  PAIRS, no data-dependent termination), normalised with w >= 0; R12 is that
  unit quaternion's rotation matrix, computed in ``W`` and rounded once.
* ``check_inliers``: CheckInliers (:462-490) with Project / FromCameraToImage
  (:515-562) in literal float32, no FMA.
* ``LiteralSolver``: the class, statefully: array swap-remove of the draws,
  iterate, best bookkeeping (:207-300).

Everything is vectorised over hypotheses (leading axis).
"""
from __future__ import annotations

import math

import numpy as np

F32 = np.float32
F64 = np.float64
LDT = np.longdouble
SWEEPS = 8                                                  # the library's fixed sweep count
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))    # and rotation order


# ---- draws -> pair indices --------------------------------------------------------
def swap_remove_literal(n: int, draws) -> list:
    """vAvailableIndices = all; three times: idx = v[r]; v[r] = v.back(); v.pop_back() (:236-256)."""
    v = list(range(n))
    out = []
    for r in draws:
        r = int(r)
        assert 0 <= r < len(v)
        out.append(v[r])
        v[r] = v[-1]
        v.pop()
    return out


def swap_remove_closed(n, draws):
    """The same mapping without the array, vectorised: draws (..., 3) -> idx (..., 3)."""
    d = np.asarray(draws, np.int64)
    r0, r1, r2 = d[..., 0], d[..., 1], d[..., 2]
    n = np.asarray(n, np.int64)
    i0 = r0
    i1 = np.where(r1 == r0, n - 1, r1)
    back1 = np.where(r0 == n - 2, n - 1, n - 2)   # what the second removal moves into slot r1
    i2 = np.where(r2 == r1, back1, np.where(r2 == r0, n - 1, r2))
    return np.stack([i0, i1, i2], axis=-1)


def max_its(n_pair: int, probability: float = 0.99, min_inliers: int = 6, max_iterations: int = 300) -> int:
    """mRansacMaxIts after SetRansacParameters (:145-203); 0 when iterate() gives up at once (:214-218)."""
    if n_pair < min_inliers:
        return 0
    if min_inliers == n_pair:
        n_it = 1.0
    else:
        eps = float(F32(F32(min_inliers) / F32(n_pair)))
        with np.errstate(divide="ignore", invalid="ignore"):
            n_it = float(np.ceil(np.log(F64(1.0 - probability)) / np.log(F64(1.0) - np.power(F64(eps), 3.0))))
    if math.isnan(n_it):
        n_it = float(max_iterations)
    n_it = min(n_it, float(max_iterations))   # clamped in double before the conversion to int
    return int(max(1.0, n_it))


# ---- closed form ------------------------------------------------------------------
def _modes(ld: bool):
    if ld:
        return LDT, (lambda x: np.asarray(x, LDT))
    return F64, (lambda x: np.asarray(x, F64).astype(F32).astype(F64))


def jacobi_top(N, W, sweeps):
    """Unit eigenvector (w, x, y, z), w >= 0, of the largest eigenvalue of the
    symmetric (H,4,4) N: cyclic Jacobi in W."""
    A = np.array(N, W)
    H = A.shape[0]
    V = np.zeros((H, 4, 4), W)
    for k in range(4):
        V[:, k, k] = 1
    one = W(1)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p, q in PAIRS:
                apq = A[:, p, q].copy()
                rot = apq != 0
                theta = (A[:, q, q] - A[:, p, p]) / (apq + apq)
                at = np.abs(theta)
                t = one / (at + np.sqrt(theta * theta + one))
                t = np.where(theta < 0, -t, t)
                c = one / np.sqrt(t * t + one)
                s = t * c
                t, c, s = np.where(rot, t, 0), np.where(rot, c, one), np.where(rot, s, 0)
                app, aqq = A[:, p, p] - t * apq, A[:, q, q] + t * apq
                for r in range(4):
                    if r != p and r != q:
                        arp, arq = A[:, r, p].copy(), A[:, r, q].copy()
                        n_p, n_q = c * arp - s * arq, s * arp + c * arq
                        A[:, r, p] = A[:, p, r] = np.where(rot, n_p, arp)
                        A[:, r, q] = A[:, q, r] = np.where(rot, n_q, arq)
                A[:, p, p], A[:, q, q] = np.where(rot, app, A[:, p, p]), np.where(rot, aqq, A[:, q, q])
                A[:, p, q] = A[:, q, p] = np.where(rot, 0, apq)
                for r in range(4):
                    vrp, vrq = V[:, r, p].copy(), V[:, r, q].copy()
                    V[:, r, p] = np.where(rot, c * vrp - s * vrq, vrp)
                    V[:, r, q] = np.where(rot, s * vrp + c * vrq, vrq)
        best = np.zeros(H, np.int64)
        lam = A[:, 0, 0].copy()
        for k in range(1, 4):
            gt = A[:, k, k] > lam
            best = np.where(gt, k, best)
            lam = np.where(gt, A[:, k, k], lam)
        qv = V[np.arange(H), :, best]
        nrm = np.sqrt(((qv[:, 0] * qv[:, 0] + qv[:, 1] * qv[:, 1]) + qv[:, 2] * qv[:, 2]) + qv[:, 3] * qv[:, 3])
        qv = qv / nrm[:, None]
        qv = np.where((qv[:, 0] < 0)[:, None], -qv, qv)
    return qv


def quat_to_R(qv, W):
    w, x, y, z = (qv[:, k] for k in range(4))
    two = W(2)
    one = W(1)
    R = np.empty((qv.shape[0], 3, 3), W)
    R[:, 0, 0] = one - two * (y * y + z * z)
    R[:, 0, 1] = two * (x * y - w * z)
    R[:, 0, 2] = two * (x * z + w * y)
    R[:, 1, 0] = two * (x * y + w * z)
    R[:, 1, 1] = one - two * (x * x + z * z)
    R[:, 1, 2] = two * (y * z - w * x)
    R[:, 2, 0] = two * (x * z - w * y)
    R[:, 2, 1] = two * (y * z + w * x)
    R[:, 2, 2] = one - two * (x * x + y * y)
    return R


def _dot3(a, b, axis_a, axis_b):
    """sum_k a[k] * b[k], k in index order, in the arrays' type."""
    ta = [np.take(a, k, axis=axis_a) for k in range(3)]
    tb = [np.take(b, k, axis=axis_b) for k in range(3)]
    return (ta[0] * tb[0] + ta[1] * tb[1]) + ta[2] * tb[2]


def closed_form(P1, P2, fix_scale, ld: bool = False, sweeps: int | None = None):
    """P1, P2 (H,3,3): column i is point i of camera 1 / 2 (float32 values).
    Returns dict R (H,3,3), t (H,3), s (H,), T12, T21 (H,4,4): float32 arrays
    (ld False) or longdouble arrays (ld True)."""
    W, st = _modes(ld)
    sweeps = sweeps if sweeps is not None else (2 * SWEEPS if ld else SWEEPS)
    P1 = np.asarray(P1, F32).astype(W).reshape(-1, 3, 3)
    P2 = np.asarray(P2, F32).astype(W).reshape(-1, 3, 3)
    H = P1.shape[0]
    fix = np.broadcast_to(np.asarray(fix_scale, bool), (H,))
    third = W(1) / W(3)
    with np.errstate(all="ignore"):
        def centroid(P):
            C = st((P[:, :, 0] + P[:, :, 1]) + P[:, :, 2])      # reduce(SUM): double sum, stored float
            C = st(C * third)                                   # C / P.cols: a scaling by 1/3
            return st(P - C[:, :, None]), C                     # float subtraction per column
        Pr1, O1 = centroid(P1)
        Pr2, O2 = centroid(P2)
        M = np.empty((H, 3, 3), W)                              # M = Pr2 * Pr1^T
        for i in range(3):
            for j in range(3):
                M[:, i, j] = st(_dot3(Pr2[:, i, :], Pr1[:, j, :], 1, 1))
        m = lambda i, j: M[:, i, j]
        # float expressions written out in the source, left to right
        N11 = st(st(m(0, 0) + m(1, 1)) + m(2, 2))
        N12 = st(m(1, 2) - m(2, 1))
        N13 = st(m(2, 0) - m(0, 2))
        N14 = st(m(0, 1) - m(1, 0))
        N22 = st(st(m(0, 0) - m(1, 1)) - m(2, 2))
        N23 = st(m(0, 1) + m(1, 0))
        N24 = st(m(2, 0) + m(0, 2))
        N33 = st(st(-m(0, 0) + m(1, 1)) - m(2, 2))
        N34 = st(m(1, 2) + m(2, 1))
        N44 = st(st(-m(0, 0) - m(1, 1)) + m(2, 2))
        N = np.empty((H, 4, 4), W)
        rows = ((N11, N12, N13, N14), (N12, N22, N23, N24), (N13, N23, N33, N34), (N14, N24, N34, N44))
        for i in range(4):
            for j in range(4):
                N[:, i, j] = rows[i][j]
        R = st(quat_to_R(jacobi_top(N, W, sweeps), W))
        P3 = np.empty((H, 3, 3), W)                             # P3 = R * Pr2
        for i in range(3):
            for j in range(3):
                P3[:, i, j] = st(_dot3(R[:, i, :], Pr2[:, :, j], 1, 1))
        nom = np.zeros(H, W)                                    # Pr1.dot(P3): a double
        den = np.zeros(H, W)                                    # sum of the float squares, a double
        for i in range(3):
            for j in range(3):
                nom = nom + Pr1[:, i, j] * P3[:, i, j]
                den = den + st(P3[:, i, j] * P3[:, i, j])
        s = np.where(fix, W(1), st(nom / den))                  # ms12i is a float
        t = np.empty((H, 3), W)                                 # O1 - s * R * O2, rounded once
        for i in range(3):
            t[:, i] = st(O1[:, i] - s * _dot3(R[:, i, :], O2, 1, 1))
        sR = st(s[:, None, None] * R)
        inv_s = W(1) / s                                        # 1.0 / ms12i, a double
        sRinv = st(inv_s[:, None, None] * np.transpose(R, (0, 2, 1)))
        tinv = np.empty((H, 3), W)
        for i in range(3):
            tinv[:, i] = st(-_dot3(sRinv[:, i, :], t, 1, 1))
    T12 = np.zeros((H, 4, 4), W)
    T21 = np.zeros((H, 4, 4), W)
    T12[:, 3, 3] = T21[:, 3, 3] = 1
    T12[:, :3, :3], T12[:, :3, 3] = sR, t
    T21[:, :3, :3], T21[:, :3, 3] = sRinv, tinv
    out = dict(R=R, t=t, s=s, T12=T12, T21=T21)
    if not ld:
        out = {k: v.astype(F32) for k, v in out.items()}
    return out


def inverse_f32(R, t, s):
    """T21 (H,4,4) float32 from float32 R12, t12, s12, as step 8.2 computes it."""
    R = np.asarray(R, F32).astype(F64).reshape(-1, 3, 3)
    t = np.asarray(t, F32).astype(F64).reshape(-1, 3)
    s = np.asarray(s, F32).astype(F64).reshape(-1)
    with np.errstate(all="ignore"):
        sRinv = ((1.0 / s)[:, None, None] * np.transpose(R, (0, 2, 1))).astype(F32).astype(F64)
        tinv = np.stack([-_dot3(sRinv[:, i, :], t, 1, 1) for i in range(3)], axis=1).astype(F32)
    T = np.zeros((R.shape[0], 4, 4), F32)
    T[:, 3, 3] = 1
    T[:, :3, :3], T[:, :3, 3] = sRinv.astype(F32), tinv
    return T


# ---- inlier check -----------------------------------------------------------------
def _image(P, K):
    """invz = 1 / z; x = X invz; y = Y invz; (fx x + cx, fy y + cy): float32, no FMA."""
    P = P.astype(F32)
    K = np.asarray(K, F32)
    with np.errstate(all="ignore"):
        invz = F32(1) / P[..., 2]
        x, y = P[..., 0] * invz, P[..., 1] * invz
        return np.stack([K[0] * x + K[2], K[1] * y + K[3]], axis=-1)


def _project(X, T, K):
    """Rcw * X + tcw: a float gemm (double accumulation, one rounding), then _image."""
    X = np.asarray(X, F32).astype(F64)                 # (n,3)
    T = np.asarray(T, F32).astype(F64)                 # (H,4,4)
    with np.errstate(all="ignore"):
        Pc = np.stack([((T[:, None, i, 0] * X[None, :, 0] + T[:, None, i, 1] * X[None, :, 1])
                        + T[:, None, i, 2] * X[None, :, 2]) + T[:, None, i, 3] for i in range(3)], axis=-1)
    return _image(Pc.astype(F32), K)                   # (H,n,2)


def check_inliers(T12, T21, X1c, X2c, K1, K2, max_err1, max_err2):
    """(mask (H,n) bool, count (H,)) of CheckInliers for transforms T12/T21 (H,4,4) float32."""
    X1c, X2c = np.asarray(X1c, F32).reshape(-1, 3), np.asarray(X2c, F32).reshape(-1, 3)
    T12 = np.asarray(T12, F32).reshape(-1, 4, 4)
    T21 = np.asarray(T21, F32).reshape(-1, 4, 4)
    P1im1, P2im2 = _image(X1c, K1), _image(X2c, K2)    # the targets: the map points' own projections
    P2im1, P1im2 = _project(X2c, T12, K1), _project(X1c, T21, K2)
    with np.errstate(all="ignore"):
        d1 = (P1im1[None] - P2im1).astype(F64)
        d2 = (P1im2 - P2im2[None]).astype(F64)
        e1 = (d1[..., 0] * d1[..., 0] + d1[..., 1] * d1[..., 1]).astype(F32)   # (float)dist.dot(dist)
        e2 = (d2[..., 0] * d2[..., 0] + d2[..., 1] * d2[..., 1]).astype(F32)
        m1 = np.asarray(max_err1, np.int64).astype(F32)                          # size_t -> float
        m2 = np.asarray(max_err2, np.int64).astype(F32)
        mask = (e1 < m1[None]) & (e2 < m2[None])
    return mask, mask.sum(axis=1).astype(np.int32)


def gather(X1c, X2c, idx):
    """P1, P2 (H,3,3) with the chosen points as columns."""
    X1c, X2c = np.asarray(X1c, F32).reshape(-1, 3), np.asarray(X2c, F32).reshape(-1, 3)
    idx = np.asarray(idx, np.int64).reshape(-1, 3)
    return np.transpose(X1c[idx], (0, 2, 1)), np.transpose(X2c[idx], (0, 2, 1))


def hypotheses(X1c, X2c, K1, K2, fix_scale, max_err1, max_err2, draws):
    """The float32 definition of every hypothesis of one problem: idx, R, t, s, T12, T21, mask, count."""
    n = np.asarray(X1c).reshape(-1, 3).shape[0]
    draws = np.asarray(draws, np.int64).reshape(-1, 3)
    if draws.shape[0] == 0:
        z = np.zeros
        return dict(idx=z((0, 3), np.int64), R=z((0, 3, 3), F32), t=z((0, 3), F32), s=z(0, F32),
                    T12=z((0, 4, 4), F32), T21=z((0, 4, 4), F32), mask=z((0, n), bool), count=z(0, np.int32))
    idx = swap_remove_closed(n, draws)
    P1, P2 = gather(X1c, X2c, idx)
    out = closed_form(P1, P2, fix_scale)
    out["idx"] = idx
    out["mask"], out["count"] = check_inliers(out["T12"], out["T21"], X1c, X2c, K1, K2, max_err1, max_err2)
    return out


# ---- sequential bookkeeping -------------------------------------------------------
def scan(counts, min_inliers: int):
    """flags per hypothesis (bit 0 updates the best, bit 1 returns), first returning index or -1, final best or -1."""
    best, flags, first, ibest = 0, [], -1, -1
    for h, c in enumerate(int(c) for c in counts):
        f = 0
        if c >= best:
            best, ibest, f = c, h, 1
            if c > min_inliers:
                f = 3
                if first < 0:
                    first = h
        flags.append(f)
    return np.array(flags, np.uint8), first, ibest


class LiteralSolver:
    """The reference's class, statefully, on given per-hypothesis results.

    ``hyp``: dict with T12 (H,4,4), R, t, s, mask (H,N), count (H,) in draw
    order (what ComputeSim3 + CheckInliers give for hypothesis h); ``n_pair``
    is N, ``indices1`` mvnIndices1 and ``n1`` mN1. SetRansacParameters has been
    applied by the caller: ``max_its`` is mRansacMaxIts."""

    def __init__(self, hyp, n_pair, min_inliers, max_its_, indices1=None, n1=None):
        self.h, self.N, self.min_inliers, self.max_its = hyp, int(n_pair), int(min_inliers), int(max_its_)
        self.indices1 = np.arange(self.N) if indices1 is None else np.asarray(indices1, np.int64)
        self.n1 = self.N if n1 is None else int(n1)
        self.its = 0
        self.best_inliers = 0
        self.best = None      # index of the hypothesis held in mBest*

    def iterate(self, n_iterations):
        """(T12 or None, bNoMore, vbInliers (mN1,), nInliers)"""
        vb = np.zeros(self.n1, bool)
        if self.N < self.min_inliers:
            return None, True, vb, 0
        cur = 0
        while self.its < self.max_its and cur < n_iterations:
            cur += 1
            h = self.its
            self.its += 1
            c = int(self.h["count"][h])
            if c >= self.best_inliers:
                self.best_inliers, self.best = c, h
                if c > self.min_inliers:
                    vb[self.indices1[np.asarray(self.h["mask"][h], bool)]] = True
                    return np.array(self.h["T12"][h]), False, vb, c
        return None, self.its >= self.max_its, vb, 0

    def find(self):
        T, _, vb, n = self.iterate(self.max_its)
        return T, vb, n
