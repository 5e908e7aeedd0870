"""The library's PnP RANSAC hypothesis and refine (csrc/pnp_ransac_dev.h)
restated in numpy, operation by operation, and the reference's sequential
bookkeeping (PnPsolver::iterate / Refine / find, src/algorithm/PnPsolver.cc
:231-426) as a literal, stateful solver.

Every quantity is an array over the hypotheses (leading axis H); nothing is
vectorised over the terms of a sum, so each element goes through the scalar
code's IEEE operations in the scalar code's order: the results are the bits the
C++ text produces when built without contraction. A sum over the points follows
the one order of the shared text: "lane" l of 64 adds the terms of points l,
l+64, ... to +0.0, then the partials of lanes 0 .. min(n, 64)-1 are added to
+0.0 in lane order.

``downstream`` (everything after the 12x12 eigenvectors: L, rho, the three
beta vectors, Gauss-Newton, R, t and the reprojection errors) is written once
for any dtype: the float64 definition calls it, and so does the longdouble
restatement the tests bound the definition with.
"""
from __future__ import annotations

import numpy as np

SWEEPS3, SWEEPS12, SWEEPSR = 6, 12, 6
RANK_TOL, ORTH_TOL, POLAR_TOL = 1e-6, 1e-15, 1e-12


def indices(n, draws):
    """pnp_indices: the pair indices of (H, 4) raw draws, the closed form of the swap-remove."""
    r = np.asarray(draws, np.int64).reshape(-1, 4)
    r0, r1, r2, r3 = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
    i1 = np.where(r1 == r0, n - 1, r1)
    b1 = np.where(r0 == n - 2, n - 1, n - 2)
    i2 = np.where(r2 == r1, b1, np.where(r2 == r0, n - 1, r2))
    s = n - 3
    b2 = np.where(s == r1, b1, np.where(s == r0, n - 1, s))
    i3 = np.where(r3 == r2, b2, np.where(r3 == r1, b1, np.where(r3 == r0, n - 1, r3)))
    return np.stack([r0, i1, i2, i3], axis=1).astype(np.int32)


def indices_literal(n, draws4):
    """The same by the reference's vector operations (:281-297)."""
    avail, out = list(range(n)), []
    for r in draws4:
        out.append(avail[r])
        avail[r] = avail[-1]
        avail.pop()
    return out


def _psum(n, term, K, zero):
    tot = [zero.copy() for _ in range(K)]
    for l in range(min(n, 64)):
        p = [zero.copy() for _ in range(K)]
        for i in range(l, n, 64):
            t = term(i)
            p = [p[k] + t[k] for k in range(K)]
        tot = [tot[k] + p[k] for k in range(K)]
    return tot


def jacobi(A, sweeps):
    """pnp_detail::jacobi on (H, n, n): (diagonal (H, n), V (H, n, n))."""
    A = A.copy()
    H, n = A.shape[0], A.shape[1]
    V = np.zeros_like(A)
    V[:, np.arange(n), np.arange(n)] = 1.0
    for _ in range(sweeps):
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = A[:, p, q].copy()
                act = apq != 0.0
                if not act.any():
                    continue
                theta = (A[:, q, q] - A[:, p, p]) / (apq + apq)
                t = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                t = np.where(theta < 0, -t, t)
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                app, aqq = A[:, p, p] - t * apq, A[:, q, q] + t * apq
                for r in range(n):
                    if r == p or r == q:
                        continue
                    arp, arq = A[:, r, p].copy(), A[:, r, q].copy()
                    np_, nq_ = c * arp - s * arq, s * arp + c * arq
                    A[:, r, p] = A[:, p, r] = np.where(act, np_, arp)
                    A[:, r, q] = A[:, q, r] = np.where(act, nq_, arq)
                A[:, p, p] = np.where(act, app, A[:, p, p])
                A[:, q, q] = np.where(act, aqq, A[:, q, q])
                A[:, p, q] = A[:, q, p] = np.where(act, 0.0, apq)
                vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
                V[:, :, p] = np.where(act[:, None], c[:, None] * vp - s[:, None] * vq, vp)
                V[:, :, q] = np.where(act[:, None], s[:, None] * vp + c[:, None] * vq, vq)
    return A[:, np.arange(n), np.arange(n)], V


def sorted_rows(d, V):
    H, n = d.shape
    ut, ds = np.zeros_like(V), np.zeros_like(d)
    hh = np.arange(H)
    for k in range(n):
        ak = d[:, k]
        rank = np.zeros(H, np.int64)
        for j in range(n):
            aj = d[:, j]
            rank += ((aj > ak) | ((aj == ak) & (j < k))).astype(np.int64)
        ds[hh, rank] = ak
        ut[hh, rank, :] = V[:, :, k]
    return ut, ds


def qr_solve(A, b):
    """pnp_detail::qr_solve on (H, nr, nc), (H, nr): X (H, nc), all zeros where eta == 0 ended it."""
    A, b = A.copy(), b.copy()
    H, nr, nc = A.shape
    dead = np.zeros(H, bool)
    A1, A2 = np.zeros((H, nc), A.dtype), np.zeros((H, nc), A.dtype)
    for k in range(nc):
        eta = np.abs(A[:, k, k])
        for i in range(k + 1, nr):
            elt = np.abs(A[:, i - 1, k])
            eta = np.where(eta < elt, elt, eta)
        dead |= eta == 0
        inv_eta = 1.0 / eta
        s = np.zeros(H, A.dtype)
        for i in range(k, nr):
            A[:, i, k] = A[:, i, k] * inv_eta
            s = s + A[:, i, k] * A[:, i, k]
        sigma = np.sqrt(s)
        sigma = np.where(A[:, k, k] < 0, -sigma, sigma)
        A[:, k, k] = A[:, k, k] + sigma
        A1[:, k] = sigma * A[:, k, k]
        A2[:, k] = -eta * sigma
        for j in range(k + 1, nc):
            s2 = np.zeros(H, A.dtype)
            for i in range(k, nr):
                s2 = s2 + A[:, i, k] * A[:, i, j]
            tau = s2 / A1[:, k]
            for i in range(k, nr):
                A[:, i, j] = A[:, i, j] - tau * A[:, i, k]
    for j in range(nc):
        tau = np.zeros(H, A.dtype)
        for i in range(j, nr):
            tau = tau + A[:, i, j] * b[:, i]
        tau = tau / A1[:, j]
        for i in range(j, nr):
            b[:, i] = b[:, i] - tau * A[:, i, j]
    X = np.zeros((H, nc), A.dtype)
    X[:, nc - 1] = b[:, nc - 1] / A2[:, nc - 1]
    for i in range(nc - 2, -1, -1):
        s = np.zeros(H, A.dtype)
        for j in range(i + 1, nc):
            s = s + A[:, i, j] * X[:, j]
        X[:, i] = (b[:, i] - s) / A2[:, i]
    X[dead] = 0.0
    return X


def polar(abt, sweeps):
    """pnp_detail::polar on (H, 3, 3): R = U V^T by one-sided Jacobi."""
    W = abt.copy()
    H = W.shape[0]
    Vr = np.zeros_like(W)
    Vr[:, [0, 1, 2], [0, 1, 2]] = 1.0
    for _ in range(sweeps):
        for p, q in ((0, 1), (0, 2), (1, 2)):
            al = W[:, 0, p] * W[:, 0, p] + W[:, 1, p] * W[:, 1, p] + W[:, 2, p] * W[:, 2, p]
            be = W[:, 0, q] * W[:, 0, q] + W[:, 1, q] * W[:, 1, q] + W[:, 2, q] * W[:, 2, q]
            ga = W[:, 0, p] * W[:, 0, q] + W[:, 1, p] * W[:, 1, q] + W[:, 2, p] * W[:, 2, q]
            act = (~(np.abs(ga) <= ORTH_TOL * np.sqrt(al * be)))[:, None]
            zeta = (be - al) / (ga + ga)
            t = 1.0 / (np.abs(zeta) + np.sqrt(zeta * zeta + 1.0))
            t = np.where(zeta < 0, -t, t)
            c = 1.0 / np.sqrt(t * t + 1.0)
            s = (t * c)[:, None]
            c = c[:, None]
            for M in (W, Vr):
                mp, mq = M[:, :, p].copy(), M[:, :, q].copy()
                M[:, :, p] = np.where(act, c * mp - s * mq, mp)
                M[:, :, q] = np.where(act, s * mp + c * mq, mq)
    sg = np.sqrt(W[:, 0, :] * W[:, 0, :] + W[:, 1, :] * W[:, 1, :] + W[:, 2, :] * W[:, 2, :])
    s0, s1, s2 = sg[:, 0], sg[:, 1], sg[:, 2]
    m = np.where(s1 < s0, np.where(s2 < s1, 2, 1), np.where(s2 < s0, 2, 0))
    smax = np.where(s0 > s1, np.where(s0 > s2, s0, s2), np.where(s1 > s2, s1, s2))
    smin = np.where(m == 0, s0, np.where(m == 1, s1, s2))
    U = W / sg[:, None, :]
    fix = smin <= POLAR_TOL * smax
    for k in range(3):
        a, b = (k + 1) % 3, (k + 2) % 3
        cr = np.stack([U[:, 1, a] * U[:, 2, b] - U[:, 2, a] * U[:, 1, b],
                       U[:, 2, a] * U[:, 0, b] - U[:, 0, a] * U[:, 2, b],
                       U[:, 0, a] * U[:, 1, b] - U[:, 1, a] * U[:, 0, b]], axis=1)
        U[:, :, k] = np.where((fix & (m == k))[:, None], cr, U[:, :, k])
    R = np.zeros_like(W)
    for i in range(3):
        for j in range(3):
            R[:, i, j] = U[:, i, 0] * Vr[:, j, 0] + U[:, i, 1] * Vr[:, j, 1] + U[:, i, 2] * Vr[:, j, 2]
    return R


def _alphas(cws, cci, pw):
    d0, d1, d2 = pw[:, 0] - cws[:, 0, 0], pw[:, 1] - cws[:, 0, 1], pw[:, 2] - cws[:, 0, 2]
    a1 = cci[:, 0, 0] * d0 + cci[:, 0, 1] * d1 + cci[:, 0, 2] * d2
    a2 = cci[:, 1, 0] * d0 + cci[:, 1, 1] * d1 + cci[:, 1, 2] * d2
    a3 = cci[:, 2, 0] * d0 + cci[:, 2, 1] * d1 + cci[:, 2, 2] * d2
    return [1.0 - a1 - a2 - a3, a1, a2, a3]


def _dot3(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def control_points(pw, sweeps3=SWEEPS3):
    """choose_control_points and the inverse of CC: cws (H, 4, 3), cci (H, 3, 3); pw (H, n, 3) float64."""
    H, n = pw.shape[:2]
    dn, z = float(n), np.zeros(H)
    c0 = _psum(n, lambda i: [pw[:, i, 0], pw[:, i, 1], pw[:, i, 2]], 3, z)
    cws = np.zeros((H, 4, 3))
    for j in range(3):
        cws[:, 0, j] = c0[j] / dn

    def gram(i):
        d = [pw[:, i, j] - cws[:, 0, j] for j in range(3)]
        return [d[0] * d[0], d[0] * d[1], d[0] * d[2], d[1] * d[1], d[1] * d[2], d[2] * d[2]]
    g = _psum(n, gram, 6, z)
    G = np.stack([np.stack([g[0], g[1], g[2]], 1), np.stack([g[1], g[3], g[4]], 1), np.stack([g[2], g[4], g[5]], 1)], 1)
    d, V = jacobi(G, sweeps3)
    uct, dc = sorted_rows(d, V)
    cci = np.zeros((H, 3, 3))
    kk = []
    for i in range(3):
        dci = np.where(dc[:, i] > 0.0, dc[:, i], 0.0)
        kk.append(np.sqrt(dci / dn))
        for j in range(3):
            cws[:, i + 1, j] = cws[:, 0, j] + kk[i] * uct[:, i, j]
    for i in range(3):
        ok = kk[i] > RANK_TOL * kk[0]
        for j in range(3):
            cci[:, i, j] = np.where(ok, uct[:, i, j] / kk[i], 0.0)
    return cws, cci


def mtm(pw, uv, K, cws, cci):
    H, n = pw.shape[:2]
    A = np.zeros((H, 12, 12))
    for r in range(12):
        def term(i):
            a = _alphas(cws, cci, pw[:, i])
            m1, m2 = [], []
            for j in range(4):
                m1 += [a[j] * K[0], np.zeros(H), a[j] * (K[2] - uv[:, i, 0])]
                m2 += [np.zeros(H), a[j] * K[1], a[j] * (K[3] - uv[:, i, 1])]
            return [m1[r] * m1[c] + m2[r] * m2[c] for c in range(12)]
        row = _psum(n, term, 12, np.zeros(H))
        for c in range(12):
            A[:, r, c] = row[c]
    return A


def downstream(ut, cws, cci, pw, uv, K, sweepsR=SWEEPSR):
    """Everything after the eigenvectors, in the dtype of ``ut``: betas (H, 3, 4), Rs (H, 3, 3, 3), ts (H, 3, 3),
    rep (H, 3), chosen (H,). The other arguments must have that dtype too."""
    dt = ut.dtype
    H, n = pw.shape[:2]
    dn, z = dt.type(n), np.zeros(H, dt)
    L, rho = np.zeros((H, 6, 10), dt), np.zeros((H, 6), dt)

    def dvdot(x, y, a, b):
        vx, vy = ut[:, 11 - x], ut[:, 11 - y]
        dx = [vx[:, 3 * a + k] - vx[:, 3 * b + k] for k in range(3)]
        dy = [vy[:, 3 * a + k] - vy[:, 3 * b + k] for k in range(3)]
        return dx[0] * dy[0] + dx[1] * dy[1] + dx[2] * dy[2]
    for i, (a, b) in enumerate(((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))):
        L[:, i, 0] = dvdot(0, 0, a, b)
        L[:, i, 1] = 2.0 * dvdot(0, 1, a, b)
        L[:, i, 2] = dvdot(1, 1, a, b)
        L[:, i, 3] = 2.0 * dvdot(0, 2, a, b)
        L[:, i, 4] = 2.0 * dvdot(1, 2, a, b)
        L[:, i, 5] = dvdot(2, 2, a, b)
        L[:, i, 6] = 2.0 * dvdot(0, 3, a, b)
        L[:, i, 7] = 2.0 * dvdot(1, 3, a, b)
        L[:, i, 8] = 2.0 * dvdot(2, 3, a, b)
        L[:, i, 9] = dvdot(3, 3, a, b)
        p1, p2 = cws[:, a], cws[:, b]
        rho[:, i] = ((p1[:, 0] - p2[:, 0]) * (p1[:, 0] - p2[:, 0]) + (p1[:, 1] - p2[:, 1]) * (p1[:, 1] - p2[:, 1])
                     + (p1[:, 2] - p2[:, 2]) * (p1[:, 2] - p2[:, 2]))

    def gauss_newton(be):
        be = be.copy()
        for _ in range(5):
            b0, b1, b2, b3 = be[:, 0], be[:, 1], be[:, 2], be[:, 3]
            A, rhs = np.zeros((H, 6, 4), dt), np.zeros((H, 6), dt)
            for i in range(6):
                l = [L[:, i, c] for c in range(10)]
                A[:, i, 0] = 2 * l[0] * b0 + l[1] * b1 + l[3] * b2 + l[6] * b3
                A[:, i, 1] = l[1] * b0 + 2 * l[2] * b1 + l[4] * b2 + l[7] * b3
                A[:, i, 2] = l[3] * b0 + l[4] * b1 + 2 * l[5] * b2 + l[8] * b3
                A[:, i, 3] = l[6] * b0 + l[7] * b1 + l[8] * b2 + 2 * l[9] * b3
                rhs[:, i] = rho[:, i] - (l[0] * b0 * b0 + l[1] * b0 * b1 + l[2] * b1 * b1 + l[3] * b0 * b2 +
                                         l[4] * b1 * b2 + l[5] * b2 * b2 + l[6] * b0 * b3 + l[7] * b1 * b3 +
                                         l[8] * b2 * b3 + l[9] * b3 * b3)
            be = be + qr_solve(A, rhs)
        return be

    betas = np.zeros((H, 3, 4), dt)
    b4 = qr_solve(L[:, :, [0, 1, 3, 6]], rho)
    neg = b4[:, 0] < 0
    be0 = np.where(neg, np.sqrt(-b4[:, 0]), np.sqrt(b4[:, 0]))
    sg = np.where(neg, -1.0, 1.0).astype(dt)
    betas[:, 0] = gauss_newton(np.stack([be0] + [sg * b4[:, k] / be0 for k in (1, 2, 3)], axis=1))
    for cand, cols in ((1, [0, 1, 2]), (2, [0, 1, 2, 3, 4])):
        bb = qr_solve(L[:, :, cols], rho)
        neg = bb[:, 0] < 0
        be0 = np.where(neg, np.sqrt(-bb[:, 0]), np.sqrt(bb[:, 0]))
        be1 = np.where(neg, np.where(bb[:, 2] < 0, np.sqrt(-bb[:, 2]), 0.0), np.where(bb[:, 2] > 0, np.sqrt(bb[:, 2]), 0.0))
        be0 = np.where(bb[:, 1] < 0, -be0, be0)
        be2 = bb[:, 3] / be0 if cand == 2 else z
        betas[:, cand] = gauss_newton(np.stack([be0, be1, be2, z], axis=1).astype(dt))

    Rs, ts, rep = np.zeros((H, 3, 3, 3), dt), np.zeros((H, 3, 3), dt), np.zeros((H, 3), dt)
    for c in range(3):
        ccs = np.zeros((H, 12), dt)
        for i in range(4):
            ccs = ccs + betas[:, c, i, None] * ut[:, 11 - i]
        ccs = ccs.reshape(H, 4, 3)

        def pcs(i, ccs):
            a = _alphas(cws, cci, pw[:, i])
            return [a[0] * ccs[:, 0, j] + a[1] * ccs[:, 1, j] + a[2] * ccs[:, 2, j] + a[3] * ccs[:, 3, j] for j in range(3)]
        flip = pcs(0, ccs)[2] < 0.0
        ccs = np.where(flip[:, None, None], -ccs, ccs)
        s6 = _psum(n, lambda i: pcs(i, ccs) + [pw[:, i, 0], pw[:, i, 1], pw[:, i, 2]], 6, z)
        pc0 = np.stack([s6[j] / dn for j in range(3)], axis=1)
        pw0 = np.stack([s6[3 + j] / dn for j in range(3)], axis=1)

        def abt_term(i):
            pc = pcs(i, ccs)
            return [(pc[j] - pc0[:, j]) * (pw[:, i, k] - pw0[:, k]) for j in range(3) for k in range(3)]
        abt = np.stack(_psum(n, abt_term, 9, z), axis=1).reshape(H, 3, 3)
        R = polar(abt, sweepsR)
        det = (R[:, 0, 0] * R[:, 1, 1] * R[:, 2, 2] + R[:, 0, 1] * R[:, 1, 2] * R[:, 2, 0] + R[:, 0, 2] * R[:, 1, 0] * R[:, 2, 1]
               - R[:, 0, 2] * R[:, 1, 1] * R[:, 2, 0] - R[:, 0, 1] * R[:, 1, 0] * R[:, 2, 2] - R[:, 0, 0] * R[:, 1, 2] * R[:, 2, 1])
        R[:, 2, :] = np.where((det < 0)[:, None], -R[:, 2, :], R[:, 2, :])
        t = np.stack([pc0[:, j] - _dot3(R[:, j], pw0) for j in range(3)], axis=1)

        def rep_term(i):
            Xc = _dot3(R[:, 0], pw[:, i]) + t[:, 0]
            Yc = _dot3(R[:, 1], pw[:, i]) + t[:, 1]
            inv_Zc = 1.0 / (_dot3(R[:, 2], pw[:, i]) + t[:, 2])
            ue = K[2] + K[0] * Xc * inv_Zc
            ve = K[3] + K[1] * Yc * inv_Zc
            u, v = uv[:, i, 0], uv[:, i, 1]
            return [np.sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve))]
        rep[:, c] = _psum(n, rep_term, 1, z)[0] / dn
        Rs[:, c], ts[:, c] = R, t
    N = np.where(rep[:, 1] < rep[:, 0], 1, 0)
    N = np.where(rep[:, 2] < rep[np.arange(H), N], 2, N)
    return dict(betas=betas, Rs=Rs, ts=ts, rep=rep, chosen=N)


def check_inliers(R, t, K, Xw, uv, max_err):
    """CheckInliers (:430-467) in its precisions: mask (H, N) bool. R (H,3,3), t (H,3) float64; Xw, uv, max_err float32."""
    X = Xw.astype(np.float64)
    c = [(R[:, i, 0, None] * X[None, :, 0] + R[:, i, 1, None] * X[None, :, 1] + R[:, i, 2, None] * X[None, :, 2]
          + t[:, i, None]) for i in range(3)]
    Xc, Yc = c[0].astype(np.float32), c[1].astype(np.float32)
    invZc = (1 / c[2]).astype(np.float32)
    ue = K[2] + K[0] * Xc.astype(np.float64) * invZc.astype(np.float64)
    ve = K[3] + K[1] * Yc.astype(np.float64) * invZc.astype(np.float64)
    dX = (uv[None, :, 0].astype(np.float64) - ue).astype(np.float32)
    dY = (uv[None, :, 1].astype(np.float64) - ve).astype(np.float32)
    e2 = dX * dX + dY * dY
    return e2 < max_err.astype(np.float32)[None, :]


def solve(pw32, uv32, K, Xw, uv, max_err, sweeps=(SWEEPS3, SWEEPS12, SWEEPSR)):
    """EPnP on the points pw32 (H, n, 3), uv32 (H, n, 2) float32 and the inlier test over (Xw, uv, max_err)."""
    with np.errstate(all="ignore"):
        pw, pu = pw32.astype(np.float64), uv32.astype(np.float64)
        K = np.asarray(K, np.float64)
        cws, cci = control_points(pw, sweeps[0])
        d, V = jacobi(mtm(pw, pu, K, cws, cci), sweeps[1])
        ut, eig = sorted_rows(d, V)
        r = downstream(ut, cws, cci, pw, pu, K, sweeps[2])
        hh = np.arange(pw.shape[0])
        r.update(ut=ut, eig=eig, cws=cws, cci=cci, R=r["Rs"][hh, r["chosen"]], t=r["ts"][hh, r["chosen"]])
        r["mask"] = check_inliers(r["R"], r["t"], K, Xw, uv, max_err)
        r["count"] = r["mask"].sum(axis=1).astype(np.int32)
    return r


def hypotheses(problem, draws, max_err=None, sweeps=(SWEEPS3, SWEEPS12, SWEEPSR)):
    """Every hypothesis of (H, 4) raw draws on a sqrtlm.pnp.PnPProblem."""
    idx = indices(problem.n_pair, draws)
    me = problem.max_err() if max_err is None else max_err
    r = solve(problem.Xw[idx], problem.uv[idx], problem.intr, problem.Xw, problem.uv, me, sweeps)
    r["idx"] = idx
    return r


def refine(problem, in_mask, max_err=None, sweeps=(SWEEPS3, SWEEPS12, SWEEPSR)):
    """Refine() on the pairs of in_mask, ascending (H = 1)."""
    who = np.flatnonzero(in_mask)
    me = problem.max_err() if max_err is None else max_err
    return solve(problem.Xw[who][None], problem.uv[who][None], problem.intr, problem.Xw, problem.uv, me, sweeps)


def downstream_ld(r, pw32, uv32, K, perturb=None):
    """The longdouble restatement of everything downstream of the ut (and control points) of ``r``."""
    ld = np.longdouble
    args = [r["ut"].astype(ld), r["cws"].astype(ld), r["cci"].astype(ld), pw32.astype(ld), uv32.astype(ld),
            np.asarray(K, np.float64).astype(ld)]
    if perturb is not None:   # +-1 ulp (of float64) on every input
        args = [a + perturb(a) for a in args]
    with np.errstate(all="ignore"):
        return downstream(*args)


def max_its(n, probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5):
    """SetRansacParameters (:178-227) literally: (mRansacMaxIts or 0 where iterate gives up, mRansacMinInliers)."""
    eps = np.float32(epsilon)
    n_min = int(np.float32(n) * eps)
    n_min = max(n_min, min_inliers, min_set)
    if n < n_min:
        return 0, n_min
    if eps < np.float32(n_min) / np.float32(n):
        eps = np.float32(n_min) / np.float32(n)
    if n_min == n:
        its = 1
    else:
        import math
        its = math.ceil(math.log(1 - probability) / math.log(1 - math.pow(float(eps), 3)))
    return max(1, min(its, max_iterations)), n_min


class LiteralSolver:
    """iterate / Refine / find of the reference, statement by statement, on
    given per-hypothesis results: ``count[h]``, and ``refined(mask_id)`` giving
    the refined count of hypothesis mask_id's mask. Hypotheses past the given
    ones raise IndexError."""

    def __init__(self, counts, refined, n_pair, min_inliers, max_its_):
        self.counts, self.refined = [int(c) for c in counts], refined
        self.N, self.mRansacMinInliers, self.mRansacMaxIts = n_pair, min_inliers, max_its_
        self.mnIterations = 0
        self.mnBestInliers = 0
        self.best = -1

    def iterate(self, nIterations):
        """(kind, hypothesis, bNoMore): kind 'refined' (a return from Refine), 'best' (mBestTcw) or None."""
        if self.N < self.mRansacMinInliers:
            return None, -1, True
        cur = 0
        while self.mnIterations < self.mRansacMaxIts or cur < nIterations:
            cur += 1
            h = self.mnIterations
            self.mnIterations += 1
            mnInliersi = self.counts[h]
            if mnInliersi >= self.mRansacMinInliers:
                if mnInliersi > self.mnBestInliers:
                    self.best, self.mnBestInliers = h, mnInliersi
                if self.refined(self.best) > self.mRansacMinInliers:
                    return "refined", self.best, False
        if self.mnIterations >= self.mRansacMaxIts:
            if self.mnBestInliers >= self.mRansacMinInliers:
                return "best", self.best, True
            return None, -1, True
        return None, -1, False

    def find(self):
        return self.iterate(self.mRansacMaxIts)[:2]
