"""Independent numpy restatement of g2oOptimizer::PoseOptimization
(g2oOptimizer.cc:385-679) that the GPU path (sqlm_pose_optimize,
sqlm_pose_refine_lidar) is held to.

The SE3 group operation (oplus) is the oracle's ``se3_oplus``: pose states are
data here, as the Sim3 states are in tests/sim3_ref.py. Everything else is
restated: map / project (types_six_dof_expmap.h:153-157), the analytic
Jacobian (types_six_dof_expmap.cpp:266-288; tests/test_pose_ref.py compares it
with ``oracle.mono_jacobians``' pose block), the two LiDAR errors and their
central-difference Jacobians (compared there with ``oracle.lidar_error`` /
``oracle.lidar_jacobian``), the Huber kernel, the 6x6 assembly, the Cholesky
solve (linear_solver_dense.h:100-118), g2o's LM rules (the ``LM`` class of
tests/sim3_ref.py) and the schedule: four rounds from the input pose, the
float / double threshold rules, the fewer-than-3 and fewer-than-10 rules, the
LiDAR stage, the final classification.

Stale errors are modelled the way g2o holds them: ``err_chi2[i]`` is the chi2
of edge i's ``_error`` as last computed -- by a trial's computeActiveErrors
while the edge is on level 0, by the check's ``computeError()`` while it is on
level 1 -- and every check reads it. (The kernel keeps one state E per problem
instead; the two must agree.) Before anything is computed it is 0.

``T`` selects the number type of everything after the pose states:
``np.float64`` is the reference the GPU is compared with, ``np.longdouble``
measures that reference's own rounding (the "spread").
"""
from __future__ import annotations

import numpy as np

from sim3_ref import DELTA, LM, huber, q_rotate

CHECKS = 5


# ---- per-edge arithmetic -----------------------------------------------------
def mono_error(q, t, K, X, uv, T=np.float64):
    """xc (n,3) = q X + t and e (n,2) = uv - (fx x/z + cx, fy y/z + cy), in type T."""
    q, t, K, X, uv = (np.asarray(a, T) for a in (q, t, K, X, uv))
    xc = q_rotate(q, X) + t
    e = np.stack([uv[:, 0] - ((xc[:, 0] / xc[:, 2]) * K[0] + K[2]), uv[:, 1] - ((xc[:, 1] / xc[:, 2]) * K[1] + K[3])],
                 axis=1)
    return xc, e


def mono_jacobian(xc, K, T=np.float64):
    """d e / d [omega; upsilon], (n,2,6)."""
    xc, K = np.asarray(xc, T), np.asarray(K, T)
    x, y, invz = xc[:, 0], xc[:, 1], T(1) / xc[:, 2]
    invz_2 = invz * invz
    fx, fy = K[0], K[1]
    J = np.zeros((xc.shape[0], 2, 6), T)
    J[:, 0, 0] = ((x * y) * invz_2) * fx
    J[:, 0, 1] = -(T(1) + ((x * x) * invz_2)) * fx
    J[:, 0, 2] = (y * invz) * fx
    J[:, 0, 3] = -invz * fx
    J[:, 0, 5] = (x * invz_2) * fx
    J[:, 1, 0] = (T(1) + (y * y) * invz_2) * fy
    J[:, 1, 1] = ((-x * y) * invz_2) * fy
    J[:, 1, 2] = (-x * invz) * fy
    J[:, 1, 4] = -invz * fy
    J[:, 1, 5] = (y * invz_2) * fy
    return J


def mono_chi2(q, t, prob, T=np.float64):
    _, e = mono_error(q, t, prob.intr, prob.Xw, prob.uv, T)
    w = np.asarray(prob.info, T)
    return e[:, 0] * (w * e[:, 0]) + e[:, 1] * (w * e[:, 1])


def lidar_errors(q, t, L, T=np.float64):
    """(m,): flat (T_cw pw - pc) . n, corner |T_cw pw - pc|."""
    q, t = np.asarray(q, T), np.asarray(t, T)
    d = (q_rotate(q, np.asarray(L.pw, T)) + t) - np.asarray(L.pc, T)
    n = np.asarray(L.n, T)
    flat = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
    corner = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return np.where(L.kind == 0, flat, corner)


def perturbed(O, q, t):
    """The 12 poses oplus((q, t), +-delta e_d), [2 d + sign], float64 (oracle)."""
    P = []
    for k in range(12):
        u = np.zeros(6)
        u[k >> 1] = -DELTA if k & 1 else DELTA
        P.append(O.se3_oplus(q, t, u))
    return P


def lidar_linearization(q, t, P, L, T=np.float64):
    """e (m,), J (m,6): central differences with the perturbed poses given as data."""
    e = lidar_errors(q, t, L, T)
    scalar = T(1.0) / (T(2) * T(DELTA))
    J = np.zeros((L.n_lid, 6), T)
    for d in range(6):
        J[:, d] = scalar * (lidar_errors(*P[2 * d], L, T) - lidar_errors(*P[2 * d + 1], L, T))
    return e, J


# ---- everything after e and J, generic over T --------------------------------
def huber_delta(th2):
    return float(np.float32(np.sqrt(np.float64(th2))))  # const float deltaMono = sqrt(5.991)


def assemble(e, J, info, active, robust, delta, lid=None, T=np.float64):
    """H (6,6), b (6,), robust chi2 over the active mono edges and, if given,
    the LiDAR edges lid = (e (m,), J (m,6), info (m,))."""
    e, J, w = np.asarray(e, T)[active], np.asarray(J, T)[active], np.asarray(info, T)[active]
    chi = e[:, 0] * (w * e[:, 0]) + e[:, 1] * (w * e[:, 1])
    rho0, rho1 = huber(chi, delta, T) if robust else (chi, np.ones_like(chi))
    ww = rho1 * w
    r = -(w[:, None] * e) * rho1[:, None]
    H = np.einsum("pra,p,prb->ab", J, ww, J)
    b = np.einsum("pra,pr->a", J, r)
    c = rho0.sum(dtype=T)
    if lid is not None and len(lid[0]):
        le, lJ, lw = (np.asarray(a, T) for a in lid)
        H = H + np.einsum("pa,p,pb->ab", lJ, lw, lJ)
        b = b + np.einsum("pa,p->a", lJ, -(lw * le))
        c = c + (le * (lw * le)).sum(dtype=T)
    return H, b, c


def solve6(H, b, lam, T=np.float64):
    """(H + lam I) dx = b by Cholesky; ok = every pivot > 0, else dx = 0."""
    n = 6
    A = np.array(H, T)
    A[np.diag_indices(n)] += T(lam)
    ok = True
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(n):
            dj = A[j, j]
            for c in range(j):
                dj = dj - A[j, c] * A[j, c]
            if not dj > 0:
                ok = False
            dj = np.sqrt(dj)
            A[j, j] = dj
            for i in range(j + 1, n):
                s = A[i, j]
                for c in range(j):
                    s = s - A[i, c] * A[j, c]
                A[i, j] = s / dj
        y = np.zeros(n, T)
        for i in range(n):
            s = T(b[i])
            for c in range(i):
                s = s - A[i, c] * y[c]
            y[i] = s / A[i, i]
        dx = np.zeros(n, T)
        for i in range(n - 1, -1, -1):
            s = y[i]
            for c in range(i + 1, n):
                s = s - A[c, i] * dx[c]
            dx[i] = s / A[i, i]
    if not ok:
        dx = np.zeros(n, T)
    return ok, dx


def compute_scale(dx, b, lam, T=np.float64):
    s = T(0)
    for j in range(6):
        s = s + dx[j] * (T(lam) * dx[j] + b[j])
    return s


def robust_sum(chi, robust, delta, T=np.float64):
    return (huber(chi, delta, T)[0] if robust else np.asarray(chi, T)).sum(dtype=T)


def run_stage(O, prob, q, t, niter, active, robust, delta, L, user_lambda, T, err_chi2, rec):
    """initializeOptimization(0); optimize(niter) over the active mono edges and
    the LiDAR pairs L (None: none). Updates err_chi2 of the active edges.
    Returns (q, t, stats)."""
    m = 0 if L is None else L.n_lid
    n_act = int(active.sum()) + m
    st = dict(iterations=0, trials=0, result=0, chi2_begin=T(0), chi2_end=T(0), lambda_end=T(0), active=n_act,
              last=None, trace_trials=[], ran=False)

    def linearize(q, t):
        xc, e = mono_error(q, t, prob.intr, prob.Xw, prob.uv, T)
        J = mono_jacobian(xc, prob.intr, T)
        lid = None
        if L is not None:
            P = perturbed(O, q, t)
            le, lJ = lidar_linearization(q, t, P, L, T)
            lid = (le, lJ, L.info)
        return e, J, lid

    if rec is not None and "lin" not in rec:  # e and J of every edge at the input pose
        e, J, lid = linearize(q, t)
        rec["lin"] = (np.asarray(e, np.float64), np.asarray(J, np.float64),
                      None if lid is None else (np.asarray(lid[0], np.float64), np.asarray(lid[1], np.float64)))
    if niter <= 0 or n_act == 0:  # optimize() returns before computing anything
        return q, t, st
    st["ran"] = True
    lm = LM(T)
    for it in range(niter):
        e, J, lid = linearize(q, t)
        H, b, chi = assemble(e, J, prob.info, active, robust, delta, lid, T)
        lm.cur = lm.ini = chi
        if it == 0:
            st["chi2_begin"] = chi
            lm.lam = T(user_lambda) if user_lambda > 0 else T(1e-5) * np.abs(np.diag(H)).max()
            lm.ni = T(2)
        while True:
            lam = lm.lam
            ok, dx = solve6(H, b, lam, T)
            scale = compute_scale(dx, b, lam, T)
            qt, tt = O.se3_oplus(q, t, np.asarray(dx, np.float64))
            c = mono_chi2(qt, tt, prob, T)
            err_chi2[active] = c[active]  # computeActiveErrors at the trial state
            chi_new = robust_sum(c[active], robust, delta, T)
            if L is not None and m:
                le = lidar_errors(qt, tt, L, T)
                chi_new = chi_new + (le * (np.asarray(L.info, T) * le)).sum(dtype=T)
            st["last"] = dict(H=H, b=b, dx=dx, lam=lam, ok=ok, scale=scale, chi_cur=chi, chi_new=chi_new, q=qt, t=tt)
            acc, end = lm.decide(chi_new, scale, ok)
            if acc:
                q, t = qt, tt
            if end:
                break
        if lm.result != 0:
            break
    st.update(iterations=lm.its, trials=lm.trials, result=lm.result, chi2_end=lm.chi2_end, lambda_end=lm.lambda_end,
              trace_trials=lm.trace_trials, trace_last_accepted=lm.trace_last_accepted)
    return q, t, st


def _check(prob, q, t, level, err_chi2, th2, final, T):
    """One classification: level-1 edges get computeError() at (q, t); every
    edge's stored chi2 is read as a float. Returns the values read."""
    c = mono_chi2(q, t, prob, T)
    err_chi2[level] = c[level]
    read = err_chi2.copy()
    with np.errstate(over="ignore", invalid="ignore"):
        cf = read.astype(np.float32)  # const float chi2 = e->chi2()
    level[:] = (cf.astype(np.float64) > np.float64(th2)) if final else (cf > np.float32(th2))
    return read


def _result(prob):
    n = prob.n_obs
    return dict(pose_q=np.array(prob.pose_q, np.float64), pose_t=np.array(prob.pose_t, np.float64), n_inliers=0,
                outlier=np.zeros(n, bool), edge_chi2=None, n_bad=[], n_bad_final=0, rounds=0, stats=[None] * 5,
                levels=[], lin=None)


def optimize(O, prob, iters=(10, 10, 10, 10), user_lambda=0.0, T=np.float64):
    """The vision schedule. Returns a dict: pose_q, pose_t, n_inliers, outlier
    (n,) bool, edge_chi2 (n, 5) in T, n_bad [per round run], n_bad_final,
    rounds, stats [5: stage dict or None], levels [level-1 mask after each
    round's check], lin (e, J, None)."""
    n = prob.n_obs
    out = _result(prob)
    out["edge_chi2"] = np.zeros((n, CHECKS), T)
    if n < 3:
        return out
    delta = huber_delta(prob.th2)
    q0, t0 = np.array(prob.pose_q, np.float64), np.array(prob.pose_t, np.float64)
    level = np.zeros(n, bool)
    err_chi2 = np.zeros(n, T)
    rec = {}
    q, t = q0, t0
    for r in range(4):
        q, t, st = run_stage(O, prob, q0, t0, iters[r], ~level, r < 3, delta, None, user_lambda, T, err_chi2,
                             rec if r == 0 else None)
        out["stats"][r] = st
        out["edge_chi2"][:, r] = _check(prob, q, t, level, err_chi2, prob.th2, False, T)
        out["n_bad"].append(int(level.sum()))
        out["levels"].append(level.copy())
        out["rounds"] += 1
        if n < 10:
            break
    out["lin"] = rec["lin"]
    out["edge_chi2"][:, 4] = _check(prob, q, t, level, err_chi2, prob.th2, True, T)
    out["n_bad_final"] = int(level.sum())
    out["outlier"] = level.copy()
    out["n_inliers"] = n - out["n_bad_final"]
    out["pose_q"], out["pose_t"] = np.array(q, np.float64), np.array(t, np.float64)
    return out


def refine(O, prob, L, outlier_in, robust_on, iters=10, user_lambda=0.0, T=np.float64):
    """The LiDAR stage from prob's pose and the final classification. The
    level-0 edges' stored errors are overwritten by the stage's trials (it has
    iters >= 1 and, with a level-0 edge, at least one trial), so nothing of the
    vision call's state is needed. Returns as ``optimize`` (stage index 4)."""
    n = prob.n_obs
    out = _result(prob)
    out["edge_chi2"] = np.zeros((n, CHECKS), T)
    if n < 3:
        return out
    delta = huber_delta(prob.th2)
    level = np.asarray(outlier_in, bool).copy()
    err_chi2 = np.zeros(n, T)
    rec = {}
    q, t, st = run_stage(O, prob, out["pose_q"], out["pose_t"], iters, ~level, bool(robust_on), delta, L, user_lambda,
                         T, err_chi2, rec)
    out["stats"][4] = st
    out["lin"] = rec["lin"]
    out["edge_chi2"][:, 4] = _check(prob, q, t, level, err_chi2, prob.th2, True, T)
    out["n_bad_final"] = int(level.sum())
    out["outlier"] = level.copy()
    out["n_inliers"] = n - out["n_bad_final"]
    out["pose_q"], out["pose_t"] = np.array(q, np.float64), np.array(t, np.float64)
    return out


def pose_optimization(O, prob, lidar_assoc=None, T=np.float64):
    """The reference call: vision, SetPose's float round trip, the optional
    LiDAR stage and another round trip. Returns (n_inliers, q, t, outlier)."""
    r = optimize(O, prob, T=T)
    if prob.n_obs < 3:
        return 0, r["pose_q"], r["pose_t"], r["outlier"]
    q, t = O.se3_from_Tcw_f32(O.se3_to_Tcw_f32(r["pose_q"], r["pose_t"]))
    if lidar_assoc is not None:
        sub = prob.copy()
        sub.pose_q[:], sub.pose_t[:] = q, t
        r = refine(O, sub, lidar_assoc((q.copy(), t.copy())), r["outlier"], prob.n_obs < 10, T=T)
        q, t = O.se3_from_Tcw_f32(O.se3_to_Tcw_f32(r["pose_q"], r["pose_t"]))
    return r["n_inliers"], q, t, r["outlier"]
