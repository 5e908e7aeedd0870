"""Independent numpy restatement of g2oOptimizer::OptimizeSim3
(g2oOptimizer.cc:1560-1793) that the GPU path (sqlm_sim3_optimize) is held to.

The Sim3 group operations (exp, multiply, inverse, oplus) are the oracle's
``sim3_*`` functions: they are the GPU's libm bits and are pinned elsewhere.
Everything else is restated here: map / project / cam_map
(types_seven_dof_expmap.h:130-171, sim3.h:144-146, se3_ops.hpp:49-55), the
central-difference Jacobians (base_binary_edge.hpp:131-205), the Huber kernel,
the 7x7 assembly (base_binary_edge.hpp:55-120), the Cholesky solve
(linear_solver_dense.h:100-118), g2o's LM rules
(optimization_algorithm_levenberg.cpp:61-189) and the two-stage schedule.

``T`` selects the number type of everything after the Sim3 states:
``np.float64`` is the reference the GPU is compared with, ``np.longdouble``
measures that reference's own rounding (the "spread").
"""
from __future__ import annotations

import numpy as np

DELTA = 1e-9
DBL_MAX = np.finfo(np.float64).max


# ---- per-edge arithmetic -----------------------------------------------------
def q_rotate(q, v):
    """Eigen's quaternion * vector: uv = 2 (q.vec x v); v + w uv + q.vec x uv. v (n,3)."""
    u0 = q[1] * v[:, 2] - q[2] * v[:, 1]
    u1 = q[2] * v[:, 0] - q[0] * v[:, 2]
    u2 = q[0] * v[:, 1] - q[1] * v[:, 0]
    u0, u1, u2 = u0 + u0, u1 + u1, u2 + u2
    c0 = q[1] * u2 - q[2] * u1
    c1 = q[2] * u0 - q[0] * u2
    c2 = q[0] * u1 - q[1] * u0
    return np.stack([v[:, 0] + q[3] * u0 + c0, v[:, 1] + q[3] * u1 + c1, v[:, 2] + q[3] * u2 + c2], axis=1)


def project_error(S, X, K, obs, T=np.float64):
    """obs - cam_map(project(S.map(X))), S (8,), X (n,3), obs (n,2), in type T."""
    S, X, K, obs = (np.asarray(a, T) for a in (S, X, K, obs))
    r = q_rotate(S, X)
    p0, p1, p2 = S[7] * r[:, 0] + S[4], S[7] * r[:, 1] + S[5], S[7] * r[:, 2] + S[6]
    u, v = p0 / p2, p1 / p2
    return np.stack([obs[:, 0] - (u * K[0] + K[2]), obs[:, 1] - (v * K[1] + K[3])], axis=1)


def perturbed(O, S, fix_scale):
    """The 14 estimates oplus(S, +-delta e_d) and their inverses, [2 d + sign], float64 (oracle)."""
    P, Pi = np.zeros((14, 8)), np.zeros((14, 8))
    for k in range(14):
        u = np.zeros(7)
        u[k >> 1] = -DELTA if k & 1 else DELTA
        P[k] = O.sim3_oplus(S, u, int(fix_scale))
        Pi[k] = O.sim3_inverse(P[k])
    return P, Pi


def edge_errors(prob, S, Si, T=np.float64):
    """e (n, 2 edges, 2): e12 at S, e21 at S^-1."""
    return np.stack([project_error(S, prob.X2c, prob.intr1, prob.obs1, T),
                     project_error(Si, prob.X1c, prob.intr2, prob.obs2, T)], axis=1)


def linearization(prob, S, Si, P, Pi, T=np.float64):
    """e (n,2,2) and J (n,2,2,7) with the perturbed Sim3 given as data."""
    e = edge_errors(prob, S, Si, T)
    n = prob.n_pair
    J = np.zeros((n, 2, 2, 7), T)
    scalar = T(1.0) / (T(2) * T(DELTA))
    for d in range(7):
        ep = edge_errors(prob, P[2 * d], Pi[2 * d], T)
        em = edge_errors(prob, P[2 * d + 1], Pi[2 * d + 1], T)
        J[:, :, :, d] = scalar * (ep - em)
    return e, J


# ---- everything after e and J, generic over T --------------------------------
def huber_delta(th2):
    return float(np.sqrt(np.float32(th2)))  # const float deltaHuber = sqrt(th2)


def edge_chi2(e, info, T=np.float64):
    """e (...,2), info (...): e^T (info I) e."""
    e, info = np.asarray(e, T), np.asarray(info, T)
    return e[..., 0] * (info * e[..., 0]) + e[..., 1] * (info * e[..., 1])


def huber(chi, delta, T=np.float64):
    chi = np.asarray(chi, T)
    delta = T(delta)
    dsqr = delta * delta
    inl = chi <= dsqr
    sq = np.sqrt(np.where(inl, T(1), chi))
    rho0 = np.where(inl, chi, T(2) * sq * delta - dsqr)
    rho1 = np.where(inl, T(1), delta / sq)
    return rho0, rho1


def assemble(e, J, info, delta, active, T=np.float64):
    """H (7,7), b (7,), robust chi2 over the active pairs. info (n,2) per edge."""
    e, J, info = np.asarray(e, T)[active], np.asarray(J, T)[active], np.asarray(info, T)[active]
    chi = edge_chi2(e, info, T)                      # (m,2)
    rho0, rho1 = huber(chi, delta, T)
    ww = rho1 * info                                 # weightedOmega = rho' Omega
    r = -(info[..., None] * e) * rho1[..., None]     # omega_r * rho'
    H = np.einsum("psra,ps,psrb->ab", J, ww, J)
    b = np.einsum("psra,psr->a", J, r)
    return H, b, rho0.sum(dtype=T)


def solve7(H, b, lam, T=np.float64):
    """(H + lam I) dx = b by Cholesky; ok = every pivot > 0, else dx = 0."""
    A = np.array(H, T)
    A[np.diag_indices(7)] += T(lam)
    ok = True
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(7):
            dj = A[j, j]
            for c in range(j):
                dj = dj - A[j, c] * A[j, c]
            if not dj > 0:
                ok = False
            dj = np.sqrt(dj)
            A[j, j] = dj
            for i in range(j + 1, 7):
                s = A[i, j]
                for c in range(j):
                    s = s - A[i, c] * A[j, c]
                A[i, j] = s / dj
        y = np.zeros(7, T)
        for i in range(7):
            s = T(b[i])
            for c in range(i):
                s = s - A[i, c] * y[c]
            y[i] = s / A[i, i]
        dx = np.zeros(7, T)
        for i in range(6, -1, -1):
            s = y[i]
            for c in range(i + 1, 7):
                s = s - A[c, i] * dx[c]
            dx[i] = s / A[i, i]
    if not ok:
        dx = np.zeros(7, T)
    return ok, dx


def compute_scale(dx, b, lam, T=np.float64):
    s = T(0)
    for j in range(7):
        s = s + dx[j] * (T(lam) * dx[j] + b[j])
    return s


class LM:
    """g2o's Levenberg state of one optimize() (levenberg.cpp:61-164 inside
    sparse_optimizer.cpp:376-414)."""

    def __init__(self, T):
        self.T = T
        self.lam = T(0); self.ni = T(2); self.cur = T(0); self.ini = T(0)
        self.qmax = 0; self.nbad = 0; self.its = 0; self.result = 0; self.trials = 0
        self.chi2_end = T(0); self.lambda_end = T(0)
        self.trace_chi2, self.trace_lambda, self.trace_trials, self.trace_last_accepted = [], [], [], []
        self.raul = False

    def decide(self, chi_new, scale, ok):
        """One trial's outcome; returns (accepted, iteration_ended)."""
        T = self.T
        temp = T(chi_new) if ok and not (np.isnan(chi_new) and np.isfinite(self.cur)) else T(DBL_MAX)
        rho = (self.cur - temp) / ((T(scale) if ok else T(0)) + T(1e-3))
        acc = False
        if rho > 0 and np.isfinite(temp):
            alpha = T(1) - (T(2) * rho - T(1)) ** 3
            alpha = min(alpha, T(2) / T(3))
            self.lam = self.lam * max(T(1) / T(3), alpha)
            self.ni = T(2)
            self.cur = temp
            acc = True
        else:
            self.lam = self.lam * self.ni
            self.ni = self.ni * T(2)
        self.qmax += 1
        self.trials += 1
        if rho < 0 and self.qmax < 10:
            return acc, False
        if self.qmax == 10 or rho == 0:
            self.result = 1
        else:
            self.nbad = self.nbad + 1 if (self.ini - self.cur) * T(1e3) < self.ini else 0
            if self.nbad >= 3:
                self.result = 1
                self.raul = True
        self.trace_chi2.append(self.cur); self.trace_lambda.append(self.lam); self.trace_trials.append(self.qmax)
        self.trace_last_accepted.append(acc)
        self.chi2_end, self.lambda_end = self.cur, self.lam
        self.its += 1
        self.qmax = 0
        return acc, True


def trial(O, S, fix_scale, H, b, lam, T=np.float64):
    """Solve, oplus: (ok, dx, scale, S_trial, S_trial^-1)."""
    ok, dx = solve7(H, b, lam, T)
    scale = compute_scale(dx, b, lam, T)
    St = O.sim3_oplus(S, np.asarray(dx, np.float64), int(fix_scale))
    return ok, dx, scale, St, O.sim3_inverse(St)


def robust_chi2(prob, S, Si, info, delta, active, T=np.float64):
    e = edge_errors(prob, S, Si, T)[active]
    return huber(edge_chi2(e, np.asarray(info, T)[active], T), delta, T)[0].sum(dtype=T)


def run_stage(O, prob, S, niter, info, delta, active, user_lambda, T, rec):
    """initializeOptimization(); optimize(niter). Returns (S, stats, E): E is the
    state of the last computed errors, or None if none was computed."""
    L = LM(T)
    Si = O.sim3_inverse(S)
    E = None
    st = dict(chi2_begin=T(0), last=None)
    for it in range(niter):
        P, Pi = perturbed(O, S, prob.fix_scale)
        e, J = linearization(prob, S, Si, P, Pi, T)
        H, b, chi = assemble(e, J, info, delta, active, T)
        if rec is not None and "lin" not in rec:
            rec["lin"] = (np.asarray(e, np.float64), np.asarray(J, np.float64), P, Pi)
        L.cur = L.ini = chi
        if it == 0:
            st["chi2_begin"] = chi
            L.lam = T(user_lambda) if user_lambda > 0 else T(1e-5) * np.abs(np.diag(H)).max()
            L.ni = T(2)
        while True:
            lam = L.lam
            ok, dx, scale, St, Sti = trial(O, S, prob.fix_scale, H, b, lam, T)
            chi_new = robust_chi2(prob, St, Sti, info, delta, active, T)
            E = (St, Sti)
            st["last"] = dict(H=H, b=b, dx=dx, lam=lam, ok=ok, scale=scale, chi_cur=chi, chi_new=chi_new, S_trial=St)
            acc, end = L.decide(chi_new, scale, ok)
            if acc:
                S, Si = St, Sti
            if end:
                break
        if L.result != 0:
            break
    st.update(iterations=L.its, trials=L.trials, result=L.result, chi2_end=L.chi2_end, lambda_end=L.lambda_end,
              trace_chi2=L.trace_chi2, trace_lambda=L.trace_lambda, trace_trials=L.trace_trials,
              trace_last_accepted=L.trace_last_accepted, raul=L.raul)
    return S, st, E


def optimize(O, prob, iters=(5, 10, 5), user_lambda=0.0, T=np.float64):
    """The whole schedule. Returns a dict: S12_out, n_inliers, n_bad, pair_state
    (n,), pair_chi2 (n, 2 checks, 2 edges), stats [stage dicts], lin (e, J, P, Pi)."""
    n = prob.n_pair
    S0 = np.array(prob.S12, np.float64)
    info = np.stack([prob.info1, prob.info2], axis=1)
    delta = huber_delta(prob.th2)
    th2 = T(prob.th2)
    state = np.zeros(n, np.uint8)
    chi2 = np.zeros((n, 2, 2), T)
    out = dict(S12_out=S0.copy(), n_inliers=0, n_bad=0, pair_state=state, pair_chi2=chi2, stats=[], lin=None)
    if n == 0:
        return out
    rec = {}
    if iters[0] <= 0:
        P, Pi = perturbed(O, S0, prob.fix_scale)
        e, J = linearization(prob, S0, O.sim3_inverse(S0), P, Pi, T)
        rec["lin"] = (np.asarray(e, np.float64), np.asarray(J, np.float64), P, Pi)
    active = np.ones(n, bool)
    S, st1, E = run_stage(O, prob, S0, iters[0], info, delta, active, user_lambda, T, rec)
    out["lin"] = rec["lin"]
    out["stats"].append(st1)

    def check(E):
        if E is None:
            return np.zeros((n, 2), T)
        return edge_chi2(edge_errors(prob, E[0], E[1], T), info, T)

    c = check(E)
    chi2[:, 0] = c
    chi2[:, 1] = c
    bad = (c > th2).any(axis=1)
    state[bad] = 1
    out["n_bad"] = int(bad.sum())
    if n - out["n_bad"] < 10:
        return out
    active = ~bad
    S, st2, E2 = run_stage(O, prob, S, iters[1] if out["n_bad"] > 0 else iters[2], info, delta, active,
                           user_lambda, T, None)
    out["stats"].append(st2)
    c = check(E2 if E2 is not None else E)
    chi2[active, 1] = c[active]
    fail = active & (c > th2).any(axis=1)
    state[fail] = 2
    out["n_inliers"] = int((state == 0).sum())
    out["S12_out"] = np.array(S, np.float64)
    return out
