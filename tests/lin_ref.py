"""Extended-precision reference of ONE Levenberg-Marquardt trial of the bundle
adjustment (pure numpy; ``np.longdouble`` is the x87 80-bit format on x86-64).

From a :class:`BAProblem` at its initial state and a damping ``lam`` it forms,
in the number type it is given, what g2o's BlockSolver forms for the first
trial: per-edge residuals, analytic Jacobians and robust weights, the blocks
``H_ll + lam I``, ``b_l``, ``H_pp + lam I``, ``b_p``, the dense Schur complement
``S`` and its right-hand side ``g``, the camera step ``dx = S^-1 g``, the
landmark back-substitution ``dl`` and the robust chi2 of any state.

Conventions follow the oracle (oracle/g2o_ref.c, oracle/se3_ref.h), i.e. g2o:

* ``H dx = b`` with ``b = -J^T W r``, ``r = obs - project(T X)``;
* pose tangent ``[omega; upsilon]``, left update ``T <- exp(d) T``
  (EdgeSE3ProjectXYZ::linearizeOplus, types_six_dof_expmap.cpp:103-139);
* ``W = info * rho'``, Huber as g2o applies it: ``rho' = 1`` if
  ``chi2 <= delta^2`` else ``delta / sqrt(chi2)``, no ``rho''`` term;
* a stereo edge (``obs_ur >= 0``) has the 3-row error ``(u, v, u_r)`` whose
  projection multiplies by the reference's **float32** ``invz`` and subtracts
  the float32 product ``bf * invz`` (EdgeStereoSE3ProjectXYZ::cam_project,
  .cpp:150-157), while its Jacobian divides by the double ``z`` (:188-234).
  That float32 value is a step function of the state, so it is taken from the
  float64 evaluation of ``z`` in every number type: it is part of the problem,
  not of the arithmetic under test;
* free cameras are the non-fixed poses with an active edge, in id order
  (hessianIndex), landmarks likewise.

LiDAR edges (EdgeLidarFlatPoint, unary on a pose, no robust kernel) add
``J^T info J`` to their camera's ``H_pp`` block, ``-J^T info e`` to its ``b_p``
and ``info e^2`` to the chi2. The error ``e = (q p_w + t - p_c) . n`` is
evaluated in the reference's number type. The Jacobian is g2o's central
difference with ``delta = 1e-9`` through oplus (base_unary_edge.hpp:82-122):
the difference of two errors that agree to ~8 digits, so its value carries
~1e-7 of cancellation noise that no analytic derivative reproduces. The
optimizer under test evaluates exactly that float64 expression (the same
operations in the same order as oracle/g2o_ref.c orc_lidar_jacobian, without
contraction), so the 1x6 float64 row is taken from the oracle at the float64
poses and used, cast, in every number type: like the stereo edge's float32
``invz`` it is part of the problem, not of the arithmetic under test.
Everything after it (the products with ``info``, the sums into the blocks,
the Schur complement, the solve) is carried in the reference's number type.
An edge is active when its level (``prob.meta["lid_level"]``, default 0) is
the optimised level and its pose is not fixed; an active LiDAR edge makes its
pose a free camera even without a vision edge at that level.

Everything is vectorised over edges / blocks; a 50-camera, 2000-landmark
problem takes about a second in longdouble.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

LD = np.longdouble


# ------------------------------------------------------------------ geometry

def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1],
                     a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _rotate(q, v):
    """q * v as Eigen's _transformVector (se3_ref.h oq_rotate)."""
    uv = _cross(q[:, :3], v)
    uv = uv + uv
    return v + q[:, 3:4] * uv + _cross(q[:, :3], uv)


def _quat_to_mat(q):
    """Eigen toRotationMatrix (se3_ref.h oq_to_mat), (N,3,3)."""
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    R = np.empty((q.shape[0], 3, 3), q.dtype)
    R[:, 0, 0] = 1 - (tyy + tzz); R[:, 0, 1] = txy - twz; R[:, 0, 2] = txz + twy
    R[:, 1, 0] = txy + twz; R[:, 1, 1] = 1 - (txx + tzz); R[:, 1, 2] = tyz - twx
    R[:, 2, 0] = txz - twy; R[:, 2, 1] = tyz + twx; R[:, 2, 2] = 1 - (txx + tyy)
    return R


def _inv3(m):
    """Inverse of (N,3,3) by cofactors (numpy.linalg has no longdouble)."""
    c = np.empty_like(m)
    for i in range(3):
        for j in range(3):
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            c[:, j, i] = m[:, i1, j1] * m[:, i2, j2] - m[:, i1, j2] * m[:, i2, j1]  # adjugate
    det = m[:, 0, 0] * c[:, 0, 0] + m[:, 0, 1] * c[:, 1, 0] + m[:, 0, 2] * c[:, 2, 0]
    return c / det[:, None, None]


def _segsum(vals, keys, n):
    """out[k] = sum of vals[i] with keys[i] == k, k < n (any float dtype)."""
    out = np.zeros((n,) + vals.shape[1:], vals.dtype)
    if keys.size == 0:
        return out
    o = np.argsort(keys, kind="stable")
    ks = keys[o]
    start = np.nonzero(np.r_[True, ks[1:] != ks[:-1]])[0]
    out[ks[start]] = np.add.reduceat(vals[o], start, axis=0)
    return out


# ------------------------------------------------------------------ edges

@dataclass
class Edges:
    """Active (level) edges at a state, in edge-id order. Mono edges have a
    zero third row."""
    eid: np.ndarray      # (E,) edge ids
    pose: np.ndarray     # (E,) pose id
    pt: np.ndarray       # (E,) point id
    stereo: np.ndarray   # (E,) bool
    r: np.ndarray        # (E,3) residual obs - proj
    proj: np.ndarray     # (E,3) projection (u, v, u_r)
    Jl: np.ndarray       # (E,3,3) d r / d X      (None without jac)
    Jp: np.ndarray       # (E,3,6) d r / d pose   (None without jac)
    chi2: np.ndarray     # (E,) r^T (info I) r
    w: np.ndarray        # (E,) info * rho'
    rho: np.ndarray      # (E,) robustified chi2


def edges(prob, dtype=LD, pose_q=None, pose_t=None, pt=None, level=0, jac=True) -> Edges:
    T = dtype
    pose_q = prob.pose_q if pose_q is None else np.asarray(pose_q, np.float64)
    pose_t = prob.pose_t if pose_t is None else np.asarray(pose_t, np.float64)
    pt = prob.pt if pt is None else np.asarray(pt, np.float64)
    eid = np.nonzero(prob.obs_level == level)[0]
    p, l = prob.obs_pose[eid].astype(np.int64), prob.obs_pt[eid].astype(np.int64)
    E = eid.size
    st = (prob.obs_ur[eid] >= 0) if prob.obs_ur is not None else np.zeros(E, bool)
    q, t, X = pose_q[p].astype(T), pose_t[p].astype(T), pt[l].astype(T)
    intr = prob.intr[p].astype(T)
    fx, fy, cx, cy = intr[:, 0], intr[:, 1], intr[:, 2], intr[:, 3]
    xc = _rotate(q, X) + t
    x, y, z = xc[:, 0], xc[:, 1], xc[:, 2]
    proj = np.zeros((E, 3), T)
    proj[:, 0] = (x / z) * fx + cx
    proj[:, 1] = (y / z) * fy + cy
    obs = np.zeros((E, 3), T)
    obs[:, :2] = prob.obs_uv[eid].astype(T)
    bf = np.zeros(E, T)
    if st.any():
        z64 = (_rotate(pose_q[p], pt[l]) + pose_t[p])[:, 2]
        with np.errstate(divide="ignore"):
            invz32 = (1.0 / z64).astype(np.float32)            # (float)(1.0f / z)
        bz32 = prob.pose_bf[p].astype(np.float32) * invz32     # float product
        invz, bz = invz32.astype(T), bz32.astype(T)
        us = x * invz * fx + cx
        vs = y * invz * fy + cy
        proj[:, 0] = np.where(st, us, proj[:, 0])
        proj[:, 1] = np.where(st, vs, proj[:, 1])
        proj[:, 2] = np.where(st, us - bz, 0)
        obs[:, 2] = np.where(st, prob.obs_ur[eid], 0).astype(T)
        bf = np.where(st, prob.pose_bf[p], 0).astype(T)
    r = obs - proj
    info = prob.obs_info[eid].astype(T)
    chi2 = r[:, 0] * (info * r[:, 0]) + r[:, 1] * (info * r[:, 1]) + r[:, 2] * (info * r[:, 2])
    delta = prob.obs_delta[eid].astype(T)
    dsq = delta * delta
    rob = (prob.obs_delta[eid] > 0) & (chi2 > dsq)
    sq = np.sqrt(np.where(rob, chi2, 1))
    rho1 = np.where(rob, delta / sq, 1)
    rho = np.where(rob, 2 * sq * delta - dsq, chi2)
    w = rho1 * info
    Jl = Jp = None
    if jac:
        R = _quat_to_mat(q)
        z2 = z * z
        # mono: -1/z * [[fx, 0, -x/z fx], [0, fy, -y/z fy]] * R
        s = -1 / z
        a0, a2 = s * fx, s * (-x / z * fx)
        b1, b2 = s * fy, s * (-y / z * fy)
        Jl = np.zeros((E, 3, 3), T)
        Jl[:, 0, :] = a0[:, None] * R[:, 0, :] + a2[:, None] * R[:, 2, :]
        Jl[:, 1, :] = b1[:, None] * R[:, 1, :] + b2[:, None] * R[:, 2, :]
        if st.any():
            s0 = -fx[:, None] * R[:, 0, :] / z[:, None] + (fx * x)[:, None] * R[:, 2, :] / z2[:, None]
            s1 = -fy[:, None] * R[:, 1, :] / z[:, None] + (fy * y)[:, None] * R[:, 2, :] / z2[:, None]
            s2 = s0 - bf[:, None] * R[:, 2, :] / z2[:, None]
            m = st[:, None]
            Jl[:, 0, :] = np.where(m, s0, Jl[:, 0, :])
            Jl[:, 1, :] = np.where(m, s1, Jl[:, 1, :])
            Jl[:, 2, :] = np.where(m, s2, 0)
        Jp = np.zeros((E, 3, 6), T)
        Jp[:, 0, 0] = x * y / z2 * fx
        Jp[:, 0, 1] = -(1 + (x * x / z2)) * fx
        Jp[:, 0, 2] = y / z * fx
        Jp[:, 0, 3] = -1 / z * fx
        Jp[:, 0, 5] = x / z2 * fx
        Jp[:, 1, 0] = (1 + y * y / z2) * fy
        Jp[:, 1, 1] = -x * y / z2 * fy
        Jp[:, 1, 2] = -x / z * fy
        Jp[:, 1, 4] = -1 / z * fy
        Jp[:, 1, 5] = y / z2 * fy
        if st.any():
            Jp[:, 2, 0] = np.where(st, Jp[:, 0, 0] - bf * y / z2, 0)
            Jp[:, 2, 1] = np.where(st, Jp[:, 0, 1] + bf * x / z2, 0)
            Jp[:, 2, 2] = np.where(st, Jp[:, 0, 2], 0)
            Jp[:, 2, 3] = np.where(st, Jp[:, 0, 3], 0)
            Jp[:, 2, 5] = np.where(st, Jp[:, 0, 5] - bf / z2, 0)
    return Edges(eid, p, l, st, r, proj, Jl, Jp, chi2, w, rho)


@dataclass
class LidarEdges:
    """Active LiDAR edges at a state, in edge-id order."""
    eid: np.ndarray      # (K,) edge ids
    pose: np.ndarray     # (K,) pose id
    e: np.ndarray        # (K,) error
    J: np.ndarray        # (K,6) the oracle's float64 numeric Jacobian, cast (None without jac)
    info: np.ndarray     # (K,)
    chi2: np.ndarray     # (K,) e info e


def lidar_level(prob):
    lv = prob.meta.get("lid_level")
    return np.zeros(prob.n_lid, np.uint8) if lv is None else np.asarray(lv, np.uint8).reshape(prob.n_lid)


def lidar_jacobians(prob, eid, pose_q=None, pose_t=None):
    """(K,6) float64: orc_lidar_jacobian per edge at float64 poses."""
    from oracle import oracle as O
    pose_q = prob.pose_q if pose_q is None else np.asarray(pose_q, np.float64)
    pose_t = prob.pose_t if pose_t is None else np.asarray(pose_t, np.float64)
    J = np.zeros((len(eid), 6))
    for k, e in enumerate(eid):
        p = prob.lid_pose[e]
        J[k] = O.lidar_jacobian(pose_q[p], pose_t[p], prob.lid_pc[e], prob.lid_pw[e], prob.lid_n[e])
    return J


def lidar_edges(prob, dtype=LD, pose_q=None, pose_t=None, level=0, jac=True) -> LidarEdges:
    T = dtype
    pose_q = prob.pose_q if pose_q is None else np.asarray(pose_q, np.float64)
    pose_t = prob.pose_t if pose_t is None else np.asarray(pose_t, np.float64)
    eid = np.nonzero((lidar_level(prob) == level) & (prob.pose_fixed[prob.lid_pose] == 0))[0]
    p = prob.lid_pose[eid].astype(np.int64)
    q, t = pose_q[p].astype(T), pose_t[p].astype(T)
    # orc_lidar_error: se3_map(p_w) - p_c, then (d0 n0 + d1 n1) + d2 n2
    d = (_rotate(q, prob.lid_pw[eid].astype(T)) + t) - prob.lid_pc[eid].astype(T)
    n = prob.lid_n[eid].astype(T)
    e = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
    info = prob.lid_info[eid].astype(T)
    J = lidar_jacobians(prob, eid, pose_q, pose_t).astype(T) if jac else None
    return LidarEdges(eid, p, e, J, info, e * (info * e))


def chi2(prob, pose_q=None, pose_t=None, pt=None, dtype=LD, level=0):
    """Total robust chi2 (activeRobustChi2) of the level's edges at a state."""
    out = edges(prob, dtype, pose_q, pose_t, pt, level, jac=False).rho.sum()
    if prob.n_lid:
        out = out + lidar_edges(prob, dtype, pose_q, pose_t, level, jac=False).chi2.sum()
    return out


# ------------------------------------------------------------------ one trial

@dataclass
class Trial:
    free: np.ndarray     # (nP,) pose ids of the free cameras, hessianIndex order
    lms: np.ndarray      # (nL,) point ids of the active landmarks
    Hpp: np.ndarray      # (nP,6,6) with lam on the diagonal
    bp: np.ndarray       # (nP,6)
    Hll: np.ndarray      # (nL,3,3) with lam on the diagonal
    bl: np.ndarray       # (nL,3)
    S: np.ndarray        # (6nP,6nP) dense Schur complement
    g: np.ndarray        # (6nP,)
    dx: np.ndarray       # (6nP,)
    dl: np.ndarray       # (n_pt,3) landmark step in point-id order (0 for inactive points)
    chi2_0: object       # robust chi2 at the linearization point
    refine_steps: int


def _solve_refined(S, g):
    """dx = S^-1 g: float64 LU solves plus iterative refinement with the
    residual in S's own number type, until that residual stops falling."""
    T = S.dtype.type
    S64 = S.astype(np.float64)
    x = np.zeros(g.shape, S.dtype)
    r = g.copy()
    best = None
    steps = 0
    for steps in range(1, 40):
        xn = x + np.linalg.solve(S64, r.astype(np.float64)).astype(S.dtype)
        rn = g - S @ xn
        nrm = np.abs(rn).max()
        if best is not None and not nrm < best:
            break
        x, r, best = xn, rn, nrm
        if nrm == T(0):
            break
    return x, steps


def first_trial(prob, lam, dtype=LD, level=0, solve=True) -> Trial:
    """solve=False stops after the blocks H_pp, b_p, H_ll, b_l (S, g, dx, dl are
    None): all lambda_init needs, and lam = 0 may leave an H_ll singular."""
    T = dtype
    ed = edges(prob, T, level=level)
    lid = lidar_edges(prob, T, level=level) if prob.n_lid else None
    lam = T(lam)
    act_pose = np.zeros(prob.n_pose, bool)
    act_pose[ed.pose] = True
    if lid is not None:
        act_pose[lid.pose] = True
    free = np.nonzero(act_pose & (prob.pose_fixed == 0))[0]
    act_pt = np.zeros(prob.n_pt, bool)
    act_pt[ed.pt] = True
    lms = np.nonzero(act_pt)[0]
    nP, nL = free.size, lms.size
    phid = -np.ones(prob.n_pose, np.int64)
    phid[free] = np.arange(nP)
    lhid = -np.ones(prob.n_pt, np.int64)
    lhid[lms] = np.arange(nL)

    wJl = ed.w[:, None, None] * ed.Jl                              # (E,3,3)
    wr = ed.w[:, None] * ed.r                                     # (E,3)
    Hll_e = np.einsum("eki,ekj->eij", wJl, ed.Jl)
    bl_e = -np.einsum("eki,ek->ei", ed.Jl, wr)
    lh = lhid[ed.pt]
    Hll = _segsum(Hll_e, lh, nL)
    bl = _segsum(bl_e, lh, nL)
    Hll[:, [0, 1, 2], [0, 1, 2]] += lam

    fe = np.nonzero(phid[ed.pose] >= 0)[0]                         # edges of free cameras
    ph = phid[ed.pose[fe]]
    Jp = ed.Jp[fe]
    Hpp = _segsum(np.einsum("eki,ekj->eij", ed.w[fe, None, None] * Jp, Jp), ph, nP)
    bp = _segsum(-np.einsum("eki,ek->ei", Jp, wr[fe]), ph, nP)
    chi2_0 = ed.rho.sum()
    if lid is not None and lid.eid.size:
        # unary edges (BaseUnaryEdge::constructQuadraticForm): every active one is on a free camera
        Ji = lid.J * lid.info[:, None]
        lh_ = phid[lid.pose]
        Hpp = Hpp + _segsum(Ji[:, :, None] * lid.J[:, None, :], lh_, nP)
        bp = bp - _segsum(Ji * lid.e[:, None], lh_, nP)
        chi2_0 = chi2_0 + lid.chi2.sum()
    Hpp[:, range(6), range(6)] += lam
    if not solve:
        return Trial(free, lms, Hpp, bp, Hll, bl, None, None, None, None, chi2_0, 0)

    # H_pl blocks, one per (landmark, free camera): repeated observations add up
    key = lh[fe] * nP + ph
    ukey, inv = np.unique(key, return_inverse=True)
    W = _segsum(np.einsum("eki,ekj->eij", Jp, wJl[fe]), inv, ukey.size)  # (nb,6,3), sorted by landmark, camera
    b_l, b_p = ukey // nP, ukey % nP
    Dinv = _inv3(Hll)
    Y = np.einsum("bik,bkj->bij", W, Dinv[b_l])                   # H_pl (H_ll + lam I)^-1
    g = (bp - _segsum(np.einsum("bik,bk->bi", Y, bl[b_l]), b_p, nP)).reshape(-1)

    # S = H_pp + lam I - sum_l sum_{i,j} Y_li W_lj^T, pairs of a landmark's blocks in chunks
    S4 = np.zeros((nP * nP, 6, 6), T)
    S4[np.arange(nP) * nP + np.arange(nP)] = Hpp
    cnt = np.bincount(b_l, minlength=nL)
    beg = np.cumsum(cnt) - cnt
    npair = cnt * cnt
    edges_l = np.r_[0, np.cumsum(npair)]
    l0 = 0
    while l0 < nL:
        l1 = int(np.searchsorted(edges_l, edges_l[l0] + 60000, side="right"))
        l1 = max(l1 - 1, l0 + 1)
        ls = np.arange(l0, l1)
        c = cnt[ls]
        tot = int(npair[ls].sum())
        if tot:
            lm_of = np.repeat(ls, npair[ls])
            k = np.arange(tot) - np.repeat(np.cumsum(npair[ls]) - npair[ls], npair[ls])
            cl = np.repeat(c, npair[ls])
            ia = beg[lm_of] + k // cl
            ib = beg[lm_of] + k % cl
            C = np.einsum("pik,pjk->pij", Y[ia], W[ib])
            S4 -= _segsum(C, b_p[ia] * nP + b_p[ib], nP * nP)
        l0 = l1
    S = S4.reshape(nP, nP, 6, 6).transpose(0, 2, 1, 3).reshape(6 * nP, 6 * nP)

    dx, steps = _solve_refined(S, g) if nP else (np.zeros(0, T), 0)
    dxp = dx.reshape(nP, 6)
    cl_ = bl - _segsum(np.einsum("bki,bk->bi", W, dxp[b_p]), b_l, nL)
    dl_act = np.einsum("lij,lj->li", Dinv, cl_)
    dl = np.zeros((prob.n_pt, 3), T)
    dl[lms] = dl_act
    return Trial(free, lms, Hpp, bp, Hll, bl, S, g, dx, dl, chi2_0, steps)


# ------------------------------------------------------------------ lambda_0

def max_diagonal(prob, dtype=LD, level=0):
    """(largest |diagonal entry| of J^T W J over all free vertices, "pose" or
    "point", the pose / point id it sits on): the blocks of an undamped
    first_trial (lam = 0)."""
    tr = first_trial(prob, 0, dtype, level, solve=False)
    dp = np.abs(tr.Hpp[:, range(6), range(6)]).max(axis=1) if tr.free.size else np.zeros(0, dtype)
    dl = np.abs(tr.Hll[:, range(3), range(3)]).max(axis=1) if tr.lms.size else np.zeros(0, dtype)
    ip = int(np.argmax(dp)) if dp.size else -1
    il = int(np.argmax(dl)) if dl.size else -1
    if il < 0 or (ip >= 0 and dp[ip] >= dl[il]):
        return dp[ip], "pose", int(tr.free[ip])
    return dl[il], "point", int(tr.lms[il])


def lambda_init(prob, dtype=LD, level=0):
    """OptimizationAlgorithmLevenberg::computeLambdaInit (levenberg.cpp:166-180,
    oracle/g2o_ref.c max_diagonal): 1e-5 x the largest diagonal entry of
    J^T W J over all free vertices, poses and landmarks alike, in `dtype`."""
    return dtype(1e-5) * max_diagonal(prob, dtype, level)[0]


# ------------------------------------------------------------------ rounding spread

def _rel(a, b):
    a, b = np.asarray(a, LD), np.asarray(b, LD)
    d = np.abs(a - b).max() if a.size else LD(0)
    s = np.abs(b).max() if b.size else LD(1)
    return float(d / s) if s > 0 else float(d)


def oplus_poses(oracle, prob, free, dx):
    """x (+) dx with the oracle's float64 SE3Quat arithmetic: all poses."""
    q, t = prob.pose_q.copy(), prob.pose_t.copy()
    d = np.asarray(dx, np.float64).reshape(-1, 6)
    for h, p in enumerate(free):
        q[p], t[p] = oracle.se3_oplus(q[p], t[p], d[h])
    return q, t


def spreads(prob, lam, ref: Trial | None = None, level=0):
    """The reference's own rounding: the same evaluation in float64 against
    longdouble, max-norm relative per quantity. Returns (dict, longdouble
    Trial, float64 Trial)."""
    ref = first_trial(prob, lam, LD, level) if ref is None else ref
    f64 = first_trial(prob, lam, np.float64, level)
    out = dict(g=_rel(f64.g, ref.g), dx=_rel(f64.dx, ref.dx), dl=_rel(f64.dl, ref.dl),
               chi2_0=_rel(f64.chi2_0, ref.chi2_0))
    return out, ref, f64


def spreads_lambda_init(prob, level=0):
    """spreads() of the trial at lambda_0 = lambda_init: the float64 side
    evaluates its own lambda_0 in float64, so the spread holds that rounding
    too. Returns (dict, longdouble Trial, float64 Trial)."""
    ref = first_trial(prob, lambda_init(prob, LD, level), LD, level)
    f64 = first_trial(prob, lambda_init(prob, np.float64, level), np.float64, level)
    out = dict(g=_rel(f64.g, ref.g), dx=_rel(f64.dx, ref.dx), dl=_rel(f64.dl, ref.dl),
               chi2_0=_rel(f64.chi2_0, ref.chi2_0))
    return out, ref, f64


def chi2_spread(prob, pose_q, pose_t, pt, level=0):
    """(longdouble chi2, relative float64-vs-longdouble spread) at a state."""
    hi = chi2(prob, pose_q, pose_t, pt, LD, level)
    lo = chi2(prob, pose_q, pose_t, pt, np.float64, level)
    return hi, float(abs(LD(lo) - hi) / hi) if hi > 0 else 0.0
