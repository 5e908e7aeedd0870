"""tests/lin_ref.py with the kind of every LiDAR edge honoured
(``prob.lid_kind``: 0 EdgeLidarFlatPoint, 1 EdgeLidarCornerPoint).

The oracle cannot express a corner edge, so this reference is a wrapper: the
vision part, the assembly, the Schur complement, the solve and the spreads are
lin_ref's own code, run with this module's ``lidar_edges`` in place of
lin_ref's. Two things are restated per corner edge:

* the error ``e = sqrt((d0^2 + d1^2) + d2^2)`` of ``d = q p_w + t - p_c``
  (types_six_dof_expmap.h:237-262) in the working number type;
* the Jacobian row: g2o's central difference with delta 1e-9 through oplus, as
  a float64 row taken as data in every number type, exactly as lin_ref takes
  the flat edge's row from the oracle (its docstring says why). For a corner
  edge the row is ``pose_ref.lidar_linearization``'s float64 row, whose
  perturbed poses come from the oracle's ``se3_oplus``; tests/test_gpu_pose.py
  established that it is bit-equal to the device's lidar_corner_jacobian.

With every kind 0 each function returns lin_ref's own result, bit for bit
(tests/test_lin_ref_corner.py).
"""
from __future__ import annotations

import contextlib
import types

import numpy as np

import lin_ref
import pose_ref
from lin_ref import LD, LidarEdges, Trial, lidar_level, oplus_poses  # noqa: F401  (re-exported)

_flat_lidar_edges = lin_ref.lidar_edges  # lin_ref's own, whatever _kind_aware() has put in its place


def kinds(prob):
    k = getattr(prob, "lid_kind", None)
    return np.zeros(prob.n_lid, np.uint8) if k is None or len(k) != prob.n_lid else np.asarray(k, np.uint8)


def lidar_jacobians(prob, eid, pose_q=None, pose_t=None):
    """(K,6) float64: orc_lidar_jacobian for a flat edge, the float64 row of
    pose_ref.lidar_linearization for a corner edge, at float64 poses."""
    from oracle import oracle as O
    eid = np.asarray(eid, np.int64)
    pose_q = prob.pose_q if pose_q is None else np.asarray(pose_q, np.float64)
    pose_t = prob.pose_t if pose_t is None else np.asarray(pose_t, np.float64)
    kd = kinds(prob)[eid]
    J = np.zeros((len(eid), 6))
    flat = np.nonzero(kd == 0)[0]
    if flat.size:
        J[flat] = lin_ref.lidar_jacobians(prob, eid[flat], pose_q, pose_t)
    cor = np.nonzero(kd != 0)[0]
    for p in np.unique(prob.lid_pose[eid[cor]]):
        k = cor[prob.lid_pose[eid[cor]] == p]
        e = eid[k]
        L = types.SimpleNamespace(pc=prob.lid_pc[e], pw=prob.lid_pw[e], n=prob.lid_n[e],
                                  kind=np.ones(e.size, np.uint8), n_lid=e.size)
        P = pose_ref.perturbed(O, pose_q[p], pose_t[p])
        J[k] = pose_ref.lidar_linearization(pose_q[p], pose_t[p], P, L, np.float64)[1]
    return J


def lidar_edges(prob, dtype=LD, pose_q=None, pose_t=None, level=0, jac=True) -> LidarEdges:
    kd = kinds(prob)
    if not kd.any():
        return _flat_lidar_edges(prob, dtype, pose_q, pose_t, level, jac)
    T = dtype
    pose_q = prob.pose_q if pose_q is None else np.asarray(pose_q, np.float64)
    pose_t = prob.pose_t if pose_t is None else np.asarray(pose_t, np.float64)
    eid = np.nonzero((lidar_level(prob) == level) & (prob.pose_fixed[prob.lid_pose] == 0))[0]
    p = prob.lid_pose[eid].astype(np.int64)
    q, t = pose_q[p].astype(T), pose_t[p].astype(T)
    d = (lin_ref._rotate(q, prob.lid_pw[eid].astype(T)) + t) - prob.lid_pc[eid].astype(T)
    n = prob.lid_n[eid].astype(T)
    flat = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
    corner = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    e = np.where(kd[eid] == 0, flat, corner)
    info = prob.lid_info[eid].astype(T)
    J = lidar_jacobians(prob, eid, pose_q, pose_t).astype(T) if jac else None
    return LidarEdges(eid, p, e, J, info, e * (info * e))


@contextlib.contextmanager
def _kind_aware():
    old = lin_ref.lidar_edges  # nested calls: the wrapper itself
    lin_ref.lidar_edges = lidar_edges
    try:
        yield
    finally:
        lin_ref.lidar_edges = old


def _wrap(fn):
    def call(*a, **kw):
        with _kind_aware():
            return fn(*a, **kw)
    call.__name__, call.__doc__ = fn.__name__, fn.__doc__
    return call


# lin_ref's own code, seeing the kind-aware LiDAR edges
chi2 = _wrap(lin_ref.chi2)
first_trial = _wrap(lin_ref.first_trial)
max_diagonal = _wrap(lin_ref.max_diagonal)
lambda_init = _wrap(lin_ref.lambda_init)
spreads = _wrap(lin_ref.spreads)
spreads_lambda_init = _wrap(lin_ref.spreads_lambda_init)
chi2_spread = _wrap(lin_ref.chi2_spread)
