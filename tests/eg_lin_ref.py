"""Extended-precision reference of ONE Levenberg-Marquardt trial of the
essential-graph optimisation (pure numpy, generic over the number type like
tests/lin_ref.py; ``np.longdouble`` is the x87 80-bit format on x86-64).

The 7x7 Jacobians of an EdgeSim3 are central differences over delta = 1e-9
(base_binary_edge.hpp:131-205), whose cancellation error no analytic reference
reproduces. They are not the arithmetic under test either: the GPU's Jacobians
and errors equal the oracle's bit for bit (tests/test_eg_gpu.py,
test_eg_numeric_jacobians_bitwise). So the reference takes A = d e / d S_i,
B = d e / d S_j and e per edge from the oracle as float64 DATA and does
everything after them in the number type it is given:

* active edges: not between two fixed vertices; free vertices: not fixed, with
  an active edge, in id order (hessianIndex);
* BaseBinaryEdge::constructQuadraticForm (base_binary_edge.hpp:55-120), Omega
  = ``pg.info`` or the identity: H_ii += A^T Omega A, H_jj += B^T Omega B,
  H_ij += A^T Omega B (and its transpose), b_i -= A^T Omega e,
  b_j -= B^T Omega e;
* (H + lam I) dx = b solved densely (lin_ref._solve_refined);
* chi2 = sum e^T Omega e at any state (e from the oracle at that state);
* the LM control of a trial (tests/test_eg_gpu_retrial.py): its gain ratio rho
  and the lambda an accepted trial leaves (levenberg.cpp:118-139).

first_trial() is a trial at any state: edge_data() on a graph at that state
(eg_retrial_cases.state_graph).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from lin_ref import LD, _rel, _segsum, _solve_refined


@dataclass
class EdgeData:
    """The oracle's float64 per-edge values at pg.Siw: what the reference takes as data."""
    act: np.ndarray      # (A,) ids of the active edges, in edge order
    free: np.ndarray     # (nP,) vertex ids of the free vertices, id order
    hi: np.ndarray       # (A,) hessianIndex of vertex 0 (-1: fixed)
    hj: np.ndarray       # (A,) hessianIndex of vertex 1
    A: np.ndarray        # (A,7,7), zero for a fixed vertex
    B: np.ndarray        # (A,7,7)
    e: np.ndarray        # (A,7)


def active(pg):
    """(active edge ids, free vertex ids, hessianIndex per vertex)."""
    fx = pg.fixed != 0
    act = np.nonzero(~(fx[pg.ei] & fx[pg.ej]))[0]
    vact = np.zeros(pg.n_kf, bool)
    vact[pg.ei[act]] = True
    vact[pg.ej[act]] = True
    free = np.nonzero(vact & ~fx)[0]
    hid = -np.ones(pg.n_kf, np.int64)
    hid[free] = np.arange(free.size)
    return act, free, hid


def edge_errors(oracle, pg, Siw=None):
    """(active edge ids, (A,7) float64 errors) at state Siw (default pg.Siw)."""
    Siw = pg.Siw if Siw is None else np.asarray(Siw, np.float64)
    act = active(pg)[0]
    e = np.array([oracle.eg_edge_error(Siw[pg.ei[k]], Siw[pg.ej[k]], pg.Sji[k]) for k in act]).reshape(-1, 7)
    return act, e


def edge_data(oracle, pg) -> EdgeData:
    act, free, hid = active(pg)
    A, B = np.zeros((act.size, 7, 7)), np.zeros((act.size, 7, 7))
    for n, k in enumerate(act):
        i, j = pg.ei[k], pg.ej[k]
        A[n], B[n] = oracle.eg_edge_jacobians(pg.Siw[i], pg.Siw[j], pg.Sji[k], pg.fix_scale,
                                              int(hid[i] >= 0), int(hid[j] >= 0))
    return EdgeData(act, free, hid[pg.ei[act]], hid[pg.ej[act]], A, B, edge_errors(oracle, pg)[1])


def _omega(pg, act, T):
    if pg.info is None:
        return np.broadcast_to(np.eye(7, dtype=T), (act.size, 7, 7))
    return pg.info[act].astype(T)


def edge_chi2(pg, act, e, dtype=LD):
    """Per-edge e^T Omega e in `dtype` for the active edges `act` with errors e."""
    e = np.asarray(e).astype(dtype)
    return np.einsum("ei,eij,ej->e", e, _omega(pg, act, dtype), e)


def chi2(oracle, pg, Siw=None, dtype=LD):
    """Total chi2 of the active edges at a state (activeChi2)."""
    act, e = edge_errors(oracle, pg, Siw)
    return edge_chi2(pg, act, e, dtype).sum()


@dataclass
class Trial:
    free: np.ndarray     # (nP,) vertex ids, hessianIndex order
    H: np.ndarray        # (7nP,7nP) with lam on the diagonal
    b: np.ndarray        # (7nP,)
    dx: np.ndarray       # (7nP,)
    chi2_0: object       # chi2 at the linearization point
    refine_steps: int


def first_trial(pg, lam, ed: EdgeData, dtype=LD) -> Trial:
    T = dtype
    nP = ed.free.size
    A, B, e = ed.A.astype(T), ed.B.astype(T), ed.e.astype(T)
    Om = _omega(pg, ed.act, T)
    AtO = np.einsum("eki,ekl->eil", A, Om)
    BtO = np.einsum("eki,ekl->eil", B, Om)
    fi, fj = ed.hi >= 0, ed.hj >= 0
    both = fi & fj
    if np.any(both & (ed.hi == ed.hj)):
        raise ValueError("eg_lin_ref has no self edges")
    H4 = _segsum(np.einsum("eil,elj->eij", AtO, A)[fi], ed.hi[fi] * (nP + 1), nP * nP)
    H4 += _segsum(np.einsum("eil,elj->eij", BtO, B)[fj], ed.hj[fj] * (nP + 1), nP * nP)
    Hij = np.einsum("eil,elj->eij", AtO, B)[both]
    H4 += _segsum(Hij, ed.hi[both] * nP + ed.hj[both], nP * nP)
    H4 += _segsum(Hij.transpose(0, 2, 1), ed.hj[both] * nP + ed.hi[both], nP * nP)
    H = H4.reshape(nP, nP, 7, 7).transpose(0, 2, 1, 3).reshape(7 * nP, 7 * nP)
    b = (_segsum(-np.einsum("eil,el->ei", AtO, e)[fi], ed.hi[fi], nP)
         + _segsum(-np.einsum("eil,el->ei", BtO, e)[fj], ed.hj[fj], nP)).reshape(-1)
    H[np.arange(7 * nP), np.arange(7 * nP)] += T(lam)
    dx, steps = _solve_refined(H, b) if nP else (np.zeros(0, T), 0)
    return Trial(ed.free, H, b, dx, edge_chi2(pg, ed.act, ed.e, T).sum(), steps)


def oplus_poses(oracle, pg, free, dx):
    """Siw (+) dx with the oracle's float64 VertexSim3Expmap::oplusImpl: all vertices."""
    S = pg.Siw.copy()
    d = np.asarray(dx, np.float64).reshape(-1, 7)
    for h, p in enumerate(free):
        S[p] = oracle.sim3_oplus(S[p], d[h], pg.fix_scale)
    return S


def pose_err(S, S_ref):
    """Max-norm error of Sim3 rows [q t s]: q and s absolute (both O(1)), t
    relative to the largest translation (at least 1)."""
    S, S_ref = np.asarray(S, LD), np.asarray(S_ref, LD)
    ts = max(LD(1), np.abs(S_ref[:, 4:7]).max())
    return float(max(np.abs(S[:, :4] - S_ref[:, :4]).max(), np.abs(S[:, 7] - S_ref[:, 7]).max(),
                     np.abs(S[:, 4:7] - S_ref[:, 4:7]).max() / ts))


def spreads(oracle, pg, lam, ed: EdgeData | None = None):
    """The reference's own rounding: the same evaluation in float64 against
    longdouble, max-norm relative per quantity; `pose` is between the two
    steps applied through the oracle's float64 oplus. Returns (dict,
    longdouble Trial, float64 Trial, longdouble-step poses, float64-step poses)."""
    ed = edge_data(oracle, pg) if ed is None else ed
    ref = first_trial(pg, lam, ed, LD)
    f64 = first_trial(pg, lam, ed, np.float64)
    S_hi = oplus_poses(oracle, pg, ref.free, ref.dx.astype(np.float64))
    S_lo = oplus_poses(oracle, pg, f64.free, f64.dx)
    out = dict(b=_rel(f64.b, ref.b), dx=_rel(f64.dx, ref.dx), pose=pose_err(S_lo, S_hi),
               chi2_0=_rel(f64.chi2_0, ref.chi2_0))
    return out, ref, f64, S_hi, S_lo


def rho(chi2_0, chi2_1, dx, b, lam):
    """The gain ratio of a trial as the LM loop forms it (levenberg.cpp:118-125
    with computeScale): (chi2_0 - chi2_1) / (sum dx (lam dx + b) + 1e-3), in
    the number type of dx. b is the undamped right-hand side."""
    T = dx.dtype.type
    dx, b = np.asarray(dx).reshape(-1), np.asarray(b).astype(dx.dtype).reshape(-1)
    scale = (dx * (T(lam) * dx + b)).sum() + T(1e-3)
    return (T(chi2_0) - T(chi2_1)) / scale


def lambda_accepted(lam, rho):
    """The damping after an accepted trial (levenberg.cpp:136-139):
    lam max(1/3, min(1 - (2 rho - 1)^3, 2/3)), in the number type of rho."""
    T = type(rho)
    alpha = min(T(1) - (T(2) * rho - T(1)) ** 3, T(2) / T(3))
    return T(lam) * max(T(1) / T(3), alpha)


def trial_rho(oracle, pg, tr: Trial, lam, dtype=LD):
    """(rho, chi2 at the trial state, trial state) of the trial `tr` made at
    pg.Siw with damping lam: the step applied through the oracle's float64
    oplus, the errors there from the oracle, chi2 and rho in `dtype`."""
    S1 = oplus_poses(oracle, pg, tr.free, tr.dx.astype(np.float64))
    c1 = chi2(oracle, pg, S1, dtype)
    return rho(tr.chi2_0, c1, tr.dx.astype(dtype), tr.b, lam), c1, S1


def chi2_spread(oracle, pg, Siw):
    """(longdouble chi2, relative float64-vs-longdouble spread) at a state."""
    act, e = edge_errors(oracle, pg, Siw)
    hi = edge_chi2(pg, act, e, LD).sum()
    lo = edge_chi2(pg, act, e, np.float64).sum()
    return hi, float(abs(LD(lo) - hi) / hi) if hi > 0 else 0.0
