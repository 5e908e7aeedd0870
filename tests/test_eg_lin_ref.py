"""tests/eg_lin_ref.py (the extended-precision reference of one essential-graph
LM trial) against the CPU oracle and against itself, and the conditions on the
inputs of tests/test_eg_gpu_first_trial.py. No GPU."""
import functools

import numpy as np
import pytest

import eg_lin_ref
from eg_first_trial_cases import CASES, GRAPH_OF

EPS = float(np.finfo(np.float64).eps)
LD = eg_lin_ref.LD
K = 100.0


@functools.lru_cache(maxsize=None)
def _graph(name):
    return CASES[name][0]()


_edge_data = {}


def _reference(oracle, name):
    """(spreads, longdouble trial, float64 trial, poses of either step); the
    oracle's per-edge values once per graph, whatever the lambda."""
    g = GRAPH_OF[name]
    if g not in _edge_data:
        _edge_data[g] = eg_lin_ref.edge_data(oracle, _graph(name))
    return eg_lin_ref.spreads(oracle, _graph(name), CASES[name][1], _edge_data[g])


def test_quadratic_form_edge_by_edge(oracle):
    """The vectorised assembly against BaseBinaryEdge::constructQuadraticForm
    written out edge by edge with a dense Jacobian row block, on the graph
    with fixed vertices, reversed and parallel edges and on the one with
    information matrices: to longdouble rounding."""
    for name in ("mixed_lam1", "info_lam1"):
        pg, lam = _graph(name), CASES[name][1]
        ed = eg_lin_ref.edge_data(oracle, pg)
        tr = eg_lin_ref.first_trial(pg, lam, ed)
        n = 7 * ed.free.size
        H, b = np.zeros((n, n), LD), np.zeros(n, LD)
        for k in range(ed.act.size):
            J = np.zeros((7, n), LD)
            if ed.hi[k] >= 0:
                J[:, 7 * ed.hi[k]:7 * ed.hi[k] + 7] = ed.A[k]
            if ed.hj[k] >= 0:
                J[:, 7 * ed.hj[k]:7 * ed.hj[k] + 7] = ed.B[k]
            Om = np.eye(7, dtype=LD) if pg.info is None else pg.info[ed.act[k]].astype(LD)
            H += J.T @ Om @ J
            b -= J.T @ (Om @ ed.e[k].astype(LD))
        H[np.arange(n), np.arange(n)] += LD(lam)
        assert np.abs(H - tr.H).max() <= 1e-17 * np.abs(H).max()
        assert np.abs(b - tr.b).max() <= 1e-17 * np.abs(b).max()
    pg = _graph("mixed_lam1")
    act, free, hid = eg_lin_ref.active(pg)
    assert act.size == pg.n_edge - 1 and not set(free) & {0, 7, 8, 20}   # edge 8 -> 7 is inactive
    assert np.any(pg.ei[act] < pg.ej[act]) and np.any(pg.ei[act] > pg.ej[act])
    pairs = list(zip(pg.ei[act], pg.ej[act]))
    assert len(set(pairs)) == len(pairs) - 5                            # five parallel edges


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_accepts_first_trial(oracle, name):
    pg, lam = _graph(name), CASES[name][1]
    assert pg.n_kf <= 300
    n, st = oracle.OracleEG(pg).optimize(1, lam)
    assert n == 1 and st["trace_trials"] == [1], st


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_and_cap(oracle, name):
    """Self-consistency of the longdouble solve; the cap on the reference's
    own rounding (a condition on the case, not a measurement: on an
    ill-conditioned graph K x spread would let anything pass); the float64
    reference's poses after the step against the oracle's after one iteration
    (both float64: K x the float64-vs-longdouble spread of those poses); the
    oracle's chi2 before and after against the longdouble chi2."""
    pg, lam = _graph(name), CASES[name][1]
    sp, ref, f64, S_hi, S_lo = _reference(oracle, name)
    assert np.abs(ref.H @ ref.dx - ref.b).max() <= 1e-17 * np.abs(ref.b).max()
    assert 0 < sp["b"] <= 1e-14 and 0 < sp["dx"] <= 1e-9, sp
    org = oracle.OracleEG(pg)
    n, st = org.optimize(1, lam)
    err = eg_lin_ref.pose_err(org.Siw, S_hi)
    chi_hi, chi_sp = eg_lin_ref.chi2_spread(oracle, pg, org.Siw)
    chi_err = float(abs(LD(st["trace_chi2"][0]) - chi_hi) / chi_hi)
    chi0_err = float(abs(LD(st["chi2_begin"]) - ref.chi2_0) / ref.chi2_0)
    print(f"{name}: spreads {sp} oracle pose err {err:.2e} chi2 err {chi_err:.2e} (spread {chi_sp:.2e}) "
          f"chi2_0 err {chi0_err:.2e}")
    assert err <= K * max(sp["pose"], 4 * EPS)
    assert chi_err <= K * max(chi_sp, 4 * EPS)
    assert chi0_err <= K * max(sp["chi2_0"], 4 * EPS)
    np.testing.assert_allclose(org.edge_chi2()[ref_act(pg)], eg_lin_ref.edge_chi2(
        pg, *eg_lin_ref.edge_errors(oracle, pg, org.Siw)).astype(np.float64), rtol=K * 4 * EPS, atol=0)


def ref_act(pg):
    return eg_lin_ref.active(pg)[0]
