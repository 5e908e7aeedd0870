"""The conditions on the inputs of tests/test_eg_gpu_retrial.py, on the CPU:
the oracle takes the recorded trials on every case of
tests/eg_retrial_cases.py, every one of those trials is decided with margin,
and the reference of every trial whose numbers are compared is well
conditioned.

The margin is a condition, not a tolerance: rho of each trial, formed as
EGSolver::optimize forms it -- (chi2_0 - chi2_1) / (sum dx (lambda dx + b) +
1e-3), chi2_1 at S (+) dx(lambda_k) -- by tests/eg_lin_ref.py in float64 and
in longdouble, is below -1e-3 for a rejected trial and above 1e-3 for an
accepted one. The GPU's chi2 and scale differ from the reference's by
rounding (<= 1e-12 relative, the ratio tests), so it cannot decide a trial
differently. The caps are those of tests/test_eg_lin_ref.py (b <= 1e-14,
dx <= 1e-9). A case that misses a condition is replaced, not excused. No GPU.
"""
import functools

import numpy as np
import pytest

import eg_lin_ref
from eg_retrial_cases import CASES, EXHAUSTED, EXPECT, GRAPH_OF, TWO_ITER, kick, lambda_at, state_graph

LD = eg_lin_ref.LD
MARGIN = 1e-3


@functools.lru_cache(maxsize=None)
def _graph(name):
    return (CASES.get(name) or EXHAUSTED[name])[0]()


def _oracle_run(oracle, pg, iterations, lam):
    org = oracle.OracleEG(pg)
    n, st = org.optimize(iterations, lam)
    return org, n, st


def _check_margins(oracle, name, pg, lam0, trials, last_accepted=True):
    """Trials 0 .. trials-2 at pg's state are rejected and trial trials-1 is
    accepted (or rejected too), each with |rho| >= MARGIN, in float64 and in
    longdouble. Returns the longdouble rho of the last trial."""
    ed = eg_lin_ref.edge_data(oracle, pg)
    for k in range(trials):
        lam = lambda_at(lam0, k)
        for dtype in (np.float64, LD):
            tr = eg_lin_ref.first_trial(pg, lam, ed, dtype)
            rho, chi1, _ = eg_lin_ref.trial_rho(oracle, pg, tr, lam, dtype)
            print(f"{name}: trial {k} lambda {lam:.6g} {np.dtype(dtype).name} chi2 {float(tr.chi2_0):.6g} -> "
                  f"{float(chi1):.6g} rho {float(rho):+.3g}")
            assert np.isfinite(chi1) and np.isfinite(rho)
            if k == trials - 1 and last_accepted:
                assert rho >= MARGIN, (name, k, lam, dtype, rho)
            else:
                assert rho <= -MARGIN, (name, k, lam, dtype, rho)
    return rho


def _check_caps(oracle, name, pg, lam):
    sp, ref, f64, S_hi, S_lo = eg_lin_ref.spreads(oracle, pg, lam)
    print(f"{name}: lambda {lam:.6g} spreads {sp}")
    assert np.abs(ref.H @ ref.dx - ref.b).max() <= 1e-17 * np.abs(ref.b).max()
    assert 0 < sp["b"] <= 1e-14 and 0 < sp["dx"] <= 1e-9, (name, sp)


def test_rho_and_lambda_accepted():
    """The two formulas against the host loop's arithmetic written out."""
    dx, b = np.array([0.5, -2.0, 0.25]), np.array([1.0, 3.0, -4.0])
    scale = 0.5 * (0.125 * 0.5 + 1.0) + -2.0 * (0.125 * -2.0 + 3.0) + 0.25 * (0.125 * 0.25 - 4.0) + 1e-3
    assert eg_lin_ref.rho(10.0, 12.0, dx, b, 0.125) == pytest.approx(-2.0 / scale, rel=1e-15)
    assert isinstance(eg_lin_ref.rho(10.0, 12.0, dx.astype(LD), b, 0.125), LD)
    assert eg_lin_ref.lambda_accepted(3.0, 0.5) == 2.0                     # alpha = 1, capped at 2/3
    assert eg_lin_ref.lambda_accepted(3.0, 1.0) == 1.0                     # alpha = 0, floored at 1/3
    assert eg_lin_ref.lambda_accepted(1.0, 0.9) == pytest.approx(1 - 0.8 ** 3, rel=1e-15)   # 0.488, between the two
    assert isinstance(eg_lin_ref.lambda_accepted(1.0, LD(0.9)), LD)


def test_kick_and_state_graph():
    pg = CASES["border3"][0]()
    base = kick(pg, 0.0, 1.5, 3.0)
    assert np.array_equal(base.Siw, pg.Siw) and base.Siw is not pg.Siw
    full = kick(pg, 1.0, 1.5, 3.0)
    assert np.array_equal(full.Siw[0], pg.Siw[0]) and np.all(np.any(full.Siw[1:] != pg.Siw[1:], axis=1))
    assert np.allclose(np.linalg.norm(full.Siw[:, :4], axis=1), 1.0, atol=1e-14) and np.all(full.Siw[:, 7] == pg.Siw[:, 7])
    assert np.array_equal(full.Sji, pg.Sji) and np.array_equal(full.ei, pg.ei)
    st = state_graph(pg, full.Siw)
    assert np.array_equal(st.Siw, full.Siw) and st.Siw is not full.Siw and np.array_equal(st.Sji, pg.Sji)
    with pytest.raises(ValueError):
        state_graph(pg, full.Siw[:-1])


def test_cases_cover_the_paths():
    """What the issue asks the set to hold, as far as the CPU can see it (the
    device path of each case is asserted on the GPU against EXPECT)."""
    assert set(TWO_ITER) <= set(CASES) and set(GRAPH_OF) == set(CASES) | set(EXHAUSTED)
    assert all(TWO_ITER[n][0] == CASES[n][2] for n in TWO_ITER)
    assert all(c[2] >= 2 for c in CASES.values()) and max(c[2] for c in CASES.values()) >= 7   # >= 6 rejections
    borders = {n: EXPECT[GRAPH_OF[n]]["border"] for n in CASES}
    assert borders["band"] == 0 and EXPECT["border3"]["R"] == 16 and EXPECT["border5"]["R"] == 32
    for n in CASES:
        pg = _graph(n)
        assert pg.n_kf <= 60
        assert (pg.info is not None) == EXPECT[GRAPH_OF[n]]["info"]
    assert _graph("info").info is not None and np.array_equal(_graph("info").info, _graph("info").info.transpose(0, 2, 1))
    pg = _graph("mixed")
    act, free, hid = eg_lin_ref.active(pg)
    assert set(np.nonzero(pg.fixed)[0]) == {0, 7, 8, 20} and act.size == pg.n_edge - 1
    assert np.any(pg.ei[act] < pg.ej[act]) and np.any(pg.ei[act] > pg.ej[act])
    pairs = list(zip(pg.ei[act], pg.ej[act]))
    assert len(set(pairs)) == len(pairs) - 5
    assert _graph("free_scale").fix_scale == 0 and TWO_ITER["free_scale"][1] >= 2
    assert any(t2 >= 2 for n, (_, t2) in TWO_ITER.items() if _graph(n).fix_scale)
    assert {acc for _, _, acc in EXHAUSTED.values()} == {False, True}


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_rejects_then_accepts(oracle, name):
    make, lam0, trials = CASES[name]
    pg = _graph(name)
    lam_j = lambda_at(lam0, trials - 1)
    org, n, st = _oracle_run(oracle, pg, 1, lam0)
    assert n == 1 and st["trace_trials"] == [trials] and st["result"] == 0, st
    assert lam_j * (1.0 / 3.0) <= st["trace_lambda"][0] <= lam_j * (2.0 / 3.0), (st["trace_lambda"], lam_j)
    # a fresh first trial at lambda_j is accepted, and leaves what the retrial left
    org2, n2, st2 = _oracle_run(oracle, pg, 1, lam_j)
    assert n2 == 1 and st2["trace_trials"] == [1], st2
    assert st2["trace_lambda"][0] == st["trace_lambda"][0] and st2["trace_chi2"][0] == st["trace_chi2"][0]
    assert np.array_equal(org2.Siw, org.Siw)
    rho = _check_margins(oracle, name, pg, lam0, trials)
    # the lambda the oracle left is the reference's formula on the reference's rho
    lam_ref = float(eg_lin_ref.lambda_accepted(lam_j, rho))
    assert abs(st["trace_lambda"][0] - lam_ref) <= 1e-6 * lam_ref, (st["trace_lambda"], lam_ref)
    _check_caps(oracle, name, pg, lam_j)


@pytest.mark.parametrize("name", sorted(TWO_ITER))
def test_second_iteration(oracle, name):
    make, lam0, trials = CASES[name]
    t1, t2 = TWO_ITER[name]
    pg = _graph(name)
    org1, n1, st1 = _oracle_run(oracle, pg, 1, lam0)
    org, n, st = _oracle_run(oracle, pg, 2, lam0)
    assert n == 2 and st["trace_trials"] == [t1, t2] and st["result"] == 0, st
    assert st["trace_chi2"][0] == st1["trace_chi2"][0] and st["trace_lambda"][0] == st1["trace_lambda"][0]
    assert st["trace_chi2"][1] < st["trace_chi2"][0] < st["chi2_begin"]        # both iterations accepted a trial
    lam2 = st["trace_lambda"][0]
    lam = lambda_at(lam2, t2 - 1)
    assert lam * (1.0 / 3.0) <= st["trace_lambda"][1] <= lam * (2.0 / 3.0)
    pg1 = state_graph(pg, org1.Siw)
    _check_margins(oracle, name + " it2", pg1, lam2, t2)
    _check_caps(oracle, name + " it2", pg1, lam)


@pytest.mark.parametrize("name", sorted(EXHAUSTED))
def test_exhausted_iteration(oracle, name):
    make, lam0, accepted = EXHAUSTED[name]
    pg = _graph(name)
    org, n, st = _oracle_run(oracle, pg, 5, lam0)
    # ten trials end the run, whatever the tenth gave (levenberg.cpp:147-151)
    assert n == 1 and st["trace_trials"] == [10] and st["result"] == 1 and st["iterations"] == 1, st
    if accepted:
        assert st["chi2_end"] < st["chi2_begin"] * (1 - MARGIN) and not np.array_equal(org.Siw, pg.Siw)
    else:
        assert st["chi2_end"] == st["chi2_begin"] and np.array_equal(org.Siw, pg.Siw)
        assert st["trace_lambda"][0] == lambda_at(lam0, 10)
    _check_margins(oracle, name, pg, lam0, 10, last_accepted=accepted)
    _check_caps(oracle, name, pg, lambda_at(lam0, 9))
