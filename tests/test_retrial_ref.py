"""The conditions on the inputs of tests/test_gpu_retrial.py, on the CPU: the
oracle takes the recorded number of trials on every case of
tests/retrial_cases.py, and every one of those trials is decided with margin.

The margin is a condition, not a tolerance: the chi2 of each trial state,
x (+) dx(lambda_k), X + dl(lambda_k), evaluated by tests/lin_ref.py in float64
and in longdouble, lies more than 1e-3 (relative) above the chi2 of the
linearization point for a rejected trial (or is not finite) and more than 1e-3
below it for the accepted one. The GPU's trial chi2 and the oracle's differ
from the reference's by rounding (<= 1e-12 relative, the ratio tests), so
neither can decide a trial differently. A case that misses the condition is
replaced, not excused. No GPU.
"""
import functools

import numpy as np
import pytest

import lin_ref
from retrial_cases import CASES, LIDAR, TWO_ITER, lambda_at, state_problem

LD = lin_ref.LD
MARGIN = 1e-3


@functools.lru_cache(maxsize=None)
def _problem(name):
    return CASES[name][0]()


def _oracle_run(oracle, prob, iterations, lam):
    og = oracle.OracleGraph(prob)
    og.lid_level[:] = lin_ref.lidar_level(prob)
    n, st = og.optimize(0, iterations, user_lambda=lam)
    return og, n, st


def _trial_chi2(oracle, prob, lam, dtype):
    """(chi2 at the linearization point, chi2 at the trial state) in dtype."""
    tr = lin_ref.first_trial(prob, lam, dtype)
    q, t = lin_ref.oplus_poses(oracle, prob, tr.free, tr.dx.astype(np.float64))
    X = prob.pt + tr.dl.astype(np.float64)
    return tr.chi2_0, lin_ref.chi2(prob, q, t, X, dtype)


def _decided(chi0, chi, accepted):
    chi0, chi = LD(chi0), LD(chi)
    if accepted:
        return bool(np.isfinite(chi) and chi < chi0 * (1 - LD(MARGIN)))
    return bool(not np.isfinite(chi) or chi > chi0 * (1 + LD(MARGIN)))


def _check_margins(oracle, name, prob, lam0, trials):
    """Trials 0 .. trials-2 at prob's state are rejected, trial trials-1 is
    accepted, each with margin, in float64 and in longdouble."""
    for k in range(trials):
        lam = lambda_at(lam0, k)
        for dtype in (np.float64, LD):
            chi0, chi = _trial_chi2(oracle, prob, lam, dtype)
            rel = float((LD(chi) - LD(chi0)) / LD(chi0))
            print(f"{name}: trial {k} lambda {lam:.6g} {np.dtype(dtype).name} chi2 {float(chi0):.6g} -> {float(chi):.6g} "
                  f"({rel:+.3g})")
            assert _decided(chi0, chi, k == trials - 1), (name, k, lam, dtype, chi0, chi)


def test_lambda_at():
    assert [lambda_at(1.0, k) for k in range(6)] == [1.0, 2.0, 8.0, 64.0, 1024.0, 32768.0]
    assert lambda_at(1e-6, 4) == 1e-6 * 1024.0 and lambda_at(3.0, 0) == 3.0


def test_cases_cover_the_paths():
    """What the issue asks the set to hold, as far as the CPU can see it (the
    device path of each case is asserted on the GPU)."""
    assert max(c[3] for c in CASES.values()) >= 4                    # >= 3 rejections somewhere
    assert all(c[3] >= 2 for c in CASES.values())                    # >= 1 rejection everywhere
    assert set(TWO_ITER) <= set(CASES) and len(TWO_ITER) >= 4
    assert any(t2 > 1 for _, t2 in TWO_ITER.values())                # a rejection inside iteration 2
    for name, (t1, _) in TWO_ITER.items():
        assert t1 == CASES[name][3]
    huber = [n for n in CASES if np.any(_problem(n).obs_delta > 0)]
    assert huber and len(huber) < len(CASES)
    for n in huber:   # the kernel is active: edges on both sides of delta at the initial state
        ed = lin_ref.edges(_problem(n), np.float64, jac=False)
        out = ed.chi2 > _problem(n).obs_delta[ed.eid] ** 2
        assert out.any() and not out.all()
    assert any(_problem(n).has_stereo for n in CASES)
    p = _problem("lidar_plain")
    assert p.n_lid == sum(LIDAR.values()) and not np.any(p.pose_fixed[p.lid_pose])
    assert lin_ref.lidar_edges(p, np.float64, jac=False).eid.size == p.n_lid   # all at level 0, all active
    assert any(np.any(_problem(n).obs_delta > 0) for n in TWO_ITER) and any(_problem(n).has_stereo for n in TWO_ITER)


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_rejects_then_accepts(oracle, name):
    make, lam0, env, trials = CASES[name]
    prob = _problem(name)
    assert prob.n_pose <= 60 and prob.n_pt <= 4000
    j = trials - 1
    lam_j = lambda_at(lam0, j)
    og, n, st = _oracle_run(oracle, prob, 1, lam0)
    assert n == 1 and st["trace_trials"] == [trials], st
    # the accepted trial multiplies lambda_j by a factor in [1/3, 2/3] (levenberg.cpp:136-139);
    # float64 multiplication is monotone, so the bounds are exact
    assert lam_j * (1.0 / 3.0) <= st["trace_lambda"][0] <= lam_j * (2.0 / 3.0), (st["trace_lambda"], lam_j)
    # a fresh first trial at lambda_j is accepted, and leaves the lambda the retrial left
    og2, n2, st2 = _oracle_run(oracle, prob, 1, lam_j)
    assert n2 == 1 and st2["trace_trials"] == [1], st2
    assert st2["trace_lambda"][0] == st["trace_lambda"][0] and st2["trace_chi2"][0] == st["trace_chi2"][0]
    _check_margins(oracle, name, prob, lam0, trials)


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_is_well_conditioned(name):
    """The sanity bounds of test_lin_ref.py::test_spreads_and_oracle_chi2 at lambda_j."""
    make, lam0, env, trials = CASES[name]
    lam = lambda_at(lam0, trials - 1)
    sp, ref, f64 = lin_ref.spreads(_problem(name), lam)
    print(f"{name}: lambda_j {lam:.6g} spreads {sp}")
    assert 0 < sp["g"] < 1e-13 and 0 < sp["dl"] and 0 < sp["dx"] < (1e-8 if lam < 1 else 1e-11), sp
    assert np.abs(ref.S @ ref.dx - ref.g).max() <= 1e-17 * np.abs(ref.g).max()


@pytest.mark.parametrize("name", sorted(TWO_ITER))
def test_second_iteration(oracle, name):
    make, lam0, env, trials = CASES[name]
    t1, t2 = TWO_ITER[name]
    prob = _problem(name)
    og1, n1, st1 = _oracle_run(oracle, prob, 1, lam0)
    og, n, st = _oracle_run(oracle, prob, 2, lam0)
    assert n == 2 and st["trace_trials"] == [t1, t2], st
    assert st["trace_chi2"][0] == st1["trace_chi2"][0] and st["trace_lambda"][0] == st1["trace_lambda"][0]
    assert st["trace_chi2"][1] < st["trace_chi2"][0] < st["chi2_begin"]        # both iterations accepted a trial
    lam2 = st["trace_lambda"][0]
    assert lambda_at(lam2, t2 - 1) * (1.0 / 3.0) <= st["trace_lambda"][1] <= lambda_at(lam2, t2 - 1) * (2.0 / 3.0)
    prob1 = state_problem(prob, og1.pose_q, og1.pose_t, og1.pt)
    _check_margins(oracle, name + " it2", prob1, lam2, t2)
    lam = lambda_at(lam2, t2 - 1)
    sp, ref, f64 = lin_ref.spreads(prob1, lam)
    print(f"{name}: iteration 2 lambda {lam:.6g} spreads {sp}")
    assert 0 < sp["g"] < 1e-13 and 0 < sp["dl"] and 0 < sp["dx"] < (1e-8 if lam < 1 else 1e-11), sp
