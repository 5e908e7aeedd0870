"""The conditions on the input of tests/test_gpu_retrial_corner.py, on the CPU,
as tests/test_retrial_ref.py shows them for the flat cases: corner_plain takes
its recorded number of trials in both iterations and every one of them is
decided with a margin of 1e-3 (relative chi2, in float64 and in longdouble)
that no rounding crosses. The oracle has no corner edge: the trials are those
of tests/lin_ref_corner.py under g2o's LM rules
(corner_retrial_cases.lm_iteration). Recorded: iteration 1 three trials (chi2
+134 %, +3770 %, -12.6 % at lambda 1e-4, 2e-4, 8e-4), iteration 2 one (-89 %).

The reference must be a usable yardstick at both states: at the initial state
the bounds of tests/test_retrial_ref.py (spread of g below 1e-13, of dx below
1e-8); at the state iteration 1 leaves, where the noisy points have moved, g
below 1e-11 and dx below 1e-8, so that K = 100 spreads stay three orders of
magnitude under the 1e-6 parity bar. No GPU.
"""
import functools

import numpy as np
import pytest

import lin_ref
import lin_ref_corner as LRC
from corner_retrial_cases import CASES, LIDAR, TWO_ITER, lambda_at, lm_iteration, trial_state

LD = lin_ref.LD
MARGIN = 1e-3


@functools.lru_cache(maxsize=None)
def _problem(name):
    return CASES[name][0]()


def _decided(chi0, chi, accepted):
    chi0, chi = LD(chi0), LD(chi)
    if accepted:
        return bool(np.isfinite(chi) and chi < chi0 * (1 - LD(MARGIN)))
    return bool(not np.isfinite(chi) or chi > chi0 * (1 + LD(MARGIN)))


def _check_margins(oracle, name, prob, lam0, trials):
    for k in range(trials):
        lam = lambda_at(lam0, k)
        for dtype in (np.float64, LD):
            tr, q, t, X, chi = trial_state(oracle, prob, lam, dtype)
            rel = float((LD(chi) - LD(tr.chi2_0)) / LD(tr.chi2_0))
            print(f"{name}: trial {k} lambda {lam:.6g} {np.dtype(dtype).name} chi2 {float(tr.chi2_0):.6g} -> "
                  f"{float(chi):.6g} ({rel:+.3g})")
            assert _decided(tr.chi2_0, chi, k == trials - 1), (name, k, lam, dtype, tr.chi2_0, chi)


def test_case_layout():
    p = _problem("corner_plain")
    assert p.n_lid == sum(LIDAR.values()) and not np.any(p.pose_fixed[p.lid_pose]) and not np.any(p.obs_delta > 0)
    k39 = p.lid_kind[p.lid_pose == 39]
    assert k39.size == 150 and np.array_equal(k39, np.arange(150) % 2)       # mixed: every wave diverges
    assert p.lid_kind[p.lid_pose == 12].all() and (p.lid_pose == 12).sum() == 40
    assert LRC.lidar_edges(p, np.float64, jac=False).eid.size == p.n_lid     # all at level 0, all active
    assert p.n_pose <= 60 and p.n_pt <= 4000


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_rejects_then_accepts(oracle, name):
    make, lam0, env, trials = CASES[name]
    t1, t2 = TWO_ITER[name]
    prob = _problem(name)
    n1, prob1, lam2, log1 = lm_iteration(oracle, prob, lam0)
    assert n1 == trials == t1, log1
    assert [l for l, _, _ in log1] == [lambda_at(lam0, k) for k in range(trials)]
    lam_j = lambda_at(lam0, trials - 1)
    assert lam_j * (1.0 / 3.0) <= lam2 <= lam_j * (2.0 / 3.0)
    _check_margins(oracle, name, prob, lam0, trials)
    # a fresh first trial at lambda_j is accepted and leaves the same state and lambda
    m, prob1b, lam2b, _ = lm_iteration(oracle, prob, lam_j)
    assert m == 1 and lam2b == lam2 and np.array_equal(prob1b.pt, prob1.pt) and np.array_equal(prob1b.pose_t, prob1.pose_t)
    # iteration 2 from the state and the lambda iteration 1 left
    n2, _, lam3, log2 = lm_iteration(oracle, prob1, lam2)
    assert n2 == t2, log2
    _check_margins(oracle, name + " it2", prob1, lam2, t2)
    for p_, lam, g_max in ((prob, lam_j, 1e-13), (prob1, lambda_at(lam2, t2 - 1), 1e-11)):
        sp, ref, f64 = LRC.spreads(p_, lam)
        print(f"{name}: lambda {lam:.6g} spreads {sp}")
        assert 0 < sp["g"] < g_max and 0 < sp["dl"] and 0 < sp["dx"] < 1e-8, sp
        assert np.abs(ref.S @ ref.dx - ref.g).max() <= 1e-17 * np.abs(ref.g).max()
