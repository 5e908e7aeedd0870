"""The problem of tests/test_gpu_retrial_corner.py: the LiDAR window of
tests/retrial_cases.py (lidar_plain's, with N(0, 0.5) on the points, no robust kernel)
with kinds, {pose 39: 150 edges of alternating kind, pose 12: 40 corner edges}.
name -> (builder, lambda_0, environment of the setup, trials of iteration 1),
the layout of retrial_cases.CASES; TWO_ITER name -> (trials of iteration 1,
trials of iteration 2) of optimize(0, 2, lambda_0).

The oracle has no corner edge, so the trial counts are those of the
kind-aware reference (tests/lin_ref_corner.py) driven by g2o's LM rules
(lm_iteration below); tests/test_retrial_ref_corner.py shows on the CPU that
every one of those decisions has a margin of 1e-3. Noise and lambda_0 were
chosen there by scanning sigma 0.3 .. 1 and lambda_0 1e-6 .. 1e-2: sigma 0.5
with lambda_0 = 1e-4 rejects twice (chi2 x 2.3, x 39) and accepts the third
trial (-13 %), and iteration 2 accepts its first (-89 %). lidar_plain's own
sigma 1 rejects as readily, but the state its accepted trial leaves has points
near the cameras: the reference's own spread of g there is 2e-11 (6.8e-13
here), too coarse a yardstick for the second iteration.
"""
import numpy as np

import corner_first_trial_cases as corc
import lin_ref
import lin_ref_corner as LRC
from retrial_cases import LIDAR, _lidar, lambda_at, noisy, state_problem  # noqa: F401

KINDS = {39: lambda j: j % 2 == 1, 12: lambda j: j >= 0}


def _corner_plain():
    return corc.set_kinds(noisy(_lidar, 0.5, False)(), KINDS)


CASES = {"corner_plain": (_corner_plain, 1e-4, {}, 3)}
TWO_ITER = {"corner_plain": (3, 1)}


def trial_state(oracle, prob, lam, dtype=np.float64):
    """(Trial, q, t, X, chi2 there): the state x (+) dx(lam), X + dl(lam) and its chi2 in dtype."""
    tr = LRC.first_trial(prob, lam, dtype)
    q, t = lin_ref.oplus_poses(oracle, prob, tr.free, tr.dx.astype(np.float64))
    X = prob.pt + tr.dl.astype(np.float64)
    return tr, q, t, X, LRC.chi2(prob, q, t, X, dtype)


def lm_iteration(oracle, prob, lam0, max_trials=10):
    """One iteration of g2o's Levenberg loop (levenberg.cpp:88-150) on the
    float64 reference: (trials, state problem after the accepted trial, the
    lambda it leaves, [(lambda, chi2_0, chi2) per trial])."""
    lam, ni, log = float(lam0), 2.0, []
    for k in range(max_trials):
        tr, q, t, X, chi = trial_state(oracle, prob, lam)
        log.append((lam, float(tr.chi2_0), float(chi)))
        # computeScale: sum over every free vertex of dx . (lambda dx + b)
        lms = tr.lms
        scale = float((tr.dx * (lam * tr.dx + tr.bp.reshape(-1))).sum()
                      + (tr.dl[lms] * (lam * tr.dl[lms] + tr.bl)).sum()) + 1e-3
        rho = float(tr.chi2_0 - chi) / scale
        if rho > 0 and np.isfinite(chi):
            alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
            return k + 1, state_problem(prob, q, t, X), lam * max(1.0 / 3.0, alpha), log
        lam *= ni
        ni *= 2.0
    raise AssertionError("no trial accepted")
