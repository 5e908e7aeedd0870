"""Conditions on the Sim3-alignment cases (tests/sim3_cases.py), asserted on the
numpy reference (tests/sim3_ref.py) alone: what tests/test_gpu_sim3.py relies
on when it holds the GPU to that reference. No GPU needed."""
import numpy as np
import pytest

import sim3_cases as SC
import sim3_ref as R
from sqrtlm import synth

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
# caps on the reference's own float64-vs-longdouble spread (relative to the
# largest entry), e and J given as data. b is a sum of 4 n products of O(1e3)
# Jacobian entries with weighted residuals: pairwise summation keeps its
# rounding within a few eps of the largest term, 64 eps leaves room for the
# cancellation between pairs. dx adds the conditioning of the damped 7x7
# system: rotation and translation columns differ by ~1e3 in scale, so
# cond(H + lambda I) up to ~1e8 for well-posed cases (n >= 9 pairs); 1e-10 keeps
# K x spread (K = 100) at 1e-8, far below any modelling error.
CAP_B, CAP_DX = 64 * EPS, 1e-10
WELL_POSED = [n for n in SC.NAMES if SC.SPECS[n][0] >= 9]


def test_noise_free_data_returns_the_true_sim3(oracle):
    for fix in (False, True):
        p = synth.make_sim3_problem(60, seed=5, pixel_noise=0.0, outlier_frac=0.0, fix_scale=fix)
        # keypoints are float32 values: compare at that rounding (1e-5 px of 700 px focal length)
        r = R.optimize(oracle, p)
        assert r["n_inliers"] == 60 and r["n_bad"] == 0
        np.testing.assert_allclose(r["S12_out"], p.meta["S12_true"], atol=2e-6)
        if fix:
            assert r["S12_out"][7] == p.S12[7]


@pytest.mark.parametrize("name", SC.NAMES)
def test_threshold_margin(oracle, name):
    """Every chi2 either threshold test reads lies outside [th2/2, 2 th2]."""
    p, r = SC.problem(name), SC.reference(oracle, name)
    c = np.asarray(r["pair_chi2"], np.float64)
    read = np.concatenate([c[:, 0].ravel(), c[r["pair_state"] != 1, 1].ravel()])
    near = read[(read >= p.th2 / 2) & (read <= 2 * p.th2)]
    assert near.size == 0, near
    dS, dchi, same = SC.ulp_spread(oracle, name)
    assert same, "a one-ulp change of the start changes a decision"
    assert dS < 1e-7, dS


def test_case_list_covers_the_schedule(oracle):
    refs = {n: SC.reference(oracle, n) for n in SC.NAMES}
    stages = [s for r in refs.values() for s in r["stats"]]
    assert any(max(s["trace_trials"], default=0) >= 2 for s in stages), "no iteration with >= 2 trials"
    assert any(s["raul"] for s in stages), "no stage ended by Raul's criterion"
    assert any(s["trace_last_accepted"] and not s["trace_last_accepted"][-1] for s in stages), \
        "no stage whose last trial was rejected"
    clean = [r for r in refs.values() if len(r["stats"]) == 2 and r["n_bad"] == 0]
    assert clean and all(r["stats"][1]["iterations"] <= 5 for r in clean), "no nBad = 0 problem"
    assert any(len(r["stats"]) == 2 and r["n_bad"] > 0 for r in refs.values()), "no nBad > 0 problem"
    short = [n for n, r in refs.items() if SC.SPECS[n][0] > 0 and len(r["stats"]) == 1]
    assert short, "no problem left with fewer than 10 pairs"
    assert any(refs[n]["n_bad"] > 0 for n in short), "no problem that drops below 10 pairs by outlier removal"
    for n in short:
        assert refs[n]["n_inliers"] == 0 and np.array_equal(refs[n]["S12_out"], SC.problem(n).S12)
    assert any(SC.problem(n).fix_scale for n in SC.NAMES) and any(not SC.problem(n).fix_scale for n in SC.NAMES)
    assert any(not np.array_equal(SC.problem(n).intr1, SC.problem(n).intr2) for n in SC.NAMES)
    assert sorted(SC.SPECS[n][0] for n in SC.NAMES) == [0, 1, 9, 10, 11, 63, 64, 65, 255, 256, 257, 600]


@pytest.mark.parametrize("name", WELL_POSED)
def test_reference_spreads_are_small(oracle, name):
    """float64 against longdouble, e and J as data: b and dx of the first trial."""
    p, r = SC.problem(name), SC.reference(oracle, name)
    e, J = r["lin"][0], r["lin"][1]
    info = np.stack([p.info1, p.info2], axis=1)
    delta, act = R.huber_delta(p.th2), np.ones(p.n_pair, bool)
    H, b, _ = R.assemble(e, J, info, delta, act)
    HL, bL, _ = R.assemble(e, J, info, delta, act, LD)
    assert float(np.abs(b - bL).max() / np.abs(bL).max()) <= CAP_B
    for lam in (1e-3, 1.0, 1e3):
        ok, dx = R.solve7(H, b, lam)
        okL, dxL = R.solve7(HL, bL, lam, LD)
        assert ok and okL
        assert float(np.abs(dx - dxL).max() / np.abs(dxL).max()) <= CAP_DX, lam


def test_fix_scale_column_is_zero(oracle):
    p, r = SC.problem("n63_fix"), SC.reference(oracle, "n63_fix")
    assert p.fix_scale and np.all(r["lin"][1][..., 6] == 0.0)
    assert r["S12_out"][7] == p.S12[7]


def test_generator_shapes():
    p = synth.make_sim3_problem(33, seed=1, intr2=SC.K2)
    assert p.n_pair == 33 and p.X1c.shape == (33, 3) and p.obs2.shape == (33, 2) and p.matched.all()
    assert np.array_equal(p.obs1, p.obs1.astype(np.float32)) and p.th2 == 10.0
    assert not np.array_equal(p.intr1, p.intr2)
    assert synth.make_sim3_problem(0).n_pair == 0
