"""Conditions on the motion-only-BA cases (tests/pose_cases.py), asserted on the
numpy reference (tests/pose_ref.py) alone: what tests/test_gpu_pose.py relies on
when it holds the GPU to that reference. No GPU needed."""
import numpy as np
import pytest

import pose_cases as SC
import pose_ref as R
from sqrtlm import pose as P
from sqrtlm import synth

LD = np.longdouble


def _read(r):
    """The chi2 values the checks that ran read (zeros: nothing was computed yet)."""
    c = np.asarray(r["edge_chi2"], np.float64)
    return c[:, list(range(r["rounds"])) + [4]].ravel()


def _near(v, th2, f):
    return v[(v >= th2 / f) & (v <= f * th2)]


# ---- the arithmetic against the oracle's primitives ---------------------------------
def test_mono_error_and_jacobian_match_the_oracle(oracle):
    p = SC.problem("n65_clean")
    q, t = p.pose_q, p.pose_t
    xc, e = R.mono_error(q, t, p.intr, p.Xw, p.uv)
    J = R.mono_jacobian(xc, p.intr)
    for i in range(0, p.n_obs, 7):
        r = oracle.quat_rotate(q, p.Xw[i]) + t
        assert np.array_equal(r, xc[i])
        _, Jp = oracle.mono_jacobians(q, t, p.intr, p.Xw[i])  # x/z where the pose-only edge has x * (1/z)
        np.testing.assert_allclose(J[i], Jp, rtol=1e-13, atol=1e-9)
    assert np.all(J[:, 0, 4] == 0) and np.all(J[:, 1, 3] == 0)
    # J is the derivative of e through oplus
    h = 1e-6
    for d in range(6):
        u = np.zeros(6)
        u[d] = h
        ep = R.mono_error(*oracle.se3_oplus(q, t, u), p.intr, p.Xw, p.uv)[1]
        em = R.mono_error(*oracle.se3_oplus(q, t, -u), p.intr, p.Xw, p.uv)[1]
        np.testing.assert_allclose((ep - em) / (2 * h), J[:, :, d], rtol=1e-5, atol=1e-4)


def test_lidar_errors_and_jacobians_match_the_oracle(oracle):
    p = SC.problem("n63")
    L = P.make_lidar_pairs(p, 40, seed=3, kinds="mixed")
    assert set(L.kind.tolist()) == {0, 1}
    q, t = p.pose_q, p.pose_t
    e, J = R.lidar_linearization(q, t, R.perturbed(oracle, q, t), L)
    for i in range(L.n_lid):
        d = oracle.quat_rotate(q, L.pw[i]) + t - L.pc[i]
        if L.kind[i] == 0:
            assert e[i] == oracle.lidar_error(q, t, L.pc[i], L.pw[i], L.n[i])
            assert np.array_equal(J[i], oracle.lidar_jacobian(q, t, L.pc[i], L.pw[i], L.n[i]))
        else:
            assert e[i] == np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            assert abs(e[i] - np.linalg.norm(d)) <= 4 * np.finfo(float).eps * e[i]


def test_noise_free_data_returns_the_true_pose(oracle):
    p = synth.make_pose_problem(60, seed=5, pixel_noise=0.0, outlier_frac=0.0)
    r = R.optimize(oracle, p)
    assert r["n_inliers"] == 60 and r["rounds"] == 4 and r["n_bad"] == [0, 0, 0, 0]
    # keypoints are float32 values: 1e-5 px of a 700 px focal length
    np.testing.assert_allclose(r["pose_q"], p.meta["q_true"], atol=2e-6)
    np.testing.assert_allclose(r["pose_t"], p.meta["t_true"], atol=2e-5)


# ---- margins -----------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.NAMES)
def test_threshold_margin(oracle, name):
    """Every chi2 a check reads lies outside [th2/2, 2 th2] (re-entry cases: [th2/1.05, 1.05 th2])."""
    p, r = SC.problem(name), SC.reference(oracle, name)
    f = 1.05 if name in SC.REENTRY else 2.0
    near = _near(_read(r), p.th2, f)
    assert near.size == 0, near
    dS, dchi, same, _ = SC.ulp_spread(oracle, name)
    assert same, "a one-ulp change of the input translation changes a decision"
    assert dS < 1e-7, dS


@pytest.mark.parametrize("name", SC.LIDAR_NAMES)
def test_lidar_threshold_margin(oracle, name):
    sub, L, oin, rob = SC.lidar_problem(oracle, name)
    r = SC.lidar_reference(oracle, name)
    near = _near(np.asarray(r["edge_chi2"][:, 4], np.float64), sub.th2, 2.0)
    assert near.size == 0, near
    dS, dchi, same, _ = SC.lidar_ulp_spread(oracle, name)
    assert same and dS < 1e-7, (same, dS)


# ---- branches ----------------------------------------------------------------------
def test_case_list_covers_the_schedule(oracle):
    refs = {n: SC.reference(oracle, n) for n in SC.NAMES}
    assert sorted(SC.SPECS[n][0] for n in SC.MAIN if n != "n12_stuck") == [0, 2, 3, 9, 10, 11, 63, 64, 65, 255, 256,
                                                                            257, 600]
    # fewer than 3: nothing runs, the pose is the input, no flag
    for n in ("n0", "n2"):
        r, p = refs[n], SC.problem(n)
        assert r["rounds"] == 0 and r["n_inliers"] == 0 and not r["outlier"].any()
        assert np.array_equal(r["pose_q"], p.pose_q) and np.array_equal(r["pose_t"], p.pose_t)
    # fewer than 10: round 0 only
    for n in ("n3", "n9"):
        assert refs[n]["rounds"] == 1 and refs[n]["stats"][1] is None and refs[n]["stats"][0]["ran"]
    for n in ("n10_clean", "n11_out"):
        assert refs[n]["rounds"] == 4 and refs[n]["stats"][3]["ran"]
    # re-entry: an edge on level 1 after one round is back on level 0 after the next
    for n in SC.REENTRY:
        lv = refs[n]["levels"]
        assert any((a & ~b).any() for a, b in zip(lv, lv[1:])), n
        assert refs[n]["n_bad"][0] > refs[n]["n_bad"][1]
    # a round with no level-0 edge runs no trial; its check evaluates every edge at the input pose
    r, p = refs["n12_stuck"], SC.problem("n12_stuck")
    assert r["n_bad"] == [12, 12, 12, 12] and r["n_inliers"] == 0
    assert [s["ran"] for s in r["stats"][:4]] == [True, False, False, False]
    assert all(s["active"] == 0 and s["trials"] == 0 for s in r["stats"][1:4])
    assert np.array_equal(r["pose_q"], p.pose_q) and np.array_equal(r["pose_t"], p.pose_t)
    assert np.array_equal(r["edge_chi2"][:, 3], R.mono_chi2(p.pose_q, p.pose_t, p))
    stages = [s for r in refs.values() for s in r["stats"] if s is not None and s["ran"]]
    assert any(max(s["trace_trials"], default=0) >= 2 for s in stages), "no iteration with >= 2 trials"
    assert any(s["trace_last_accepted"] and not s["trace_last_accepted"][-1] for s in stages), \
        "no stage whose last trial was rejected: the stale errors would equal the fresh ones"
    assert any(r["n_bad_final"] > 0 for r in refs.values()) and any(
        r["n_bad_final"] == 0 and r["rounds"] == 4 for r in refs.values())
    assert any(not np.array_equal(SC.problem(n).intr, SC.problem("n63").intr) for n in SC.NAMES)


def test_lidar_case_list(oracle):
    got = {n: SC.lidar_problem(oracle, n) for n in SC.LIDAR_NAMES}
    assert sorted(L.n_lid for _, L, _, _ in got.values()) == [0, 1, 64, 64, 64, 257, 700]
    kinds = [set(L.kind.tolist()) for _, L, _, _ in got.values() if L.n_lid > 1]
    assert {0} in kinds and {1} in kinds and {0, 1} in kinds
    assert got["l64_flat_robust"][3] and got["l64_flat_robust"][0].n_obs == 9
    assert got["l64_mixed_allout"][2].all()
    r = SC.lidar_reference(oracle, "l64_mixed_allout")
    assert r["stats"][4]["active"] == 64 and r["stats"][4]["ran"]  # LiDAR edges only
    r = SC.lidar_reference(oracle, "l700_mixed")
    assert r["stats"][4]["active"] == 700 + int((~got["l700_mixed"][2]).sum())


def test_float_and_double_threshold_rules():
    """(float)chi2 > (float)th2 in the rounds, (double)(float)chi2 > th2 at the end:
    5.991f is above 5.991, so a chi2 that rounds to 5.991f is an inlier in a
    round and an outlier in the final classification."""
    p = synth.make_pose_problem(4, seed=1)
    th2 = p.th2
    for chi, rnd, fin in ((5.9910001, False, True), (5.99, False, False), (5.9911, True, True), (np.nan, False, False)):
        for final, want in ((False, rnd), (True, fin)):
            level = np.ones(4, bool)
            err = np.full(4, chi)
            # level-1 edges would be recomputed: mark them level 0 so the stored value is read
            level[:] = False
            R._check(p, p.pose_q, p.pose_t, level, err, th2, final, np.float64)
            assert level.tolist() == [want] * 4, (chi, final)
    assert R.huber_delta(5.991) == float(np.float32(np.sqrt(5.991)))


def test_generator_shapes():
    p = synth.make_pose_problem(33, seed=1, intr=SC.K2)
    assert isinstance(p, P.PoseProblem) and p.n_obs == 33 and p.Xw.shape == (33, 3) and p.uv.shape == (33, 2)
    for a in (p.Xw, p.uv, p.info, p.intr):
        assert np.array_equal(a, a.astype(np.float32))
    assert set(np.unique(p.info)) <= set(synth.orb_inv_level_sigma2(8).astype(np.float64))
    assert p.th2 == 5.991 and not p.outlier.any()
    assert synth.make_pose_problem(0).n_obs == 0
