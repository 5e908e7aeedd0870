"""tests/lin_ref.py (the extended-precision reference of one LM trial) against
the CPU oracle and against itself. No GPU."""
import numpy as np
import pytest

import lin_ref
from first_trial_cases import CASES
from sqrtlm import synth

EPS = float(np.finfo(np.float64).eps)
LD = lin_ref.LD


@pytest.fixture(scope="module")
def stereo_prob():
    return CASES["stereo_half"][0]()


def test_edges_match_oracle_float64(oracle, stereo_prob):
    """Residuals and Jacobians, evaluated in float64, against the oracle's
    per-edge functions: the same formulas in the same order, so a few ulps of
    the largest term (the projection for r, the row's largest entry for J)."""
    prob = stereo_prob
    ed = lin_ref.edges(prob, np.float64)
    og = oracle.OracleGraph(prob)
    og.compute_errors()
    r_or = np.concatenate([og.obs_err, og.obs_err3[:, None]], axis=1)
    r_or[~ed.stereo, 2] = 0.0
    scale = np.abs(ed.proj).max(axis=1, keepdims=True)
    assert np.all(np.abs(ed.r - r_or) <= 4 * EPS * scale)
    assert ed.stereo.any() and (~ed.stereo).any()
    for e in np.r_[np.nonzero(ed.stereo)[0][:150], np.nonzero(~ed.stereo)[0][:150]]:
        p, l = prob.obs_pose[e], prob.obs_pt[e]
        a = (prob.pose_q[p], prob.pose_t[p], prob.intr[p])
        if ed.stereo[e]:
            Jl, Jp = oracle.stereo_jacobians(*a, prob.pose_bf[p], prob.pt[l])
            pr = oracle.stereo_project(*a, prob.pose_bf[p], prob.pt[l])
            assert np.all(np.abs(ed.proj[e] - pr) <= 4 * EPS * np.abs(pr).max())
            nr = 3
        else:
            Jl, Jp = oracle.mono_jacobians(*a, prob.pt[l])
            nr = 2
            assert not ed.Jl[e, 2].any() and not ed.Jp[e, 2].any()
        for mine, ref in ((ed.Jl[e, :nr], Jl), (ed.Jp[e, :nr], Jp)):
            assert np.all(np.abs(mine - ref) <= 4 * EPS * np.abs(ref).max(axis=1, keepdims=True)), (e, mine, ref)


def test_mono_jacobians_are_derivatives(oracle, stereo_prob):
    """J_p against central differences of the longdouble residual through the
    oracle's oplus (T <- exp(d) T, d = [omega; upsilon]), J_l through X + d:
    h = 1e-6 leaves h^2 truncation and eps64 / h from the float64 oplus, both
    << 1e-7. Mono edges only: a stereo projection multiplies by a float32
    invz, a step function at this h (its Jacobian is checked against the
    oracle's above)."""
    prob = stereo_prob
    ed = lin_ref.edges(prob)
    h = 1e-6
    pick = np.nonzero(~ed.stereo)[0][:6]
    scale = np.abs(ed.Jp[pick]).max()
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        rs = []
        for sgn in (1.0, -1.0):
            q, t = prob.pose_q.copy(), prob.pose_t.copy()
            for p in set(prob.obs_pose[pick]):
                q[p], t[p] = oracle.se3_oplus(q[p], t[p], sgn * d)
            rs.append(lin_ref.edges(prob, LD, q, t, jac=False).r[pick])
        num = (rs[0] - rs[1]) / (2 * LD(h))
        assert np.abs(num - ed.Jp[pick][:, :, k]).max() <= 1e-7 * scale
    for k in range(3):
        rs = []
        for sgn in (1.0, -1.0):
            X = prob.pt.copy()
            X[:, k] += sgn * h
            rs.append(lin_ref.edges(prob, LD, pt=X, jac=False).r[pick])
        num = (rs[0] - rs[1]) / (2 * LD(h))
        assert np.abs(num - ed.Jl[pick][:, :, k]).max() <= 1e-7 * scale


def test_trial_solves_the_full_damped_system():
    """dx and dl satisfy (J^T W J + lam I) [dx; dl] = -J^T W r assembled densely
    edge by edge: checks the Schur complement, g, the refined solve and the
    back-substitution together, to longdouble rounding."""
    prob = synth.make_problem(7, 40, k_min=2, k_max=5, seed=3, n_fixed=2)
    lam = 0.5
    tr = lin_ref.first_trial(prob, lam)
    ed = lin_ref.edges(prob)
    nP, nL = tr.free.size, tr.lms.size
    ph = -np.ones(prob.n_pose, int)
    ph[tr.free] = np.arange(nP)
    lh = -np.ones(prob.n_pt, int)
    lh[tr.lms] = np.arange(nL)
    n = 6 * nP + 3 * nL
    H, b = np.zeros((n, n), LD), np.zeros(n, LD)
    for e in range(ed.eid.size):
        J = np.zeros((3, n), LD)
        if ph[ed.pose[e]] >= 0:
            J[:, 6 * ph[ed.pose[e]]:6 * ph[ed.pose[e]] + 6] = ed.Jp[e]
        c = 6 * nP + 3 * lh[ed.pt[e]]
        J[:, c:c + 3] = ed.Jl[e]
        H += ed.w[e] * (J.T @ J)
        b -= ed.w[e] * (J.T @ ed.r[e])
    H[np.arange(n), np.arange(n)] += LD(lam)
    x = np.concatenate([tr.dx, tr.dl[tr.lms].reshape(-1)])
    assert np.abs(H @ x - b).max() <= 1e-16 * np.abs(b).max()
    assert np.abs(tr.S @ tr.dx - tr.g).max() <= 1e-17 * np.abs(tr.g).max()


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_accepts_first_trial(oracle, name):
    """The condition on the inputs of tests/test_gpu_first_trial.py."""
    make, lam, _ = CASES[name]
    prob = make()
    assert prob.n_pose <= 60 and prob.n_pt <= 4000 and prob.n_lid == 0
    n, st = oracle.OracleGraph(prob).optimize(0, 1, user_lambda=lam)
    assert n == 1 and st["trace_trials"] == [1], st


@pytest.mark.parametrize("name", ["mid_lam1e-3", "mid_lam1", "mid_lam1e3", "stereo_half", "dups", "fixed_robust",
                                  "border"])
def test_spreads_and_oracle_chi2(oracle, name):
    """The float64-vs-longdouble spread of every quantity, and the oracle's
    first trace entry against the longdouble chi2 at x (+) dx, X + dl: within
    the spread of that same number between the reference's float64 and
    longdouble evaluations (x 100, floor 4 eps, as the GPU test bounds)."""
    make, lam, _ = CASES[name]
    prob = make()
    sp, ref, f64 = lin_ref.spreads(prob, lam)
    assert 0 < sp["g"] < 1e-13 and 0 < sp["dl"] and 0 < sp["dx"] < (1e-8 if lam < 1 else 1e-11), sp
    assert np.abs(ref.S @ ref.dx - ref.g).max() <= 1e-17 * np.abs(ref.g).max()
    chi = {}
    for key, tr in (("hi", ref), ("lo", f64)):
        q, t = lin_ref.oplus_poses(oracle, prob, tr.free, tr.dx.astype(np.float64))
        X = prob.pt + tr.dl.astype(np.float64)
        chi[key] = lin_ref.chi2(prob, q, t, X, LD if key == "hi" else np.float64)
    spread = float(abs(LD(chi["lo"]) - chi["hi"]) / chi["hi"])
    n, st = oracle.OracleGraph(prob).optimize(0, 1, user_lambda=lam)
    err = float(abs(LD(st["trace_chi2"][0]) - chi["hi"]) / chi["hi"])
    print(f"{name}: spreads {sp} chi2 oracle err {err:.2e} spread {spread:.2e}")
    assert err <= 100 * max(spread, 4 * EPS)
    assert float(abs(LD(st["chi2_begin"]) - ref.chi2_0) / ref.chi2_0) <= 100 * max(sp["chi2_0"], 4 * EPS)
