"""tests/lin_ref.py (the extended-precision reference of one LM trial) against
the CPU oracle and against itself. No GPU."""
import numpy as np
import pytest

import lin_ref
import lidar_first_trial_cases as lidc
from first_trial_cases import CASES
from sqrtlm import synth

ALL_CASES = {**CASES, **lidc.CASES}

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


def _small_lidar():
    """7 keyframes (2 fixed), LiDAR edges on a fixed pose (inactive), on two
    free ones, some at level 1, in an order not grouped by pose; keyframe 6
    keeps no vision edge at level 0."""
    prob = synth.make_problem(7, 40, k_min=2, k_max=5, seed=3, n_fixed=2)
    lidc.add_lidar(prob, {1: 5, 3: 9, 6: 12}, shuffle_seed=9)
    prob.meta["lid_level"] = (np.arange(prob.n_lid) % 3 == 0).astype(np.uint8)
    prob.obs_level = np.where(prob.obs_pose == 6, 1, prob.obs_level).astype(np.uint8)
    return prob


def _check_full_damped_system(prob, lam, with_lidar):
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
    if with_lidar:
        lid = lin_ref.lidar_edges(prob)
        act = (lin_ref.lidar_level(prob) == 0) & (prob.pose_fixed[prob.lid_pose] == 0)
        assert 0 < act.sum() < prob.n_lid and np.array_equal(lid.eid, np.nonzero(act)[0])
        assert 6 in tr.free and not np.any(ed.pose == 6)              # free through LiDAR alone
        for k in range(lid.eid.size):
            J = np.zeros((1, n), LD)
            J[0, 6 * ph[lid.pose[k]]:6 * ph[lid.pose[k]] + 6] = lid.J[k]
            H += lid.info[k] * (J.T @ J)
            b -= lid.info[k] * (J.T @ lid.e[k:k + 1])
    H[np.arange(n), np.arange(n)] += LD(lam)
    x = np.concatenate([tr.dx, tr.dl[tr.lms].reshape(-1)])
    assert np.abs(H @ x - b).max() <= 1e-16 * np.abs(b).max()
    assert np.abs(tr.S @ tr.dx - tr.g).max() <= 1e-17 * np.abs(tr.g).max()


def test_trial_solves_the_full_damped_system():
    """dx and dl satisfy (J^T W J + lam I) [dx; dl] = -J^T W r assembled densely
    edge by edge: checks the Schur complement, g, the refined solve and the
    back-substitution together, to longdouble rounding."""
    _check_full_damped_system(synth.make_problem(7, 40, k_min=2, k_max=5, seed=3, n_fixed=2), 0.5, False)


def test_trial_solves_the_full_damped_system_with_lidar(oracle):
    """The same identity with the unary LiDAR rows in the dense system."""
    _check_full_damped_system(_small_lidar(), 0.5, True)


def _oracle_trial(oracle, name):
    """(problem, lambda, level, oracle graph after one trial, iterations, stats)."""
    make, lam, _ = ALL_CASES[name]
    prob = make()
    level = lidc.LEVEL.get(name, 0)
    og = oracle.OracleGraph(prob)
    og.lid_level[:] = lin_ref.lidar_level(prob)
    n, st = og.optimize(level, 1, user_lambda=lam)
    return prob, lam, level, og, n, st


@pytest.mark.parametrize("name", sorted(ALL_CASES))
def test_oracle_accepts_first_trial(oracle, name):
    """The condition on the inputs of tests/test_gpu_first_trial.py and
    tests/test_gpu_first_trial_lidar.py."""
    prob, lam, level, og, n, st = _oracle_trial(oracle, name)
    assert prob.n_pose <= 60 and prob.n_pt <= 4000
    if name in CASES:
        assert prob.n_lid == 0
    else:
        assert prob.n_lid > 0 and prob.n_pt <= 3000
    assert n == 1 and st["trace_trials"] == [1], st


@pytest.mark.parametrize("name", ["mid_lam1e-3", "mid_lam1", "mid_lam1e3", "stereo_half", "dups", "fixed_robust",
                                  "border"] + sorted(lidc.CASES))
def test_spreads_and_oracle_chi2(oracle, name):
    """The float64-vs-longdouble spread of every quantity, and the oracle's
    first trace entry against the longdouble chi2 at x (+) dx, X + dl: within
    the spread of that same number between the reference's float64 and
    longdouble evaluations (x 100, floor 4 eps, as the GPU test bounds)."""
    prob, lam, level, og, n, st = _oracle_trial(oracle, name)
    sp, ref, f64 = lin_ref.spreads(prob, lam, level=level)
    has_lm = ref.lms.size > 0
    assert 0 < sp["g"] < 1e-13 and (0 < sp["dl"] or not has_lm) and 0 < sp["dx"] < (1e-8 if lam < 1 else 1e-11), sp
    assert np.abs(ref.S @ ref.dx - ref.g).max() <= 1e-17 * np.abs(ref.g).max()
    chi = {}
    for key, tr in (("hi", ref), ("lo", f64)):
        q, t = lin_ref.oplus_poses(oracle, prob, tr.free, tr.dx.astype(np.float64))
        X = prob.pt + tr.dl.astype(np.float64)
        chi[key] = lin_ref.chi2(prob, q, t, X, LD if key == "hi" else np.float64, level)
    spread = float(abs(LD(chi["lo"]) - chi["hi"]) / chi["hi"])
    err = float(abs(LD(st["trace_chi2"][0]) - chi["hi"]) / chi["hi"])
    print(f"{name}: spreads {sp} chi2 oracle err {err:.2e} spread {spread:.2e}")
    assert err <= 100 * max(spread, 4 * EPS)
    assert float(abs(LD(st["chi2_begin"]) - ref.chi2_0) / ref.chi2_0) <= 100 * max(sp["chi2_0"], 4 * EPS)


@pytest.mark.parametrize("name", sorted(lidc.CASES))
def test_oracle_state_matches_reference(oracle, name):
    """The oracle's points and poses after its first trial against X0 + dl and
    oplus(x, dx) of the longdouble reference, and its chi2 against the
    longdouble chi2 at its own state: each within 100 x max(spread, 4 eps) of
    that quantity, the bound of the GPU test. The oracle differentiates the
    LiDAR error itself, so this is what shows on the CPU that taking the
    float64 Jacobian row as data leaves nothing of its 1e-7 noise in the
    comparison."""
    prob, lam, level, og, n, st = _oracle_trial(oracle, name)
    sp, ref, f64 = lin_ref.spreads(prob, lam, level=level)
    assert lin_ref.lidar_edges(prob, level=level, jac=False).eid.size > 0
    out = {}
    if ref.lms.size:
        dmax = np.abs(ref.dl).max()
        X_hi = prob.pt.astype(LD) + ref.dl
        out["dl"] = (float(np.abs(og.pt - X_hi).max() / dmax), float(np.abs((prob.pt + f64.dl) - X_hi).max() / dmax))
    else:
        assert np.array_equal(og.pt, prob.pt)
    q_hi, t_hi = lin_ref.oplus_poses(oracle, prob, ref.free, ref.dx.astype(np.float64))
    q_lo, t_lo = lin_ref.oplus_poses(oracle, prob, f64.free, f64.dx)
    ts = max(1.0, np.abs(t_hi).max())
    out["pose"] = (max(np.abs(og.pose_q - q_hi).max(), np.abs(og.pose_t - t_hi).max() / ts),
                   max(np.abs(q_lo - q_hi).max(), np.abs(t_lo - t_hi).max() / ts))
    chi_hi, chi_sp = lin_ref.chi2_spread(prob, og.pose_q, og.pose_t, og.pt, level)
    out["chi2"] = (float(abs(LD(st["trace_chi2"][0]) - chi_hi) / chi_hi), chi_sp)
    print(f"{name}: " + " ".join(f"{k} {e / max(s, 4 * EPS):.2g} ({e:.1e}/{s:.1e})" for k, (e, s) in out.items()), sp)
    for k, (e, s) in out.items():
        assert e <= 100 * max(s, 4 * EPS), (name, k, e, s)


def test_lidar_edges_match_oracle_bits(oracle):
    """The reference's float64 LiDAR error is bit-equal to orc_lidar_error per
    edge, the Jacobian row it uses bit-equal to orc_lidar_jacobian, in the
    float64 and the longdouble evaluation alike; the active set is the
    oracle's (level, fixed pose)."""
    prob = lidc.CASES["lid_level"][0]()
    for level in (0, 1):
        lo = lin_ref.lidar_edges(prob, np.float64, level=level)
        hi = lin_ref.lidar_edges(prob, LD, level=level)
        act = (lin_ref.lidar_level(prob) == level) & (prob.pose_fixed[prob.lid_pose] == 0)
        assert np.array_equal(lo.eid, np.nonzero(act)[0]) and 0 < lo.eid.size < prob.n_lid
        assert not np.any(prob.lid_pose[lo.eid] == 0) and np.any(prob.lid_pose == 0)
        assert lo.e.dtype == np.float64 and hi.e.dtype == LD and hi.J.dtype == LD
        for k, e in enumerate(lo.eid):
            p = prob.lid_pose[e]
            a = (prob.pose_q[p], prob.pose_t[p], prob.lid_pc[e], prob.lid_pw[e], prob.lid_n[e])
            assert lo.e[k] == oracle.lidar_error(*a), (e, lo.e[k], oracle.lidar_error(*a))
            J = oracle.lidar_jacobian(*a)
            assert np.array_equal(lo.J[k], J) and np.array_equal(hi.J[k], J.astype(LD))
        assert np.abs(hi.e - lo.e).max() <= 8 * EPS * np.abs(prob.lid_pw).max()


def test_no_lidar_is_unchanged():
    """A problem without LiDAR edges takes none of the LiDAR code: same bits
    whether the arrays are empty or every edge is on another level."""
    prob = synth.make_problem(7, 40, k_min=2, k_max=5, seed=3, n_fixed=2)
    a = lin_ref.first_trial(prob, 0.5, np.float64)
    off = lidc.add_lidar(prob.copy(), {3: 9})
    off.meta["lid_level"] = np.ones(off.n_lid, np.uint8)
    b = lin_ref.first_trial(off, 0.5, np.float64)
    for k in ("free", "lms", "Hpp", "bp", "S", "g", "dx", "dl"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.chi2_0 == b.chi2_0
    assert lin_ref.chi2(prob, dtype=np.float64) == lin_ref.chi2(off, dtype=np.float64)


# ------------------------------------------------------------------ sharded first trial (CPU side)

import sharded_first_trial_cases as shc  # noqa: E402


@pytest.mark.parametrize("name", sorted(shc.LAMBDA0))
def test_lambda_init_matches_oracle(oracle, name):
    """lin_ref.lambda_init against the oracle's computeLambdaInit: the oracle's
    first trial at user_lambda = 0 (its own lambda_0) and at user_lambda =
    float(lambda_init(longdouble)) give the same chi2 within 100 x max(spread,
    4 eps), the spread being that of the trial chi2 between the reference's
    float64 and longdouble evaluations, each with its own lambda_0. The oracle
    accepts that trial, and the largest diagonal entry sits on a pose that at
    least two ranks see at worlds 2 and 3 under the run's owner map."""
    prob = shc.problem(name)
    lam_hi, lam_lo = lin_ref.lambda_init(prob, LD), lin_ref.lambda_init(prob, np.float64)
    assert lam_hi.dtype == LD and float(abs(LD(lam_lo) - lam_hi) / lam_hi) <= 16 * EPS
    st = {}
    for key, lam in (("own", 0.0), ("ref", float(lam_hi))):
        og = oracle.OracleGraph(prob)
        n, st[key] = og.optimize(0, 1, user_lambda=lam)
        assert n == 1 and st[key]["trace_trials"] == [1], st[key]
    sp, ref, f64 = lin_ref.spreads_lambda_init(prob)
    chi = {}
    for key, tr in (("hi", ref), ("lo", f64)):
        q, t = lin_ref.oplus_poses(oracle, prob, tr.free, tr.dx.astype(np.float64))
        chi[key] = lin_ref.chi2(prob, q, t, prob.pt + tr.dl.astype(np.float64), LD if key == "hi" else np.float64)
    spread = float(abs(LD(chi["lo"]) - chi["hi"]) / chi["hi"])
    a, b = LD(st["own"]["trace_chi2"][0]), LD(st["ref"]["trace_chi2"][0])
    print(f"{name}: lambda_0 {float(lam_hi):.17g} chi2 own {float(a):.17g} ref {float(b):.17g} spread {spread:.2e}")
    assert float(abs(a - b) / b) <= 100 * max(spread, 4 * EPS)
    assert float(abs(b - chi["hi"]) / chi["hi"]) <= 100 * max(spread, 4 * EPS)
    # the oracle's lambda after the trial is lambda_0 times a factor in [1/3, 2/3]
    assert 1 / 3 - 1e-12 <= st["own"]["trace_lambda"][0] / float(lam_hi) <= 2 / 3 + 1e-12
    val, kind, pose = lin_ref.max_diagonal(prob)
    assert kind == "pose" and lin_ref.max_diagonal(prob, np.float64)[1:] == (kind, pose)
    for world in shc.WORLDS:
        own = shc.owner_map(name, world)
        assert np.unique(own[prob.obs_pt[prob.obs_pose == pose]]).size >= 2, (name, world, pose)


@pytest.mark.parametrize("name,world", shc.pairs())
def test_shard_geometry(name, world):
    """Every (case, world) of tests/test_gpu_first_trial_sharded.py: at least
    two ranks' row ranges overlap, so k_gather_add sums; the degenerate cases
    have the property they are named for."""
    prob = shc.problem(name)
    rng = [shc.row_range(name, world, r) for r in range(world)]
    locs = [shc.local_problem(name, world, r) for r in range(world)]
    assert sum(loc.n_obs for loc in locs) == prob.n_obs and sum(loc.n_pt for loc in locs) == prob.n_pt
    nP = shc.free_cameras(name).size
    assert nP == lin_ref.first_trial(prob, 1.0, np.float64, shc.level(name), solve=False).free.size
    if name in shc.LIDAR_ONLY:
        # rank 0 alone holds active edges (LiDAR); the others send nothing
        assert rng[0] == (0, nP) and all(r == (0, 0) for r in rng[1:])
        assert all(loc.n_obs > 0 and not np.any(loc.obs_level == shc.level(name)) for loc in locs)
        return
    assert shc.overlapping_ranks(name, world), rng
    if name == "long_red":       # every rank touches every free camera
        assert all(r == (0, nP) for r in rng)
    if name == "fixed_only_rank":
        fo = shc.fixed_only_landmarks(prob)
        own = shc.owner_map(name, world)
        assert fo.any() and np.array_equal(own == 1, fo)
        assert locs[1].n_obs > 0 and np.all(prob.pose_fixed[locs[1].obs_pose] != 0) and rng[1] == (0, 0)
        assert rng[0][1] > rng[0][0] and rng[2][1] > rng[2][0]
    if name == "interleaved":
        assert np.array_equal(shc.owner_map(name, world), np.arange(prob.n_pt) % 3)
        assert all(r == (0, nP) for r in rng)           # every rank spans the whole band
    if name == "empty_rank":
        assert locs[1].n_pt == 0 and locs[1].n_obs == 0 and rng[1] == (0, 0)
        assert locs[0].n_pt > 0 and locs[2].n_pt > 0
