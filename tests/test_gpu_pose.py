"""sqlm_pose_optimize / sqlm_pose_refine_lidar (batched GPU PoseOptimization)
against the numpy reference tests/pose_ref.py on the cases of
tests/pose_cases.py.

Tolerances. Linearization and first trial: K x the reference's own
float64-vs-longdouble spread of that quantity on that problem, floored at
4 eps, K = 100 -- the rule and constant of tests/test_gpu_first_trial.py and
tests/test_gpu_sim3.py. Errors are relative to the quantity's largest entry.
Whole schedule: n_inliers, n_bad[], rounds, the flags and the over-threshold
pattern of every check identical (test_pose_ref.py asserts the margin that
makes this a fair demand); the pose and each stage's first and final chi2
within max(1e-6, 10 x the reference's spread under a one-ulp perturbation of
the input translation), chi2 relative to max(1, chi2). Trial and iteration
counts are printed, not asserted: acceptances at the noise floor may
legitimately differ.

Ratios (GPU error / spread) measured on an MI355X when the test was written:

  linearization, 13 vision and 7 LiDAR cases: mono e 1.0, J 0.37, LiDAR e 1.0,
  J 1.0 -- every e and J is bit-equal to the float64 reference (the error IS
  the spread, or both are under the 4 eps floor);
  first trial (vision: n9, n65_clean, n255_o35, n600_o35; LiDAR: l64_corner,
  l257_mixed, l64_flat_robust, l64_mixed_allout; lambda 1e-3, 1, 1e3), largest
  over the 24 runs: H 0.22, b 0.81, dx 8.4, pose 0.16, chi2_begin 0.20,
  edge_chi2 1.00, chi2_after 1.05, level-1 chi2 1.00;
  whole schedule: flags, counts, rounds and over-threshold patterns identical
  on all 16 vision and 7 LiDAR cases; pose off by at most 1.1e-11 on the vision
  cases and 9.7e-9 on l64_mixed_allout (whose one-ulp spread is 5.3e-9), stage
  chi2 by at most 1.4e-10 relative; trial counts differ from the reference's
  on 10 vision cases (converged rounds) and on no LiDAR case.

A deliberately wrong scratch build (rounds 1-3 start from the previous round's
estimate instead of the input pose; nothing of it is committed) fails
test_schedule on all 11 cases with at least 10 edges, the two re-entry cases
among them: the first chi2 of round 1 is off by 0.92 ... 0.998 relative, which
is why chi2_begin is asserted beside chi2_end (flags and the final pose alone
survive that bug, the rounds converge to the same optimum). It also fails
test_first_trial on 9 of 12 (after rounds without iterations the pose is not
the input pose); the linearization, LiDAR, batch and facade tests still pass.
"""
import numpy as np
import pytest

import pose_cases as SC
import pose_ref as R
from sqrtlm import pose as P
from sqrtlm.optimizer import Context, Optimizer

pytestmark = pytest.mark.gpu

K = 100.0
LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
FLOOR = 4 * EPS
RUNNING = [n for n in SC.NAMES if SC.SPECS[n][0] >= 3]
FIRST = ["n9", "n65_clean", "n255_o35", "n600_o35"]
LID_FIRST = ["l64_corner", "l257_mixed", "l64_flat_robust", "l64_mixed_allout"]

_runs: dict = {}


def _maxrel(a, b):
    a, b = np.asarray(a, LD), np.asarray(b, LD)
    if b.size == 0:
        return 0.0
    s = np.abs(b).max()
    return float(np.abs(a - b).max() / (s if s > 0 else 1))


def _rel(a, b):
    return abs(float(LD(a) - LD(b)) / float(b))


def _ratio(label, err, spread, out=None):
    r = err / max(spread, FLOOR)
    print(f"  {label}: err {err:.3e} spread {spread:.3e} ratio {r:.3g}")
    if out is not None:
        out[label] = r
    return r


def _pose(q, t):
    return np.concatenate([np.asarray(q, np.float64), np.asarray(t, np.float64)])


def _collect(ctx, res, n_obs, want_step):
    q, t, n_in, flag, st = res
    run = dict(q=q[0], t=t[0], n_in=int(n_in[0]), flag=flag, st=st[0], chi2=ctx.pose_edge_chi2())
    run["e"], run["J"], run["le"], run["lJ"] = ctx.pose_linearization()
    if want_step:
        run["H"], run["b"], run["dx"] = ctx.pose_last_step(0)
    return run


def run_alone(ctx, name, iters=None, user_lambda=None):
    """The vision case alone on the GPU (once per argument set), with all introspection."""
    it, lam = SC.args(name)
    it = it if iters is None else tuple(iters)
    lam = lam if user_lambda is None else float(user_lambda)
    key = (name, it, lam)
    if key not in _runs:
        p = SC.problem(name)
        _runs[key] = _collect(ctx, ctx.pose_optimize([p], it, lam), p.n_obs, p.n_obs >= 3 and it[0] > 0)
    return _runs[key]


def run_lidar_alone(ctx, oracle, name, iters=10, user_lambda=0.0):
    key = ("lidar", name, int(iters), float(user_lambda))
    if key not in _runs:
        sub, L, oin, rob = SC.lidar_problem(oracle, name)
        _runs[key] = _collect(ctx, ctx.pose_refine_lidar([sub], [L], oin, [rob], iters, user_lambda), sub.n_obs, True)
    return _runs[key]


# ---- 1. linearization ---------------------------------------------------------
def _check_mono_lin(p, run, lin64):
    xcL, eL = R.mono_error(p.pose_q, p.pose_t, p.intr, p.Xw, p.uv, LD)
    JL = R.mono_jacobian(xcL, p.intr, LD)
    e64, J64 = lin64[0], lin64[1]
    re_ = _ratio("e", _maxrel(run["e"], eL), _maxrel(e64, eL))
    rJ = _ratio("J", _maxrel(run["J"], JL), _maxrel(J64, JL))
    print(f"  bit-equal to the float64 reference: e {np.array_equal(run['e'], e64)} J {np.array_equal(run['J'], J64)}")
    assert re_ <= K and rJ <= K


@pytest.mark.parametrize("name", RUNNING)
def test_linearization(gpu_ctx, oracle, name):
    p, ref = SC.problem(name), SC.reference(oracle, name)
    print(name)
    _check_mono_lin(p, run_alone(gpu_ctx, name), ref["lin"])


@pytest.mark.parametrize("name", SC.LIDAR_NAMES)
def test_lidar_linearization(gpu_ctx, oracle, name):
    sub, L, oin, rob = SC.lidar_problem(oracle, name)
    ref, run = SC.lidar_reference(oracle, name), run_lidar_alone(gpu_ctx, oracle, name)
    print(name)
    _check_mono_lin(sub, run, ref["lin"])  # every mono edge, the level-1 ones too
    if L.n_lid == 0:
        assert run["le"].size == 0
        return
    le64, lJ64 = ref["lin"][2]
    leL, lJL = R.lidar_linearization(sub.pose_q, sub.pose_t, R.perturbed(oracle, sub.pose_q, sub.pose_t), L, LD)
    re_ = _ratio("lidar e", _maxrel(run["le"], leL), _maxrel(le64, leL))
    rJ = _ratio("lidar J", _maxrel(run["lJ"], lJL), _maxrel(lJ64, lJL))
    print(f"  bit-equal to the float64 reference: e {np.array_equal(run['le'], le64)} J {np.array_equal(run['lJ'], lJ64)}")
    assert re_ <= K and rJ <= K


# ---- 2. first trial -----------------------------------------------------------
def _first_trial(oracle, p, run, stage, lam, active, robust, L, col, must_accept):
    """H, b, dx, the updated pose, chi2_begin, the per-edge chi2 and the chi2
    after the trial of a run of one iteration with one trial, fed the GPU's own e and J."""
    st = run["st"]
    assert st["iterations"][stage] == 1 and st["trials"][stage] == 1
    delta = R.huber_delta(p.th2)
    e, J = run["e"], run["J"]  # pinned by the linearization tests
    lid = None if L is None else (run["le"], run["lJ"], L.info)
    out = {}
    HL, bL, chiL = R.assemble(e, J, p.info, active, robust, delta, lid, LD)
    H6, b6, chi6 = R.assemble(e, J, p.info, active, robust, delta, lid)
    _ratio("H", _maxrel(run["H"], HL), _maxrel(H6, HL), out)
    _ratio("b", _maxrel(run["b"], bL), _maxrel(b6, bL), out)
    okL, dxL = R.solve6(HL, bL, lam, LD)
    ok6, dx6 = R.solve6(H6, b6, lam)
    assert okL and ok6
    _ratio("dx", _maxrel(run["dx"], dxL), _maxrel(dx6, dxL), out)
    _ratio("chi2_begin", _rel(st["chi2_begin"][stage], chiL), _rel(chi6, chiL), out)
    # the updated pose: oplus in the oracle's float64 arithmetic
    S_hi = _pose(*oracle.se3_oplus(p.pose_q, p.pose_t, np.asarray(dxL, np.float64)))
    S_lo = _pose(*oracle.se3_oplus(p.pose_q, p.pose_t, dx6))
    qg, tg = oracle.se3_oplus(p.pose_q, p.pose_t, run["dx"])
    _ratio("pose", _maxrel(_pose(qg, tg), S_hi), _maxrel(S_lo, S_hi), out)
    accepted = st["chi2_end"][stage] < st["chi2_begin"][stage]
    assert accepted or not must_accept
    # per-edge chi2 of the level-0 edges (read at the trial state) and the robust chi2 after the trial
    cL, c6 = R.mono_chi2(qg, tg, p, LD), R.mono_chi2(qg, tg, p)
    _ratio("edge_chi2", _maxrel(run["chi2"][active, col], cL[active]), _maxrel(c6[active], cL[active]), out)
    newL, new6 = R.robust_sum(cL[active], robust, delta, LD), R.robust_sum(c6[active], robust, delta)
    if L is not None and L.n_lid:
        leL, le6 = R.lidar_errors(qg, tg, L, LD), R.lidar_errors(qg, tg, L)
        newL = newL + (leL * (np.asarray(L.info, LD) * leL)).sum(dtype=LD)
        new6 = new6 + (le6 * (L.info * le6)).sum()
    if accepted:
        _ratio("chi2_after", _rel(st["chi2_end"][stage], newL), _rel(new6, newL), out)
    else:  # a start at the vision optimum may leave the LiDAR stage nothing to gain
        assert st["chi2_end"][stage] == st["chi2_begin"][stage] and float(new6) >= st["chi2_begin"][stage]
    assert max(out.values()) <= K, out
    return qg, tg, S_hi, S_lo, accepted


@pytest.mark.parametrize("lam", [1e-3, 1.0, 1e3])
@pytest.mark.parametrize("name", FIRST)
def test_first_trial(gpu_ctx, oracle, name, lam):
    p = SC.problem(name)
    run = run_alone(gpu_ctx, name, (1, 0, 0, 0), lam)
    print(name, lam)
    qg, tg, S_hi, S_lo, _ = _first_trial(oracle, p, run, 0, lam, np.ones(p.n_obs, bool), True, None, 0, True)
    got = _pose(run["q"], run["t"])
    if p.n_obs < 10:  # round 0 only: the pose is the trial's
        assert _ratio("pose_out", _maxrel(got, S_hi), _maxrel(S_lo, S_hi)) <= K
    else:  # rounds 1-3 restart from the input pose and, with no iteration, stay there
        assert np.array_equal(got, _pose(p.pose_q, p.pose_t))
        assert run["st"]["rounds"] == 4 and run["st"]["trials"][1:4] == [0, 0, 0]


@pytest.mark.parametrize("lam", [1e-3, 1.0, 1e3])
@pytest.mark.parametrize("name", LID_FIRST)
def test_lidar_first_trial(gpu_ctx, oracle, name, lam):
    sub, L, oin, rob = SC.lidar_problem(oracle, name)
    run = run_lidar_alone(gpu_ctx, oracle, name, 1, lam)
    print(name, lam)
    qg, tg, S_hi, S_lo, accepted = _first_trial(oracle, sub, run, 4, lam, ~oin, rob, L, 4, False)
    if accepted:
        assert _ratio("pose_out", _maxrel(_pose(run["q"], run["t"]), S_hi), _maxrel(S_lo, S_hi)) <= K
    else:
        assert np.array_equal(_pose(run["q"], run["t"]), _pose(sub.pose_q, sub.pose_t))
    # level-1 edges are evaluated at the stage's estimate
    if oin.any():
        cL, c6 = R.mono_chi2(run["q"], run["t"], sub, LD), R.mono_chi2(run["q"], run["t"], sub)
        assert _ratio("level-1 chi2", _maxrel(run["chi2"][oin, 4], cL[oin]), _maxrel(c6[oin], cL[oin])) <= K


# ---- 3. whole schedule on every shape ----------------------------------------------
def _check_result(p, ref, spread, q, t, n_in, flag, st, chi2):
    dS, dchi, _, dbeg = spread
    print("  gpu its", st["iterations"], "trials", st["trials"], "| ref its",
          [None if s is None else s["iterations"] for s in ref["stats"]], "trials",
          [None if s is None else s["trials"] for s in ref["stats"]])
    assert st["n_corr"] == p.n_obs
    assert n_in == ref["n_inliers"] and st["n_bad_final"] == ref["n_bad_final"]
    assert st["rounds"] == ref["rounds"] and st["n_bad"][:ref["rounds"]] == ref["n_bad"]
    assert np.array_equal(flag != 0, ref["outlier"])
    tol = max(1e-6, 10 * dS)
    err = float(np.abs(_pose(q, t) - _pose(ref["pose_q"], ref["pose_t"])).max())
    print(f"  pose err {err:.3e} tol {tol:.3e} (ulp spread {dS:.3e})")
    assert err <= tol
    for k, s in enumerate(ref["stats"]):
        if s is None:
            assert st["iterations"][k] == 0 and st["trials"][k] == 0
            continue
        assert st["active"][k] == s["active"]
        assert (st["trials"][k] > 0) == s["ran"]
        for what, d in (("chi2_begin", dbeg), ("chi2_end", dchi)):
            c_ref = float(s[what])
            e_ = abs(st[what][k] - c_ref) / max(1.0, c_ref)
            tl = max(1e-6, 10 * d[k] / max(1.0, c_ref))
            print(f"  stage {k} {what} gpu {st[what][k]:.12g} ref {c_ref:.12g} err {e_:.3e} tol {tl:.3e}")
            assert e_ <= tl
    if p.n_obs:  # the chi2 every check read, against the thresholds
        c = np.asarray(ref["edge_chi2"], np.float64)
        assert np.array_equal(chi2 > p.th2, c > p.th2)
        assert not chi2[:, ref["rounds"]:4].any() and not c[:, ref["rounds"]:4].any()  # checks that did not run
    if p.n_obs < 3:
        assert n_in == 0 and not flag.any() and np.array_equal(_pose(q, t), _pose(p.pose_q, p.pose_t))


@pytest.mark.parametrize("name", SC.NAMES)
def test_schedule(gpu_ctx, oracle, name):
    run = run_alone(gpu_ctx, name)
    print(name)
    _check_result(SC.problem(name), SC.reference(oracle, name), SC.ulp_spread(oracle, name), run["q"], run["t"],
                  run["n_in"], run["flag"], run["st"], run["chi2"])


@pytest.mark.parametrize("name", SC.LIDAR_NAMES)
def test_lidar_schedule(gpu_ctx, oracle, name):
    sub = SC.lidar_problem(oracle, name)[0]
    run = run_lidar_alone(gpu_ctx, oracle, name)
    print(name)
    assert run["st"]["n_lidar"] == SC.lidar_problem(oracle, name)[1].n_lid
    _check_result(sub, SC.lidar_reference(oracle, name), SC.lidar_ulp_spread(oracle, name), run["q"], run["t"],
                  run["n_in"], run["flag"], run["st"], run["chi2"])


def test_facade_two_call_sequence(gpu_ctx, oracle):
    for name, m in (("n257", 300), ("n9", 120), ("n2", 50)):
        p0 = SC.problem(name)
        assoc = lambda pose, p0=p0, m=m: P.make_lidar_pairs(p0, m, seed=2)
        for lid in (None, assoc):
            want_n, want_q, want_t, want_out = R.pose_optimization(oracle, p0, lid)
            p = p0.copy()
            n_in = Optimizer.PoseOptimization(p, lid, ctx=gpu_ctx)
            assert n_in == want_n and np.array_equal(p.outlier, want_out), (name, lid is not None)
            err = float(np.abs(_pose(p.pose_q, p.pose_t) - _pose(want_q, want_t)).max())
            print(name, "lidar" if lid else "vision", "n_in", n_in, "pose err", err)
            assert err <= 1e-6
            if p0.n_obs < 3:
                assert n_in == 0 and np.array_equal(_pose(p.pose_q, p.pose_t), _pose(p0.pose_q, p0.pose_t))


# ---- 4. batch invariance -----------------------------------------------------------
def _split(off, a):
    return [a[off[k]:off[k + 1]] for k in range(len(off) - 1)]


def _same(a, b, n):
    for k in ("q", "t", "flag", "chi2", "e", "J", "le", "lJ"):
        assert np.array_equal(a[k], b[k]), (n, k)
    assert a["n_in"] == b["n_in"] and a["st"] == b["st"], n


def _unbatch(ctx, res, names):
    q, t, n_in, flag, st = res
    off, loff = ctx.pose_obs_off, ctx.pose_lid_off
    chi2, (e, J, le, lJ) = ctx.pose_edge_chi2(), ctx.pose_linearization()
    return {n: dict(q=q[k], t=t[k], n_in=int(n_in[k]), flag=_split(off, flag)[k], st=st[k], chi2=_split(off, chi2)[k],
                    e=_split(off, e)[k], J=_split(off, J)[k], le=_split(loff, le)[k], lJ=_split(loff, lJ)[k])
            for k, n in enumerate(names)}


def test_batch_invariance(gpu_ctx, oracle):
    order = list(np.random.default_rng(7).permutation(len(SC.NAMES)))
    names = [SC.NAMES[k] for k in order]
    for it, lam in (((10, 10, 10, 10), 0.0), ((1, 10, 10, 10), 0.0)):
        alone = {n: run_alone(gpu_ctx, n, it, lam) for n in names}
        for ns in (names, names[::-1], names[:2]):  # a small batch after a large one: no stale state
            got = _unbatch(gpu_ctx, gpu_ctx.pose_optimize([SC.problem(n) for n in ns], it, lam), ns)
            for n in ns:
                _same(alone[n], got[n], n)
    lnames = SC.LIDAR_NAMES
    lalone = {n: run_lidar_alone(gpu_ctx, oracle, n) for n in lnames}
    for ns in (lnames, lnames[::-1]):
        c = [SC.lidar_problem(oracle, n) for n in ns]
        res = gpu_ctx.pose_refine_lidar([x[0] for x in c], [x[1] for x in c], np.concatenate([x[2] for x in c]),
                                        [x[3] for x in c])
        got = _unbatch(gpu_ctx, res, ns)
        for n in ns:
            _same(lalone[n], got[n], n)


def test_buffer_growth(gpu_ctx, oracle):
    """A larger call after a smaller one on a fresh context: the buffers grow, the results do not change."""
    with Context(0) as ctx:
        small = _collect(ctx, ctx.pose_optimize([SC.problem("n3")]), 3, True)
        _same(run_alone(gpu_ctx, "n3"), small, "n3")
        ns = ["n600_o35", "n257", "n0", "n65_clean"]
        got = _unbatch(ctx, ctx.pose_optimize([SC.problem(n) for n in ns]), ns)
        for n in ns:
            _same(run_alone(gpu_ctx, n), got[n], n)
        sub, L, oin, rob = SC.lidar_problem(oracle, "l1_flat")
        _same(run_lidar_alone(gpu_ctx, oracle, "l1_flat"), _collect(ctx, ctx.pose_refine_lidar([sub], [L], oin, [rob]),
                                                                    sub.n_obs, True), "l1_flat")
        sub, L, oin, rob = SC.lidar_problem(oracle, "l700_mixed")
        _same(run_lidar_alone(gpu_ctx, oracle, "l700_mixed"),
              _collect(ctx, ctx.pose_refine_lidar([sub], [L], oin, [rob]), sub.n_obs, True), "l700_mixed")


# ---- 5. argument checks ------------------------------------------------------------
def test_argument_errors_and_empty_batch(oracle):
    import ctypes as C
    from sqrtlm import _lib
    with Context(0) as ctx:
        Lb, p = _lib.lib(), _lib.ptr
        buf = np.zeros(64)
        assert Lb.sqlm_pose_get_edge_chi2(ctx._h, p(buf)) == -7  # SQLM_ERR_STATE before any call
        assert Lb.sqlm_pose_get_linearization(ctx._h, p(buf), p(buf), None, None) == -7
        assert Lb.sqlm_pose_get_last_step(ctx._h, 0, p(buf), p(buf), p(buf)) == -7
        a = P.pack([SC.problem("n11_out"), SC.problem("n9")])
        q, t, n_in, flag = np.zeros((2, 4)), np.zeros((2, 3)), np.zeros(2, np.int32), np.zeros(20, np.uint8)

        def call(n_prob=2, iters=None, th2=5.991, **over):
            b = {**a, **over}
            return Lb.sqlm_pose_optimize(ctx._h, n_prob, p(b["pose_q"]), p(b["pose_t"]), p(b["intr"]), p(b["obs_off"]),
                                         p(b["Xw"]), p(b["uv"]), p(b["info"]), p(iters), C.c_double(th2),
                                         C.c_double(0), p(q), p(t), p(n_in), p(flag), None)

        assert call(n_prob=-1) == -1
        for k in ("pose_q", "pose_t", "intr", "obs_off", "Xw", "uv", "info"):
            assert call(**{k: None}) == -1, k
        assert call(obs_off=np.array([0, 11, 5], np.int64)) == -1
        assert call(iters=np.array([10, -1, 10, 10], np.int32)) == -1
        assert call(th2=0.0) == -1
        assert call(n_prob=0) == 0
        assert call() == 0 and n_in.tolist() == [8, 9]
        assert call(iters=np.array([0, 0, 0, 0], np.int32)) == 0
        assert Lb.sqlm_pose_get_last_step(ctx._h, 0, p(buf), p(buf), p(buf)) == -7  # no trial ran
        assert Lb.sqlm_pose_get_last_step(ctx._h, 2, p(buf), p(buf), p(buf)) == -1
        sub, L, oin, rob = SC.lidar_problem(oracle, "l1_flat")
        with pytest.raises(Exception):
            ctx.pose_refine_lidar([sub], [L], oin, [rob], iters=0)  # iters >= 1
