"""sqlm_sim3_optimize (batched GPU OptimizeSim3) against the numpy reference
tests/sim3_ref.py on the cases of tests/sim3_cases.py.

Tolerances. Linearization and first trial: K x the reference's own
float64-vs-longdouble spread of that quantity on that problem, floored at
4 eps, K = 100 -- the rule and constant of tests/test_gpu_first_trial.py.
Errors are relative to the quantity's largest entry. Whole schedule:
n_inliers, n_bad and pair_state identical (test_sim3_ref.py asserts the
margin that makes this a fair demand); S12_out and each stage's final chi2
within max(1e-6, 10 x the reference's spread under a one-ulp perturbation of
the initial S12), chi2 relative to max(1, chi2). Trial and iteration counts
are printed, not asserted: acceptances at the noise floor of the numeric
Jacobians may legitimately differ.

Ratios (GPU error / spread) measured on an MI355X when the test was written:

  linearization, all 11 non-empty cases: e 1.0, J 1.0 -- the GPU's e and J
  are bit-equal to the float64 reference (the error IS the spread);
  first trial (n9, n65_clean, n255_fix_k2, n600; lambda 1e-3, 1, 1e3), largest
  over the 12 runs: H 0.19, b 0.11, dx 1.10, S12 0.23, chi2_begin 0.10,
  pair_chi2 1.00, chi2_after 1.11;
  whole schedule: states and counts identical on all 12 cases; S12_out off by
  at most 5.8e-9 (n64_k2, whose one-ulp spread is 4.1e-9), stage chi2 by at
  most 2.4e-9 relative (n1); trial counts differ from the reference's on n9,
  n10_clean, n63_fix, n65_clean and n255_fix_k2 (converged problems, trials
  that change chi2 in the 14th digit).

A deliberately wrong scratch build (the inverse edge's error evaluated at S12
instead of S12^-1 in the linearization, the perturbed errors left right;
nothing of it is committed) gives: e ratio 6.9e14 ... 2.4e15 on every case, J
ratio still 1.0 (test_linearization fails 11 of 11), test_schedule fails 11
of 12 (all but the empty problem; n_inliers 0 where the reference has up to
478), while test_first_trial still passes: it is fed the GPU's
own e and J, which is why test_linearization pins them first.
"""
import numpy as np
import pytest

import sim3_cases as SC
import sim3_ref as R
from sqrtlm.optimizer import Optimizer

pytestmark = pytest.mark.gpu

K = 100.0
LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
FLOOR = 4 * EPS
NONEMPTY = [n for n in SC.NAMES if SC.SPECS[n][0] > 0]

_runs: dict = {}


def _maxrel(a, b):
    a, b = np.asarray(a, LD), np.asarray(b, LD)
    s = np.abs(b).max()
    return float(np.abs(a - b).max() / (s if s > 0 else 1))


def _ratio(label, err, spread, out=None):
    r = err / max(spread, FLOOR)
    print(f"  {label}: err {err:.3e} spread {spread:.3e} ratio {r:.3g}")
    if out is not None:
        out[label] = r
    return r


def run_alone(ctx, name, iters=None, user_lambda=0.0):
    """The case alone on the GPU (once per argument set), with all introspection."""
    key = (name, None if iters is None else tuple(iters), float(user_lambda))
    if key not in _runs:
        p = SC.problem(name)
        S, n_in, state, st = ctx.sim3_optimize([p], iters, user_lambda)
        run = dict(S=S[0], n_in=int(n_in[0]), state=state, st=st[0], chi2=ctx.sim3_pair_chi2())
        run["e"], run["J"] = ctx.sim3_linearization()
        if p.n_pair and (iters is None or iters[0] > 0):
            run["H"], run["b"], run["dx"] = ctx.sim3_last_step(0)
        _runs[key] = run
    return _runs[key]


# ---- 1. linearization ---------------------------------------------------------
@pytest.mark.parametrize("name", NONEMPTY)
def test_linearization(gpu_ctx, oracle, name):
    p, ref = SC.problem(name), SC.reference(oracle, name)
    run = run_alone(gpu_ctx, name)
    e64, J64, P, Pi = ref["lin"]
    eL, JL = R.linearization(p, p.S12, oracle.sim3_inverse(p.S12), P, Pi, LD)
    print(name)
    re_ = _ratio("e", _maxrel(run["e"], eL), _maxrel(e64, eL))
    rJ = _ratio("J", _maxrel(run["J"], JL), _maxrel(J64, JL))
    print(f"  bit-equal to the float64 reference: e {np.array_equal(run['e'], e64)} J {np.array_equal(run['J'], J64)}")
    assert re_ <= K and rJ <= K
    if p.fix_scale:
        assert np.all(run["J"][..., 6] == 0.0)
    else:
        assert np.abs(run["J"][..., 6]).max() > 0


# ---- 2. first trial -----------------------------------------------------------
@pytest.mark.parametrize("lam", [1e-3, 1.0, 1e3])
@pytest.mark.parametrize("name", ["n9", "n65_clean", "n255_fix_k2", "n600"])
def test_first_trial(gpu_ctx, oracle, name, lam):
    p = SC.problem(name)
    run = run_alone(gpu_ctx, name, (1, 0, 0), lam)
    st = run["st"]
    assert st["iterations"][0] == 1 and st["trials"][0] == 1 and st["trace_trials"][0] == [1]
    info = np.stack([p.info1, p.info2], axis=1)
    delta, act = R.huber_delta(p.th2), np.ones(p.n_pair, bool)
    e, J = run["e"], run["J"]  # pinned by test_linearization
    out = {}
    print(name, lam)
    HL, bL, chiL = R.assemble(e, J, info, delta, act, LD)
    H6, b6, chi6 = R.assemble(e, J, info, delta, act)
    _ratio("H", _maxrel(run["H"], HL), _maxrel(H6, HL), out)
    _ratio("b", _maxrel(run["b"], bL), _maxrel(b6, bL), out)
    okL, dxL = R.solve7(HL, bL, lam, LD)
    ok6, dx6 = R.solve7(H6, b6, lam)
    assert okL and ok6
    _ratio("dx", _maxrel(run["dx"], dxL), _maxrel(dx6, dxL), out)
    _ratio("chi2_begin", abs(float(LD(st["chi2_begin"][0]) - chiL) / float(chiL)), abs(float(chi6 - chiL) / float(chiL)),
           out)
    # the updated S12: oplus in the oracle's float64 Sim3 arithmetic
    S_hi = oracle.sim3_oplus(p.S12, np.asarray(dxL, np.float64), int(p.fix_scale))
    S_lo = oracle.sim3_oplus(p.S12, dx6, int(p.fix_scale))
    S_gpu = oracle.sim3_oplus(p.S12, run["dx"], int(p.fix_scale))
    _ratio("S12", _maxrel(S_gpu, S_hi), _maxrel(S_lo, S_hi), out)
    # the trial was accepted: S12_out is oplus(S12, dx) unless fewer than 10 pairs are left
    assert st["trace_chi2"][0][0] < st["chi2_begin"][0]
    assert np.array_equal(run["S"], S_gpu if p.n_pair - st["n_bad"] >= 10 else p.S12)
    # per-pair chi2 and the robust chi2 after the trial, at the state the GPU reports
    Sg, Sgi = S_gpu, oracle.sim3_inverse(S_gpu)
    cL = R.edge_chi2(R.edge_errors(p, Sg, Sgi, LD), info, LD)
    c6 = R.edge_chi2(R.edge_errors(p, Sg, Sgi), info)
    _ratio("pair_chi2", _maxrel(run["chi2"][:, 0], cL), _maxrel(c6, cL), out)
    chi_newL = R.huber(cL, delta, LD)[0].sum(dtype=LD)
    chi_new6 = R.huber(c6, delta)[0].sum()
    _ratio("chi2_after", abs(float(LD(st["trace_chi2"][0][0]) - chi_newL) / float(chi_newL)),
           abs(float(chi_new6 - chi_newL) / float(chi_newL)), out)
    assert max(out.values()) <= K, out
    if p.fix_scale:
        assert run["S"][7] == p.S12[7] and run["H"][6, 6] == 0.0 and run["dx"][6] == 0.0


# ---- 3 / 4. whole schedule on every shape ----------------------------------------
def _check_schedule(oracle, name, S, n_in, state, st):
    p, ref = SC.problem(name), SC.reference(oracle, name)
    dS, dchi, _ = SC.ulp_spread(oracle, name)
    print(name, "gpu its", st["iterations"], "trials", st["trace_trials"], "| ref its",
          [s["iterations"] for s in ref["stats"]], "trials", [s["trace_trials"] for s in ref["stats"]])
    assert st["n_corr"] == p.n_pair
    assert n_in == ref["n_inliers"] and st["n_bad"] == ref["n_bad"]
    assert np.array_equal(state, ref["pair_state"])
    tolS = max(1e-6, 10 * dS)
    errS = float(np.abs(S - ref["S12_out"]).max())
    print(f"  S12_out err {errS:.3e} tol {tolS:.3e} (ulp spread {dS:.3e})")
    assert errS <= tolS
    for k, s in enumerate(ref["stats"]):
        c_ref = float(s["chi2_end"])
        err = abs(st["chi2_end"][k] - c_ref) / max(1.0, c_ref)
        tol = max(1e-6, 10 * dchi[k] / max(1.0, c_ref))
        print(f"  stage {k + 1} chi2_end gpu {st['chi2_end'][k]:.12g} ref {c_ref:.12g} err {err:.3e} tol {tol:.3e}")
        assert err <= tol
    if p.fix_scale:
        assert S[7] == p.S12[7]
    if len(ref["stats"]) < 2:  # fewer than 10 pairs left (or none at all)
        assert n_in == 0 and np.array_equal(S, p.S12)
        assert st["iterations"][1] == 0 and not np.any(state == 2)


@pytest.mark.parametrize("name", SC.NAMES)
def test_schedule(gpu_ctx, oracle, name):
    run = run_alone(gpu_ctx, name)
    _check_schedule(oracle, name, run["S"], run["n_in"], run["state"], run["st"])
    p, ref = SC.problem(name), SC.reference(oracle, name)
    if p.n_pair:  # the chi2 the two checks read
        c = np.asarray(ref["pair_chi2"], np.float64)
        assert np.array_equal(run["chi2"] > p.th2, c > p.th2)


# ---- 5. batch invariance -----------------------------------------------------------
def _split(pair_off, a):
    return [a[pair_off[k]:pair_off[k + 1]] for k in range(len(pair_off) - 1)]


def test_batch_invariance(gpu_ctx, oracle):
    order = list(np.random.default_rng(7).permutation(len(SC.NAMES)))
    names = [SC.NAMES[k] for k in order]
    alone = {n: run_alone(gpu_ctx, n) for n in names}

    def batch(ns):
        S, n_in, state, st = gpu_ctx.sim3_optimize([SC.problem(n) for n in ns])
        off = gpu_ctx.sim3_pair_off
        chi2, (e, J) = gpu_ctx.sim3_pair_chi2(), gpu_ctx.sim3_linearization()
        return {n: dict(S=S[k], n_in=int(n_in[k]), state=_split(off, state)[k], st=st[k], chi2=_split(off, chi2)[k],
                        e=_split(off, e)[k], J=_split(off, J)[k]) for k, n in enumerate(ns)}

    fwd, rev = batch(names), batch(names[::-1])
    small = batch(names[:2])  # a small batch after a large one on the same context: no stale state
    for got, ns in ((fwd, names), (rev, names), (small, names[:2])):
        for n in ns:
            a, b = alone[n], got[n]
            assert np.array_equal(a["S"], b["S"]) and a["n_in"] == b["n_in"], n
            assert np.array_equal(a["state"], b["state"]) and np.array_equal(a["chi2"], b["chi2"]), n
            assert np.array_equal(a["e"], b["e"]) and np.array_equal(a["J"], b["J"]), n
            assert a["st"] == b["st"], n
    for n in names:
        _check_schedule(oracle, n, fwd[n]["S"], fwd[n]["n_in"], fwd[n]["state"], fwd[n]["st"])


# ---- 6. facade, argument checks -----------------------------------------------------
def test_optimize_sim3_mirror(gpu_ctx, oracle):
    name = "n64_k2"
    run = run_alone(gpu_ctx, name)
    p = SC.problem(name).copy()
    n_in = Optimizer.OptimizeSim3(p, p.th2, p.fix_scale, ctx=gpu_ctx)
    assert n_in == run["n_in"] > 0
    assert np.array_equal(p.S12, run["S"])
    assert np.array_equal(p.matched, run["state"] == 0) and (~p.matched).sum() > 0
    # a second call sees only the surviving matches, as the reference's vpMatches1 would
    n2 = Optimizer.OptimizeSim3(p, ctx=gpu_ctx)
    assert 0 < n2 <= n_in and p.matched.sum() == n2


def test_argument_errors_and_empty_batch(oracle):
    import ctypes as C
    from sqrtlm import _lib, sim3
    from sqrtlm.optimizer import Context
    with Context(0) as ctx:
        L, p = _lib.lib(), _lib.ptr
        buf = np.zeros(64)
        assert L.sqlm_sim3_get_pair_chi2(ctx._h, p(buf)) == -7  # SQLM_ERR_STATE before any call
        assert L.sqlm_sim3_get_linearization(ctx._h, p(buf), p(buf)) == -7
        assert L.sqlm_sim3_get_last_step(ctx._h, 0, p(buf), p(buf), p(buf)) == -7
        a = sim3.pack([SC.problem("n11_out"), SC.problem("n9")])
        S, n_in, state = np.zeros((2, 8)), np.zeros(2, np.int32), np.zeros(20, np.uint8)

        def call(n_prob=2, iters=None, **over):
            b = {**a, **over}
            return L.sqlm_sim3_optimize(ctx._h, n_prob, p(b["S12"]), p(b["intr1"]), p(b["intr2"]), p(b["fix_scale"]),
                                        p(b["th2"]), p(b["pair_off"]), p(b["X1c"]), p(b["X2c"]), p(b["obs1"]),
                                        p(b["obs2"]), p(b["info1"]), p(b["info2"]), p(iters), C.c_double(0), p(S),
                                        p(n_in), p(state), None)

        assert call(n_prob=-1) == -1
        for k in ("S12", "intr1", "intr2", "fix_scale", "th2", "pair_off", "X1c", "X2c", "obs1", "obs2", "info1",
                  "info2"):
            assert call(**{k: None}) == -1, k
        assert call(pair_off=np.array([0, 11, 5], np.int64)) == -1
        assert call(iters=np.array([5, -1, 5], np.int32)) == -1
        assert call(n_prob=0) == 0
        assert call() == 0 and n_in.tolist() == [0, 0]
        assert call(iters=np.array([0, 0, 0], np.int32)) == 0
        assert L.sqlm_sim3_get_last_step(ctx._h, 0, p(buf), p(buf), p(buf)) == -7  # no trial ran
        assert L.sqlm_sim3_get_last_step(ctx._h, 2, p(buf), p(buf), p(buf)) == -1
