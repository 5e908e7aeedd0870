"""sqlm_sim3_ransac (batched GPU Sim3Solver) against the numpy definition
tests/sim3_ransac_ref.py on the cases of tests/sim3_ransac_cases.py.

Tolerances. Index mapping, inlier masks and counts (given the GPU's own
transforms), T21 from (R12, t12, s12), flags and the replayed iterate()/find():
identical, no margin -- given their inputs the arithmetic is fixed, with no
transcendental function. Closed form (R12, t12, s12 of every hypothesis against
the longdouble closed form from the same float inputs, each quantity relative
to its own largest entry): K x spread, K = 100, the rule and constant of
tests/test_gpu_first_trial.py. The spread of a hypothesis is the larger of the
float32 definition's own distance from the longdouble result and the
longdouble result's largest change under eight seeded +-1-float-ulp
perturbations of its six input points (which makes the bound follow the
conditioning of near-collinear triples), floored at 4 float32 eps. No
hypothesis is left out; a NaN must be a NaN on both sides.

Measured on an MI355X when the test was written (52 tests, 1.3 s): R12, t12
and s12 of every hypothesis of every case are bit-equal to the float32
definition, NaN included, so a ratio (GPU error / spread) can be 1.0 at most.
Largest ratio per case, over R, t, s:

  n3_h1 0.12, n20_h4_fix 0.35, n63_h5 0.73, n64_h300_k2 1.0, n65_h13_fix_k2
  0.61, n129_h8_never 0.29, n20_min_eq_n 0.09, n300_h300 1.0, n20_translation
  0 (R = I, t and s exact), n20_same_free 0.20, n20_same_fix 0.39.

It is 1.0 where the definition's own distance from the longdouble result is
the spread (some hypothesis among 300 whose float32 rounding exceeds all eight
one-ulp input perturbations), never above: no arithmetic reason brings it near
K. The largest spreads are near-collinear triples: 5.5e-5 on R and 1.8e-4 on
t among the 300 random triples of n64_h300_k2, and 2.0 (an undetermined
rotation) where two of the three drawn pairs are the same pair (n20_same_*).
Masks, counts, T21, flags and the replayed iterate(5) / find() are identical
to the definition; all outputs are bitwise equal alone, in a shuffled batch,
in the reversed batch and in a small batch after a large one. Chain: 104
RANSAC inliers of 105 planted, sqlm_sim3_optimize keeps 104.

A deliberately wrong scratch build (the second projection of the inlier check
using T12 where T21 belongs; nothing of it is committed) fails 14 of the 52:
test_inlier_check on all 11 cases, test_closed_form[n20_same_fix] (the three
copies of the coinciding pair are no longer inliers), the chain test and the
count assertions of test_argument_errors_and_empty_batch. The index-mapping,
closed-form, bookkeeping and batch-invariance tests still pass: they do not
read the masks, or hold the library to its own counts -- which is why
test_inlier_check pins masks and counts to the definition first.
"""
import numpy as np
import pytest

import sim3_ransac_cases as SC
import sim3_ransac_ref as R
from sqrtlm import sim3

pytestmark = pytest.mark.gpu

K = 100.0
EPS32 = float(np.finfo(np.float32).eps)
FLOOR = 4 * EPS32
LD = np.longdouble

_runs: dict = {}
_spreads: dict = {}


def _collect(ctx, k, n_hyp, res):
    """Everything the library reports about problem k of the last call."""
    run = dict(res)
    hy = [ctx.sim3_ransac_hypothesis(k, h) for h in range(n_hyp)]
    run["idx"] = np.array([a[0] for a in hy], np.int32).reshape(n_hyp, 3)
    run["T12"] = np.array([a[1] for a in hy], np.float32).reshape(n_hyp, 4, 4)
    run["T21"] = np.array([a[2] for a in hy], np.float32).reshape(n_hyp, 4, 4)
    n = int(ctx.sim3_ransac_pairs[k])
    run["mask"] = np.array([ctx.sim3_ransac_inliers(k, h) for h in range(n_hyp)], np.uint8).reshape(n_hyp, n).astype(bool)
    return run


def _batch(ctx, names):
    cs = [SC.case(n) for n in names]
    res = ctx.sim3_ransac([c["problem"] for c in cs], [c["draws"] for c in cs], [c["max_err"] for c in cs],
                          [c["min_inliers"] for c in cs])
    return {n: _collect(ctx, k, cs[k]["n_hyp"], res[k]) for k, n in enumerate(names)}


def run_alone(ctx, name):
    if name not in _runs:
        _runs[name] = _batch(ctx, [name])[name]
    return _runs[name]


def _same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in
               ("n_inliers", "flags", "R12", "t12", "s12", "idx", "T12", "T21", "mask")) and \
        a["first_return"] == b["first_return"] and a["best"] == b["best"]


# ---- 1. index mapping ---------------------------------------------------------------
@pytest.mark.parametrize("name", SC.NAMES)
def test_index_mapping(gpu_ctx, name):
    c, run = SC.case(name), run_alone(gpu_ctx, name)
    n = c["problem"].n_pair
    for h in range(c["n_hyp"]):
        assert run["idx"][h].tolist() == R.swap_remove_literal(n, c["draws"][h]), h


@pytest.mark.parametrize("n", [3, 4, 5])
def test_index_mapping_exhaustive(gpu_ctx, n):
    import itertools
    draws = np.array(list(itertools.product(range(n), range(n - 1), range(n - 2))), np.int32)
    p, e1, e2 = sim3.make_sim3_ransac_problem(n, seed=n, outlier_frac=0.0)
    res = gpu_ctx.sim3_ransac([p], [draws], [(e1, e2)], 3)[0]
    assert res["n_inliers"].shape == (len(draws),)
    for h, d in enumerate(draws):
        assert gpu_ctx.sim3_ransac_hypothesis(0, h)[0].tolist() == R.swap_remove_literal(n, d), (n, d)


# ---- 2. closed form ------------------------------------------------------------------
def _rel(a, b):
    """max |a - b| per hypothesis, relative to the hypothesis's largest |b| (longdouble)."""
    a, b = np.asarray(a, LD).reshape(len(b), -1), np.asarray(b, LD).reshape(len(b), -1)
    with np.errstate(all="ignore"):
        s = np.abs(b).max(axis=1)
        return np.abs(a - b).max(axis=1) / np.where(s > 0, s, 1)


def spreads(name):
    """Per hypothesis and quantity: the longdouble result and the spread the bound is built from."""
    if name not in _spreads:
        c, ref = SC.case(name), SC.reference(name)
        p = c["problem"]
        P1, P2 = R.gather(p.X1c, p.X2c, ref["idx"])
        ld = R.closed_form(P1, P2, p.fix_scale, ld=True)
        rng = np.random.default_rng([0x5EED, len(name)])
        sp = {q: _rel(ref[q], ld[q]) for q in ("R", "t", "s")}
        for _ in range(8):
            up1, up2 = rng.integers(0, 2, P1.shape).astype(bool), rng.integers(0, 2, P2.shape).astype(bool)
            Q1 = np.where(up1, np.nextafter(P1, np.float32(np.inf)), np.nextafter(P1, np.float32(-np.inf)))
            Q2 = np.where(up2, np.nextafter(P2, np.float32(np.inf)), np.nextafter(P2, np.float32(-np.inf)))
            pert = R.closed_form(Q1, Q2, p.fix_scale, ld=True)
            for q in sp:
                with np.errstate(all="ignore"):
                    sp[q] = np.fmax(sp[q], _rel(pert[q], ld[q]))
        _spreads[name] = (ld, sp)
    return _spreads[name]


@pytest.mark.parametrize("name", [n for n in SC.NAMES if SC.case(n)["n_hyp"] > 0])
def test_closed_form(gpu_ctx, name):
    c, ref, run = SC.case(name), SC.reference(name), run_alone(gpu_ctx, name)
    ld, sp = spreads(name)
    worst = {}
    for q, g in (("R", run["R12"]), ("t", run["t12"]), ("s", run["s12"])):
        want = np.asarray(ld[q], LD).reshape(c["n_hyp"], -1)
        got = np.asarray(g, np.float32).reshape(c["n_hyp"], -1)
        nan = np.isnan(want).any(axis=1)
        assert np.array_equal(np.isnan(got), np.isnan(want)), f"{q}: NaN on one side only"
        err = _rel(got, want)
        with np.errstate(all="ignore"):
            ratio = err / np.fmax(sp[q], FLOOR)
        ratio = np.where(nan, 0.0, ratio)
        assert not np.isnan(ratio).any()
        worst[q] = (float(ratio.max()), int(ratio.argmax()), float(err[~nan].max()) if (~nan).any() else 0.0,
                    float(np.where(nan, 0, sp[q]).max()))
        assert ratio.max() <= K, (q, worst[q])
    equal = all(np.array_equal(run[a], ref[b], equal_nan=True) for a, b in (("R12", "R"), ("t12", "t"), ("s12", "s")))
    print(f"{name}: H {c['n_hyp']} " + " ".join(f"{q} ratio {w[0]:.3g} (h {w[1]}, err {w[2]:.2e}, spread <= {w[3]:.2e})"
                                                  for q, w in worst.items())
          + f" | bit-equal to the float32 definition: {equal}")
    if c["problem"].fix_scale:
        assert np.all(run["s12"] == 1.0)
    if name == "n20_translation":
        assert np.array_equal(run["R12"], np.broadcast_to(np.eye(3, dtype=np.float32), (c["n_hyp"], 3, 3)))
    if name == "n20_same_free":
        assert np.isnan(run["s12"][0]) and np.isnan(run["t12"][0]).all() and run["n_inliers"][0] == 0
    if name == "n20_same_fix":
        assert np.isfinite(run["t12"][0]).all() and run["mask"][0][:3].all()


# ---- 3. inlier check -----------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in SC.NAMES if SC.case(n)["n_hyp"] > 0])
def test_inlier_check(gpu_ctx, name):
    c, run = SC.case(name), run_alone(gpu_ctx, name)
    p = c["problem"]
    mask, count = R.check_inliers(run["T12"], run["T21"], p.X1c, p.X2c, p.intr1, p.intr2, c["max_err"][0], c["max_err"][1])
    assert np.array_equal(run["mask"], mask)
    assert np.array_equal(run["n_inliers"], count) and np.array_equal(run["mask"].sum(axis=1), count)
    assert np.array_equal(run["T21"], R.inverse_f32(run["R12"], run["t12"], run["s12"]), equal_nan=True)
    with np.errstate(all="ignore"):
        sR = (run["s12"].astype(np.float64)[:, None, None] * run["R12"].astype(np.float64)).astype(np.float32)
    assert np.array_equal(run["T12"][:, :3, :3], sR, equal_nan=True)
    assert np.array_equal(run["T12"][:, :3, 3], run["t12"], equal_nan=True)
    assert np.all(run["T12"][:, 3] == [0, 0, 0, 1]) and np.all(run["T21"][:, 3] == [0, 0, 0, 1])


# ---- 4. bookkeeping --------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.NAMES)
def test_bookkeeping(gpu_ctx, name):
    c, run = SC.case(name), run_alone(gpu_ctx, name)
    flags, first, best = R.scan(run["n_inliers"], c["min_inliers"])
    assert np.array_equal(run["flags"], flags) and run["first_return"] == first and run["best"] == best
    p = c["problem"]
    n1 = p.n_pair + 7
    ind = np.sort(np.random.default_rng(1).permutation(n1)[:p.n_pair])
    hyp = dict(count=run["n_inliers"], mask=run["mask"], T12=run["T12"])

    def make():
        s = sim3.Sim3Solver(p, *c["max_err"], draws=c["draws"], indices1=ind, n1=n1, ctx=gpu_ctx)
        s.SetRansacParameters(0.99, c["min_inliers"], SC.SPECS[name][3])
        return s, R.LiteralSolver(hyp, p.n_pair, c["min_inliers"], c["n_hyp"], ind, n1)

    s, lit = make()
    assert s.mRansacMaxIts == c["n_hyp"]
    calls = 0
    while True:
        a, b = s.iterate(5), lit.iterate(5)
        calls += 1
        assert (a[0] is None) == (b[0] is None) and a[1] == b[1] and a[3] == b[3], calls
        assert a[2].shape == (n1,) and np.array_equal(a[2], b[2])
        if a[0] is not None:
            assert np.array_equal(a[0], b[0])
            h = lit.best
            assert np.array_equal(s.GetEstimatedRotation(), run["R12"][h])
            assert np.array_equal(s.GetEstimatedTranslation(), run["t12"][h])
            assert s.GetEstimatedScale() == float(run["s12"][h])
        if a[1]:
            break
        assert calls <= c["n_hyp"] + 1
    assert (lit.best if lit.best is not None else -1) == s._best
    s, lit = make()
    a, b = s.find(), lit.find()
    assert (a[0] is None) == (b[0] is None) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    if a[0] is not None:
        assert np.array_equal(a[0], b[0]) and lit.best == run["first_return"]


# ---- 5. batch invariance ---------------------------------------------------------------
def test_batch_invariance(gpu_ctx):
    order = list(np.random.default_rng(7).permutation(len(SC.NAMES)))
    names = [SC.NAMES[k] for k in order]
    alone = {n: run_alone(gpu_ctx, n) for n in names}
    fwd, rev = _batch(gpu_ctx, names), _batch(gpu_ctx, names[::-1])
    small = _batch(gpu_ctx, ["n20_h4_fix", "n3_h1"])   # a small batch after a large one on the same context
    inorder = _batch(gpu_ctx, SC.NAMES)                # the problem without hypotheses in the middle
    for got in (fwd, rev, small, inorder):
        for n in got:
            assert _same(alone[n], got[n]), n
    solvers = [sim3.Sim3Solver(SC.case(n)["problem"], *SC.case(n)["max_err"], draws=SC.case(n)["draws"]) for n in names]
    for s, n in zip(solvers, names):
        s.SetRansacParameters(0.99, SC.case(n)["min_inliers"], SC.SPECS[n][3])
    sim3.Sim3Solver.solve_batch(solvers, ctx=gpu_ctx)  # several solvers, one call
    for s, n in zip(solvers, names):
        T, vb, n_in = s.find()
        h = alone[n]["first_return"]
        assert (T is None) == (h < 0)
        if h >= 0:
            assert np.array_equal(T, alone[n]["T12"][h]) and np.array_equal(vb, alone[n]["mask"][h])
            assert n_in == alone[n]["n_inliers"][h]


# ---- 6. chain ----------------------------------------------------------------------------
def test_chain_ransac_then_optimize_sim3(gpu_ctx):
    c = SC.chain_case()
    p = c["problem"]
    s = sim3.Sim3Solver(p, *c["max_err"], draws=c["draws"], ctx=gpu_ctx)
    s.SetRansacParameters(0.99, c["min_inliers"], 300)       # LoopClosing.cc:438
    T, no_more, vb, n_in = None, False, None, 0
    while T is None and not no_more:
        T, no_more, vb, n_in = s.iterate(5)                  # :481
    assert T is not None and n_in > c["min_inliers"] and vb.sum() == n_in
    assert not (vb & p.meta["outlier"]).any()
    sub = SC.chain_subproblem(c, s.GetEstimatedRotation(), s.GetEstimatedTranslation(), s.GetEstimatedScale(), vb)
    S, n_opt, state, st = gpu_ctx.sim3_optimize([sub])       # :513
    print("chain: RANSAC inliers", n_in, "OptimizeSim3 inliers", int(n_opt[0]))
    assert n_opt[0] >= 20                                    # :516
    S_true = p.meta["S12_true"]
    assert abs(S[0][7] - S_true[7]) < 0.01 and np.abs(S[0][4:7] - S_true[4:7]).max() < 0.05


# ---- 7. argument errors, empty batches ---------------------------------------------------
def test_argument_errors_and_empty_batch():
    from sqrtlm import _lib
    from sqrtlm.optimizer import Context
    with Context(0) as ctx:
        L, p = _lib.lib(), _lib.ptr
        i4, f16 = np.zeros(4, np.int32), np.zeros(16, np.float32)
        assert L.sqlm_sim3_ransac_get_inliers(ctx._h, 0, 0, p(i4)) == -7        # SQLM_ERR_STATE before any call
        assert L.sqlm_sim3_ransac_get_hypothesis(ctx._h, 0, 0, p(i4), p(f16), p(f16)) == -7
        cs = [SC.case("n20_h4_fix"), SC.case("n5_lt_min"), SC.case("n63_h5")]
        a = sim3.pack_ransac([c["problem"] for c in cs], [c["max_err"] for c in cs], [c["draws"] for c in cs],
                             [c["min_inliers"] for c in cs])
        H = int(a["hyp_off"][-1])
        o = dict(n_inliers=np.zeros(H, np.int32), flags=np.zeros(H, np.uint8), R12=np.zeros((H, 9), np.float32),
                 t12=np.zeros((H, 3), np.float32), s12=np.zeros(H, np.float32), first_return=np.zeros(3, np.int32),
                 best=np.zeros(3, np.int32))
        order = ("intr1", "intr2", "fix_scale", "min_inliers", "pair_off", "X1c", "X2c", "max_err1", "max_err2",
                 "hyp_off", "draws", "n_inliers", "flags", "R12", "t12", "s12", "first_return", "best")

        def call(n_prob=3, **over):
            b = {**a, **o, **over}
            return L.sqlm_sim3_ransac(ctx._h, n_prob, *[p(b[k]) for k in order])

        assert call(n_prob=-1) == -1
        for k in order:
            assert call(**{k: None}) == -1, k
        assert call(pair_off=np.array([0, 20, 10, 88], np.int64)) == -1
        assert call(hyp_off=np.array([0, 4, 2, 9], np.int64)) == -1
        bad = a["draws"].copy()
        bad[0] = [20, 0, 0]                                   # draw 0 of a 20-pair problem is in [0, 19]
        assert call(draws=bad) == -1
        bad = a["draws"].copy()
        bad[5] = [0, 0, 61]                                   # draw 2 of a 63-pair problem is in [0, 60]
        assert call(draws=bad) == -1
        bad[5] = [0, -1, 0]
        assert call(draws=bad) == -1
        neg = a["max_err2"].copy()
        neg[3] = -1
        assert call(max_err2=neg) == -1
        # a problem with a hypothesis and only 2 pairs
        assert call(pair_off=np.array([0, 20, 22, 85], np.int64), hyp_off=np.array([0, 4, 5, 9], np.int64)) == -1
        assert call(n_prob=0) == 0
        assert L.sqlm_sim3_ransac_get_inliers(ctx._h, 0, 0, p(i4)) == -1        # a call was made; no such problem
        assert call() == 0
        assert o["first_return"].tolist() == [0, -1, 4] and o["best"][1] == -1
        mask = np.zeros(64, np.uint8)
        assert L.sqlm_sim3_ransac_get_inliers(ctx._h, 1, 0, p(mask)) == -1      # the problem has no hypotheses
        assert L.sqlm_sim3_ransac_get_inliers(ctx._h, 3, 0, p(mask)) == -1
        assert L.sqlm_sim3_ransac_get_inliers(ctx._h, 2, 5, p(mask)) == -1
        assert L.sqlm_sim3_ransac_get_inliers(ctx._h, 2, 4, p(mask)) == 0 and mask[:63].sum() == o["n_inliers"][8]
        no_h = np.zeros(4, np.int64)
        assert call(hyp_off=no_h) == 0 and o["first_return"].tolist() == [-1, -1, -1]   # problems, no hypotheses
