"""sqlm_pnp_ransac (batched GPU PnPsolver) against the numpy definition
tests/pnp_ransac_ref.py on the cases of tests/pnp_ransac_cases.py.

Tolerances: none. The definition is the shared text of the kernels restated
operation by operation, IEEE double operations without contraction and without
a transcendental function, and every sum over points has the one order both
sides follow; so the pair indices, the 12x12 eigenvectors and eigenvalues, the
three beta vectors, the reprojection errors, the chosen candidate, R, t, the
inlier masks and counts of every hypothesis and of every refine must be
identical, NaN for NaN, and so must the flags, first_return, best, Tcw and
n_refined of the host scan and the replayed iterate(5) / find(). How close the
definition is to EPnP's mathematics is the business of the CPU tests
(tests/test_pnp_ransac_abi.py, tests/test_pnp_ransac_accuracy.py), which run
the same text compiled for the host.
"""
import numpy as np
import pytest

import pnp_ransac_cases as PC
import pnp_ransac_ref as R
from sqrtlm import pnp
from sqrtlm._lib import SqlmError

pytestmark = pytest.mark.gpu

_runs: dict = {}


def _same(a, b):
    """Bit for bit, a NaN for a NaN (its sign and payload are the processor's, not the arithmetic's)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return a.tobytes() == b.tobytes()
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all()) and np.where(na, 0, a).tobytes() == np.where(nb, 0, b).tobytes()


def _call(ctx, names):
    cs = [PC.case(n) for n in names]
    res = ctx.pnp_ransac([c["problem"] for c in cs], [c["draws"] for c in cs], [c["min_inliers"] for c in cs])
    for k, (c, r) in enumerate(zip(cs, res)):
        H = c["n_hyp"]
        r["mask"] = np.array([ctx.pnp_ransac_inliers(k, h) for h in range(H)], np.uint8).reshape(H, c["problem"].n_pair)
        r["hyp"] = [ctx.pnp_ransac_hypothesis(k, h) for h in range(H)]
        r["refined"] = {int(h): ctx.pnp_ransac_refined(k, int(h)) for h in np.flatnonzero(r["flags"] & 2)}
        r["no_refine"] = []      # what asking for the refine of a hypothesis that is no record does
        for h in np.flatnonzero((r["flags"] & 2) == 0)[:2]:
            try:
                ctx.pnp_ransac_refined(k, int(h))
                r["no_refine"].append("returned")
            except SqlmError as e:
                r["no_refine"].append("error")
    return dict(zip(names, res))


def _batch(ctx):
    """Every case in one call, the problem without hypotheses in the middle (run once, shared)."""
    if "all" not in _runs:
        _runs["all"] = _call(ctx, PC.NAMES)
    return _runs["all"]


@pytest.mark.parametrize("name", PC.NAMES)
def test_hypotheses(gpu_ctx, name):
    g, r = _batch(gpu_ctx)[name], PC.reference(name)
    H = PC.case(name)["n_hyp"]
    assert g["n_inliers"].shape == (H,)
    for h in range(H):
        d = g["hyp"][h]
        for what, a, b in (("idx", d["idx"], r["idx"][h]), ("ut", d["ut"], r["ut"][h]), ("eig", d["eig"], r["eig"][h]),
                           ("betas", d["betas"], r["betas"][h]), ("rep_err", d["rep_err"], r["rep"][h]),
                           ("R", g["R"][h], r["R"][h]), ("t", g["t"][h], r["t"][h]),
                           ("mask", g["mask"][h].astype(bool), r["mask"][h])):
            assert _same(a, b), f"{name} hypothesis {h}: {what}"
        assert d["chosen"] == int(r["chosen"][h]), f"{name} hypothesis {h}: chosen"
    assert _same(g["n_inliers"], r["count"])


@pytest.mark.parametrize("name", PC.NAMES)
def test_refines(gpu_ctx, name):
    g, r = _batch(gpu_ctx)[name], PC.reference(name)
    assert sorted(g["refined"]) == sorted(r["refined"])
    for h, v in r["refined"].items():
        d = g["refined"][h]
        for what, a, b in (("ut", d["ut"], v["ut"][0]), ("eig", d["eig"], v["eig"][0]), ("betas", d["betas"], v["betas"][0]),
                           ("rep_err", d["rep_err"], v["rep"][0]), ("R", d["R"], v["R"][0]), ("t", d["t"], v["t"][0]),
                           ("mask", d["mask"].astype(bool), v["mask"][0])):
            assert _same(a, b), f"{name} refine of {h}: {what}"
        assert d["n_inliers"] == int(v["count"][0]) and d["chosen"] == int(v["chosen"][0])
    assert all(v == "error" for v in g["no_refine"])   # the reference never refines such a mask


@pytest.mark.parametrize("name", PC.NAMES)
def test_bookkeeping(gpu_ctx, name):
    g, r = _batch(gpu_ctx)[name], PC.reference(name)
    assert _same(g["flags"], r["flags"])
    assert (g["first_return"], g["best"]) == (r["first_return"], r["best"])
    T = np.eye(4, dtype=np.float32)
    n_ref = 0
    if r["first_return"] >= 0:
        rec = max(h for h in r["refined"] if h <= r["first_return"])
        v = r["refined"][rec]
        T[:3, :3], T[:3, 3], n_ref = v["R"][0].astype(np.float32), v["t"][0].astype(np.float32), int(v["count"][0])
    assert _same(g["Tcw"], T) and g["n_refined"] == n_ref


def test_what_a_call_stores_depends_on_its_own_inputs_alone(gpu_ctx):
    ref = _batch(gpu_ctx)
    order = ["n300_h5", "n20_same", "n129_h300", "n4_h1_min_eq_n", "n30_fail_then_ok", "n63_h3_k2"]
    runs = [_call(gpu_ctx, order), _call(gpu_ctx, order[::-1]), _call(gpu_ctx, ["n30_fail_then_ok"])]
    for run in runs:
        for name, g in run.items():
            a = ref[name]
            for key in ("n_inliers", "flags", "R", "t", "mask", "Tcw"):
                assert _same(g[key], a[key]), (name, key)
            assert (g["first_return"], g["best"], g["n_refined"]) == (a["first_return"], a["best"], a["n_refined"])
            for h, d in g["refined"].items():
                assert _same(d["R"], a["refined"][h]["R"]) and _same(d["mask"], a["refined"][h]["mask"])
            for d, e in zip(g["hyp"], a["hyp"]):
                assert _same(d["ut"], e["ut"]) and _same(d["betas"], e["betas"])


@pytest.mark.parametrize("name", ["n129_h300", "n20_its4", "n65_h5", "n30_fail_then_ok", "n15_h5_refine10", "n129_never",
                                  "n8_lt_min"])
def test_solver_replays_iterate(gpu_ctx, name):
    """PnPsolver.iterate(5) called until bNoMore, and find(), against the literal solver fed the definition."""
    c, r = PC.case(name), PC.reference(name)
    p, H = c["problem"], c["n_hyp"]

    def fresh():
        s = pnp.PnPsolver(p, draws=c["draws"], ctx=gpu_ctx)
        s.mRansacMinInliers, s.mRansacMaxIts = c["min_inliers"], PC.MAX_ITS.get(name, max(H - 5, 1)) if H else 0
        s._draws = c["draws"]
        lit = R.LiteralSolver(r["count"], lambda h: int(r["refined"][h]["count"][0]), p.n_pair, c["min_inliers"],
                              s.mRansacMaxIts)
        return s, lit
    s, lit = fresh()
    for _ in range(H + 2):
        if H and max(s.mnIterations + 5, s.mRansacMaxIts) > H:
            break       # a call runs to mRansacMaxIts and at least 5 hypotheses: past the case's
        T, no_more, vb, n = s.iterate(5)
        kind, h, lit_no_more = lit.iterate(5)
        assert no_more == lit_no_more and s.mnIterations == lit.mnIterations
        if kind is None:
            assert T is None and n == 0 and vb.size == 0
        else:
            v = r["refined"][h] if kind == "refined" else None
            Rr, tr = (v["R"][0], v["t"][0]) if v else (r["R"][h], r["t"][h])
            mask = v["mask"][0] if v else r["mask"][h]
            assert _same(T[:3, :3], Rr.astype(np.float32)) and _same(T[:3, 3], tr.astype(np.float32))
            assert _same(vb, mask) and n == int(mask.sum())
        if no_more:
            break
    if H:
        s, lit = fresh()
        s.mRansacMaxIts = lit.mRansacMaxIts = H
        T, vb, n = s.find()
        kind, h = lit.find()
        assert (T is None) == (kind is None)
        if kind is not None:
            v = r["refined"][h] if kind == "refined" else None
            Rr, tr = (v["R"][0], v["t"][0]) if v else (r["R"][h], r["t"][h])
            mask = v["mask"][0] if v else r["mask"][h]
            assert _same(T[:3, :3], Rr.astype(np.float32)) and _same(T[:3, 3], tr.astype(np.float32))
            assert _same(vb, mask) and n == int(mask.sum())


def test_planted_pose_is_recovered(gpu_ctx):
    """End to end on a planted candidate with 30 % mismatches and half a pixel of noise: the refined pose is the
    planted one within what that noise allows (1e-2 on R, 5e-2 m on t: ten times the 1e-3 / 5e-3 such noise moved
    a 100-inlier EPnP in the numpy definition), and nearly every planted inlier is found."""
    p = pnp.make_pnp_problem(150, seed=31, outlier_frac=0.3, pixel_noise=0.5)
    s = pnp.PnPsolver(p, rng=np.random.default_rng(5), ctx=gpu_ctx)
    s.SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991)
    T, no_more, vb, n = s.iterate(5)
    assert T is not None and not no_more
    assert np.abs(T[:3, :3] - p.meta["Rcw"]).max() < 1e-2 and np.abs(T[:3, 3] - p.meta["tcw"]).max() < 5e-2
    planted = ~p.meta["outlier"]
    assert n == int(vb.sum()) and (vb & planted).sum() >= 0.95 * planted.sum() and (vb & ~planted).sum() <= 2


def test_argument_errors_and_empty_batch(gpu_ctx):
    c = PC.case("n20_same")
    p = c["problem"]
    bad = c["draws"].copy()
    bad[2, 3] = p.n_pair - 3          # draw 3 must lie in [0, N-4]
    with pytest.raises(SqlmError):
        gpu_ctx.pnp_ransac([p], [bad], [c["min_inliers"]])
    with pytest.raises(SqlmError):
        gpu_ctx.pnp_ransac([p], [c["draws"]], [p.n_pair + 1])   # N < minInliers has no hypotheses
    assert gpu_ctx.pnp_ransac([], [], []) == []
    r = gpu_ctx.pnp_ransac([PC.case("n8_lt_min")["problem"]], [np.zeros((0, 4), np.int32)], [10])[0]
    assert r["first_return"] == -1 and r["best"] == -1 and r["n_refined"] == 0 and _same(r["Tcw"], np.eye(4, dtype=np.float32))
