"""Conditions on the Sim3 RANSAC cases (tests/sim3_ransac_cases.py), asserted on
the numpy definition (tests/sim3_ransac_ref.py) alone: what
tests/test_gpu_sim3_ransac.py relies on when it holds the GPU to that
definition. No GPU needed."""
import itertools

import numpy as np
import pytest

import sim3_ransac_cases as SC
import sim3_ransac_ref as R
from sqrtlm import sim3, synth

U32 = 2.0 ** -24  # unit roundoff of float32


# ---- the draw -> pair index mapping ------------------------------------------------
@pytest.mark.parametrize("n", [3, 4, 5])
def test_closed_form_mapping_equals_the_literal_swap_remove(n):
    triples = list(itertools.product(range(n), range(n - 1), range(n - 2)))
    assert len(triples) == n * (n - 1) * (n - 2)
    got = R.swap_remove_closed(n, np.array(triples))
    for t, g in zip(triples, got):
        lit = R.swap_remove_literal(n, t)
        assert lit == g.tolist(), (n, t)
        assert len(set(lit)) == 3


def test_mapping_on_random_draws():
    rng = np.random.default_rng(3)
    for n in (6, 64, 65, 301):
        d = np.stack([rng.integers(0, n - i, 500) for i in range(3)], axis=1)
        d[:20, 1] = d[:20, 0].clip(max=n - 2)   # the collisions the closed form must resolve
        d[20:40, 2] = d[20:40, 1].clip(max=n - 3)
        d[40:60, 0] = n - 2
        got = R.swap_remove_closed(n, d)
        assert all(R.swap_remove_literal(n, t) == g.tolist() for t, g in zip(d, got))


def test_max_its_formula():
    assert R.max_its(100, 0.99, 20, 300) == 300       # ceil(log(0.01) / log(1 - 0.2^3)) = 574, capped
    assert R.max_its(20, 0.99, 15, 300) == 9          # ceil(4.605 / -log(1 - 0.421875))
    assert R.max_its(20, 0.99, 20, 300) == 1 and R.max_its(19, 0.99, 20, 300) == 0
    assert R.max_its(10 ** 6, 0.99, 6, 300) == 300    # pow(eps, 3) underflows 1 - x to 1: log 0, -inf, capped
    assert R.max_its(50, 1.0, 6, 300) == 300 and R.max_its(50, 0.0, 6, 300) == 1


# ---- noise-free data: the planted Sim3 comes back --------------------------------------
@pytest.mark.parametrize("name", ["n20_h4_fix", "n63_h5", "n64_h300_k2"])
def test_noise_free_mismatches_return_the_planted_sim3(name):
    """The first returning hypothesis has exactly the planted inliers and the true Sim3.

    Bound. The points are float32 roundings of exact ones: each coordinate is
    off by at most e = u * Xmax (u = 2^-24). A rotation fitted to three points
    whose triangle has smallest altitude h turns by at most ~ e' / h for a
    point error e'; with three coordinates, two point sets and the float32
    stores of the relative coordinates, M, N and R (each another error of the
    size of e) we allow ang = 16 e / h. The scale is a ratio of lengths of
    order h: 16 e / h relative. The translation O1 - s R O2 inherits both,
    times |O2|, plus e for the centroids."""
    c, ref = SC.case(name), SC.reference(name)
    p = c["problem"]
    h = ref["first_return"]
    assert h >= 0
    assert np.array_equal(ref["mask"][h], ~p.meta["outlier"])
    S = p.meta["S12_true"]
    R_true = synth.quat_to_mat(S[:4])[0]
    tri1 = p.X1c[ref["idx"][h]]
    sides = [np.linalg.norm(tri1[(k + 1) % 3] - tri1[k]) for k in range(3)]
    area2 = np.linalg.norm(np.cross(tri1[1] - tri1[0], tri1[2] - tri1[0]))
    alt = area2 / max(sides) / max(S[7], 1.0)        # the smaller of the two triangles' smallest altitudes
    e = U32 * max(np.abs(p.X1c).max(), np.abs(p.X2c).max())
    ang = 16 * e / alt
    O2 = np.linalg.norm(p.X2c[ref["idx"][h]].mean(axis=0))
    errR = np.abs(ref["R"][h] - R_true).max()
    errs = abs(float(ref["s"][h]) - S[7]) / S[7]
    errt = np.abs(ref["t"][h] - S[4:7]).max()
    tol_t = 2 * ang * S[7] * O2 + e
    print(f"{name}: h {h} altitude {alt:.2f} m  R {errR:.2e}/{ang:.2e}  s {errs:.2e}/{ang:.2e}  t {errt:.2e}/{tol_t:.2e}")
    assert alt > 1.0, "the case's good triple is badly conditioned"
    assert errR <= ang and errt <= tol_t
    if p.fix_scale:
        assert ref["s"][h] == 1.0
    else:
        assert errs <= ang


# ---- what the case list covers -----------------------------------------------------------
def test_case_list_covers_the_shapes():
    cs = {n: SC.case(n) for n in SC.NAMES}
    assert sorted(c["problem"].n_pair for c in cs.values()) == [3, 5, 20, 20, 20, 20, 20, 63, 64, 65, 129, 300]
    assert sorted(set(c["n_hyp"] for c in cs.values())) == [0, 1, 4, 5, 8, 13, 300]
    assert any(c["problem"].fix_scale for c in cs.values()) and any(not c["problem"].fix_scale for c in cs.values())
    assert any(not np.array_equal(c["problem"].intr1, c["problem"].intr2) for c in cs.values())
    mid = SC.NAMES.index("n5_lt_min")
    assert 0 < mid < len(SC.NAMES) - 1 and cs["n5_lt_min"]["n_hyp"] == 0
    assert cs["n5_lt_min"]["problem"].n_pair < cs["n5_lt_min"]["min_inliers"]
    assert cs["n20_min_eq_n"]["min_inliers"] == 20 and cs["n20_min_eq_n"]["n_hyp"] == 1
    for c in cs.values():   # every draw is in its range and the thresholds are the truncated ones
        d, n = c["draws"], c["problem"].n_pair
        assert d.shape == (c["n_hyp"], 3) and np.all(d >= 0) and np.all(d <= n - 1 - np.arange(3))
        lv = c["problem"].meta["levels"]
        s2 = sim3.orb_level_sigma2()
        assert np.array_equal(c["max_err"][0], np.floor(9.210 * s2[lv[:, 0]].astype(np.float64)).astype(np.int32))
    assert sim3.ransac_max_err(sim3.orb_level_sigma2()).tolist() == [9, 13, 19, 27, 39, 57, 82, 118]


def test_case_list_covers_the_bookkeeping():
    refs = {n: SC.reference(n) for n in SC.NAMES}
    cs = {n: SC.case(n) for n in SC.NAMES}
    assert any(r["first_return"] == 0 for r in refs.values()), "no return at hypothesis 0"
    assert any(r["first_return"] > 4 for r in refs.values()), "no return later than the first call's five"
    never = [n for n, r in refs.items() if cs[n]["n_hyp"] > 1 and r["first_return"] < 0]
    assert never and all(refs[n]["best"] >= 0 and refs[n]["count"][refs[n]["best"]] > 0 for n in never)

    def tie(r):
        b = 0
        for c, f in zip(r["count"], r["flags"]):
            if f & 1 and c == b and b > 0:
                return True
            b = max(b, c) if f & 1 else b
        return False
    assert any(tie(r) for r in refs.values()), "no tie c_h == b that updates the best"
    # a hypothesis with fewer inliers than the best so far neither updates nor returns, even above minInliers
    assert any(np.any((r["count"] > cs[n]["min_inliers"]) & (r["flags"] == 0)) for n, r in refs.items())
    last = [n for n, r in refs.items() if cs[n]["n_hyp"] > 1 and r["flags"][-1] == 3]
    assert last, "no return at the last hypothesis"
    for n in last:   # bNoMore on the call after it
        s = SC.literal(n)
        out = []
        while len(out) <= cs[n]["n_hyp"] + 1 and not (out and out[-1][1]):
            out.append(s.iterate(5))
        assert out[-1][1] and out[-1][0] is None and out[-2][0] is not None and not out[-2][1]


@pytest.mark.parametrize("name", SC.NAMES)
def test_scan_equals_the_literal_class(name):
    c, ref = SC.case(name), SC.reference(name)
    s = SC.literal(name)
    flags = np.zeros(c["n_hyp"], np.uint8)
    n_more = 0
    for _ in range(c["n_hyp"] + 2):
        before = s.its
        T, no_more, vb, n_in = s.iterate(1)
        if s.its > before:
            h = s.its - 1
            flags[h] = (3 if T is not None else (1 if s.best == h else 0))
            if T is not None:
                assert n_in == ref["count"][h] and np.array_equal(vb, ref["mask"][h])
                assert np.array_equal(T, ref["T12"][h])
            else:
                assert n_in == 0 and not vb.any()
        n_more += no_more
    assert np.array_equal(flags, ref["flags"]) and n_more >= 2
    assert s.best == (ref["best"] if c["n_hyp"] else None)
    T, vb, n_in = SC.literal(name).find()
    assert (T is None) == (ref["first_return"] < 0)
    if T is not None:
        assert np.array_equal(T, ref["T12"][ref["first_return"]]) and n_in == ref["count"][ref["first_return"]]


# ---- the special hypotheses -------------------------------------------------------------
def test_exact_translation_gives_the_identity_rotation():
    c, ref = SC.case("n20_translation"), SC.reference("n20_translation")
    S = c["problem"].meta["S12_true"]
    assert c["n_hyp"] == 5 and not c["problem"].meta["outlier"].any()
    for h in range(5):
        assert np.array_equal(ref["R"][h], np.eye(3, dtype=np.float32)), h
        assert ref["s"][h] == np.float32(S[7]) and np.array_equal(ref["t"][h], S[4:7].astype(np.float32))
        assert ref["count"][h] == 20
    ld = R.closed_form(*R.gather(c["problem"].X1c, c["problem"].X2c, ref["idx"]), False, ld=True)
    assert np.array_equal(ld["R"], np.broadcast_to(np.eye(3), (5, 3, 3)))


def test_coinciding_points():
    free, fix = SC.reference("n20_same_free"), SC.reference("n20_same_fix")
    assert free["idx"][0].tolist() == [0, 1, 2] and fix["idx"][0].tolist() == [0, 1, 2]
    # den = 0: 0 / 0, a NaN transform, every comparison false
    assert np.isnan(free["s"][0]) and np.isnan(free["t"][0]).all() and free["count"][0] == 0
    assert np.array_equal(free["R"][0], np.eye(3, dtype=np.float32))
    # fixed scale: R = I, s = 1, t = O1 - O2: finite, and the three copies of the pair are inliers
    assert np.array_equal(fix["R"][0], np.eye(3, dtype=np.float32)) and fix["s"][0] == 1.0
    assert np.isfinite(fix["t"][0]).all() and fix["mask"][0][:3].all()
    ld = R.closed_form(*R.gather(SC.case("n20_same_free")["problem"].X1c, SC.case("n20_same_free")["problem"].X2c,
                                 free["idx"][:1]), False, ld=True)
    assert np.isnan(ld["s"][0]) and np.isnan(ld["t"][0]).all()


def test_jacobi_has_converged_after_the_fixed_sweeps():
    """Twice the sweeps change nothing on the well-conditioned hypotheses, and the quaternion is the eigenvector."""
    for name in ("n64_h300_k2", "n300_h300"):
        c, ref = SC.case(name), SC.reference(name)
        p = c["problem"]
        P1, P2 = R.gather(p.X1c, p.X2c, ref["idx"])
        more = R.closed_form(P1, P2, p.fix_scale, sweeps=2 * R.SWEEPS)
        for k in ("R", "t", "s"):
            assert np.array_equal(more[k], ref[k], equal_nan=True), (name, k)
    rng = np.random.default_rng(5)
    A = rng.normal(size=(200, 4, 4)).astype(np.float32).astype(np.float64)
    A = A + np.transpose(A, (0, 2, 1))
    q = R.jacobi_top(A, np.float64, R.SWEEPS)
    w, V = np.linalg.eigh(A)
    assert np.abs(np.abs(np.einsum("hi,hi->h", q, V[:, :, -1])) - 1).max() < 1e-12
    assert np.all(q[:, 0] >= 0) and np.abs(np.linalg.norm(q, axis=1) - 1).max() < 1e-15


def test_chain_case_is_accepted_with_margin(oracle):
    """The planted candidate of the chain test: RANSAC returns, and OptimizeSim3 on its
    inliers keeps far more than the 20 that LoopClosing.cc:516 asks for."""
    import sim3_ref
    c = SC.chain_case()
    p = c["problem"]
    r = R.hypotheses(p.X1c, p.X2c, p.intr1, p.intr2, p.fix_scale, c["max_err"][0], c["max_err"][1], c["draws"])
    _, first, _ = R.scan(r["count"], c["min_inliers"])
    assert first >= 0
    planted = int((~p.meta["outlier"]).sum())
    assert r["count"][first] >= 0.9 * planted and not (r["mask"][first] & p.meta["outlier"]).any()
    sub = SC.chain_subproblem(c, r["R"][first], r["t"][first], r["s"][first], r["mask"][first])
    out = sim3_ref.optimize(oracle, sub)
    print("chain: RANSAC inliers", int(r["count"][first]), "of", planted, "planted; OptimizeSim3 inliers", out["n_inliers"])
    assert out["n_inliers"] >= 3 * 20


def test_generator():
    p, e1, e2 = sim3.make_sim3_ransac_problem(40, seed=3, outlier_frac=0.25, point_noise=0.01, intr2=SC.K2)
    assert p.n_pair == 40 and e1.shape == e2.shape == (40,) and e1.dtype == np.int32
    assert p.meta["outlier"].sum() == 10 and not np.array_equal(p.intr1, p.intr2)
    assert np.array_equal(p.X1c, p.X1c.astype(np.float32)) and np.array_equal(p.X2c, p.X2c.astype(np.float32))
    lv = np.tile([[0, 7]], (12, 1))
    p, e1, e2 = sim3.make_sim3_ransac_problem(12, seed=1, outlier_frac=0.0, levels=lv, fix_scale=True)
    assert e1.tolist() == [9] * 12 and e2.tolist() == [118] * 12 and p.fix_scale and p.meta["S12_true"][7] == 1.0
