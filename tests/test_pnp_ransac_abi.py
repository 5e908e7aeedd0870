"""The host side of sqlm_pnp_ransac without a GPU: the kernels' shared text
compiled for the CPU (sqlm_pnp_ransac_hypothesis_host / _refine_host) equals
the numpy definition bit for bit on every case, NaN for NaN; max_its against
the literal formula; the 4-draw index mapping exhaustively against the literal
vector; the scan against the literal solver, iterate(5) called again and again
after early returns; the Jacobi sweep counts; argument errors."""
import ctypes as C

import numpy as np
import pytest

import pnp_ransac_cases as PC
import pnp_ransac_ref as R
from sqrtlm import pnp
from sqrtlm._lib import lib, ptr, SQLM_OK


def _same(a, b):
    """Bit for bit, a NaN for a NaN (its sign and payload are the processor's, not the arithmetic's)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return a.tobytes() == b.tobytes()
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all()) and np.where(na, 0, a).tobytes() == np.where(nb, 0, b).tobytes()


_KEYS = (("ut", "ut"), ("eig", "eig"), ("betas", "betas"), ("rep_err", "rep"), ("R", "R"), ("t", "t"))


@pytest.mark.parametrize("name", PC.NAMES)
def test_host_build_equals_the_definition_bit_for_bit(name):
    c, r = PC.case(name), PC.reference(name)
    p = c["problem"]
    for h in range(c["n_hyp"]):
        o = pnp.hypothesis_host(p, c["draws"][h])
        assert _same(o["idx"], r["idx"][h]), (h, "idx")
        for a, b in _KEYS:
            assert _same(o[a], r[b][h]), (h, a)
        assert _same(o["mask"].astype(bool), r["mask"][h]) and o["n_inliers"] == r["count"][h]
        assert o["chosen"] == r["chosen"][h]
    for h, v in r["refined"].items():
        o = pnp.refine_host(p, r["mask"][h])
        for a, b in _KEYS:
            assert _same(o[a], v[b][0]), (h, a)
        assert _same(o["mask"].astype(bool), v["mask"][0]) and o["n_inliers"] == int(v["count"][0])
        assert o["chosen"] == int(v["chosen"][0])


def test_nan_and_inf_inputs_give_no_inliers_on_both_sides():
    c = PC.case("n20_same")
    p = c["problem"]
    for bad in (np.nan, np.inf):
        q = pnp.PnPProblem(intr=p.intr, Xw=p.Xw.copy(), uv=p.uv.copy(), sigma2=p.sigma2)
        q.Xw[int(R.indices(q.n_pair, c["draws"][3:4])[0, 0]), 1] = bad
        o = pnp.hypothesis_host(q, c["draws"][3])
        r = R.hypotheses(q, c["draws"][3:4])
        assert o["n_inliers"] == 0 and r["count"][0] == 0
        for a, b in _KEYS:
            assert _same(o[a], r[b][0]), a


def test_sweep_counts_are_converged_with_two_to_spare():
    """The library's Jacobi sweep counts are the smallest at which doubling them changes no stored bit of any
    hypothesis and refine of any case, plus two: two sweeps fewer already equal twice as many."""
    lib_sw = np.array([R.SWEEPS3, R.SWEEPS12, R.SWEEPSR])
    for name in PC.NAMES:
        c, r = PC.case(name), PC.reference(name)
        p = c["problem"]
        for h in range(c["n_hyp"]):
            a = pnp.hypothesis_host(p, c["draws"][h], sweeps=lib_sw - 2)
            b = pnp.hypothesis_host(p, c["draws"][h], sweeps=2 * (lib_sw - 2))
            d = pnp.hypothesis_host(p, c["draws"][h])
            for k in ("ut", "eig", "betas", "rep_err", "R", "t", "mask"):
                assert _same(a[k], b[k]) and _same(a[k], d[k]), (name, h, k)
        for h in r["refined"]:
            a = pnp.refine_host(p, r["mask"][h], sweeps=lib_sw - 2)
            b = pnp.refine_host(p, r["mask"][h], sweeps=2 * (lib_sw - 2))
            d = pnp.refine_host(p, r["mask"][h])
            for k in ("ut", "eig", "betas", "rep_err", "R", "t", "mask"):
                assert _same(a[k], b[k]) and _same(a[k], d[k]), (name, h, k)


def test_max_its_against_the_literal_formula():
    for n in list(range(0, 40)) + [63, 64, 65, 99, 100, 101, 150, 299, 300, 1000, 2001]:
        for min_in in (4, 8, 10, 15, 50):
            for eps in (0.4, 0.5, 0.9):
                for max_it in (3, 300):
                    assert pnp.pnp_max_its(n, 0.99, min_in, max_it, 4, eps) == R.max_its(n, 0.99, min_in, max_it, 4, eps), \
                        (n, min_in, eps, max_it)
    assert pnp.pnp_max_its(10, 0.99, 10, 300, 4, 0.5) == (1, 10)      # N == minInliers: one iteration
    assert pnp.pnp_max_its(9, 0.99, 10, 300, 4, 0.5) == (0, 10)       # N < minInliers: iterate gives up at once
    assert pnp.pnp_max_its(31, 0.99, 10, 300, 4, 0.5)[1] == 15        # (int)(31 * 0.5f)
    assert pnp.pnp_max_its(20, 0.99, 18, 300, 4, 0.5)[0] < 5          # iterate(5) runs past mRansacMaxIts


def test_index_mapping_exhaustively():
    dummy = pnp.make_pnp_problem(6, seed=1, outlier_frac=0.0)
    for n in (4, 5, 6):
        p = pnp.PnPProblem(intr=dummy.intr, Xw=dummy.Xw[:n], uv=dummy.uv[:n], sigma2=dummy.sigma2[:n])
        for a in range(n):
            for b in range(n - 1):
                for c in range(n - 2):
                    for d in range(n - 3):
                        o = pnp.hypothesis_host(p, [a, b, c, d])
                        assert o["idx"].tolist() == R.indices_literal(n, (a, b, c, d))


def _iterate(st, flags, max_its_, n):
    """iterate(n) on the flags of the scan, as sqrtlm.pnp.PnPsolver replays them; st = [mnIterations, best]."""
    cur = 0
    while st[0] < max_its_ or cur < n:
        cur += 1
        h = st[0]
        st[0] += 1
        if flags[h] & 2:
            st[1] = h
        if flags[h] & 4:
            return "refined", st[1], False
    if st[0] >= max_its_:
        return ("best", st[1], True) if st[1] >= 0 else (None, -1, True)
    return None, -1, False


def test_scan_against_the_literal_solver():
    rng = np.random.default_rng(7)
    for trial in range(60):
        H = int(rng.integers(1, 40))
        min_in = int(rng.integers(4, 12))
        counts = rng.integers(0, 25, H).astype(np.int32)
        refined_of = {h: int(rng.integers(0, 25)) for h in range(H)}
        flags_l, first_l, best_l = PC.scan_literal(counts, refined_of, min_in)
        recs = [h for h in range(H) if flags_l[h] & 2]
        flags, first, best, n_rec = pnp.scan(counts, [refined_of[h] for h in recs], min_in)
        assert _same(flags, flags_l) and (first, best, n_rec) == (first_l, best_l, len(recs))
        # the records do not depend on the refined counts: the first phase finds them without
        f0, _, b0, n0 = pnp.scan(counts, None, min_in)
        assert _same(f0 & 3, flags & 3) and not (f0 & 4).any() and (b0, n0) == (best, n_rec)
        # iterate(5) after early returns, the || of the loop condition included
        max_its_ = int(rng.integers(1, H + 1))
        lit, st = R.LiteralSolver(counts, lambda h: refined_of[h], 1 << 20, min_in, max_its_), [0, -1]
        while max(st[0] + 5, max_its_) <= H:      # a call runs to max_its_ and at least 5 hypotheses
            got, want = _iterate(st, flags, max_its_, 5), lit.iterate(5)
            assert got == want and st[0] == lit.mnIterations
    for name in PC.NAMES:
        c, r = PC.case(name), PC.reference(name)
        recs = sorted(r["refined"])
        flags, first, best, n_rec = pnp.scan(r["count"], [int(r["refined"][h]["count"][0]) for h in recs], c["min_inliers"])
        assert _same(flags, r["flags"]) and (first, best, n_rec) == (r["first_return"], r["best"], len(recs))


def test_argument_errors():
    L = lib()
    c = PC.case("n20_same")
    p = c["problem"]
    with pytest.raises(Exception):
        pnp.hypothesis_host(p, [0, 0, 0, p.n_pair - 3])                 # draw 3 must lie in [0, N-4]
    with pytest.raises(Exception):
        pnp.hypothesis_host(p, [-1, 0, 0, 0])
    small = pnp.PnPProblem(intr=p.intr, Xw=p.Xw[:3], uv=p.uv[:3], sigma2=p.sigma2[:3])
    with pytest.raises(Exception):
        pnp.hypothesis_host(small, [0, 0, 0, 0])                        # fewer than 4 pairs
    cnt = np.zeros(3, np.int32)
    assert L.sqlm_pnp_ransac_scan(-1, ptr(cnt), None, 0, 4, None, None, None, None) != SQLM_OK
    assert L.sqlm_pnp_ransac_scan(3, None, None, 0, 4, None, None, None, None) != SQLM_OK
    assert L.sqlm_pnp_ransac_scan(0, None, None, 0, 4, None, None, None, None) == SQLM_OK
    assert L.sqlm_pnp_ransac_hypothesis_host(20, *([None] * 16)) != SQLM_OK
    assert L.sqlm_pnp_ransac_refine_host(20, *([None] * 15)) != SQLM_OK
    assert L.sqlm_pnp_ransac(None, 0, *([None] * 16)) != SQLM_OK
    assert L.sqlm_pnp_ransac_get_inliers(None, 0, 0, None) != SQLM_OK
