"""The Sim3 RANSAC entry points exist at every layer: header, library, binding,
Python facade; their argument checks and the host-only helpers answer without
a GPU. The host evaluation of a hypothesis is the kernel's source text compiled
for the CPU: it must equal the numpy definition bit for bit."""
import os
import re

import numpy as np
import pytest

import sim3_ransac_cases as SC
import sim3_ransac_ref as R
from sqrtlm import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sqlm_sim3_ransac", "sqlm_sim3_ransac_get_inliers", "sqlm_sim3_ransac_get_hypothesis",
         "sqlm_sim3_ransac_max_its", "sqlm_sim3_ransac_scan", "sqlm_sim3_ransac_hypothesis_host"]


def test_header_binding_and_library_carry_the_names():
    hdr = open(os.path.join(ROOT, "include", "sqrtlm.h")).read()
    declared = set(re.findall(r"\b(sqlm_[A-Za-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for n in NAMES:
        assert n in declared, n
        assert n in _lib.EXPORTS, n
        assert hasattr(L, n), n


def test_invalid_arguments():
    L, p = _lib.lib(), _lib.ptr
    d, i = np.zeros(64), np.zeros(64, np.int32)
    off = np.zeros(2, np.int64)
    f = np.zeros(64, np.float32)
    # no context
    assert L.sqlm_sim3_ransac(None, 0, None, None, None, None, p(off), None, None, None, None, p(off), None, None,
                              None, None, None, None, None, None) == -1
    assert L.sqlm_sim3_ransac(None, 1, p(d), p(d), p(i), p(i), p(off), p(d), p(d), p(i), p(i), p(off), p(i), p(i),
                              p(i), p(f), p(f), p(f), p(i), p(i)) == -1
    assert L.sqlm_sim3_ransac_get_inliers(None, 0, 0, p(i)) == -1
    assert L.sqlm_sim3_ransac_get_hypothesis(None, 0, 0, p(i), p(f), p(f)) == -1
    assert L.sqlm_sim3_ransac_scan(-1, p(i), 6, p(i), None, None) == -1
    assert L.sqlm_sim3_ransac_scan(3, None, 6, p(i), None, None) == -1
    assert L.sqlm_sim3_ransac_scan(0, None, 6, None, None, None) == 0
    # the host evaluation: fewer than 3 pairs, a draw out of its range, a missing array
    c = SC.case("n20_h4_fix")
    args = _host_args(c, np.array([0, 1, 2], np.int32))
    assert L.sqlm_sim3_ransac_hypothesis_host(*args) == 0
    assert L.sqlm_sim3_ransac_hypothesis_host(2, *args[1:]) == -1
    for bad in ([20, 0, 0], [0, 19, 0], [0, 0, 18], [-1, 0, 0]):
        assert L.sqlm_sim3_ransac_hypothesis_host(*_host_args(c, np.array(bad, np.int32))) == -1, bad
    assert L.sqlm_sim3_ransac_hypothesis_host(*args[:4], None, *args[5:]) == -1


def test_max_its_equals_the_formula():
    L = _lib.lib()
    for n in list(range(0, 70)) + [100, 129, 150, 300, 1000, 10 ** 6, 2 ** 31 - 100]:
        for m in (3, 6, 20, 64, 100):
            for prob, cap in ((0.99, 300), (0.99, 5), (0.5, 300), (0.999, 10 ** 6)):
                got = L.sqlm_sim3_ransac_max_its(n, prob, m, cap)
                assert got == R.max_its(n, prob, m, cap), (n, m, prob, cap, got)
    assert L.sqlm_sim3_ransac_max_its(20, 0.99, 20, 300) == 1    # N == minInliers
    assert L.sqlm_sim3_ransac_max_its(19, 0.99, 20, 300) == 0    # N < minInliers: iterate() gives up at once
    assert L.sqlm_sim3_ransac_max_its(100, 0.99, 20, 300) == 300
    assert L.sqlm_sim3_ransac_max_its(50, 1.0, 6, 300) == 300    # log(0): clamped in double, no conversion of inf
    assert L.sqlm_sim3_ransac_max_its(50, 0.0, 6, 300) == 1
    assert L.sqlm_sim3_ransac_max_its(50, float("nan"), 6, 300) == 300


def test_scan_equals_the_literal_class():
    L, p = _lib.lib(), _lib.ptr
    rng = np.random.default_rng(11)
    for trial in range(200):
        H = int(rng.integers(1, 40))
        m = int(rng.integers(0, 12))
        counts = rng.integers(0, 16, H).astype(np.int32)
        flags = np.zeros(H, np.uint8)
        first, best = np.zeros(1, np.int64), np.zeros(1, np.int64)
        assert L.sqlm_sim3_ransac_scan(H, p(counts), m, p(flags), p(first), p(best)) == 0
        s = R.LiteralSolver(dict(count=counts, mask=np.zeros((H, 16), bool), T12=np.zeros((H, 4, 4), np.float32)), 16, m, H)
        want = np.zeros(H, np.uint8)
        rets = []
        step = int(rng.integers(1, 7))
        for _ in range(H + 2):          # iterate(step) until bNoMore: which hypotheses return
            T, no_more, _, n_in = s.iterate(step)
            if T is not None:
                rets.append(s.its - 1)
                assert n_in == counts[s.its - 1]
            if no_more:
                break
        # replay once more hypothesis by hypothesis for the update flags
        s2 = R.LiteralSolver(s.h, 16, m, H)
        for h in range(H):
            T, _, _, _ = s2.iterate(1)
            want[h] = 3 if T is not None else (1 if s2.best == h else 0)
        assert np.array_equal(flags, want), (counts, m)
        assert rets == np.flatnonzero(flags == 3).tolist()
        assert first[0] == (rets[0] if rets else -1) and best[0] == s2.best
        f2, fr, b2 = R.scan(counts, m)
        assert np.array_equal(f2, flags) and fr == first[0] and b2 == best[0]


def _host_args(c, draws):
    p, q = c["problem"], _lib.ptr
    n = p.n_pair
    out = dict(idx=np.zeros(3, np.int32), R=np.zeros((3, 3), np.float32), t=np.zeros(3, np.float32),
               s=np.zeros(1, np.float32), T12=np.zeros((4, 4), np.float32), T21=np.zeros((4, 4), np.float32),
               mask=np.zeros(n, np.uint8), count=np.zeros(1, np.int32))
    _host_args.out = out
    _host_args.keep = np.ascontiguousarray(draws, np.int32)
    return (n, q(p.intr1), q(p.intr2), int(p.fix_scale), q(p.X1c), q(p.X2c), q(c["max_err"][0]), q(c["max_err"][1]),
            q(_host_args.keep), q(out["idx"]), q(out["R"]), q(out["t"]), q(out["s"]), q(out["T12"]), q(out["T21"]),
            q(out["mask"]), q(out["count"]))


@pytest.mark.parametrize("name", [n for n in SC.NAMES if SC.SPECS[n][0] >= 6])
def test_host_build_of_the_kernel_arithmetic_equals_the_definition(name):
    """Every hypothesis of the case (at most 40 of them, the overridden ones included): bit for bit, NaN included."""
    L = _lib.lib()
    c, ref = SC.case(name), SC.reference(name)
    for h in range(min(c["n_hyp"], 40)):
        assert L.sqlm_sim3_ransac_hypothesis_host(*_host_args(c, c["draws"][h])) == 0
        o = _host_args.out
        assert np.array_equal(o["idx"], ref["idx"][h]), h
        for k, r in (("R", "R"), ("t", "t"), ("T12", "T12"), ("T21", "T21")):
            assert np.array_equal(o[k], ref[r][h], equal_nan=True), (h, k)
        assert np.array_equal(o["s"][0], ref["s"][h], equal_nan=True), h
        assert np.array_equal(o["mask"].astype(bool), ref["mask"][h]) and o["count"][0] == ref["count"][h], h
        assert np.array_equal(o["T21"], R.inverse_f32(o["R"], o["t"], o["s"])[0], equal_nan=True), h


def test_python_facade():
    from sqrtlm import sim3
    from sqrtlm.optimizer import Context
    for f in ("sim3_ransac", "sim3_ransac_inliers", "sim3_ransac_hypothesis"):
        assert callable(getattr(Context, f))
    for f in ("SetRansacParameters", "iterate", "find", "GetEstimatedRotation", "GetEstimatedTranslation",
              "GetEstimatedScale", "solve_batch"):
        assert callable(getattr(sim3.Sim3Solver, f)), f
    p, e1, e2 = sim3.make_sim3_ransac_problem(30, seed=2)
    s = sim3.Sim3Solver(p, e1, e2, rng=np.random.default_rng(1))
    assert s.mRansacMaxIts == R.max_its(30, 0.99, 6, 300) == s.draws.shape[0]
    s.SetRansacParameters(0.99, 20, 300)
    assert s.mRansacMaxIts == R.max_its(30, 0.99, 20, 300) and s.draws.shape == (s.mRansacMaxIts, 3)
    assert np.all(s.draws >= 0) and np.all(s.draws <= 29 - np.arange(3))
    s.SetRansacParameters(0.99, 31, 300)   # N < minInliers: bNoMore at once, no GPU call
    T, no_more, vb, n_in = s.iterate(5)
    assert T is None and no_more and vb.shape == (30,) and not vb.any() and n_in == 0
    with pytest.raises(ValueError):
        sim3.Sim3Solver(p, e1, e2)
    a = sim3.pack_ransac([p, p], [(e1, e2)] * 2, [np.zeros((2, 3), np.int32), np.zeros((0, 3), np.int32)], 6)
    assert a["pair_off"].tolist() == [0, 30, 60] and a["hyp_off"].tolist() == [0, 2, 2]
    assert a["max_err1"].shape == (60,) and a["draws"].dtype == np.int32 and a["min_inliers"].tolist() == [6, 6]
