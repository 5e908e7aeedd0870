"""The essential graph's LM retrial after a rejected step, its second iteration
and its exhausted iteration against the extended-precision reference.

tests/test_eg_gpu_first_trial.py pins a trial that is both the first of its
run and accepted. EGSolver::optimize (sqlm_eg.hip) does more than that: after
rho < 0 it launches the trial again on the same H0 / b with lambda *= ni --
k_egcr_gather (or k_eg_damp) re-gathers D, E, G, Go, Sc, rc (or A) with the new
lambda, the solve runs over the buffers the rejected trial left, Sd[1] and the
errors are overwritten while Sd[0] must stay; an accepted trial swaps Sd and
the next iteration re-linearizes, re-assembles H0 and b and takes lambda from
max(1/3, alpha); and after ten trials the iteration gives up. Every graph of
tests/test_eg_gpu.py accepts every trial, so none of this ran in a test, and a
retrial that kept anything of the rejected trial would still converge.

The harness, the rule and K are those of tests/test_eg_gpu_first_trial.py: b,
dx (sqlm_eg_get_last_step: the last trial launched), the poses, chi2 before
and after and the per-edge chi2 against tests/eg_lin_ref.py, each within
K = 100 x the reference's own float64-vs-longdouble spread (floor 4 eps), on
every layout the case admits (default = cyclic reduction, SQLM_EG_CR=0,
SQLM_EG_DENSE=1), the default layout's path asserted against
eg_retrial_cases.EXPECT, b and chi2_begin bit-identical across layouts. The
graphs (tests/eg_retrial_cases.py) are thrown far off their optimum and reject
3 .. 7 trials before they accept one; tests/test_eg_retrial_ref.py shows on
the CPU that every decision has |rho| >= 1e-3 and that every reference
compared is within the caps of tests/test_eg_lin_ref.py.

a. test_eg_retrial_matches_reference: eg_optimize(1, lambda_0) takes the
   recorded j + 1 trials; the step against the reference at lambda_j =
   lambda_0 2^(j (j + 1) / 2); trace_lambda[0] within 1e-6 of the oracle's.
b. test_eg_retrial_same_bits_as_fresh_trial: the same graph started at
   lambda_j accepts its first trial and gives the same bits (b, dx, poses,
   per-edge chi2, chi2, the lambda left).
c. test_eg_second_iteration_matches_reference: eg_optimize(2, lambda_0); the
   last trial of iteration 2 against the reference made at the S_1 and the
   lambda_2 that eg_optimize(1, lambda_0) returned, rejections inside
   iteration 2 included. The GPU's own S_1 and lambda_2 are the reference's
   inputs on purpose: the trial, not the LM control, is under test (lambda_2
   is held to the oracle's at 1e-6). The lambda iteration 2 leaves is held to
   the reference's rho at that S_1 through lambda max(1/3, min(1 - (2 rho -
   1)^3, 2/3)), at 1e-6: on five of the eight cases that factor is at neither
   bound, so this lambda shows k_eg_scale and both chi2 of iteration 2.
d. test_eg_fresh_linearization_same_bits: eg_set_problem at S_1, then
   eg_optimize(1, lambda_2): the same bits as (c), and within the rule.
   S_iw is the whole device state.
e. test_eg_jacobians_bitwise_at_states_used: sqlm_eg_get_jacobians at S_0 and
   at every layout's S_1 equals oracle.eg_edge_jacobians bit for bit: the
   reference takes the oracle's Jacobians as data, and these states are one
   or two radians from the optimum, where Sim3 log runs through acos and the
   branches of include/sqlm_libm.h that the few-degree drift of
   test_eg_numeric_jacobians_bitwise does not reach.
f. test_eg_exhausted_all_rejected: ten rejected trials: result 1, one
   iteration, chi2_end == chi2_begin, the poses bit-equal to the input, the
   last step against the reference at lambda_9, the per-edge chi2 against the
   reference's at S_0 (+) dx: the rejected trial's errors, as g2o leaves
   them. The same call again gives the same bits, and a following accepted
   run those of a freshly set problem.
g. test_eg_exhausted_tenth_accepted: the tenth trial accepted: result 1 all
   the same, the poses those of that trial, the lambda left within 1e-6 of
   the oracle's.

Ratios (GPU error / spread) measured on an MI355X when the test was written;
dx per layout (default, SQLM_EG_CR=0, SQLM_EG_DENSE=1), the other columns the
largest of the three layouts:

    (a) retrial       trials  b      dx     dx     dx     pose   chi2_0  chi2    edge_chi2
    band              5       0.17   2.2    1.1    1.1    1.9    0.038   0.072   0.17
    band_deep         8       0.17   4.1    3.1    3.1    2.9    0.038   0.096   0.15
    border3           5       0.16   1      0.31   0.37   1.4    0.037   0.089   0.19
    border3_deep      8       0.12   1.3    2.7    2.4    1.8    0.18    0.1     0.14
    border5           4       0.19   5.1    5.1    3.1    7.5    0.013   0.1     0.17
    free_scale        5       0.07   1.8    0.25   1.4    1.9    0.071   0.06    0.14
    info              5       0.21   0.96   0.91   0.89   2.2    0.09    0.22    0.074
    mixed             6       0.13   2.1    3      3.7    0.9    0.07    0.093   0.14

    (c) iteration 2, (d)
    band              5, 1    0.13   1.7    1.5    1.5    1.2    0.072   0.1     0.17
    band_deep         8, 1    0.16   2.5    1.3    1.3    2.3    0.096   0.055   0.19
    border3           5, 1    0.17   1.2    2.7    0.5    2.7    0.089   0.13    0.34
    border3_deep      8, 1    0.15   3.2    3.1    1.4    3.1    0.1     0.1     0.23
    border5           4, 1    0.18   4.5    3.1    3      4.5    0.1     0.079   0.086
    free_scale        5, 2    0.15   5.1    7.7    0.96   7.1    0.06    0.061   0.19
    info              5, 1    0.33   2      11     5.5    9.9    0.22    0.23    0.32
    mixed             6, 3    0.21   4.1    0.51   2.1    2.9    0.093   0.056   0.13

    (f) all_rejected  10      0.12   2.3    2.1    2.5    -      0.18    -       0.12
    (g) tenth_accepted 10     0.16   6.9    5.5    3.8    5      0.037   0.14    0.088

The largest is 11 (dx of info's second iteration on the arrow Cholesky,
1.6e-12 against a spread of 1.4e-13). (b) was bit-equal on every case and
layout, (d) bit-equal to (c) likewise (the one table serves both), (e)
bit-equal at all 32 states: the retrial keeps nothing of the rejected trials,
the second iteration nothing of the first. No defect showed.

Deliberately wrong scratch builds of sqlm_eg.hip (wrong numbers only, nothing
of them is committed; `stale lambda` is the lambda of the trial before, in a
retrial). A stale lambda in the solve gives a step that is rejected once more,
so those builds show first in the trial counts:

* k_egcr_gather with the stale lambda: all of (a) .. (e) fail on the default
  layout, every case one trial too many ([6] for [5], [9] for [8], ...); (f)
  dx 6.3e12; (g) rejects its tenth trial (chi2_end == chi2_begin).
* k_eg_damp with the stale lambda: the same on SQLM_EG_CR=0, the default
  layout passing first: (a) .. (e) one trial too many on every case, (f) dx
  6.3e12 on the arrow Cholesky, (g) rejects its tenth trial.
* Go refreshed only by the first trial of a run (stale in iteration 2; the
  issue's `Go not refreshed on a retrial`, see below): (c), (d) and (e)'s
  S_1 fail on the six cases with a border, iteration 2 taking 6 .. 8 trials
  for 1 .. 3; the two band cases, which have no Go product, pass.
* k_eg_scale with the stale lambda: rho alone is wrong, and only where the
  lambda factor is not at its cap does the API show it: (a), (b) and (c) of
  band_deep and border3_deep (trace_lambda 2.9e-2 and 1.2e-1 off, 3e4 x and
  1e5 x the 1e-6 bar; (b) differs in trace_lambda) and (g) (3.8e-3). The
  other cases' decisions and lambdas are unchanged by it.
* the errors computed again at Sd[0] before the copy-out: (f) edge_chi2
  1.3e15; nothing else.

Two builds pass everything, and no case can make them fail, because they
compute the same numbers:

* the H0 memset skipped after the first iteration: k_eg_assemble assigns
  every destination block (it does not accumulate), the destinations are
  fixed for the whole run, and nothing else writes H0, so from the second
  iteration on the memset clears zeros;
* Go refreshed only by the first trial of each iteration: G and Go are
  gathered from F0 and b, which no trial changes and which do not hold
  lambda, so a retrial's Go equals the one it would replace.
"""
import functools

import numpy as np
import pytest

import eg_lin_ref
from eg_retrial_cases import CASES, EXHAUSTED, EXPECT, GRAPH_OF, TWO_ITER, lambda_at, state_graph
from test_eg_gpu_first_trial import FLOOR, K, LD, _check_path, _maxrel, layouts_of, ratios, run_gpu

pytestmark = pytest.mark.gpu

BITS = ("b", "dx", "S", "edge_chi2")


@functools.lru_cache(maxsize=None)
def _graph(name):
    return (CASES.get(name) or EXHAUSTED[name])[0]()


def _layouts(name):
    return layouts_of(name, EXPECT[GRAPH_OF[name]])


_edge_data, _refs = {}, {}


def _reference(oracle, pg, lam):
    """eg_lin_ref.spreads() of the trial at pg's state and lam: once per
    (state, lambda), the oracle's per-edge values once per state."""
    state = (pg.Siw.tobytes(), pg.fixed.tobytes(), pg.fix_scale, pg.ei.tobytes(), pg.ej.tobytes(), pg.Sji.tobytes(),
             None if pg.info is None else pg.info.tobytes())
    if state not in _edge_data:
        _edge_data[state] = eg_lin_ref.edge_data(oracle, pg)
    if (state, lam) not in _refs:
        _refs[state, lam] = eg_lin_ref.spreads(oracle, pg, lam, _edge_data[state])
    return _refs[state, lam]


def _run(ctx, name, monkeypatch, layout, lam=None, iterations=1, pg=None):
    lam0 = (CASES.get(name) or EXHAUSTED[name])[1]
    return run_gpu(ctx, name, monkeypatch, layout, pg=_graph(name) if pg is None else pg,
                   lam=lam0 if lam is None else lam, iterations=iterations)


def _path(name, layout, run, pg=None):
    _check_path(name, layout, run, _graph(name) if pg is None else pg, EXPECT[GRAPH_OF[name]])


def _lam_j(name):
    return lambda_at(CASES[name][1], CASES[name][2] - 1)


def _retrial(name, run):
    trials = CASES[name][2]
    st = run["st"]
    assert run["n"] == 1 and st["iterations"] == 1 and st["result"] == 0, st
    assert st["trace_trials"] == [trials] and st["trials"] == trials, st


def _bits(a, b, keys=BITS):
    """Names of the quantities of two runs that differ in any bit."""
    return [k for k in keys if not np.array_equal(a[k], b[k])]


def _show(tag, rt, *more):
    print(f"{tag}: " + " ".join(f"{k} {v[0]:.2g} ({v[1]:.1e}/{v[2]:.1e})" for k, v in rt.items()), *more)


def _hold(tag, rt, *more):
    _show(tag, rt, *more)
    for k, v in rt.items():
        assert v[0] <= K, (tag, k, v)


def _same_across_layouts(runs):
    for layout, run in runs.items():
        assert np.array_equal(run["b"], runs["default"]["b"]), layout
        assert run["st"]["chi2_begin"] == runs["default"]["st"]["chi2_begin"], layout


_oracle_runs = {}


def _oracle(oracle, name, iterations):
    if (name, iterations) not in _oracle_runs:
        org = oracle.OracleEG(_graph(name))
        _oracle_runs[name, iterations] = org.optimize(iterations, (CASES.get(name) or EXHAUSTED[name])[1])[1]
    return _oracle_runs[name, iterations]


@pytest.mark.parametrize("name", sorted(CASES))
def test_eg_retrial_matches_reference(gpu_ctx, oracle, monkeypatch, name):
    sto = _oracle(oracle, name, 1)
    runs = {}
    for layout in _layouts(name):
        run = runs[layout] = _run(gpu_ctx, name, monkeypatch, layout)
        _retrial(name, run)
        _path(name, layout, run)
        assert abs(run["st"]["trace_lambda"][0] - sto["trace_lambda"][0]) <= 1e-6 * sto["trace_lambda"][0]
        _hold(f"(a) {name} {layout}", ratios(oracle, name, run, _graph(name), _reference(oracle, _graph(name), _lam_j(name))),
              run["st"]["trace_trials"], run["info"])
    _same_across_layouts(runs)


@pytest.mark.parametrize("name", sorted(CASES))
def test_eg_retrial_same_bits_as_fresh_trial(gpu_ctx, monkeypatch, name):
    for layout in _layouts(name):
        a = _run(gpu_ctx, name, monkeypatch, layout)
        _retrial(name, a)
        b = _run(gpu_ctx, name, monkeypatch, layout, lam=_lam_j(name))
        assert b["n"] == 1 and b["st"]["trace_trials"] == [1] and b["st"]["trials"] == 1, b["st"]
        assert not _bits(a, b), (layout, _bits(a, b))
        for k in ("chi2_begin", "chi2_end", "trace_chi2", "trace_lambda", "lambda_end"):
            assert a["st"][k] == b["st"][k], (layout, k, a["st"][k], b["st"][k])


_two = {}


def _two_iterations(ctx, name, monkeypatch, layout):
    """(run of eg_optimize(1), run of eg_optimize(2), lambda_2, lambda of
    iteration 2's last trial, the graph at S_1): once per case and layout."""
    if (name, layout) not in _two:
        t1, t2 = TWO_ITER[name]
        r1 = _run(ctx, name, monkeypatch, layout)
        _retrial(name, r1)
        r2 = _run(ctx, name, monkeypatch, layout, iterations=2)
        st = r2["st"]
        assert r2["n"] == 2 and st["iterations"] == 2 and st["result"] == 0, st
        assert st["trace_trials"] == [t1, t2] and st["trials"] == t1 + t2, st
        assert st["trace_chi2"][0] == r1["st"]["trace_chi2"][0] and st["trace_lambda"][0] == r1["st"]["trace_lambda"][0]
        assert st["chi2_begin"] == r1["st"]["chi2_begin"]
        lam2 = r1["st"]["trace_lambda"][0]
        _two[name, layout] = (r1, r2, lam2, lambda_at(lam2, t2 - 1), state_graph(_graph(name), r1["S"]))
    return _two[name, layout]


def _as_first(r2):
    """Iteration 2 of a two-iteration run in the terms of ratios(): its
    linearization point's chi2 is the first iteration's trace entry."""
    return dict(r2, st=dict(r2["st"], chi2_begin=r2["st"]["trace_chi2"][0]))


@pytest.mark.parametrize("name", sorted(TWO_ITER))
def test_eg_second_iteration_matches_reference(gpu_ctx, oracle, monkeypatch, name):
    sto = _oracle(oracle, name, 2)
    for layout in _layouts(name):
        r1, r2, lam2, lam, pg1 = _two_iterations(gpu_ctx, name, monkeypatch, layout)
        _path(name, layout, r2)
        assert sto["trace_trials"] == r2["st"]["trace_trials"]
        assert abs(lam2 - sto["trace_lambda"][0]) <= 1e-6 * sto["trace_lambda"][0], (lam2, sto["trace_lambda"])
        reference = _reference(oracle, pg1, lam)
        _hold(f"(c) {name} {layout}", ratios(oracle, name, _as_first(r2), pg1, reference),
              r2["st"]["trace_trials"], f"lambda_2 {lam2:.6g} trial lambda {lam:.6g}")
        # The lambda iteration 2 leaves shows its rho (k_eg_scale, the two chi2). Held to the reference's at
        # the GPU's own S_1, not to the oracle's: the numeric Jacobians turn the 1e-13 between the two S_1
        # into 1e-5 of that lambda (1e-13 of relative noise on S_1 moves the oracle's own by 3e-4).
        rho = eg_lin_ref.trial_rho(oracle, pg1, reference[1], lam, LD)[0]
        left = float(eg_lin_ref.lambda_accepted(lam, rho))
        assert abs(r2["st"]["trace_lambda"][1] - left) <= 1e-6 * left, (layout, r2["st"]["trace_lambda"], left, rho)


@pytest.mark.parametrize("name", sorted(TWO_ITER))
def test_eg_fresh_linearization_same_bits(gpu_ctx, oracle, monkeypatch, name):
    t1, t2 = TWO_ITER[name]
    for layout in _layouts(name):
        r1, r2, lam2, lam, pg1 = _two_iterations(gpu_ctx, name, monkeypatch, layout)
        run = _run(gpu_ctx, name, monkeypatch, layout, lam=lam2, pg=pg1)
        st = run["st"]
        assert run["n"] == 1 and st["trace_trials"] == [t2] and st["trials"] == t2, st
        _path(name, layout, run, pg1)
        assert not _bits(r2, run), (layout, _bits(r2, run))
        assert st["chi2_begin"] == r2["st"]["trace_chi2"][0], layout
        assert st["trace_chi2"][0] == r2["st"]["trace_chi2"][1] and st["chi2_end"] == r2["st"]["chi2_end"], layout
        assert st["trace_lambda"][0] == r2["st"]["trace_lambda"][1], layout
        _hold(f"(d) {name} {layout}", ratios(oracle, name, run, pg1, _reference(oracle, pg1, lam)))


def _oracle_jacobians(oracle, pg):
    out = np.zeros((pg.n_edge, 2, 7, 7))
    for e in range(pg.n_edge):
        i, j = pg.ei[e], pg.ej[e]
        out[e] = oracle.eg_edge_jacobians(pg.Siw[i], pg.Siw[j], pg.Sji[e], pg.fix_scale,
                                          int(pg.fixed[i] == 0), int(pg.fixed[j] == 0))
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_eg_jacobians_bitwise_at_states_used(gpu_ctx, oracle, monkeypatch, name):
    """The reference takes the oracle's Jacobians as data: the GPU's are the
    same bits at every linearization point of (a) .. (d), far from the optimum."""
    states = {"S0": _graph(name)}
    for layout in _layouts(name):
        states["S1 " + layout] = _two_iterations(gpu_ctx, name, monkeypatch, layout)[4]
    for tag, pg in states.items():
        gpu_ctx.eg_set_problem(pg)
        Jg = gpu_ctx.eg_jacobians()
        Jo = _oracle_jacobians(oracle, pg)
        assert np.abs(Jo).max() > 0.1
        diff = np.nonzero(np.any(Jg.reshape(pg.n_edge, -1) != Jo.reshape(pg.n_edge, -1), axis=1))[0]
        assert diff.size == 0, (name, tag, diff[:8], np.abs(Jg - Jo).max())


def _exhausted(ctx, name, monkeypatch, layout):
    make, lam0, accepted = EXHAUSTED[name]
    run = _run(ctx, name, monkeypatch, layout, iterations=5)
    st = run["st"]
    assert st["trace_trials"] == [10] and st["trials"] == 10, st
    assert run["n"] == 1 and st["iterations"] == 1 and st["result"] == 1, st
    _path(name, layout, run)
    return run


def test_eg_exhausted_all_rejected(gpu_ctx, oracle, monkeypatch):
    name = "all_rejected"
    pg, lam0 = _graph(name), EXHAUSTED[name][1]
    assert not EXHAUSTED[name][2]
    lam9 = lambda_at(lam0, 9)
    reference = _reference(oracle, pg, lam9)
    sp, ref = reference[0], reference[1]
    runs = {}
    for layout in _layouts(name):
        run = runs[layout] = _exhausted(gpu_ctx, name, monkeypatch, layout)
        st = run["st"]
        assert st["chi2_end"] == st["chi2_begin"] and st["trace_chi2"] == [st["chi2_begin"]], st
        assert st["trace_lambda"] == [lambda_at(lam0, 10)] and st["lambda_end"] == lambda_at(lam0, 10), st
        assert np.array_equal(run["S"], pg.Siw)
        # the last trial launched: the tenth, rejected
        rt = {}
        rt["b"] = _maxrel(run["b"].reshape(-1), ref.b), sp["b"]
        rt["dx"] = _maxrel(run["dx"].reshape(-1), ref.dx), sp["dx"]
        rt["chi2_0"] = float(abs(LD(st["chi2_begin"]) - ref.chi2_0) / ref.chi2_0), sp["chi2_0"]
        # the errors are the rejected trial's, as g2o leaves them: at S_0 (+) dx of the GPU
        S_t = eg_lin_ref.oplus_poses(oracle, pg, ref.free, run["dx"])
        act, e = eg_lin_ref.edge_errors(oracle, pg, S_t)
        c_hi = eg_lin_ref.edge_chi2(pg, act, e, LD)
        c_lo = eg_lin_ref.edge_chi2(pg, act, e, np.float64)
        rt["edge_chi2"] = _maxrel(run["edge_chi2"][act], c_hi), _maxrel(c_lo, c_hi)
        c_0 = eg_lin_ref.edge_chi2(pg, *eg_lin_ref.edge_errors(oracle, pg), LD)
        assert _maxrel(c_hi, c_0) > 1e-3 and c_hi.sum() > ref.chi2_0          # not the errors of S_0
        _hold(f"(f) {name} {layout}", {k: (err / max(s, FLOOR), err, s) for k, (err, s) in rt.items()}, st["trace_trials"])
        # the context's state is S_0 still: the same call again gives the same bits, ...
        n2, st2 = gpu_ctx.eg_optimize(5, lam0)
        b2, dx2 = gpu_ctx.eg_last_step()
        again = dict(b=b2, dx=dx2, S=gpu_ctx.eg_poses(), edge_chi2=gpu_ctx.eg_edge_chi2())
        assert not _bits(run, again), (layout, _bits(run, again))
        assert (n2, st2["trace_trials"], st2["chi2_begin"], st2["chi2_end"]) == (1, [10], st["chi2_begin"], st["chi2_end"])
        # ... and a run that accepts gives those of a freshly set problem
        n3, st3 = gpu_ctx.eg_optimize(1, 1.0)
        b3, dx3 = gpu_ctx.eg_last_step()
        after = dict(b=b3, dx=dx3, S=gpu_ctx.eg_poses(), edge_chi2=gpu_ctx.eg_edge_chi2(), st=st3)
        fresh = _run(gpu_ctx, name, monkeypatch, layout, lam=1.0)
        assert fresh["st"]["trace_trials"] == [1] and not np.array_equal(fresh["S"], pg.Siw)
        assert not _bits(fresh, after), (layout, _bits(fresh, after))
        assert st3["trace_chi2"] == fresh["st"]["trace_chi2"] and st3["chi2_begin"] == st["chi2_begin"]
    _same_across_layouts(runs)


def test_eg_exhausted_tenth_accepted(gpu_ctx, oracle, monkeypatch):
    name = "tenth_accepted"
    pg, lam0 = _graph(name), EXHAUSTED[name][1]
    assert EXHAUSTED[name][2]
    lam9 = lambda_at(lam0, 9)
    sto = _oracle(oracle, name, 5)
    assert sto["trace_trials"] == [10] and sto["result"] == 1
    runs = {}
    for layout in _layouts(name):
        run = runs[layout] = _exhausted(gpu_ctx, name, monkeypatch, layout)
        st = run["st"]
        assert st["chi2_end"] < st["chi2_begin"] and st["trace_chi2"] == [st["chi2_end"]], st
        assert lam9 * (1.0 / 3.0) <= st["trace_lambda"][0] <= lam9 * (2.0 / 3.0), st
        assert abs(st["trace_lambda"][0] - sto["trace_lambda"][0]) <= 1e-6 * sto["trace_lambda"][0], (st, sto)
        _hold(f"(g) {name} {layout}", ratios(oracle, name, run, pg, _reference(oracle, pg, lam9)), st["trace_trials"])
    _same_across_layouts(runs)
