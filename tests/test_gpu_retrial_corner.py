"""The LM retrial after a rejected step, and the second iteration, with
EdgeLidarCornerPoint edges: checks (a), (b), (d) and (e) of
tests/test_gpu_retrial.py on corner_plain (tests/corner_retrial_cases.py:
{pose 39: 150 edges of alternating kind, pose 12: 40 corner edges}), against
tests/lin_ref_corner.py under the same K = 100 x spread (floor 4 eps).

a. optimize(0, 1, lambda_0) takes the recorded 3 trials; the step against the
   reference at lambda_j.
b. the same problem started at lambda_j accepts its first trial: the same bits.
d. optimize(0, 2, lambda_0): iteration 2's last trial against the reference at
   the state and lambda_2 that optimize(0, 1, lambda_0) returned.
e. set_problem at that state, optimize(0, 1, lambda_2): the plain linearization
   where (d) used the speculative one, against the same reference.

The oracle has no corner edge; the trial counts are the reference's
(tests/test_retrial_ref_corner.py). Ratios measured on an MI355X when the test
was written:

                          trials  g      dx     dl     pose   chi2
    (a) retrial           3       0.10   1.2    0.43   1.2    1.0
    (d) iteration 2       3, 1    0.79   0.87   1.1    0.87   0.94
    (e) fresh             1       0.79   0.87   1.1    0.87   0.94

(b) was bit-equal, and (e) was bit-equal to (d) in g, dx, poses, points,
per-edge chi2, per-edge LiDAR errors and the trial chi2.
"""
import functools

import numpy as np
import pytest

import lin_ref_corner as LRC
from corner_retrial_cases import CASES, LIDAR, TWO_ITER, lambda_at, state_problem
from test_gpu_first_trial import K, _setenv, run_problem
from test_gpu_first_trial_corner import ratios

pytestmark = pytest.mark.gpu
NAME = "corner_plain"


@functools.lru_cache(maxsize=None)
def _problem():
    return CASES[NAME][0]()


def _lam_j():
    return lambda_at(CASES[NAME][1], CASES[NAME][3] - 1)


@functools.lru_cache(maxsize=None)
def _reference():
    return LRC.spreads(_problem(), _lam_j())


_state_refs = {}


def _state_reference(q, t, X, lam):
    key = (lam, q.tobytes(), t.tobytes(), X.tobytes())
    if key not in _state_refs:
        prob1 = state_problem(_problem(), q, t, X)
        _state_refs[key] = (prob1, LRC.spreads(prob1, lam))
    return _state_refs[key]


def _run(ctx, monkeypatch, lam=None, iterations=1, prob=None):
    prob = _problem() if prob is None else prob
    run = run_problem(ctx, prob, CASES[NAME][1] if lam is None else lam, _setenv(monkeypatch), dict(CASES[NAME][2]),
                      iterations=iterations)
    run["edge_chi2"] = ctx.edge_chi2()
    run["lid_err"] = ctx.lidar_error()
    return run


def _retrial(run):
    trials = CASES[NAME][3]
    assert run["n"] == 1 and run["st"]["iterations"] == 1
    assert run["st"]["trace_trials"] == [trials] and run["st"]["trials"] == trials, run["st"]
    assert run["st"]["n_active_edges"] == _problem().n_obs + sum(LIDAR.values())


def _show(tag, rt, *more):
    print(f"{tag}: " + " ".join(f"{k} {v[0]:.2g} ({v[1]:.1e}/{v[2]:.1e})" for k, v in rt.items()), *more)


def _bits(a, b, keys=("g", "dx", "q", "t", "X", "edge_chi2", "lid_err")):
    return [k for k in keys if not np.array_equal(a[k], b[k])]


def test_retrial_matches_reference(gpu_ctx, oracle, monkeypatch):
    run = _run(gpu_ctx, monkeypatch)
    _retrial(run)
    rt = ratios(oracle, _problem(), 0, run, _reference())
    _show(NAME, rt, run["st"]["trace_trials"], run["info"], run["lay"])
    for k, v in rt.items():
        assert v[0] <= K, (k, v)


def test_retrial_same_bits_as_fresh_trial(gpu_ctx, monkeypatch):
    a = _run(gpu_ctx, monkeypatch)
    _retrial(a)
    b = _run(gpu_ctx, monkeypatch, lam=_lam_j())
    assert b["n"] == 1 and b["st"]["trace_trials"] == [1] and b["st"]["trials"] == 1, b["st"]
    assert not _bits(a, b), _bits(a, b)
    assert a["st"]["trace_chi2"][0] == b["st"]["trace_chi2"][0]
    assert a["st"]["trace_lambda"][0] == b["st"]["trace_lambda"][0]
    assert a["st"]["chi2_begin"] == b["st"]["chi2_begin"]


def _two_iterations(ctx, monkeypatch):
    t1, t2 = TWO_ITER[NAME]
    r1 = _run(ctx, monkeypatch)
    _retrial(r1)
    r2 = _run(ctx, monkeypatch, iterations=2)
    st = r2["st"]
    assert r2["n"] == 2 and st["trace_trials"] == [t1, t2] and st["trials"] == t1 + t2, st
    assert st["trace_chi2"][0] == r1["st"]["trace_chi2"][0] and st["trace_lambda"][0] == r1["st"]["trace_lambda"][0]
    lam2 = r1["st"]["trace_lambda"][0]
    lam_j = _lam_j()
    assert lam_j * (1.0 / 3.0) <= lam2 <= lam_j * (2.0 / 3.0)
    return r1, r2, lam2, lambda_at(lam2, t2 - 1)


def test_second_iteration_matches_reference(gpu_ctx, oracle, monkeypatch):
    r1, r2, lam2, lam = _two_iterations(gpu_ctx, monkeypatch)
    prob1, reference = _state_reference(r1["q"], r1["t"], r1["X"], lam)
    run = dict(r2, st=dict(trace_chi2=[r2["st"]["trace_chi2"][1]]))
    rt = ratios(oracle, prob1, 0, run, reference)
    _show(f"{NAME} iteration 2", rt, r2["st"]["trace_trials"], f"lambda_2 {lam2:.6g} trial lambda {lam:.6g}")
    for k, v in rt.items():
        assert v[0] <= K, (k, v)


def test_fresh_linearization_matches_reference(gpu_ctx, oracle, monkeypatch):
    t1, t2 = TWO_ITER[NAME]
    r1, r2, lam2, lam = _two_iterations(gpu_ctx, monkeypatch)
    prob1, reference = _state_reference(r1["q"], r1["t"], r1["X"], lam)
    run = _run(gpu_ctx, monkeypatch, lam=lam2, prob=prob1)
    assert run["n"] == 1 and run["st"]["trace_trials"] == [t2] and run["st"]["trials"] == t2, run["st"]
    rt = ratios(oracle, prob1, 0, run, reference)
    differ = _bits(r2, run)
    same_chi2 = run["st"]["trace_chi2"][0] == r2["st"]["trace_chi2"][1]
    _show(f"{NAME} fresh linearization", rt,
          f"against iteration 2 of the two-iteration run: differing {differ or 'nothing'}, chi2 equal {same_chi2}")
    for k, v in rt.items():
        assert v[0] <= K, (k, v)
