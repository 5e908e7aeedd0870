"""The LM retrial after a rejected step, and the second iteration, against the
extended-precision reference.

tests/test_gpu_first_trial.py pins a trial that is both the first of its run
and accepted. Two stateful paths of the host driver (sqlm_lm.cpp) lie beyond
it: after a rejected trial lm_host launches the trial again with a larger
lambda and without swap_state -- launch_damp re-damps the landmark factors,
the trial state buffers and every speculative buffer of the rejected trial
are overwritten, possibly while its side-stream camera pass is still joined
through ev_spec_join -- and the second iteration runs on the linearization the
accepted trial made speculatively at its own state, swapped in by swap_state.
A retrial that kept anything of the rejected trial (damping on top of the old
damping, a stale dx, a stale S diagonal), or a second iteration on stale
weights, still converges and passes every 1e-6 end-state test.

The harness, the rule and K are those of tests/test_gpu_first_trial.py: g, dx
(sqlm_get_last_step: the last trial the run launched, here the accepted one),
the landmark step, the updated poses and the trial chi2 at the returned state
against tests/lin_ref.py, each within K = 100 x the reference's own
float64-vs-longdouble spread of that quantity (floor 4 eps). The cases
(tests/retrial_cases.py) reject 2 .. 8 trials before they accept one;
tests/test_retrial_ref.py shows on the CPU that every one of those decisions
has a margin of 1e-3, which no rounding crosses.

a. test_retrial_matches_reference: optimize(0, 1, lambda_0) takes the
   recorded j + 1 trials; the step is compared with the reference at
   lambda_j = lambda_0 2^(j (j + 1) / 2).
b. test_retrial_same_bits_as_fresh_trial: the same problem started at
   lambda_j accepts its first trial, and gives the same bits: a retrial is the
   same launches on the same linearization with another lambda.
c. test_schedules_same_bits: (a) under SQLM_NO_SPEC=1, SQLM_TRIAL_STORES=1,
   SQLM_NO_POSE_FUSE=1 and SQLM_TILE_PROD=0, one Huber and one no-robust case.
d. test_second_iteration_matches_reference: optimize(0, 2, lambda_0); the
   step of iteration 2's last trial against the reference made at the state
   (q1, t1, X1) and the lambda_2 that optimize(0, 1, lambda_0) returned, m
   rejections inside iteration 2 included. The GPU's own state and lambda_2
   are the reference's inputs on purpose: the trial, not the LM control, is
   under test (lambda_2 is held to the oracle's at 1e-6, the parity bar).
e. test_fresh_linearization_matches_reference: set_problem at (q1, t1, X1),
   optimize(0, 1, lambda_2): the plain linearize kernel at the state where (d)
   used the speculative linearization, against the same reference.

The device keeps each pose as (q, t) and as the rotation matrix made from that
q by the same q_to_mat (k_pose_prep after set_problem, k_pose_update in a
trial), so (q1, t1) carries the whole pose state bit for bit and (e) starts
from the state (d)'s second iteration had; no ratio is spent on it.

Ratios (GPU error / spread) measured on an MI355X when the test was written,
with the trials per iteration:

    (a) retrial           trials  g      dx     dl     pose   chi2
    border_plain          4       1.3    0.28   0.23   0.29   0.14
    classes_plain         6       0.94   4.5    4.8    2.9    0.071
    cr_huber              7       0.82   0.16   0.37   0.22   0.10
    cr_huber_deep         9       0.085  0.063  0.090  0.064  0.81
    cr_plain              4       0.22   0.36   0.49   0.12   0.80
    fixed_plain           3       0.15   0.46   0.24   0.47   0.091
    lidar_plain           3       0.069  2.4    0.53   1.8    1.0
    rows_plain            3       1.0    4.2    1.9    4.2    0.025
    stereo_plain          9       0.37   1.3    0.60   2.4    0.21

    (d) iteration 2, (e)  trials  g      dx     dl     pose   chi2
    border_plain          4, 1    4.6    1.8    2.8    1.6    0.073
    classes_plain         6, 3    1.4    0.70   0.82   0.57   0.0072
    cr_huber              7, 1    0.78   0.15   0.15   0.35   0.13
    cr_huber_deep         9, 5    1.7    0.58   0.78   0.30   2.3
    cr_plain              4, 3    0.35   0.49   0.16   0.52   0.20
    fixed_plain           3, 3    0.46   0.46   0.44   0.47   0.13
    stereo_plain          9, 1    0.62   3.6    1.0    1.6    0.079

The largest is 4.8 (dl of classes_plain, 3.1e-13 against a spread of 6.5e-14).
(b) and (c) were bit-equal on every case, and (e) was bit-equal to (d) in g,
dx, poses, points, per-edge chi2 and the trial chi2 on all seven cases (the one
table serves both): the retrial keeps nothing of the rejected trials, the
speculative linearization is the plain one. No defect showed.

Deliberately wrong builds of the driver, tried on scratch copies (wrong
numbers only; `stale lambda` is the lambda of the trial before, in a retrial):

* launch_damp with the stale lambda (the issue's first mutation): only the
  row kernel damps there (the tiled path damps where it consumes), so
  rows_plain alone fails: (a) g 1.0e12, (b) g, dx, q, t, X, edge chi2 differ.
* swap_state without the swap of obs_s / obs_s_nx (iteration 2 on the weights
  of the iteration-1 state): (d) cr_huber g 3.3e13; (d) and (e) of
  cr_huber_deep take 8 trials in iteration 2 where the oracle takes 5. The
  constant-weight cases have one s buffer and pass.
* launch_rcs_tiles with the stale lambda: (a) fails on the eight tiled cases,
  g 1.3e10 (lidar_plain) .. 6.6e13 (classes_plain) or another trial count;
  (b) differs in g, dx, q, t, X, edge chi2 on all eight; (d), (e) g 4.4e12 ..
  9.1e12 or another trial count; (c) fails on cr_huber.
* launch_rcs_reduce with the stale lambda (a stale S diagonal): (a) fails on
  the eight tiled cases, dx 2.2e5 (lidar_plain) .. 4.4e10 (classes_plain), g
  untouched; (b) differs in dx, q, t, X, edge chi2; (d), (e) dx 2.7e9 ..
  3.4e11 on the four cases that reject inside iteration 2.
* the landmark update with the stale lambda: (a), (b) fail on all nine cases
  (cr_huber dl 2.8e14; (b) differs in X and edge chi2), (d), (e) on six, (c)
  on classes_plain.

Every failing ratio is >= 2e3 x K.
"""
import functools

import numpy as np
import pytest

import lin_ref
from retrial_cases import CASES, LIDAR, TWO_ITER, lambda_at, state_problem
from test_gpu_first_trial import K, _same_bits, _setenv, ratios, run_problem

pytestmark = pytest.mark.gpu

# the path every case is there for: exec_info()["tile_kernel"], rcs_layout()["kind"]
# (None: not this case's subject)
EXPECT = {
    "classes_plain": ("tile_producer", None),
    "cr_huber": ("tile_producer", "band"),
    "cr_huber_deep": ("tile_producer", "band"),
    "cr_plain": ("tile_producer", "band"),
    "border_plain": ("tile_producer", "band+border"),
    "rows_plain": ("rows", "dense"),
    "stereo_plain": ("tile_stereo", None),
    "fixed_plain": ("tile_producer", None),
    "lidar_plain": ("tile_producer", None),
}
SCHEDULE_CASES = ("cr_huber", "classes_plain")      # one Huber (stored weights), one no-robust (constant weights)
SCHEDULES = ("SQLM_NO_SPEC", "SQLM_TRIAL_STORES", "SQLM_NO_POSE_FUSE", "SQLM_TILE_PROD")


@functools.lru_cache(maxsize=None)
def _problem(name):
    return CASES[name][0]()


def _lam_j(name):
    return lambda_at(CASES[name][1], CASES[name][3] - 1)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(spreads, longdouble trial, float64 trial) of the accepted trial: at lambda_j."""
    return lin_ref.spreads(_problem(name), _lam_j(name))


_state_refs = {}


def _state_reference(name, q, t, X, lam):
    """The same at another state (iteration 2), computed once per (case, state, lambda)."""
    key = (name, lam, q.tobytes(), t.tobytes(), X.tobytes())
    if key not in _state_refs:
        prob1 = state_problem(_problem(name), q, t, X)
        _state_refs[key] = (prob1, lin_ref.spreads(prob1, lam))
    return _state_refs[key]


def _run(ctx, name, monkeypatch, extra_env=None, lam=None, iterations=1, prob=None):
    make, lam0, env, trials = CASES[name]
    env = {**env, **(extra_env or {})}
    setenv = _setenv(monkeypatch)
    setenv("SQLM_TRIAL_STORES", env.pop("SQLM_TRIAL_STORES", None))
    prob = _problem(name) if prob is None else prob
    run = run_problem(ctx, prob, lam0 if lam is None else lam, setenv, env, iterations=iterations)
    run["edge_chi2"] = ctx.edge_chi2()
    run["lid_err"] = ctx.lidar_error() if prob.n_lid else np.zeros(0)
    return run


def _retrial(name, run):
    trials = CASES[name][3]
    assert run["n"] == 1 and run["st"]["iterations"] == 1
    assert run["st"]["trace_trials"] == [trials], run["st"]["trace_trials"]
    assert run["st"]["trials"] == trials


def _check_path(name, run):
    kern, kind = EXPECT[name]
    info, lay = run["info"], run["lay"]
    prob = _problem(name)
    assert info["tile_kernel"] == kern, info
    if kind is not None:
        assert lay["kind"] == kind, lay
    if name == "classes_plain":
        assert len(info["tile_classes"]) > 1, info                    # the three-stream fork / join
    if name.startswith("cr_"):
        assert lay["p"] >= 5, lay                                     # >= 3 cyclic-reduction levels
    if name == "border_plain":
        assert lay["border_cams"] > 0, lay
    if name == "rows_plain":
        assert not info["tile_classes"], info
    if name == "stereo_plain":
        assert prob.has_stereo
    if name == "fixed_plain":
        assert lay["n_free"] == prob.n_pose - 3
    if name == "lidar_plain":
        assert run["st"]["n_active_edges"] == prob.n_obs + sum(LIDAR.values())
    assert bool(np.any(prob.obs_delta > 0)) == ("huber" in name)


def _show(tag, rt, *more):
    print(f"{tag}: " + " ".join(f"{k} {v[0]:.2g} ({v[1]:.1e}/{v[2]:.1e})" for k, v in rt.items()), *more)


def _bits(a, b, keys=("g", "dx", "q", "t", "X", "edge_chi2", "lid_err")):
    """Names of the quantities of two runs that differ in any bit."""
    return [k for k in keys if not np.array_equal(a[k], b[k])]


@pytest.mark.parametrize("name", sorted(CASES))
def test_retrial_matches_reference(gpu_ctx, oracle, monkeypatch, name):
    run = _run(gpu_ctx, name, monkeypatch)
    _retrial(name, run)
    _check_path(name, run)
    rt = ratios(oracle, name, run, _reference(name), _problem(name))
    _show(name, rt, run["st"]["trace_trials"], run["info"], run["lay"])
    for k, v in rt.items():
        assert v[0] <= K, (name, k, v)


@pytest.mark.parametrize("name", sorted(CASES))
def test_retrial_same_bits_as_fresh_trial(gpu_ctx, monkeypatch, name):
    a = _run(gpu_ctx, name, monkeypatch)
    _retrial(name, a)
    b = _run(gpu_ctx, name, monkeypatch, lam=_lam_j(name))
    assert b["n"] == 1 and b["st"]["trace_trials"] == [1] and b["st"]["trials"] == 1, b["st"]
    assert not _bits(a, b), _bits(a, b)
    assert a["st"]["trace_chi2"][0] == b["st"]["trace_chi2"][0]
    assert a["st"]["trace_lambda"][0] == b["st"]["trace_lambda"][0]
    assert a["st"]["chi2_begin"] == b["st"]["chi2_begin"]


@pytest.mark.parametrize("switch", SCHEDULES)
@pytest.mark.parametrize("name", SCHEDULE_CASES)
def test_schedules_same_bits(gpu_ctx, monkeypatch, name, switch):
    a = _run(gpu_ctx, name, monkeypatch)
    b = _run(gpu_ctx, name, monkeypatch, {switch: "0" if switch == "SQLM_TILE_PROD" else "1"})
    _retrial(name, a)
    _retrial(name, b)
    if switch == "SQLM_TILE_PROD":
        assert a["info"]["tile_kernel_id"] == 4 and b["info"]["tile_kernel_id"] == 2, (a["info"], b["info"])
    _same_bits(a, b)
    assert not _bits(a, b, ("edge_chi2",))
    assert a["st"]["trace_lambda"] == b["st"]["trace_lambda"]


def _two_iterations(ctx, name, monkeypatch):
    """(run of optimize(0, 1), run of optimize(0, 2), lambda_2, lambda of iteration 2's last trial)."""
    t1, t2 = TWO_ITER[name]
    r1 = _run(ctx, name, monkeypatch)
    _retrial(name, r1)
    r2 = _run(ctx, name, monkeypatch, iterations=2)
    st = r2["st"]
    assert r2["n"] == 2 and st["trace_trials"] == [t1, t2] and st["trials"] == t1 + t2, st
    assert st["trace_chi2"][0] == r1["st"]["trace_chi2"][0] and st["trace_lambda"][0] == r1["st"]["trace_lambda"][0]
    lam2 = r1["st"]["trace_lambda"][0]
    return r1, r2, lam2, lambda_at(lam2, t2 - 1)


@pytest.mark.parametrize("name", sorted(TWO_ITER))
def test_second_iteration_matches_reference(gpu_ctx, oracle, monkeypatch, name):
    r1, r2, lam2, lam = _two_iterations(gpu_ctx, name, monkeypatch)
    og = oracle.OracleGraph(_problem(name))
    og.lid_level[:] = lin_ref.lidar_level(_problem(name))
    n, st = og.optimize(0, 2, user_lambda=CASES[name][1])
    assert st["trace_trials"] == r2["st"]["trace_trials"]
    assert abs(lam2 - st["trace_lambda"][0]) <= 1e-6 * st["trace_lambda"][0], (lam2, st["trace_lambda"])
    prob1, reference = _state_reference(name, r1["q"], r1["t"], r1["X"], lam)
    # iteration 2's last trial: its chi2 is the run's second trace entry
    run = dict(r2, st=dict(trace_chi2=[r2["st"]["trace_chi2"][1]]))
    rt = ratios(oracle, name, run, reference, prob1)
    _show(f"{name} iteration 2", rt, r2["st"]["trace_trials"], f"lambda_2 {lam2:.6g} trial lambda {lam:.6g}")
    for k, v in rt.items():
        assert v[0] <= K, (name, k, v)


@pytest.mark.parametrize("name", sorted(TWO_ITER))
def test_fresh_linearization_matches_reference(gpu_ctx, oracle, monkeypatch, name):
    t1, t2 = TWO_ITER[name]
    r1, r2, lam2, lam = _two_iterations(gpu_ctx, name, monkeypatch)
    prob1, reference = _state_reference(name, r1["q"], r1["t"], r1["X"], lam)
    run = _run(gpu_ctx, name, monkeypatch, lam=lam2, prob=prob1)
    assert run["n"] == 1 and run["st"]["trace_trials"] == [t2] and run["st"]["trials"] == t2, run["st"]
    rt = ratios(oracle, name, run, reference, prob1)
    differ = _bits(r2, run)
    same_chi2 = run["st"]["trace_chi2"][0] == r2["st"]["trace_chi2"][1]
    _show(f"{name} fresh linearization", rt,
          f"against iteration 2 of the two-iteration run: differing {differ or 'nothing'}, chi2 equal {same_chi2}")
    for k, v in rt.items():
        assert v[0] <= K, (name, k, v)
