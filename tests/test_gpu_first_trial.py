"""The first LM trial's linear algebra against an extended-precision reference.

Every other GPU parity test compares the end state of several LM iterations at
1e-6, which a slightly wrong reduced camera system survives (LM corrects
itself). Here one trial runs -- optimize(0, 1, user_lambda) -- and the step
itself is compared with tests/lin_ref.py (numpy longdouble): the reduced
right-hand side g and the camera step dx (sqlm_get_last_step), the landmark
back-substitution (points() - initial points), the updated poses, and the
trial chi2 against the longdouble chi2 of the state the GPU returned.

Tolerance: K x the reference's own float64-vs-longdouble rounding spread of
that quantity on that problem (floored at 4 eps), measured on the reference
alone. K = 100 (chosen once; a kernel that sums in another order than numpy
passes, a wrong block shows at >= 1e-6 relative, i.e. ratios >= 1e6).

Ratios (GPU error / spread) measured on an MI355X when the test was written:

    case          g     dx     dl     pose   chi2
    border        1.9   0.31   0.32   0.30   0.40
    cls3          0.27  0.20   0.12   0.27   0.018
    cls4          1.4   1.4    1.9    0.87   0.31
    cls6          0.85  2.2    4.6    1.8    0.096
    cls8          0.83  0.16   0.54   0.20   0.0047
    cls9          0.95  0.52   0.63   0.50   0.017
    cr_levels     0.43  0.033  0.085  0.030  0.035
    dups          1.9   0.95   1.2    0.76   0.49
    fixed_plain   0.26  0.47   0.33   0.46   0.66
    fixed_robust  0.90  0.30   0.45   0.30   0.54
    long_red      0.50  2.3    0.64   0.46   0.16
    long_track    0.80  6.7    2.2    0.93   0.32
    mid_lam1      0.97  0.35   0.82   0.37   0.0046
    mid_lam1e-3   0.22  0.49   0.50   0.49   2.1
    mid_lam1e3    0.82  1.2    1.0    0.21   0.30
    rows          1.5   0.92   1.1    1.0    0.11
    stereo_all    1.1   0.56   0.85   0.61   0.053
    stereo_half   1.2   0.29   0.27   0.17   0.053

The largest is 6.7 (dx of long_track, 8.5e-14 against a spread of 1.3e-14).
With one lambda left off a diagonal entry of S (rcs_put_s) the dx ratios were
7.6e4 .. 5.5e9, with one tile partial left out of a g row (k_rcs_reduce) the
g ratios 1.9e11 .. 3.2e12: both far beyond K, both tried on scratch builds.

Each case also asserts the device path it is there for (sqlm_get_exec_info,
sqlm_get_rcs_layout), so that a planner change cannot silently empty it.
"""
import functools

import numpy as np
import pytest

import lidar_first_trial_cases as lidc
import lin_ref
from first_trial_cases import CASES

pytestmark = pytest.mark.gpu

K = 100.0
EPS = float(np.finfo(np.float64).eps)
FLOOR = 4 * EPS
SWITCHES = ("SQLM_TILE_PROD", "SQLM_NO_SPEC", "SQLM_NO_POSE_FUSE", "SQLM_CR_B_MIN")

# the path every case is there for: exec_info()["tile_kernel"], tile classes
# that must be present, rcs_layout()["kind"] (None: not this case's subject)
EXPECT = {
    "mid_lam1e-3": ("tile_producer", None, None),
    "mid_lam1": ("tile_producer", None, None),
    "mid_lam1e3": ("tile_producer", None, None),
    "cls3": ("tile_producer", {3}, None),
    "cls4": ("tile_producer", {4}, None),
    "cls6": ("tile_producer", {6}, None),
    "cls8": ("tile_producer", {8}, "dense"),
    "cls9": ("tile_producer", {9}, "dense"),
    "long_track": ("tile_mono", None, None),
    "rows": ("rows", set(), "dense"),
    "stereo_half": ("tile_stereo", None, None),
    "stereo_all": ("tile_stereo", None, None),
    "stereo_cls8": ("tile_stereo", {8}, None),
    "stereo_cls9": ("tile_stereo", {9}, None),
    "dups": ("tile_mono", None, None),
    "long_red": ("tile_producer", {3}, None),
    "cr_levels": ("tile_producer", None, "band"),
    "border": ("tile_producer", None, "band+border"),
    "fixed_robust": ("tile_producer", None, None),
    "fixed_plain": ("tile_producer", None, None),
}
CLASS_CASES = ("cls3", "cls4", "cls6", "cls8", "cls9")


# the harness also runs the LiDAR cases of tests/test_gpu_first_trial_lidar.py
ALL_CASES = {**CASES, **lidc.CASES}


def _level(name):
    return lidc.LEVEL.get(name, 0)


@functools.lru_cache(maxsize=None)
def _problem(name):
    return ALL_CASES[name][0]()


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(spreads, longdouble trial, float64 trial) of the case: computed once."""
    return lin_ref.spreads(_problem(name), ALL_CASES[name][1], level=_level(name))


def run_problem(ctx, prob, lam, setenv, env, level=0, set_lidar=None, iterations=1):
    """One iteration of `prob` on the GPU (tests/test_gpu_retrial.py: two);
    setenv(key, value or None). set_lidar(ctx) replaces the problem's own LiDAR
    edges after set_problem."""
    for k in SWITCHES:
        setenv(k, env.get(k))
    ctx.set_problem(prob)
    if set_lidar is not None:
        set_lidar(ctx)
    elif prob.meta.get("lid_level") is not None:
        ctx.set_lidar_level(prob.meta["lid_level"])
    n, st = ctx.optimize(level, iterations, user_lambda=lam)
    g, dx = ctx.last_step()
    q, t = ctx.poses()
    return dict(n=n, st=st, g=g, dx=dx, q=q, t=t, X=ctx.points(), info=ctx.exec_info(), lay=ctx.rcs_layout())


def run_gpu(ctx, name, setenv, extra_env=None):
    """One trial of case `name` on the GPU; setenv(key, value or None)."""
    return run_problem(ctx, _problem(name), ALL_CASES[name][1], setenv, {**ALL_CASES[name][2], **(extra_env or {})},
                       _level(name))


def _maxrel(a, b):
    a, b = np.asarray(a, lin_ref.LD), np.asarray(b, lin_ref.LD)
    return float(np.abs(a - b).max() / np.abs(b).max())


def ratios(oracle, name, run, reference=None, prob=None):
    """GPU error / reference spread per quantity (and both, for the table).
    reference: (spreads, longdouble trial, float64 trial) in place of the
    case's own (the same problem at another lambda). prob: the problem the
    reference was made from, in place of the case's own (with reference;
    tests/test_gpu_retrial.py)."""
    prob = _problem(name) if prob is None else prob
    level = _level(name)
    sp, ref, f64 = reference or _reference(name)
    out = {}

    def put(key, err, spread):
        out[key] = (err / max(spread, FLOOR), err, spread)

    put("g", _maxrel(run["g"].reshape(-1), ref.g), sp["g"])
    put("dx", _maxrel(run["dx"].reshape(-1), ref.dx), sp["dx"])
    # points: X0 + dl, the float64 sum's rounding is part of the spread
    if ref.lms.size:
        dmax = np.abs(ref.dl).max()
        X_hi = prob.pt.astype(lin_ref.LD) + ref.dl
        X_lo = prob.pt + f64.dl
        put("dl", float(np.abs(run["X"] - X_hi).max() / dmax), float(np.abs(X_lo - X_hi).max() / dmax))
    else:  # no active landmark (a level with LiDAR edges only): no point may move
        put("dl", float(np.abs(run["X"] - prob.pt).max()), 0.0)
    # poses: oplus(initial, dx) in the oracle's float64 SE3Quat arithmetic
    q_hi, t_hi = lin_ref.oplus_poses(oracle, prob, ref.free, ref.dx.astype(np.float64))
    q_lo, t_lo = lin_ref.oplus_poses(oracle, prob, f64.free, f64.dx)
    ts = max(1.0, np.abs(t_hi).max())
    put("pose", max(np.abs(run["q"] - q_hi).max(), np.abs(run["t"] - t_hi).max() / ts),
        max(np.abs(q_lo - q_hi).max(), np.abs(t_lo - t_hi).max() / ts))
    # trial chi2 at the state the GPU returned
    chi_hi, chi_sp = lin_ref.chi2_spread(prob, run["q"], run["t"], run["X"], level)
    put("chi2", float(abs(lin_ref.LD(run["st"]["trace_chi2"][0]) - chi_hi) / chi_hi), chi_sp)
    return out


def _one_accepted_trial(run):
    assert run["n"] == 1 and run["st"]["iterations"] == 1
    assert run["st"]["trace_trials"] == [1], run["st"]["trace_trials"]
    assert run["st"]["trials"] == 1


def _check_path(name, run):
    kern, classes, kind = EXPECT[name]
    info, lay = run["info"], run["lay"]
    assert info["tile_kernel"] == kern, info
    if classes is not None:
        assert classes <= info["tile_classes"] if classes else not info["tile_classes"], info
    if kind is not None:
        assert lay["kind"] == kind, lay


def _setenv(monkeypatch):
    def f(k, v):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    return f


def _same_bits(a, b):
    for k in ("g", "dx", "q", "t", "X"):
        assert np.array_equal(a[k], b[k]), k
    assert a["st"]["trace_chi2"] == b["st"]["trace_chi2"]
    assert a["st"]["trace_trials"] == b["st"]["trace_trials"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_first_trial_matches_reference(gpu_ctx, oracle, monkeypatch, name):
    run = run_gpu(gpu_ctx, name, _setenv(monkeypatch))
    _one_accepted_trial(run)
    _check_path(name, run)
    rt = ratios(oracle, name, run)
    print(f"{name}: " + " ".join(f"{k} {v[0]:.2g} ({v[1]:.1e}/{v[2]:.1e})" for k, v in rt.items()),
          run["info"], run["lay"])
    for k, v in rt.items():
        assert v[0] <= K, (name, k, v)


def test_case_paths(gpu_ctx, monkeypatch):
    """What the cases are there for, beyond the kernel / layout of EXPECT."""
    runs = {n: run_gpu(gpu_ctx, n, _setenv(monkeypatch))
            for n in CLASS_CASES + ("mid_lam1", "long_track", "dups", "long_red", "cr_levels", "border")}
    union = set()
    for n in CLASS_CASES:
        union |= runs[n]["info"]["tile_classes"]
    assert union == {3, 4, 6, 8, 9}, union
    assert len(runs["mid_lam1"]["info"]["tile_classes"]) > 1           # the three-stream fork / join
    lt = runs["long_track"]["info"]
    assert lt["tile_maxk"] > 32 and lt["tile_dups"] == 0, lt            # too long for the producer wave
    assert runs["dups"]["info"]["tile_dups"] == 1
    lr = runs["long_red"]["info"]
    assert lr["n_long_s"] > 0 and lr["n_long_g"] > 0, lr                # workgroup sums in k_rcs_reduce
    assert runs["cr_levels"]["lay"]["p"] >= 5, runs["cr_levels"]["lay"]  # >= 3 cyclic-reduction levels
    assert runs["border"]["lay"]["border_cams"] > 0
    for n in ("fixed_robust", "fixed_plain"):
        p = _problem(n)
        fixed = p.pose_fixed[p.obs_pose] != 0
        n_free = np.bincount(p.obs_pt[~fixed], minlength=p.n_pt)
        n_fix = np.bincount(p.obs_pt[fixed], minlength=p.n_pt)
        assert np.any((n_free == 1) & (n_fix > 0)) and np.any((n_free == 0) & (n_fix > 0))  # the h < 0 skips
    assert np.any(_problem("fixed_robust").obs_delta > 0) and not np.any(_problem("fixed_plain").obs_delta > 0)


@pytest.mark.parametrize("name", CLASS_CASES + ("mid_lam1",))
def test_plain_tile_kernel_same_bits(gpu_ctx, monkeypatch, name):
    """k_rcs_tile (SQLM_TILE_PROD=0) against the producer / consumer kernel."""
    a = run_gpu(gpu_ctx, name, _setenv(monkeypatch))
    b = run_gpu(gpu_ctx, name, _setenv(monkeypatch), {"SQLM_TILE_PROD": "0"})
    assert a["info"]["tile_kernel_id"] == 4 and b["info"]["tile_kernel_id"] == 2, (a["info"], b["info"])
    assert a["info"]["tile_classes"] == b["info"]["tile_classes"]
    _same_bits(a, b)


@pytest.mark.parametrize("switch", ["SQLM_NO_SPEC", "SQLM_NO_POSE_FUSE"])
def test_schedules_same_bits(gpu_ctx, monkeypatch, switch):
    a = run_gpu(gpu_ctx, "mid_lam1", _setenv(monkeypatch))
    b = run_gpu(gpu_ctx, "mid_lam1", _setenv(monkeypatch), {switch: "1"})
    _one_accepted_trial(b)
    _same_bits(a, b)


def test_last_step_arguments(gpu_ctx, monkeypatch):
    import ctypes as C
    from sqrtlm import _lib
    from sqrtlm.optimizer import Context
    L = _lib.lib()
    buf = (C.c_double * 6)()
    with Context(0) as fresh:
        assert L.sqlm_get_last_step(fresh._h, buf, buf) == -7         # no problem
        fresh.set_problem(_problem("cls3"))
        assert L.sqlm_get_last_step(fresh._h, buf, buf) == -7         # set, never optimized
    run_gpu(gpu_ctx, "cls3", _setenv(monkeypatch))
    assert L.sqlm_get_last_step(gpu_ctx._h, None, buf) == -1
    assert L.sqlm_get_last_step(gpu_ctx._h, buf, None) == -1
