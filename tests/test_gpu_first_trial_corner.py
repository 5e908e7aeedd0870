"""The first LM trial of BA with EdgeLidarCornerPoint edges (local BA pass 3 with
using_sharp_point) against the extended-precision reference with kinds,
tests/lin_ref_corner.py. The oracle has no corner edge, so the run is pinned
trial by trial, not by end state.

Harness and rule are those of tests/test_gpu_first_trial_lidar.py: one trial --
optimize(level, 1, user_lambda) -- and g, dx (sqlm_get_last_step), the landmark
step, the updated poses and the trial chi2 at the returned state, each within
K = 100 x the reference's own float64-vs-longdouble spread (floor 4 eps). The
kind of an edge selects lidar_error / lidar_jacobian or lidar_corner_error /
lidar_corner_jacobian in k_camera_pass<ST, true> and the error in k_lidar_chi2.
tests/test_lin_ref_corner.py shows on the CPU that a reference which ignores
the kinds is more than 1e6 x K spreads away on every case.

Beyond the ratios: sqlm_get_lidar_error on the active edges is bit-equal to the
float64 error of either kind at the returned poses, in caller order, also
under SQLM_NO_SPEC=1; inactive edges read 0; no active error is 0.

Ratios (GPU error / spread) measured on an MI355X when the test was written:

    case               g      dx     dl     pose   chi2
    cor_level          0.73   0.69   0.46   0.45   0.28
    cor_level_l1       0.51   0.97   -      0.97   0.49
    cor_mixed          0.73   0.65   0.58   0.39   0.074
    cor_mixed_lam1e-3  0.067  0.051  0.054  0.021  0.49
    cor_mixed_lam1e3   1.4    2.3    1.0    0.14   0.39
    cor_one            0.58   0.27   0.37   0.19   0.29
    cor_only_cam       0.58   0.36   0.27   0.39   0.33
    cor_stereo         1.1    0.32   0.70   0.38   0.17

The largest is 2.3 (dx of cor_mixed_lam1e3, 6.8e-15 against a spread of
3.0e-15). cor_level_l1 has LiDAR-only cameras and no landmark: dl has no ratio
and no point may move. Every per-edge error of either kind was bit-equal.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import corner_first_trial_cases as corc
import lidar_first_trial_cases as lidc
import lin_ref
import lin_ref_corner as LRC
from test_gpu_first_trial import FLOOR, K, _maxrel, _one_accepted_trial, _same_bits, _setenv, run_problem

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _problem(name):
    return corc.CASES[name][0]()


def _level(name):
    return corc.LEVEL.get(name, 0)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(spreads, longdouble trial, float64 trial) of the case: computed once."""
    return LRC.spreads(_problem(name), corc.CASES[name][1], level=_level(name))


def _run(ctx, name, monkeypatch, extra_env=None, prob=None):
    prob = _problem(name) if prob is None else prob
    run = run_problem(ctx, prob, corc.CASES[name][1], _setenv(monkeypatch), {**corc.CASES[name][2], **(extra_env or {})},
                      _level(name))
    run["lid_err"] = ctx.lidar_error()
    return run


def ratios(oracle, prob, level, run, reference):
    """tests/test_gpu_first_trial.py::ratios with the kind-aware chi2."""
    sp, ref, f64 = reference
    out = {}

    def put(key, err, spread):
        out[key] = (err / max(spread, FLOOR), err, spread)

    put("g", _maxrel(run["g"].reshape(-1), ref.g), sp["g"])
    put("dx", _maxrel(run["dx"].reshape(-1), ref.dx), sp["dx"])
    if ref.lms.size:
        dmax = np.abs(ref.dl).max()
        X_hi = prob.pt.astype(lin_ref.LD) + ref.dl
        X_lo = prob.pt + f64.dl
        put("dl", float(np.abs(run["X"] - X_hi).max() / dmax), float(np.abs(X_lo - X_hi).max() / dmax))
    else:  # no active landmark (a level with LiDAR edges only): no point may move
        put("dl", float(np.abs(run["X"] - prob.pt).max()), 0.0)
    q_hi, t_hi = lin_ref.oplus_poses(oracle, prob, ref.free, ref.dx.astype(np.float64))
    q_lo, t_lo = lin_ref.oplus_poses(oracle, prob, f64.free, f64.dx)
    ts = max(1.0, np.abs(t_hi).max())
    put("pose", max(np.abs(run["q"] - q_hi).max(), np.abs(run["t"] - t_hi).max() / ts),
        max(np.abs(q_lo - q_hi).max(), np.abs(t_lo - t_hi).max() / ts))
    chi_hi, chi_sp = LRC.chi2_spread(prob, run["q"], run["t"], run["X"], level)
    put("chi2", float(abs(lin_ref.LD(run["st"]["trace_chi2"][0]) - chi_hi) / chi_hi), chi_sp)
    return out


def _active(prob, level):
    return (lin_ref.lidar_level(prob) == level) & (prob.pose_fixed[prob.lid_pose] == 0)


def _check_lidar_error(prob, run, level):
    """ctx.lidar_error() against the float64 error of either kind at the returned poses, bit for bit."""
    act = _active(prob, level)
    ref = LRC.lidar_edges(prob, np.float64, run["q"], run["t"], level, jac=False)
    assert np.array_equal(ref.eid, np.nonzero(act)[0]) and ref.eid.size > 0
    got = run["lid_err"]
    assert got.shape == (prob.n_lid,)
    bad = np.nonzero(got[ref.eid] != ref.e)[0]
    assert bad.size == 0, (bad[:8], prob.lid_kind[ref.eid][bad[:8]], got[ref.eid][bad[:8]], ref.e[bad[:8]])
    assert np.all(ref.e != 0.0)                 # so a slot left at its initial 0 cannot pass
    assert not np.any(got[~act])                # never computed: 0
    assert prob.lid_kind[ref.eid].any()         # corner edges among the active ones


def _check_path(name, prob, run):
    level = _level(name)
    act = _active(prob, level)
    cnt = np.bincount(prob.lid_pose[act], minlength=prob.n_pose)
    vis = np.zeros(prob.n_pose, bool)
    vis[prob.obs_pose[prob.obs_level == level]] = True
    free = np.nonzero((vis | (cnt > 0)) & (prob.pose_fixed == 0))[0]
    assert run["lay"]["n_free"] == free.size, (run["lay"], free.size)
    if name == "cor_one":
        assert cnt[29] == 150 and cnt.sum() == 150 and prob.lid_kind.all()
    if name.startswith("cor_mixed"):
        assert {p: int(cnt[p]) for p in lidc.MULTI} == {**lidc.MULTI, 0: 0}
        assert np.any(np.diff(prob.lid_pose) < 0)
    if name.startswith("cor_level"):
        assert 0 < act.sum() < (prob.pose_fixed[prob.lid_pose] == 0).sum()
    if name == "cor_level_l1":
        assert not vis.any() and not run["info"]["tile_classes"] and np.array_equal(run["X"], prob.pt)
        only = [p for p in free if prob.lid_kind[act & (prob.lid_pose == p)].all()]
        assert only, "a camera with corner edges only"
    if name == "cor_stereo":
        assert prob.has_stereo and run["info"]["tile_kernel"] == "tile_stereo" and cnt[29] == 100
    if name == "cor_only_cam":
        c = corc.ONLY_CAM
        assert not vis[c] and cnt[c] >= 100 and c in free
        ref = _reference(name)[1]
        h = int(np.nonzero(ref.free == c)[0][0])
        row = ref.S[6 * h:6 * h + 6].copy()
        row[:, 6 * h:6 * h + 6] = 0
        assert not row.any()                     # isolated S block, zero coupling


@pytest.mark.parametrize("name", sorted(corc.CASES))
def test_first_trial_matches_reference(gpu_ctx, oracle, monkeypatch, name):
    prob = _problem(name)
    run = _run(gpu_ctx, name, monkeypatch)
    _one_accepted_trial(run)
    _check_path(name, prob, run)
    rt = ratios(oracle, prob, _level(name), run, _reference(name))
    print(f"{name}: " + " ".join(f"{k} {v[0]:.2g} ({v[1]:.1e}/{v[2]:.1e})" for k, v in rt.items()),
          run["info"], run["lay"])
    _check_lidar_error(prob, run, _level(name))
    for k, v in rt.items():
        assert v[0] <= K, (name, k, v)


@pytest.mark.parametrize("name", ["cor_one", "cor_mixed", "cor_level", "cor_only_cam"])
def test_lidar_error_without_speculation(gpu_ctx, monkeypatch, name):
    """SQLM_NO_SPEC=1: no speculative camera pass writes lid_err, k_lidar_chi2 alone does."""
    run = _run(gpu_ctx, name, monkeypatch, {"SQLM_NO_SPEC": "1"})
    _one_accepted_trial(run)
    _check_lidar_error(_problem(name), run, _level(name))


@pytest.mark.parametrize("switch", ["SQLM_NO_SPEC", "SQLM_NO_POSE_FUSE"])
def test_schedules_same_bits(gpu_ctx, monkeypatch, switch):
    a = _run(gpu_ctx, "cor_mixed", monkeypatch)
    b = _run(gpu_ctx, "cor_mixed", monkeypatch, {switch: "1"})
    _one_accepted_trial(b)
    _same_bits(a, b)
    assert np.array_equal(a["lid_err"], b["lid_err"])


def test_edges_on_a_fixed_pose_change_no_bit(gpu_ctx, monkeypatch):
    """cor_mixed without the 40 corner edges of the fixed pose 0: the same result."""
    a = _run(gpu_ctx, "cor_mixed", monkeypatch)
    p = corc.mixed_without_fixed()
    full = _problem("cor_mixed")
    assert p.n_lid == full.n_lid - 40
    b = _run(gpu_ctx, "cor_mixed", monkeypatch, prob=p)
    _one_accepted_trial(b)
    _same_bits(a, b)
    assert a["st"]["n_active_edges"] == b["st"]["n_active_edges"]
    assert np.array_equal(a["lid_err"][full.lid_pose != 0], b["lid_err"])


def test_explicit_zero_kinds_change_no_bit(gpu_ctx, monkeypatch):
    """lid_multi with sqlm_set_lidar_kind(all 0), and with NULL, against lid_multi without the call."""
    prob = lidc.CASES["lid_multi"][0]()
    a = run_problem(gpu_ctx, prob, 1.0, _setenv(monkeypatch), {})
    a_err = gpu_ctx.lidar_error()
    for kind in (np.zeros(prob.n_lid, np.uint8), None):
        b = run_problem(gpu_ctx, prob, 1.0, _setenv(monkeypatch), {}, set_lidar=lambda ctx: ctx.set_lidar_kind(kind))
        _same_bits(a, b)
        assert np.array_equal(a_err, gpu_ctx.lidar_error())
        assert a["st"]["n_active_edges"] == b["st"]["n_active_edges"]


def test_kinds_are_not_ignored(gpu_ctx, monkeypatch):
    """cor_mixed against the same edges all flat: another system, another step."""
    a = _run(gpu_ctx, "cor_mixed", monkeypatch)
    b = _run(gpu_ctx, "cor_mixed", monkeypatch, prob=corc.zero_kinds(_problem("cor_mixed")))
    assert _maxrel(a["g"], b["g"]) > 1e-3 and _maxrel(a["dx"], b["dx"]) > 1e-3


def test_lidar_kind_arguments(gpu_ctx, monkeypatch):
    from sqrtlm import _lib
    from sqrtlm.optimizer import Context
    L = _lib.lib()
    prob = _problem("cor_mixed")
    kind = prob.lid_kind.copy()
    with Context(0) as fresh:
        assert L.sqlm_set_lidar_kind(fresh._h, _lib.ptr(kind)) == -7         # no problem
    assert L.sqlm_set_lidar_kind(None, _lib.ptr(kind)) == -1
    gpu_ctx.set_problem(prob)
    bad = kind.copy()
    bad[-1] = 2
    assert L.sqlm_set_lidar_kind(gpu_ctx._h, _lib.ptr(bad)) == -1            # a value above 1
    # the rejected call left the kinds of set_problem in place
    a = _run(gpu_ctx, "cor_mixed", monkeypatch)

    def rejected(ctx):
        assert L.sqlm_set_lidar_kind(ctx._h, _lib.ptr(bad)) == -1
    b = run_problem(gpu_ctx, prob, 1.0, _setenv(monkeypatch), {}, set_lidar=rejected)
    _same_bits(a, b)

    # sqlm_set_lidar after the kinds resets every edge to flat
    def reset(ctx):
        _lib.check(L.sqlm_set_lidar(ctx._h, C.c_int64(prob.n_lid), _lib.ptr(prob.lid_pose), _lib.ptr(prob.lid_pc),
                                    _lib.ptr(prob.lid_pw), _lib.ptr(prob.lid_n), _lib.ptr(prob.lid_info)),
                   "sqlm_set_lidar")
    c = run_problem(gpu_ctx, prob, 1.0, _setenv(monkeypatch), {}, set_lidar=reset)
    d = run_problem(gpu_ctx, corc.zero_kinds(prob), 1.0, _setenv(monkeypatch), {})
    _same_bits(c, d)
    assert _maxrel(a["dx"], c["dx"]) > 1e-3
