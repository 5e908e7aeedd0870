"""The first LM trial of LiDAR-augmented BA (local BA pass 3: vision edges plus
EdgeLidarFlatPoint unary pose edges) against the extended-precision reference.

The harness is that of tests/test_gpu_first_trial.py: one trial --
optimize(level, 1, user_lambda) -- and g, dx (sqlm_get_last_step), the landmark
step, the updated poses and the trial chi2 at the returned state are compared
with tests/lin_ref.py, each within K = 100 x the reference's own
float64-vs-longdouble spread of that quantity (floor 4 eps). The LiDAR terms
enter H_pp / b_p in k_camera_pass<ST, true> and the trial chi2 in
k_lidar_chi2; the reference takes the float64 central-difference Jacobian row
as data (lin_ref's docstring says why), which holds because the device
evaluates lidar_error / lidar_jacobian without contraction, bit-equal to the
oracle's.

Beyond the ratios, per case: sqlm_get_lidar_error on the active edges is
bit-equal to the reference's float64 error at the poses the GPU returned, in
the caller's edge order (k_lidar_chi2 and the dev_lid_edge permutation, edge by
edge), also under SQLM_NO_SPEC=1 where k_lidar_chi2 is its only producer;
inactive edges (fixed pose, other level) read 0 as in the oracle's lid_err.

Ratios (GPU error / spread) measured on an MI355X when the test was written:

    case               g      dx     dl     pose   chi2
    lid_border         1.9    0.32   0.26   0.31   0.14
    lid_level          0.73   0.42   0.31   0.35   0.53
    lid_level_l1       0.96   19     -      13     1.0
    lid_multi          0.73   0.42   0.40   0.28   0.14
    lid_multi_lam1e-3  0.067  0.019  0.052  0.011  0.44
    lid_multi_lam1e3   1.4    2.2    1.1    0.14   0.25
    lid_one            0.58   0.42   0.32   0.27   0.60
    lid_only_cam       0.58   0.36   0.27   0.39   0.29
    lid_rows           1.5    2.4    6.3    2.4    0.013
    lid_stereo         1.1    0.22   0.28   0.24   0.12

The largest is 19 (dx of lid_level_l1, 1.1e-13 against a spread of 6.0e-15:
five LiDAR-only cameras, no landmark, so dl has no ratio and no point may
move). Every per-edge error was bit-equal, every schedule and the association
route bit-identical: the device Jacobian is the oracle's, the case of ratios
around 1e6 on every problem did not arise, and no kernel or grouping bug
showed.

Two mutations of k_camera_pass<ST, true>, tried on scratch builds (ratios of
lid_one / lid_multi / lid_stereo):

* H accumulated as J[r] * J[c], without info: dx 1.0e13 / 9.4e13 / 1.8e12,
  dl 1.0e13 / 2.7e13 / 3.3e12, pose 6.1e12 / 5.1e13 / 5.3e12 (g, which holds
  no H, stays at 0.58 / 0.73 / 1.1);
* the lane loop taking one trip only (every edge beyond a camera's first 64
  dropped): g 1.1e13 / 2.0e13 / 8.1e12, dx 6.3e10 / 4.6e11 / 3.1e10,
  dl 5.4e10 / 1.6e11 / 1.5e10, pose 1.0e11 / 6.0e11 / 3.0e10.

Both are >= 1e8 x K. The trial chi2 stays inside K under both (it is compared
at the state the GPU returned, and k_lidar_chi2 is not the mutated kernel), as
do the per-edge errors.

lid_level also runs at level 1 (lid_level_l1): the oracle accepts that trial.
Each case asserts the path it is there for (_check_path).
"""
import functools

import numpy as np
import pytest

import lidar_cases as LC
import lidar_first_trial_cases as lidc
import lin_ref
from test_gpu_first_trial import (K, _one_accepted_trial, _problem, _reference, _same_bits, _setenv, ratios, run_gpu,
                                  run_problem)

pytestmark = pytest.mark.gpu

# the path every case is there for: exec_info()["tile_kernel"] and
# rcs_layout()["kind"] (None: not this case's subject)
EXPECT = {
    "lid_one": (None, None),
    "lid_multi_lam1e-3": (None, None),
    "lid_multi": (None, None),
    "lid_multi_lam1e3": (None, None),
    "lid_level": (None, None),
    "lid_level_l1": ("no_tiles", None),
    "lid_stereo": ("tile_stereo", None),
    "lid_border": (None, "band+border"),
    "lid_rows": ("rows", "dense"),
    "lid_only_cam": (None, None),
}


def _active(prob, level):
    return (lin_ref.lidar_level(prob) == level) & (prob.pose_fixed[prob.lid_pose] == 0)


def _check_lidar_error(prob, run, level):
    """ctx.lidar_error() against the float64 error at the returned poses, bit for bit."""
    act = _active(prob, level)
    ref = lin_ref.lidar_edges(prob, np.float64, run["q"], run["t"], level, jac=False)
    assert np.array_equal(ref.eid, np.nonzero(act)[0]) and ref.eid.size > 0
    got = run["lid_err"]
    assert got.shape == (prob.n_lid,)
    bad = np.nonzero(got[ref.eid] != ref.e)[0]
    assert bad.size == 0, (bad[:8], got[ref.eid][bad[:8]], ref.e[bad[:8]])
    assert np.all(ref.e != 0.0)                 # so a slot left at its initial 0 cannot pass
    assert not np.any(got[~act])                # never computed: 0, as the oracle's lid_err


def _run(ctx, name, monkeypatch, extra_env=None):
    run = run_gpu(ctx, name, _setenv(monkeypatch), extra_env)
    run["lid_err"] = ctx.lidar_error()
    return run


def _check_path(name, run):
    prob, level = _problem(name), lidc.LEVEL.get(name, 0)
    info, lay = run["info"], run["lay"]
    kern, kind = EXPECT[name]
    if kern == "no_tiles":
        assert not info["tile_classes"], info
    elif kern is not None:
        assert info["tile_kernel"] == kern, info
    if kind is not None:
        assert lay["kind"] == kind, lay
    act = _active(prob, level)
    cnt = np.bincount(prob.lid_pose[act], minlength=prob.n_pose)
    vis = np.zeros(prob.n_pose, bool)
    vis[prob.obs_pose[prob.obs_level == level]] = True
    free = np.nonzero((vis | (cnt > 0)) & (prob.pose_fixed == 0))[0]
    assert lay["n_free"] == free.size, (lay, free.size)
    if name == "lid_one":
        assert cnt[29] == 150 and cnt.sum() == 150                       # 64 + 64 + 22
    if name.startswith("lid_multi"):
        assert {p: int(cnt[p]) for p in lidc.MULTI} == {**lidc.MULTI, 0: 0}  # the fixed pose's 40 are skipped
        assert int((prob.lid_pose == 0).sum()) == 40 and prob.pose_fixed[0] and 0 not in free
        assert lay["n_free"] == prob.n_pose - 2
        assert np.any(np.diff(prob.lid_pose) < 0)                          # not grouped by pose: a real permutation
        assert np.all(cnt[[6, 7, 8, 10, 15, 21]] == 0)                     # free cameras with none in between
    if name.startswith("lid_level"):
        assert 0 < act.sum() < (prob.pose_fixed[prob.lid_pose] == 0).sum()   # the level filter drops some
    if name == "lid_level_l1":
        assert not vis.any() and np.array_equal(run["X"], prob.pt)         # LiDAR-only cameras, no landmark moves
    if name == "lid_stereo":
        assert prob.has_stereo and cnt[29] == 100
    if name == "lid_border":
        assert lay["border_cams"] > 0 and {p: int(cnt[p]) for p in lidc.BORDER} == lidc.BORDER
        h = {p: int(np.nonzero(free == p)[0][0]) for p in lidc.BORDER}
        print(f"lid_border: B {lay['B']} border_cams {lay['border_cams']} n_free {lay['n_free']}, LiDAR on "
              + ", ".join(f"pose {p} = free camera {h[p]}" for p in h))
    if name == "lid_only_cam":
        c = lidc.ONLY_CAM
        assert not vis[c] and cnt[c] >= 100 and c in free and not prob.pose_fixed[c]
        ref = _reference(name)[1]
        h = int(np.nonzero(ref.free == c)[0][0])
        row = ref.S[6 * h:6 * h + 6].copy()
        row[:, 6 * h:6 * h + 6] = 0
        assert not row.any()                                               # isolated S block, zero coupling


@pytest.mark.parametrize("name", sorted(lidc.CASES))
def test_first_trial_matches_reference(gpu_ctx, oracle, monkeypatch, name):
    run = _run(gpu_ctx, name, monkeypatch)
    _one_accepted_trial(run)
    _check_path(name, run)
    rt = ratios(oracle, name, run)
    print(f"{name}: " + " ".join(f"{k} {v[0]:.2g} ({v[1]:.1e}/{v[2]:.1e})" for k, v in rt.items()),
          run["info"], run["lay"])
    _check_lidar_error(_problem(name), run, lidc.LEVEL.get(name, 0))
    for k, v in rt.items():
        assert v[0] <= K, (name, k, v)


@pytest.mark.parametrize("name", ["lid_one", "lid_multi", "lid_level", "lid_only_cam"])
def test_lidar_error_without_speculation(gpu_ctx, monkeypatch, name):
    """SQLM_NO_SPEC=1: no speculative camera pass writes lid_err, k_lidar_chi2 alone does."""
    run = _run(gpu_ctx, name, monkeypatch, {"SQLM_NO_SPEC": "1"})
    _one_accepted_trial(run)
    _check_lidar_error(_problem(name), run, lidc.LEVEL.get(name, 0))


@pytest.mark.parametrize("switch", ["SQLM_NO_SPEC", "SQLM_NO_POSE_FUSE"])
def test_schedules_same_bits(gpu_ctx, monkeypatch, switch):
    a = _run(gpu_ctx, "lid_multi", monkeypatch)
    b = _run(gpu_ctx, "lid_multi", monkeypatch, {switch: "1"})
    _one_accepted_trial(b)
    _same_bits(a, b)
    assert np.array_equal(a["lid_err"], b["lid_err"])


def test_edges_on_a_fixed_pose_change_no_bit(gpu_ctx, monkeypatch):
    """lid_multi without the 40 edges of the fixed pose 0: the same result."""
    a = _run(gpu_ctx, "lid_multi", monkeypatch)
    p = lidc.multi_without_fixed()
    full = _problem("lid_multi")
    assert p.n_lid == full.n_lid - 40
    b = run_problem(gpu_ctx, p, 1.0, _setenv(monkeypatch), {})
    _one_accepted_trial(b)
    _same_bits(a, b)
    assert a["st"]["n_active_edges"] == b["st"]["n_active_edges"]
    assert np.array_equal(a["lid_err"][full.lid_pose != 0], gpu_ctx.lidar_error())


@functools.lru_cache(maxsize=None)
def _association():
    prob, clouds = LC.lba_case()
    return prob, clouds, LC.lba_association_args(clouds, prob.pose_q, prob.pose_t)


def test_association_route_same_bits(gpu_ctx, monkeypatch):
    """Edges that sqlm_set_lidar_from_clouds builds on the device against the
    same pairs (sqlm_lidar_associate returns them) through sqlm_set_lidar: one
    trial, the same bits, the same per-edge errors."""
    prob, clouds, args = _association()
    cur = int(clouds.pose_index[clouds.current])
    idx, d2, xyz, acc = gpu_ctx.lidar_associate(args["map_clouds"], args["map_Twc"], args["query_xyz"],
                                                args["query_Twc"], args["thr"])
    k = np.nonzero(acc)[0]
    assert 0 < k.size < acc.size
    pairs = prob.copy()
    pairs.lid_pose = np.full(k.size, cur, np.int32)
    pairs.lid_pc = np.asarray(clouds.query_xyz, np.float32)[k].astype(np.float64)
    pairs.lid_pw = xyz[k].astype(np.float64)
    pairs.lid_n = np.asarray(clouds.query_normal, np.float32)[k].astype(np.float64)
    pairs.lid_info = np.full(k.size, float(clouds.weight))
    pairs.validate()
    b = run_problem(gpu_ctx, pairs, 1.0, _setenv(monkeypatch), {})
    b_err = gpu_ctx.lidar_error()
    n = []

    def from_clouds(ctx):
        n.append(ctx.set_lidar_from_clouds(cur, args["map_clouds"], args["map_Twc"], args["query_xyz"],
                                           args["query_Twc"], clouds.query_normal, clouds.weight, args["thr"]))
    a = run_problem(gpu_ctx, prob.copy(), 1.0, _setenv(monkeypatch), {}, set_lidar=from_clouds)
    a_err = gpu_ctx.lidar_error(n[0])
    assert n == [k.size]
    assert a["n"] == b["n"] == 1 and a["st"]["trials"] == b["st"]["trials"]
    _same_bits(a, b)
    assert a["st"]["n_active_edges"] == b["st"]["n_active_edges"] == prob.n_obs + k.size
    assert np.array_equal(a_err, b_err) and np.all(b_err != 0.0)
    ref = lin_ref.lidar_edges(pairs, np.float64, b["q"], b["t"], jac=False)
    if b["st"]["trace_trials"] == [1]:          # accepted: the staged error is that of the returned state
        assert np.array_equal(b_err, ref.e)


def test_lidar_error_arguments(gpu_ctx, monkeypatch):
    import ctypes as C
    from sqrtlm import _lib
    from sqrtlm.optimizer import Context
    L = _lib.lib()
    prob = _problem("lid_one")
    buf = (C.c_double * prob.n_lid)()
    with Context(0) as fresh:
        assert L.sqlm_get_lidar_error(fresh._h, buf) == -7              # no problem
        fresh.set_problem(prob)
        assert L.sqlm_get_lidar_error(fresh._h, buf) == -7              # set, never optimized
    _run(gpu_ctx, "lid_one", monkeypatch)
    assert L.sqlm_get_lidar_error(gpu_ctx._h, None) == -1
    assert L.sqlm_get_lidar_error(gpu_ctx._h, buf) == 0
    gpu_ctx.set_problem(prob)                                           # new edges: nothing computed yet
    assert L.sqlm_get_lidar_error(gpu_ctx._h, buf) == -7
