"""The first LM trial of the landmark-sharded BA against the extended-precision
reference of tests/lin_ref.py: what tests/test_gpu_first_trial.py does for the
unsharded path, with its cases, its ratios() and its rule -- GPU error <= K x
the reference's own float64-vs-longdouble spread of that quantity on that
problem, floored at 4 eps, K = 100 -- or bit equality. No other tolerance.

The other sharded tests (test_gpu_sharded.py, test_gpu_rccl.py) compare ten LM
iterations with the oracle at 1e-6 on two mono generators; a slightly wrong
gathered system survives that. Here one trial runs on every rank and
sqlm_get_last_step gives the gathered right-hand side and the broadcast step.

a. Self-loop (one rank, RCCL to itself, in-process): every case of both case
   tables must give the bits of the unsharded run -- g, dx, poses, points,
   chi2 -- and the same solver layout. The sharded path sums the same tile
   partials in the same order into the BSR S and scatters it (k_cr_scatter)
   where the unsharded path reduces straight into the CR superblocks.
b. Worlds 2 and 3 over the host transport (gloo), contiguous landmark ranges
   (shard()): RANGE_CASES of tests/sharded_first_trial_cases.py. One spawn per
   world, every rank process loops over all runs of its world on one context.
c. Degenerate owner maps at world 3 (shard_by_owner): a rank that owns exactly
   the landmarks seen by fixed cameras only (empty row range, sends nothing,
   its points still move); landmark index % 3 (every rank spans the whole
   band); a middle rank without any landmark. The last was admitted after
   reading the zero-size paths (`tools/plan_check shard` runs the planner
   on n_pt = n_obs = 0; every buffer is sized max(n, 1), every launch
   wrapper returns on an empty grid, zero-length sends and receives are
   skipped on both ends); ranks >= 1 of lid_level_l1 take the same path.
d. lambda_0 from the summed pose diagonals (k_pose_diag, all-reduce,
   k_pose_maxdiag): three problems at user_lambda = 0 against the reference at
   lin_ref.lambda_init; the spread holds the float64 evaluation of lambda_0.

Assembly of a multi-rank run for ratios(): g, dx, poses and stats of rank 0, X
put together by owner. Also asserted per run: one accepted trial on every
rank; dx, q, t and the trial chi2 bit-equal across ranks; g of a rank >= 1
zero outside its row range; the solver layout of every rank; every rank's own
points within the dl bound.

The LM scale term (trace_lambda[0] through the all-reduced computeScale) is
not pinned: g2o's factor 1 - (2 rho - 1)^3 is clamped to 1/3 unless it exceeds
it, and the longdouble reference gives 0.29 on fixed_plain, 1.7e-4 on
lid_level_l1 and -8.7 .. -16.3 on every other run here (rho 1.57 .. 1.79): no
case has a factor >= 0.4, so lambda after the trial is lambda / 3 whatever the
scale is.

Ratios (GPU error / spread) measured on an MI355X when the test was written:

    run               world  g     dx     dl     pose   chi2
    mid_lam1e-3       2      0.22  0.43   0.44   0.43   0.22
    mid_lam1          2      0.94  0.34   0.82   0.41   0.094
    mid_lam1e3        2      0.75  1.2    1.0    0.21   0.41
    rows              2      1.5   1.3    1.6    1.3    0.71
    long_track        2      0.65  5.7    1.9    0.74   0.21
    stereo_half       2      1.1   0.30   0.32   0.26   0.020
    dups              2      1.9   0.97   1.1    0.83   0.22
    long_red          2      0.50  2.0    0.55   0.33   0.20
    cr_levels         2      0.43  0.038  0.088  0.042  0.43
    border            2      1.9   0.28   0.26   0.27   0.29
    fixed_robust      2      0.90  0.29   0.43   0.30   0.40
    fixed_plain       2      0.26  0.42   0.30   0.40   0.11
    lid_multi         2      0.73  0.39   0.40   0.31   0.92
    lid_border        2      1.9   0.29   0.28   0.27   0.32
    lid_rows          2      1.5   2.4    5.6    2.3    0.21
    lid_level_l1      2      0.96  19     0      13     1.0
    lam0_mid_lam1     2      0.76  1.9    1.0    0.21   0.14
    lam0_border       2      5.4   1.3    0.71   0.26   0.68
    lam0_stereo_half  2      1.3   1.4    0.85   0.14   0.44
    mid_lam1e-3       3      0.22  0.46   0.46   0.46   0.52
    mid_lam1          3      0.91  0.30   0.73   0.30   0.57
    mid_lam1e3        3      0.82  1.2    1.0    0.21   0.32
    rows              3      1.5   1.4    1.5    1.4    0.16
    long_track        3      0.65  7.4    2.5    1.1    0.16
    stereo_half       3      1.1   0.28   0.30   0.20   0.31
    dups              3      1.9   0.99   1.5    0.99   0.70
    long_red          3      0.41  2.3    0.61   0.40   0.0082
    cr_levels         3      0.43  0.051  0.093  0.042  0.17
    border            3      1.9   0.29   0.29   0.29   0.33
    fixed_robust      3      0.90  0.32   0.45   0.31   0.22
    fixed_plain       3      0.26  0.44   0.34   0.41   0.37
    lid_multi         3      0.73  0.44   0.46   0.43   0.40
    lid_border        3      1.9   0.27   0.25   0.27   0.013
    lid_rows          3      1.5   1.9    6.0    1.9    0.46
    lid_level_l1      3      0.96  19     0      13     1.0
    lam0_mid_lam1     3      0.82  1.9    1.0    0.21   0.39
    lam0_border       3      5.4   1.5    0.71   0.26   0.75
    lam0_stereo_half  3      1.3   1.3    0.85   0.14   0.29
    fixed_only_rank   3      0.26  0.45   0.34   0.43   0.31
    interleaved       3      0.94  0.38   0.87   0.45   0.14
    empty_rank        3      0.94  0.34   0.82   0.41   0.094

The largest is 19 (dx of lid_level_l1 at both worlds, 1.1e-13 against a spread
of 6.0e-15; rank 0 alone holds active edges there, so it is the unsharded
run's ratio). Every self-loop case of (a) gave the bits of the unsharded run,
none needed the K rule in their place.

Wrong builds tried on scratch copies of the library (none committed):

- k_gather_add ignoring the last rank's g range: 39 of the 41 reference
  comparisons fail, g ratios 1.2e14 .. 8.0e14 (g wrong by 0.33 .. 1.0 relative),
  dx 1.4e10 .. 2.0e14, dl 7.4e11 .. 4.0e14. The two that pass are lid_level_l1
  at worlds 2 and 3, whose last rank sends nothing.
- lambda added by every rank (the device's rank test answering "rank 0" on
  every rank: k_rcs :919, rcs_put_s, and the scale term): the same 39 fail, g
  unchanged (ratios 0.22 .. 5.4), dx 9.1e6 .. 8.6e13, dl 9.2e6 .. 2.5e12; the
  smallest are mid_lam1e-3's, where a second or third 1e-3 weighs least.
- the pose-diagonal all-reduce skipped (lambda_0 from one rank's share): the
  six lambda_0 comparisons fail, g 1.7e13 .. 3.5e13 (g wrong by ~2e-2: it holds
  (H_ll + lambda I)^-1), dx 6.6e12 .. 4.9e13, dl 4.7e12 .. 1.7e13, and
  test_sharded_case_paths (lambda after the trial outside lambda_0 / 3 .. 2/3
  lambda_0); every run with a user lambda passes, as it must.
"""
import functools
import os
import time
import traceback

import numpy as np
import pytest

import lin_ref
import sharded_first_trial_cases as shc
import test_gpu_first_trial as ft
import test_gpu_first_trial_lidar as fl
from dist_util import gloo_allreduce, gloo_p2p, run_ranks
from test_gpu_first_trial import FLOOR, K, ratios

pytestmark = pytest.mark.gpu

# rcs_layout()["kind"] of a case, where it is the case's subject
KIND = {**{n: e[2] for n, e in ft.EXPECT.items()}, **{n: e[1] for n, e in fl.EXPECT.items()}}
# exec_info()["tile_kernel"] every rank that holds active vision edges must report
KERNEL = {"rows": "rows", "lid_rows": "rows", "long_track": "tile_mono", "stereo_half": "tile_stereo"}
# one spawn of a world took 3.4 s when the test was written (process start, HIP
# and gloo initialisation, all 22 runs of world 3); the margin is for a cold
# page cache and a busy host, not for the runs (1 .. 43 ms each)
SPAWN_S = 3.4
TIMEOUT = SPAWN_S + 60.0


# ------------------------------------------------------------------ a. self-loop

@pytest.fixture(scope="module")
def loop_ctx():
    from sqrtlm.optimizer import Context, comm_unique_id
    with Context(0) as ctx:
        ctx.set_comm_selfloop(comm_unique_id())
        yield ctx


@pytest.mark.parametrize("name", sorted(ft.ALL_CASES))
def test_selfloop_same_bits_as_unsharded(gpu_ctx, loop_ctx, monkeypatch, name):
    a = ft.run_gpu(gpu_ctx, name, ft._setenv(monkeypatch))
    b = ft.run_gpu(loop_ctx, name, ft._setenv(monkeypatch))
    assert loop_ctx.comm_info()["transport"] == "rccl-selfloop"
    ft._one_accepted_trial(b)
    ft._same_bits(a, b)
    assert a["lay"]["kind"] == b["lay"]["kind"] and a["lay"]["n_free"] == b["lay"]["n_free"]
    assert a["info"]["tile_kernel"] == b["info"]["tile_kernel"]


# ------------------------------------------------------------------ b - d. several ranks

def _agree(failed):
    """True on every rank if any rank failed: all take the same decision."""
    import torch
    import torch.distributed as dist
    t = torch.tensor([1 if failed else 0], dtype=torch.int32)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return bool(t.item())


def _rank(rank, world, names):
    """One rank process: every run of its world on one context. A run's
    exception is recorded, and the later runs still go, where all ranks know of
    it (an all-reduce before and after optimize())."""
    from sqrtlm.optimizer import Context
    out = {}
    with Context(0) as ctx:
        ctx.set_host_comm(rank, world, gloo_allreduce, gloo_p2p)
        for name in names:
            err = None
            try:
                loc = shc.local_problem(name, world, rank)
                env = shc.setup_env(name)
                for k in ft.SWITCHES:  # read by the library at every setup
                    if env.get(k) is None:
                        os.environ.pop(k, None)
                    else:
                        os.environ[k] = env[k]
                ctx.set_problem(loc)
                if loc.meta.get("lid_level") is not None:
                    ctx.set_lidar_level(loc.meta["lid_level"])
            except Exception:  # noqa: BLE001
                err = traceback.format_exc()
            if _agree(err is not None):
                out[name] = dict(error=err or "another rank failed before optimize()")
                continue
            res = None
            try:
                t0 = time.perf_counter()
                n, st = ctx.optimize(shc.level(name), 1, user_lambda=shc.user_lambda(name))
                g, dx = ctx.last_step()
                q, t = ctx.poses()
                res = dict(n=n, st=st, g=g, dx=dx, q=q, t=t, X=ctx.points(), info=ctx.exec_info(),
                           lay=ctx.rcs_layout(), sec=time.perf_counter() - t0)
            except Exception:  # noqa: BLE001
                err = traceback.format_exc()
            out[name] = dict(error=err or "another rank failed in optimize()") if _agree(err is not None) else res
    return out


@functools.lru_cache(maxsize=None)
def _world(world):
    """Results by rank of every run of `world`: spawned once."""
    t0 = time.perf_counter()
    res = run_ranks(_rank, world, shc.runs(world), timeout=TIMEOUT)
    print(f"world {world}: {len(shc.runs(world))} runs on {world} ranks in {time.perf_counter() - t0:.1f} s")
    return res


@functools.lru_cache(maxsize=None)
def _reference_lambda0(base):
    return lin_ref.spreads_lambda_init(ft._problem(base))


def _assemble(name, world, runs):
    """g, dx, poses, stats of rank 0; X by owner."""
    prob, owner = shc.problem(name), shc.owner_map(name, world)
    X = np.zeros_like(prob.pt)
    for r, run in enumerate(runs):
        X[owner == r] = run["X"]
    return dict(runs[0], X=X)


@pytest.mark.parametrize("name,world", shc.pairs())
def test_sharded_first_trial_matches_reference(oracle, name, world):
    runs = [res[name] for res in _world(world)]
    for r, run in enumerate(runs):
        assert "error" not in run, (r, run["error"])
    base, prob, owner = shc.base(name), shc.problem(name), shc.owner_map(name, world)
    reference = _reference_lambda0(base) if name in shc.LAMBDA0 else ft._reference(base)
    rt = ratios(oracle, base, _assemble(name, world, runs), reference)
    print(f"{name} world {world}: " + " ".join(f"{k} {v[0]:.2g} ({v[1]:.1e}/{v[2]:.1e})" for k, v in rt.items()),
          [(run["info"]["tile_kernel"], run["lay"]["kind"], f"{run['sec'] * 1e3:.0f} ms") for run in runs])
    for k, v in rt.items():
        assert v[0] <= K, (name, world, k, v)
    sp, ref, f64 = reference
    nP = ref.free.size
    for r, run in enumerate(runs):
        ft._one_accepted_trial(run)
        assert run["lay"]["n_free"] == nP
        if KIND.get(base) is not None:
            assert run["lay"]["kind"] == KIND[base], (r, run["lay"])
        loc = shc.local_problem(name, world, r)
        if base in KERNEL and np.any(loc.obs_level == shc.level(name)):
            assert run["info"]["tile_kernel"] == KERNEL[base], (r, run["info"])
        # every rank applied the step rank 0 solved for
        for k in ("dx", "q", "t"):
            assert np.array_equal(run[k], runs[0][k]), (r, k)
        assert run["st"]["trace_chi2"][0] == runs[0]["st"]["trace_chi2"][0], r
        # a rank's own share of g lives inside its row range
        lo, hi = shc.row_range(name, world, r)
        if r > 0:
            assert not run["g"][:lo].any() and not run["g"][hi:].any(), (r, lo, hi)
            assert hi == lo or (run["g"][lo].any() and run["g"][hi - 1].any()), (r, lo, hi)
        # its own points, within the dl bound
        mine = owner == r
        if ref.lms.size and mine.any():
            dmax = np.abs(ref.dl).max()
            X_hi = prob.pt.astype(lin_ref.LD) + ref.dl
            err = float(np.abs(run["X"] - X_hi[mine]).max() / dmax)
            assert err <= K * max(rt["dl"][2], FLOOR), (r, err, rt["dl"])
        else:
            assert np.array_equal(run["X"], prob.pt[mine]), r


def test_sharded_case_paths():
    """What the runs are there for, beyond the layout / kernel asserted above."""
    w2, w3 = _world(2), _world(3)
    for res in (w2, w3):
        assert any(r["dups"]["info"]["tile_dups"] == 1 for r in res)
        assert all(r["long_track"]["info"]["tile_maxk"] > 32 for r in res)     # too long for the producer kernel
        assert all(r["border"]["lay"]["border_cams"] > 0 for r in res)
        assert all(r["cr_levels"]["lay"]["p"] >= 5 for r in res)
        # LiDAR-only level: the other ranks hold no tile, no landmark moved
        assert all(r["lid_level_l1"]["info"]["tile_kernel"] == "none" for r in res)
    # the fixed-only rank and the empty rank still moved with the others
    fo = shc.fixed_only_landmarks(shc.problem("fixed_only_rank"))
    moved = np.abs(w3[1]["fixed_only_rank"]["X"] - shc.problem("fixed_only_rank").pt[fo]).max(axis=1)
    assert fo.sum() == w3[1]["fixed_only_rank"]["X"].shape[0] and np.all(moved > 0)
    assert w3[1]["empty_rank"]["X"].shape == (0, 3) and w3[1]["empty_rank"]["info"]["tile_kernel"] == "none"
    assert not w3[1]["empty_rank"]["g"].any() and w3[1]["empty_rank"]["dx"].any()
    # lambda_0: the library's own, lambda after the trial is lambda_0 / 3 .. 2/3 lambda_0
    for name, (base, _) in shc.LAMBDA0.items():
        lam0 = float(lin_ref.lambda_init(ft._problem(base)))
        for res in (w2, w3):
            assert 1 / 3 - 1e-9 <= res[0][name]["st"]["trace_lambda"][0] / lam0 <= 2 / 3 + 1e-9


def test_last_step_on_sharded_context_states(loop_ctx, monkeypatch):
    """sqlm_get_last_step no longer refuses a context with a communicator; the
    other documented states are unchanged."""
    import ctypes as C
    from sqrtlm import _lib
    from sqrtlm.optimizer import Context, comm_unique_id
    L = _lib.lib()
    buf = (C.c_double * 6)()
    with Context(0) as fresh:
        fresh.set_comm_selfloop(comm_unique_id())
        assert L.sqlm_get_last_step(fresh._h, buf, buf) == -7         # no problem
        fresh.set_problem(ft._problem("cls3"))
        assert L.sqlm_get_last_step(fresh._h, buf, buf) == -7         # set, never optimized
    ft.run_gpu(loop_ctx, "cls3", ft._setenv(monkeypatch))
    assert L.sqlm_get_last_step(loop_ctx._h, None, buf) == -1
    g, dx = loop_ctx.last_step()
    assert g.any() and dx.any()
