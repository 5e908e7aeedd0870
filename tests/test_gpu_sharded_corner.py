"""Landmark-sharded BA with EdgeLidarCornerPoint edges. LiDAR edges are owned by
rank 0; their kinds travel with them (sqrtlm.shard.shard_by_owner).

a. The one-rank RCCL self-loop on cor_mixed gives the bits of the unsharded run.
b. Two ranks over the host transport (gloo): the first trial against
   tests/lin_ref_corner.py under K = 100 x spread (floor 4 eps), the rule of
   tests/test_gpu_first_trial_sharded.py. Ratios measured on an MI355X when the
   test was written:

    case       world  g     dx    dl    pose  chi2
    cor_mixed  2      0.74  0.71  0.58  0.49  0.35
"""
import traceback

import numpy as np
import pytest

import corner_first_trial_cases as corc
import test_gpu_first_trial as ft
import test_gpu_first_trial_corner as fc
from dist_util import gloo_allreduce, gloo_p2p, run_ranks
from sqrtlm import shard
from test_gpu_first_trial import K

pytestmark = pytest.mark.gpu
NAME = "cor_mixed"
WORLD = 2
TIMEOUT = 3.4 + 60.0   # one spawn of a world (tests/test_gpu_first_trial_sharded.py) plus margin for a busy host


@pytest.fixture(scope="module")
def loop_ctx():
    from sqrtlm.optimizer import Context, comm_unique_id
    with Context(0) as ctx:
        ctx.set_comm_selfloop(comm_unique_id())
        yield ctx


def test_selfloop_same_bits_as_unsharded(gpu_ctx, loop_ctx, monkeypatch):
    a = fc._run(gpu_ctx, NAME, monkeypatch)
    b = fc._run(loop_ctx, NAME, monkeypatch)
    assert loop_ctx.comm_info()["transport"] == "rccl-selfloop"
    ft._one_accepted_trial(b)
    ft._same_bits(a, b)
    assert np.array_equal(a["lid_err"], b["lid_err"])
    assert a["lay"]["kind"] == b["lay"]["kind"] and a["lay"]["n_free"] == b["lay"]["n_free"]


def _owner(prob, world):
    return (np.arange(prob.n_pt) % world).astype(np.int32)   # interleaved: both ranks see every camera


def _rank(rank, world, name):
    """One rank process: its share of the problem, one trial."""
    from sqrtlm.optimizer import Context
    try:
        prob = corc.CASES[name][0]()
        loc = shard.shard_by_owner(prob, _owner(prob, world), rank)
        with Context(0) as ctx:
            ctx.set_host_comm(rank, world, gloo_allreduce, gloo_p2p)
            ctx.set_problem(loc)
            n, st = ctx.optimize(0, 1, user_lambda=corc.CASES[name][1])
            g, dx = ctx.last_step()
            q, t = ctx.poses()
            return dict(n=n, st=st, g=g, dx=dx, q=q, t=t, X=ctx.points(), info=ctx.exec_info(), lay=ctx.rcs_layout(),
                        n_lid=loc.n_lid, kinds=int(loc.lid_kind.sum()))
    except Exception:  # noqa: BLE001
        return dict(error=traceback.format_exc())


def test_two_ranks_match_reference(oracle):
    prob = fc._problem(NAME)
    owner = _owner(prob, WORLD)
    runs = run_ranks(_rank, WORLD, NAME, timeout=TIMEOUT)
    for r, run in enumerate(runs):
        assert "error" not in run, (r, run["error"])
    assert runs[0]["n_lid"] == prob.n_lid and runs[0]["kinds"] == int(prob.lid_kind.sum()) > 0
    assert runs[1]["n_lid"] == 0                       # the other rank ignores them
    X = np.zeros_like(prob.pt)
    for r, run in enumerate(runs):
        X[owner == r] = run["X"]
        ft._one_accepted_trial(run)
        for k in ("dx", "q", "t"):
            assert np.array_equal(run[k], runs[0][k]), (r, k)
    rt = fc.ratios(oracle, prob, 0, dict(runs[0], X=X), fc._reference(NAME))
    print(f"{NAME} world {WORLD}: " + " ".join(f"{k} {v[0]:.2g} ({v[1]:.1e}/{v[2]:.1e})" for k, v in rt.items()))
    for k, v in rt.items():
        assert v[0] <= K, (k, v)
