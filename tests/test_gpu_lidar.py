"""sqlm_lidar_associate / sqlm_set_lidar_from_clouds (the LiDAR association of
local-BA pass 3 as an exact brute-force 1-NN on the GPU) against the numpy
reference tests/lidar_ref.py.

Everything is np.array_equal: every float that decides a result (the world
coordinates, the squared distance, the threshold test) is produced by IEEE
operations in a fixed order on both sides, so bit-equality is the bound; no
tolerance appears in this file. Shapes sit at the kernel's own boundaries: T
(map points per LDS tile) and W (queries per workgroup) are read from
sqlm_lidar_get_exec_info; nothing is larger than 5 T map points x 2 W queries.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import lidar_cases as LC
import lidar_ref as LR
from sqrtlm import _lib
from sqrtlm.optimizer import Context, Optimizer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("nn_index", "nn_sq_dist", "nn_xyz", "accepted")


def run_gpu(ctx, case):
    idx, d2, xyz, acc = ctx.lidar_associate(case["map_clouds"], case["map_Twc"], case["query_xyz"], case["query_Twc"],
                                            case["thr"])
    return dict(nn_index=idx, nn_sq_dist=d2, nn_xyz=xyz, accepted=acc, n_pairs=ctx.lidar_n_pairs)


def assert_same(got, ref, what=""):
    for k in KEYS:
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), (what, k)
    assert got["n_pairs"] == ref["n_pairs"], what


@pytest.fixture(scope="module")
def tiles(gpu_ctx):
    """(T, W) as the library reports them."""
    run_gpu(gpu_ctx, LC.threshold_case())
    info = gpu_ctx.lidar_exec_info()
    T, W = info["map_tile"], info["query_tile"]
    assert T >= 64 and W >= 64 and W % 64 == 0
    return T, W


def _size(sym, T, W):
    return {"1": 1, "T-1": T - 1, "T": T, "T+1": T + 1, "2T+3": 2 * T + 3, "63": 63, "64": 64, "65": 65, "W+1": W + 1}[sym]


@pytest.mark.parametrize("nq", ["1", "63", "64", "65", "W+1"])
@pytest.mark.parametrize("nm", ["1", "T-1", "T", "T+1", "2T+3"])
def test_one_cloud_at_the_tile_boundaries(gpu_ctx, tiles, nm, nq):
    T, W = tiles
    n_map, n_query = _size(nm, T, W), _size(nq, T, W)
    case = LC.random_case((n_map,), n_query, seed=n_map * 7 + n_query)
    ref = LR.associate(**case)
    got = run_gpu(gpu_ctx, case)
    assert_same(got, ref, (nm, nq))
    info = gpu_ctx.lidar_exec_info()
    assert (info["n_map"], info["n_query"], info["n_pairs"]) == (n_map, n_query, ref["n_pairs"])
    assert info["segments"] >= 1
    if n_map >= T and n_query >= 63:
        assert 0 < ref["n_pairs"] < n_query  # both outcomes of the threshold


@pytest.mark.parametrize("world", [False, True])
@pytest.mark.parametrize("sizes,nq", [(("T+1", "0", "T-1"), "65"), (("2T+3", "0", "1"), "W+1"), (("1", "0", "1"), "1"),
                                      (("0", "T", "0"), "64")])
def test_three_clouds_with_an_empty_one(gpu_ctx, tiles, sizes, nq, world):
    """Clouds with their own T_wc (the matrix is found from map_off, empty
    clouds skipped), and the same clouds given as world points (map_Twc = NULL)."""
    T, W = tiles
    ns = tuple(0 if s == "0" else _size(s, T, W) for s in sizes)
    case = LC.random_case(ns, _size(nq, T, W), seed=sum(ns) + 11, world=world)
    ref = LR.associate(**case)
    assert_same(run_gpu(gpu_ctx, case), ref, (sizes, nq, world))
    if world:  # untouched coordinates
        assert np.array_equal(ref["map_w"], np.concatenate(case["map_clouds"]))


def test_threshold_equality_and_empty_map(gpu_ctx):
    case = LC.threshold_case()
    ref = LR.associate(**case)
    got = run_gpu(gpu_ctx, case)
    assert_same(got, ref)
    assert got["accepted"].tolist() == [0, 1, 0] and got["nn_sq_dist"][0] == np.float32(0.3125) == np.float32(case["thr"])
    for clouds, Twc in (([], None), ([np.zeros((0, 3), np.float32)] * 3, np.zeros((3, 4, 4), np.float32))):
        e = dict(case, map_clouds=clouds, map_Twc=Twc)
        got = run_gpu(gpu_ctx, e)
        assert_same(got, LR.associate(**e), "empty")
        assert got["nn_index"].tolist() == [-1] * 3 and got["n_pairs"] == 0
        assert gpu_ctx.lidar_exec_info()["segments"] == 0
    # no query: SQLM_OK, zero pairs
    got = run_gpu(gpu_ctx, dict(case, query_xyz=np.zeros((0, 3), np.float32)))
    assert got["n_pairs"] == 0 and got["nn_index"].size == 0


def test_tie_in_one_segment(gpu_ctx, tiles):
    T, _ = tiles
    case, low, tied = LC.tie_case(T + 5, T, 3, T - 2)
    ref = LR.associate(**case)
    got = run_gpu(gpu_ctx, case)
    assert_same(got, ref)
    assert [int(got["nn_index"][i]) for i in tied] == [low] * len(tied)


def test_reuse_small_after_large(gpu_ctx, tiles):
    """A small association after a large one on the same context gives the
    small one's stand-alone result (no stale buffer contents are read)."""
    T, W = tiles
    large = LC.random_case((3 * T, 2 * T), 2 * W, seed=21)
    small = LC.random_case((T - 1,), 63, seed=22)
    assert_same(run_gpu(gpu_ctx, large), LR.associate(**large), "large")
    after = run_gpu(gpu_ctx, small)
    assert_same(after, LR.associate(**small), "small after large")
    with Context(0) as fresh:
        alone = run_gpu(fresh, small)
    assert_same(after, alone, "stand-alone")


# ---- SQLM_LIDAR_SPLIT: the result does not depend on the map segments ---------

CHILD = r"""
import sys, numpy as np
sys.path[:0] = [sys.argv[2] + '/tests', sys.argv[2], sys.argv[2] + '/sqrtlm-slam_amd']
import lidar_cases as LC
from sqrtlm.optimizer import Context
ctx = Context(0)
out = {}
ctx.lidar_associate(**{k if k != 'thr' else 'dist_sq_threshold': v for k, v in LC.threshold_case().items()})
T, W = ctx.lidar_exec_info()['map_tile'], ctx.lidar_exec_info()['query_tile']
cases = {'rand': LC.random_case((2 * T + 3, 0, 2 * T), W + 1, seed=31),
         'tie': LC.tie_case(3 * T, 2 * T, 10, 5)[0]}
for name, c in cases.items():
    idx, d2, xyz, acc = ctx.lidar_associate(c['map_clouds'], c['map_Twc'], c['query_xyz'], c['query_Twc'], c['thr'])
    out.update({name + '_nn_index': idx, name + '_nn_sq_dist': d2, name + '_nn_xyz': xyz, name + '_accepted': acc,
                name + '_n_pairs': ctx.lidar_n_pairs, name + '_segments': ctx.lidar_exec_info()['segments']})
np.savez(sys.argv[1], T=T, W=W, **out)
ctx.close()
"""


def _child(tmp_path, split):
    out = str(tmp_path / f"split_{split}.npz")
    env = dict(os.environ)
    env.pop("SQLM_LIDAR_SPLIT", None)
    if split:
        env["SQLM_LIDAR_SPLIT"] = str(split)
    subprocess.run([sys.executable, "-c", CHILD, out, ROOT], env=env, check=True, timeout=100)
    return np.load(out)


def test_segment_invariance(tmp_path):
    """SQLM_LIDAR_SPLIT 1, 3 and 7 (each in a fresh process: the knob is read from
    the environment) give byte-identical outputs, equal to the reference; the
    tie case has its two copies in different segments for 3 and 7."""
    runs = {s: _child(tmp_path, s) for s in (1, 3, 7)}
    T, W = int(runs[1]["T"]), int(runs[1]["W"])
    refs = {"rand": LR.associate(**LC.random_case((2 * T + 3, 0, 2 * T), W + 1, seed=31))}
    tie, low, tied = LC.tie_case(3 * T, 2 * T, 10, 5)
    refs["tie"] = LR.associate(**tie)
    assert [int(refs["tie"]["nn_index"][i]) for i in tied] == [low] * len(tied) == [10] * len(tied)
    # 5 T (+3) map points: split 1 -> 1 segment; 3 -> 3 segments of 2 tiles (the
    # copies at 10 and 3 T + 5 apart); 7 -> one segment per tile
    assert int(runs[1]["rand_segments"]) == 1 and int(runs[1]["tie_segments"]) == 1
    assert int(runs[3]["rand_segments"]) == 3 and int(runs[3]["tie_segments"]) == 3
    assert int(runs[7]["rand_segments"]) == 5 and int(runs[7]["tie_segments"]) == 5
    for s, r in runs.items():
        for name, ref in refs.items():
            for k in KEYS:
                assert r[f"{name}_{k}"].tobytes() == ref[k].tobytes(), (s, name, k)
            assert int(r[f"{name}_n_pairs"]) == ref["n_pairs"], (s, name)
        assert [int(r["tie_nn_index"][i]) for i in tied] == [10] * len(tied)


# ---- argument checks on a live context ----------------------------------------

def test_argument_checks_on_a_context():
    L, p = _lib.lib(), _lib.ptr
    f = np.zeros(64, np.float32)
    off = np.array([0, 4], np.int64)
    down = np.array([0, 4, 2], np.int64)
    prob, _ = LC.lba_case()
    with Context(0) as ctx:
        h = ctx._h
        assert L.sqlm_lidar_get_exec_info(h, p(np.zeros(8, np.int32))) == -7  # no association yet
        # SQLM_ERR_STATE before sqlm_set_problem
        assert L.sqlm_set_lidar_from_clouds(h, 1, 1, p(off), p(f), p(f), 2, p(f), p(f), p(f), 1.0, 1.0, None) == -7
        ctx.set_problem(prob)
        ok = (1, p(off), p(f), p(f), 2, p(f), p(f))
        bad = [(1, None, p(f), p(f), 2, p(f), p(f)), (1, p(off), None, p(f), 2, p(f), p(f)),
               (1, p(off), p(f), p(f), 2, None, p(f)), (1, p(off), p(f), p(f), 2, p(f), None),
               (-1, p(off), p(f), p(f), 2, p(f), p(f)), (1, p(off), p(f), p(f), -2, p(f), p(f)),
               (2, p(down), p(f), p(f), 2, p(f), p(f))]
        for a in bad:
            assert L.sqlm_lidar_associate(h, *a, 1.0, None, None, None, None, None) == -1, a
            assert L.sqlm_set_lidar_from_clouds(h, 1, *a, p(f), 1.0, 1.0, None) == -1, a
        assert L.sqlm_set_lidar_from_clouds(h, 1, *ok, None, 1.0, 1.0, None) == -1  # no normals
        for pose in (-1, prob.n_pose, 0):  # out of range, and pose 0 is fixed
            assert L.sqlm_set_lidar_from_clouds(h, pose, *ok, p(f), 1.0, 1.0, None) == -1, pose
        assert prob.pose_fixed[0]
        assert L.sqlm_lidar_get_exec_info(h, p(np.zeros(8, np.int32))) == -7  # none of them reached the device
        # every output may be NULL; n_query = 0 is SQLM_OK with zero pairs
        assert L.sqlm_lidar_associate(h, *ok, 1.0, None, None, None, None, None) == 0
        n = np.full(1, -1, np.int64)
        assert L.sqlm_set_lidar_from_clouds(h, 1, 1, p(off), p(f), p(f), 0, None, None, None, 1.0, 1.0, p(n)) == 0
        assert n[0] == 0


# ---- the pairs as EdgeLidarFlatPoint edges -------------------------------------

def _set_lidar(ctx, pairs):
    lp, pc, pw, nm, w = (np.ascontiguousarray(a) for a in pairs)
    p = _lib.ptr
    _lib.check(_lib.lib().sqlm_set_lidar(ctx._h, _lib.C.c_int64(lp.size), p(lp), p(pc), p(pw), p(nm), p(w)),
               "sqlm_set_lidar")


def test_set_lidar_from_clouds_equals_set_lidar(gpu_ctx):
    """6 keyframes, about 200 landmarks, 4 x 300 map points, 200 queries: the
    edges set by sqlm_set_lidar_from_clouds and the reference's pairs given to
    sqlm_set_lidar lead optimize(0, 20) to the same bits."""
    prob, clouds = LC.lba_case()
    args = LC.lba_association_args(clouds, prob.pose_q, prob.pose_t)
    ref = LR.associate(**args)
    assert 0 < ref["n_pairs"] < 200
    cur = int(clouds.pose_index[clouds.current])
    res = []
    for how in ("clouds", "pairs"):
        gpu_ctx.set_problem(prob.copy())
        if how == "clouds":
            n = gpu_ctx.set_lidar_from_clouds(cur, args["map_clouds"], args["map_Twc"], args["query_xyz"],
                                              args["query_Twc"], clouds.query_normal, clouds.weight, args["thr"])
            assert n == ref["n_pairs"]
        else:
            _set_lidar(gpu_ctx, LR.pairs(ref, cur, clouds.query_xyz, clouds.query_normal, clouds.weight))
        n_it, st = gpu_ctx.optimize(0, 20)
        q, t = gpu_ctx.poses()
        res.append((n_it, q, t, gpu_ctx.points(), gpu_ctx.edge_chi2(), st["chi2_begin"], st["chi2_end"],
                    st["n_active_edges"]))
    for a, b in zip(*res):
        assert np.array_equal(a, b)


def _stats_equal(a, b):
    keys = [k for k in a if not k.startswith("ms_")]  # wall times differ
    assert keys and all(a[k] == b[k] for k in keys), [k for k in keys if a[k] != b[k]]


def test_facade_local_ba_with_clouds(gpu_ctx):
    """Optimizer.LocalBundleAdjustment(prob, lidar=clouds) against the same
    schedule driven stepwise on a second context, the pass-3 pairs coming from
    lidar_ref at that context's pass-2 poses."""
    prob, clouds = LC.lba_case()
    pa = prob.copy()
    ra = Optimizer.LocalBundleAdjustment(pa, ctx=gpu_ctx, lidar=clouds)
    n_pairs = gpu_ctx.lidar_n_pairs
    assert ra.ran
    with Context(0) as cb:
        cb.set_problem(prob.copy())
        st = [None] * 3
        _, st[0] = cb.optimize(0, 5)
        level = cb.edge_level()
        level[(cb.edge_chi2() > 5.991) | (cb.depth_positive() == 0)] = 1
        cb.set_edge_level(level)
        cb.set_robust(None)
        _, st[1] = cb.optimize(0, 10)
        q2, t2 = cb.poses()
        ref = LR.associate(**LC.lba_association_args(clouds, q2, t2))
        _set_lidar(cb, LR.pairs(ref, int(clouds.pose_index[clouds.current]), clouds.query_xyz, clouds.query_normal,
                                clouds.weight))
        _, st[2] = cb.optimize(0, 20)
        outl = ((cb.edge_chi2() > 5.991) | (cb.depth_positive() == 0)).astype(np.uint8)
        qb, tb = cb.poses()
        Xb = cb.points()
    print("pairs", ref["n_pairs"], "of", ref["accepted"].size)
    assert n_pairs == ref["n_pairs"] > 0
    assert ref["n_pairs"] < ref["accepted"].size and np.any((ref["accepted"] == 0) & (ref["nn_index"] >= 0))
    assert st[2]["n_active_edges"] == st[1]["n_active_edges"] + n_pairs
    assert np.array_equal(pa.pose_q, qb) and np.array_equal(pa.pose_t, tb) and np.array_equal(pa.pt, Xb)
    assert np.array_equal(ra.outlier, outl)
    for a, b in zip(ra.stats, st):
        _stats_equal(a, b)
    # lidar=None is the unchanged single-call body
    pn = prob.copy()
    rn = Optimizer.LocalBundleAdjustment(pn, ctx=gpu_ctx)
    assert rn.ran and rn.stats[2]["n_active_edges"] == st[1]["n_active_edges"]
