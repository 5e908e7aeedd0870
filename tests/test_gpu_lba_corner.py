"""Optimizer.LocalBundleAdjustment with flat and corner LiDAR clouds (pass 3 of
g2oOptimizer.cc:1034-1107, using_flat_point and using_sharp_point): the façade
against the same schedule driven stepwise on a second context -- pass 1, pass
2, one cloud-set call at the pass-2 poses, optimize(0, 20). The oracle has no
corner edge, so there is no end-state comparison: the run is pinned trial by
trial by tests/test_gpu_first_trial_corner.py and tests/test_gpu_retrial_corner.py.
"""
import numpy as np
import pytest

import corner_cloud_cases as CC
import lidar_ref
from sqrtlm.optimizer import Context, Optimizer

pytestmark = pytest.mark.gpu


def _stats_equal(a, b):
    keys = [k for k in a if not k.startswith("ms_")]  # wall times differ
    assert keys and all(a[k] == b[k] for k in keys), [k for k in keys if a[k] != b[k]]


def test_facade_local_ba_with_corner_clouds(gpu_ctx):
    prob, clouds = CC.lba_corner_case()
    cur = int(clouds.pose_index[clouds.current])
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
        sets = CC.cloud_sets(clouds, q2, t2)
        n = cb.set_lidar_from_cloud_sets(cur, sets)
        _, st[2] = cb.optimize(0, 20)
        outl = ((cb.edge_chi2() > 5.991) | (cb.depth_positive() == 0)).astype(np.uint8)
        qb, tb = cb.poses()
        Xb = cb.points()
        err = cb.lidar_error(sum(n))
    # the inputs: what the searches must find at the pass-2 poses, on the CPU
    refs = [lidar_ref.associate(**CC.search_args(s)) for s in sets]
    print("pairs", n, "of", [r["accepted"].size for r in refs])
    assert n == [r["n_pairs"] for r in refs] and n_pairs == sum(n)
    assert all(0 < r["n_pairs"] < r["accepted"].size for r in refs)
    assert st[2]["n_active_edges"] == st[1]["n_active_edges"] + n[0] + n[1]
    assert st[1]["n_active_edges"] == int((level == 0).sum())
    assert st[2]["chi2_end"] <= st[2]["chi2_begin"] and st[2]["iterations"] > 0
    assert np.all(err[n[0]:] > 0.0) and np.all(err != 0.0)
    assert np.array_equal(pa.pose_q, qb) and np.array_equal(pa.pose_t, tb) and np.array_equal(pa.pt, Xb)
    assert np.array_equal(ra.outlier, outl)
    for a, b in zip(ra.stats, st):
        _stats_equal(a, b)
    # without corner clouds the façade takes the path it always took: fewer edges, another result
    flat_only = CC.lba_corner_case()[1]
    flat_only.corner_xyz = None
    pf = prob.copy()
    rf = Optimizer.LocalBundleAdjustment(pf, ctx=gpu_ctx, lidar=flat_only)
    assert rf.stats[2]["n_active_edges"] == st[1]["n_active_edges"] + gpu_ctx.lidar_n_pairs
    assert gpu_ctx.lidar_n_pairs == n[0] and not np.array_equal(pf.pose_t, pa.pose_t)
