"""tests/lidar_ref.py (the numpy reference of the LiDAR association) against an
exact kd-tree, scipy.spatial.cKDTree standing in for PCL's KdTreeFLANN, and on
the hand-built tie and threshold cases."""
import numpy as np
import pytest

import lidar_cases as LC
import lidar_ref as LR


@pytest.mark.parametrize("sizes,nq,world", [((700,), 300, False), ((300, 0, 500), 257, False), ((1200,), 64, True)])
def test_reference_finds_the_kd_tree_minimum(sizes, nq, world):
    """For every query the float64 squared distance to the reference's chosen
    point is within 1e-5 relative of the tree's minimum: distances, not
    indices, so near-ties need no exclusion. (The float32 distance carries a
    relative error of a few 2^-24 = 6e-8 per term; 1e-5 is two orders above it.)"""
    from scipy.spatial import cKDTree
    case = LC.random_case(sizes, nq, seed=len(sizes) + nq, world=world)
    r = LR.associate(**case)
    mw, qw = r["map_w"].astype(np.float64), r["query_w"].astype(np.float64)
    d_tree, _ = cKDTree(mw).query(qw, k=1)
    d_ref = ((qw - mw[r["nn_index"]]) ** 2).sum(axis=1)
    print("largest relative excess over the tree's minimum:", (d_ref / d_tree ** 2 - 1.0).max())
    assert np.all(d_ref <= d_tree ** 2 * (1.0 + 1e-5))
    # the float32 distance the reference reports is that distance
    assert np.allclose(r["nn_sq_dist"], d_ref, rtol=1e-5)
    assert 0 < r["n_pairs"] < nq  # the threshold splits the queries


def test_transform_is_the_parenthesised_double_expression():
    rng = np.random.default_rng(1)
    T = LC.rigid_f32(rng)
    p = rng.uniform(-50, 50, (40, 3)).astype(np.float32)
    out = LR.transform(p, T)
    assert out.dtype == np.float32
    for i in range(40):
        for r in range(3):
            m = [float(T[r, c]) for c in range(4)]
            x, y, z = (float(v) for v in p[i])
            assert out[i, r] == np.float32(((m[0] * x + m[1] * y) + m[2] * z) + m[3])


def test_tie_resolves_to_the_lower_index():
    case, low, tied = LC.tie_case(400, 300, 17, 123)
    r = LR.associate(**case)
    mw = r["map_w"]
    assert np.array_equal(mw[17], mw[400 + 123])
    for i in tied:
        assert r["nn_index"][i] == low == 17
    assert r["nn_sq_dist"][0] == 0.0
    # several chunks, the copies in different ones: still the lower index
    idx, d2 = LR.nearest(r["query_w"], mw, chunk=64)
    assert np.array_equal(idx, r["nn_index"]) and np.array_equal(d2, r["nn_sq_dist"])


def test_query_at_exactly_the_threshold_is_rejected():
    case = LC.threshold_case()
    r = LR.associate(**case)
    assert r["nn_sq_dist"].tolist() == [0.3125, 0.265625, 1.0]
    assert r["accepted"].tolist() == [0, 1, 0] and r["n_pairs"] == 1
    assert r["nn_index"].tolist() == [0, 0, 0]


def test_empty_map():
    for clouds in ([], [np.zeros((0, 3), np.float32)] * 2):
        r = LR.associate(clouds, None, np.ones((5, 3), np.float32), np.eye(4, dtype=np.float32), 10.0)
        assert r["nn_index"].tolist() == [-1] * 5 and r["n_pairs"] == 0 and not r["accepted"].any()
        assert np.all(np.isinf(r["nn_sq_dist"])) and not r["nn_xyz"].any()


def test_planar_scene_shows_both_outcomes():
    """The generator's noise and the threshold of the local-BA case are chosen
    so that the reference alone accepts some queries and rejects others."""
    prob, clouds = LC.lba_case()
    assert [c.shape[0] for c in clouds.xyz] == [200, 300, 300, 300, 300] and clouds.others == [1, 2, 3, 4]
    assert not prob.pose_fixed[clouds.pose_index[clouds.current]]
    r = LR.associate(**LC.lba_association_args(clouds, prob.pose_q, prob.pose_t))
    print("accepted", r["n_pairs"], "of", r["accepted"].size)
    assert 20 <= r["n_pairs"] <= r["accepted"].size - 20
    lp, pc, pw, nm, w = LR.pairs(r, 5, clouds.query_xyz, clouds.query_normal, clouds.weight)
    assert lp.tolist() == [5] * r["n_pairs"] and pc.shape == pw.shape == nm.shape == (r["n_pairs"], 3)
    assert np.allclose(np.linalg.norm(nm, axis=1), 1.0, atol=1e-6) and np.all(w == 50.0)
