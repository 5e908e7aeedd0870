"""The corner-edge entry points at every layer that needs no GPU: declared in
include/sqrtlm.h, exported, bound, refusing a NULL context; the Python mirror
(BAProblem.lid_kind, shard, LidarClouds' corner clouds, the corner-cloud
generator)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sqrtlm import _lib, lidar, shard, synth
from sqrtlm.optimizer import Context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sqlm_set_lidar_kind", "sqlm_set_lidar_from_cloud_sets"]


def test_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "sqrtlm.h")).read()
    assert re.search(r"\bint\s+sqlm_set_lidar_kind\s*\(\s*sqlm_ctx\s*\*\s*ctx\s*,\s*const\s+uint8_t\s*\*\s*kind\s*\)\s*;", hdr)
    assert re.search(r"\bint\s+sqlm_set_lidar_from_cloud_sets\s*\(\s*sqlm_ctx\s*\*\s*ctx\s*,\s*int32_t\s+pose_index\s*,"
                     r"\s*int\s+n_sets\s*,\s*const\s+sqlm_lidar_set\s*\*\s*sets\s*,\s*int64_t\s*\*\s*n_pairs\s*\)\s*;", hdr)
    assert hdr.index("int sqlm_set_lidar_level(") < hdr.index("int sqlm_set_lidar_kind(") < hdr.index("int sqlm_optimize(")
    assert hdr.index("int sqlm_set_lidar_from_clouds(") < hdr.index("} sqlm_lidar_set;") \
        < hdr.index("int sqlm_set_lidar_from_cloud_sets(") < hdr.index("int sqlm_lidar_get_exec_info(")
    fields = re.search(r"typedef struct sqlm_lidar_set \{(.*?)\} sqlm_lidar_set;", hdr, re.S).group(1)
    got = re.findall(r"(\w+);", fields)
    assert got == [n for n, _ in _lib.LidarSet._fields_] == [
        "kind", "n_map_clouds", "map_off", "map_xyz", "map_Twc", "n_query", "query_xyz", "query_Twc", "query_normal",
        "info", "dist_sq_threshold"]
    assert C.sizeof(_lib.LidarSet) == 80
    L = _lib.lib()
    for n in NAMES:
        assert n in _lib.EXPORTS and hasattr(L, n), n
    assert callable(Context.set_lidar_kind) and callable(Context.set_lidar_from_cloud_sets)
    kind = np.zeros(4, np.uint8)
    assert L.sqlm_set_lidar_kind(None, _lib.ptr(kind)) == -1
    assert L.sqlm_set_lidar_kind(None, None) == -1
    assert L.sqlm_set_lidar_from_cloud_sets(None, 0, 0, None, None) == -1
    cap = open(os.path.join(ROOT, "include", "sqrtlm_capture.h")).read()
    assert re.search(r"uint8_t\s*\*\s*lid_kind\s*;", cap)
    assert cap.index("double *res_chi2;") < cap.index("*lid_kind;")     # appended: older callers' layout holds


def test_problem_kinds():
    p = synth.add_lidar_flat(synth.make_problem(6, 50, pair_window=3, seed=1), 5, 10)
    assert p.lid_kind.dtype == np.uint8 and p.lid_kind.shape == (10,) and not p.lid_kind.any()
    p.lid_kind = np.arange(10) % 2
    p.validate()
    q = p.copy()
    q.lid_kind[0] = 1
    assert p.lid_kind[0] == 0 and q.lid_kind.sum() == 6
    p.lid_kind = np.r_[p.lid_kind[:9], 2].astype(np.uint8)
    with pytest.raises(ValueError):
        p.validate()
    p.lid_kind = np.ones(9, np.uint8)
    with pytest.raises(ValueError):
        p.validate()
    # replacing the edges of an all-flat problem needs no word about kinds
    r = synth.add_lidar_flat(synth.make_problem(6, 50, pair_window=3, seed=1), 5, 10)
    synth.add_lidar_flat(r, 4, 7, append=True)
    assert r.lid_kind.shape == (17,) and not r.lid_kind.any()


def test_shard_keeps_the_kinds_on_rank_0():
    p = synth.add_lidar_flat(synth.make_problem(6, 50, pair_window=3, seed=1), 5, 10)
    p.lid_kind = (np.arange(10) % 3 == 0).astype(np.uint8)
    p.validate()
    owner = np.arange(p.n_pt) % 2
    a, b = shard.shard_by_owner(p, owner, 0), shard.shard_by_owner(p, owner, 1)
    assert np.array_equal(a.lid_kind, p.lid_kind) and a.n_lid == 10
    assert b.n_lid == 0 and b.lid_kind.shape == (0,)


def test_corner_clouds():
    p = synth.make_problem(6, 50, pair_window=3, seed=1)
    kfs = np.array([5, 1, 2], np.int32)
    c = synth.make_lidar_clouds(p.pose_q[kfs], p.pose_t[kfs], kfs, n_points=[20, 30, 30], current=0, seed=3)
    assert c.corner_xyz is None and c.corner_weight == 30.0
    Twc = [np.eye(4, dtype=np.float32)] * 3
    assert [s["kind"] for s in c.cloud_sets(Twc)] == [0]
    cor = synth.make_lidar_corner_clouds(p.pose_q[kfs], p.pose_t[kfs], n_points=[20, 30, 30], seed=4, noise=0.0)
    again = lidar.make_corner_clouds(p.pose_q[kfs], p.pose_t[kfs], n_points=[20, 30, 30], seed=4, noise=0.0)
    assert [a.shape for a in cor] == [(20, 3), (30, 3), (30, 3)] and all(a.dtype == np.float32 for a in cor)
    assert all(np.array_equal(a, b) for a, b in zip(cor, again))
    c.corner_xyz = cor
    c.__post_init__()
    sets = c.cloud_sets(Twc)
    assert [s["kind"] for s in sets] == [0, 1] and sets[1]["query_normal"] is None and sets[1]["info"] == 30.0
    assert len(sets[1]["map_clouds"]) == 2 and sets[1]["query_xyz"].shape == (20, 3)
    # without noise every point lies on a line 4 m to either side of the first camera centre
    from sqrtlm.synth import quat_to_mat
    R = quat_to_mat(p.pose_q[kfs])
    pw = np.concatenate([(cor[k].astype(np.float64) - p.pose_t[kfs[k]]) @ R[k] for k in range(3)])
    c0 = -R[0].T @ p.pose_t[kfs[0]]
    assert np.allclose(np.abs(pw[:, 0] - c0[0]), 4.0, atol=1e-4)
    assert len({tuple(x) for x in np.round(pw, 3)}) == pw.shape[0]       # distinct points along the lines
    with pytest.raises(ValueError):
        lidar.LidarClouds(c.xyz, c.normal, c.pose_index, corner_xyz=cor[:2])
