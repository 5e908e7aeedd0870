"""sqlm_set_lidar_from_cloud_sets: the association of local-BA pass 3 for both
kinds of LiDAR edge in one call (g2oOptimizer.cc:1034-1107), flat set then
corner set, against separate sqlm_lidar_associate calls, tests/lidar_ref.py
and the sqlm_set_lidar + sqlm_set_lidar_kind route. Fixture: three map clouds
of 300 points and 200 queries per kind (tests/corner_cloud_cases.py).
"""
import functools

import numpy as np
import pytest

import corner_cloud_cases as CC
import lidar_ref
from test_gpu_first_trial import _same_bits, _setenv, run_problem

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case():
    prob, clouds = CC.lba_corner_case()
    sets = CC.cloud_sets(clouds, prob.pose_q, prob.pose_t)
    refs = [lidar_ref.associate(**CC.search_args(s)) for s in sets]
    return prob, clouds, sets, refs


def _pairs_problem(prob, clouds, sets, results):
    """prob with the accepted pairs of every set as edges: flat then corner, each in query order."""
    cur = int(clouds.pose_index[clouds.current])
    p = prob.copy()
    pc, pw, nm, info, kind = [], [], [], [], []
    for s, (idx, d2, xyz, acc) in zip(sets, results):
        k = np.nonzero(acc)[0]
        pc.append(np.asarray(s["query_xyz"], np.float32)[k].astype(np.float64))
        pw.append(xyz[k].astype(np.float64))
        n = s["query_normal"]
        nm.append(np.zeros((k.size, 3)) if n is None else np.asarray(n, np.float32)[k].astype(np.float64))
        info.append(np.full(k.size, float(s["info"])))
        kind.append(np.full(k.size, s["kind"], np.uint8))
    p.lid_pc, p.lid_pw, p.lid_n = np.concatenate(pc), np.concatenate(pw), np.concatenate(nm)
    p.lid_info, p.lid_kind = np.concatenate(info), np.concatenate(kind)
    p.lid_pose = np.full(p.lid_info.size, cur, np.int32)
    p.validate()
    return p


def test_sets_match_separate_searches_and_reference(gpu_ctx):
    prob, clouds, sets, refs = _case()
    assert [s["kind"] for s in sets] == [0, 1] and sets[1]["query_normal"] is None
    gpu_ctx.set_problem(prob)
    n = gpu_ctx.set_lidar_from_cloud_sets(int(clouds.pose_index[clouds.current]), sets)
    info = gpu_ctx.lidar_exec_info()
    assert gpu_ctx.lidar_n_pairs == sum(n)
    for s, r, n_k in zip(sets, refs, n):
        a = CC.search_args(s)
        idx, d2, xyz, acc = gpu_ctx.lidar_associate(a["map_clouds"], a["map_Twc"], a["query_xyz"], a["query_Twc"], a["thr"])
        assert len(s["map_clouds"]) == 3 and all(c.shape[0] == 300 for c in s["map_clouds"]) and acc.size == 200
        assert np.array_equal(idx, r["nn_index"]) and np.array_equal(d2, r["nn_sq_dist"])
        assert np.array_equal(xyz, r["nn_xyz"]) and np.array_equal(acc, r["accepted"])
        assert n_k == int(acc.sum()) == r["n_pairs"] and 0 < n_k < acc.size
    assert info["n_pairs"] == n[1] and info["n_query"] == 200 and info["n_map"] == 900   # the last set that searched


def test_cloud_set_route_same_bits(gpu_ctx, monkeypatch):
    """One trial on the edges the cloud-set call builds against the same pairs
    through sqlm_set_lidar + sqlm_set_lidar_kind: the same bits, the same
    per-edge errors, flat then corner with each kind's info."""
    prob, clouds, sets, refs = _case()
    cur = int(clouds.pose_index[clouds.current])
    results = [(r["nn_index"], r["nn_sq_dist"], r["nn_xyz"], r["accepted"]) for r in refs]
    pairs = _pairs_problem(prob, clouds, sets, results)
    nf, nc = refs[0]["n_pairs"], refs[1]["n_pairs"]
    assert not pairs.lid_kind[:nf].any() and pairs.lid_kind[nf:].all() and pairs.n_lid == nf + nc
    assert np.all(pairs.lid_info[:nf] == clouds.weight) and np.all(pairs.lid_info[nf:] == CC.CORNER_WEIGHT)
    assert clouds.weight != CC.CORNER_WEIGHT
    b = run_problem(gpu_ctx, pairs, 1.0, _setenv(monkeypatch), {})
    b_err = gpu_ctx.lidar_error()
    n = []
    a = run_problem(gpu_ctx, prob.copy(), 1.0, _setenv(monkeypatch), {},
                    set_lidar=lambda ctx: n.append(ctx.set_lidar_from_cloud_sets(cur, sets)))
    a_err = gpu_ctx.lidar_error(sum(n[0]))
    assert n == [[nf, nc]]
    assert a["n"] == b["n"] == 1 and a["st"]["trials"] == b["st"]["trials"]
    _same_bits(a, b)
    assert a["st"]["n_active_edges"] == b["st"]["n_active_edges"] == prob.n_obs + nf + nc
    assert np.array_equal(a_err, b_err) and np.all(b_err != 0.0) and np.all(b_err[nf:] > 0.0)
    # the corner set alone differs: the kinds and the corner info reached the solver
    c = run_problem(gpu_ctx, prob.copy(), 1.0, _setenv(monkeypatch), {},
                    set_lidar=lambda ctx: ctx.set_lidar_from_cloud_sets(cur, sets[:1]))
    assert not np.array_equal(a["dx"], c["dx"])


def test_one_flat_set_is_set_lidar_from_clouds(gpu_ctx, monkeypatch):
    prob, clouds, sets, refs = _case()
    cur = int(clouds.pose_index[clouds.current])
    s = sets[0]
    n = []
    a = run_problem(gpu_ctx, prob.copy(), 1.0, _setenv(monkeypatch), {},
                    set_lidar=lambda ctx: n.append(ctx.set_lidar_from_cloud_sets(cur, [s])[0]))
    a_err = gpu_ctx.lidar_error(n[0])
    b = run_problem(gpu_ctx, prob.copy(), 1.0, _setenv(monkeypatch), {},
                    set_lidar=lambda ctx: n.append(ctx.set_lidar_from_clouds(
                        cur, s["map_clouds"], s["map_Twc"], s["query_xyz"], s["query_Twc"], s["query_normal"], s["info"],
                        s["dist_sq_threshold"])))
    assert n == [refs[0]["n_pairs"]] * 2
    _same_bits(a, b)
    assert np.array_equal(a_err, gpu_ctx.lidar_error(n[1]))


def test_empty_map_set_leaves_the_other_alone(gpu_ctx, monkeypatch):
    prob, clouds, sets, refs = _case()
    cur = int(clouds.pose_index[clouds.current])
    empty = dict(sets[0], map_clouds=[], map_Twc=np.zeros((0, 16), np.float32))
    noq = dict(sets[0], query_xyz=np.zeros((0, 3), np.float32), query_normal=np.zeros((0, 3), np.float32))
    a = run_problem(gpu_ctx, prob.copy(), 1.0, _setenv(monkeypatch), {},
                    set_lidar=lambda ctx: ctx.set_lidar_from_cloud_sets(cur, [sets[1]]))
    a_err = gpu_ctx.lidar_error(refs[1]["n_pairs"])
    for other in (empty, noq):
        n = []
        b = run_problem(gpu_ctx, prob.copy(), 1.0, _setenv(monkeypatch), {},
                        set_lidar=lambda ctx: n.append(ctx.set_lidar_from_cloud_sets(cur, [other, sets[1]])))
        assert n == [[0, refs[1]["n_pairs"]]]
        assert gpu_ctx.lidar_exec_info()["n_pairs"] == refs[1]["n_pairs"]
        _same_bits(a, b)
        assert np.array_equal(a_err, gpu_ctx.lidar_error(refs[1]["n_pairs"]))


def test_split_does_not_matter(gpu_ctx, monkeypatch):
    prob, clouds, sets, refs = _case()
    cur = int(clouds.pose_index[clouds.current])
    runs = []
    for split in ("1", "3", "7"):
        monkeypatch.setenv("SQLM_LIDAR_SPLIT", split)
        n = []
        r = run_problem(gpu_ctx, prob.copy(), 1.0, _setenv(monkeypatch), {},
                        set_lidar=lambda ctx: n.append(ctx.set_lidar_from_cloud_sets(cur, sets)))
        r["lid_err"] = gpu_ctx.lidar_error(sum(n[0]))
        assert n[0] == [refs[0]["n_pairs"], refs[1]["n_pairs"]]
        runs.append(r)
    monkeypatch.delenv("SQLM_LIDAR_SPLIT")
    for r in runs[1:]:
        _same_bits(runs[0], r)
        assert np.array_equal(runs[0]["lid_err"], r["lid_err"])


def test_cloud_set_arguments(gpu_ctx):
    import ctypes as C
    from sqrtlm import _lib
    from sqrtlm.optimizer import Context
    L = _lib.lib()
    prob, clouds, sets, refs = _case()
    cur = int(clouds.pose_index[clouds.current])
    arr = (_lib.LidarSet * 1)()
    with Context(0) as fresh:
        assert L.sqlm_set_lidar_from_cloud_sets(fresh._h, cur, 0, None, None) == -7      # no problem
    assert L.sqlm_set_lidar_from_cloud_sets(None, cur, 0, None, None) == -1
    gpu_ctx.set_problem(prob)
    assert L.sqlm_set_lidar_from_cloud_sets(gpu_ctx._h, 0, 0, None, None) == -1          # a fixed pose
    assert L.sqlm_set_lidar_from_cloud_sets(gpu_ctx._h, prob.n_pose, 0, None, None) == -1
    assert L.sqlm_set_lidar_from_cloud_sets(gpu_ctx._h, cur, 1, None, None) == -1        # sets missing
    with pytest.raises(_lib.SqlmError):
        gpu_ctx.set_lidar_from_cloud_sets(cur, [dict(sets[0], kind=2)])                  # no such kind
    with pytest.raises(_lib.SqlmError):
        gpu_ctx.set_lidar_from_cloud_sets(cur, [sets[1], dict(sets[0], query_normal=None)])  # a flat set needs normals
    assert gpu_ctx.set_lidar_from_cloud_sets(cur, []) == []                              # no set: no edge
    assert C.sizeof(arr) == 80
