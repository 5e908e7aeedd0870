"""The motion-only-BA entry points exist at every layer: header, library,
binding, Python facade; their argument checks answer without a GPU."""
import ctypes as C
import os
import re

import numpy as np

from sqrtlm import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sqlm_pose_optimize", "sqlm_pose_refine_lidar", "sqlm_pose_get_edge_chi2", "sqlm_pose_get_linearization",
         "sqlm_pose_get_last_step"]


def test_header_binding_and_library_carry_the_names():
    hdr = open(os.path.join(ROOT, "include", "sqrtlm.h")).read()
    declared = set(re.findall(r"\b(sqlm_[A-Za-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for n in NAMES:
        assert n in declared, n
        assert n in _lib.EXPORTS, n
        assert hasattr(L, n), n
    assert "sqlm_pose_stats" in hdr


def test_stats_struct_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "sqrtlm.h")).read()
    for macro, val in (("SQLM_POSE_STAGES", _lib.POSE_STAGES), ("SQLM_POSE_CHECKS", _lib.POSE_CHECKS)):
        m = re.search(r"#define %s (\d+)" % macro, hdr)
        assert m and int(m.group(1)) == val == 5
    S = _lib.POSE_STAGES
    # 8 ints, 4 S ints, 3 S doubles; no padding (28 ints end 8-aligned)
    assert C.sizeof(_lib.PoseStats) == 8 * 4 + 4 * S * 4 + 3 * S * 8
    body = hdr[hdr.index("typedef struct sqlm_pose_stats"):hdr.index("} sqlm_pose_stats;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b([a-z_0-9]+)(?:\[[A-Z_0-9]+\])+[,;]|\b([a-z_0-9]+)[,;]", body)
    names = [a or b for a, b in fields]
    assert names == [f[0] for f in _lib.PoseStats._fields_], names
    for want in ("n_corr", "rounds", "n_bad", "iterations", "trials", "result", "chi2_begin", "chi2_end", "lambda_end"):
        assert want in names


def _vision(L, ctx, n_prob, off, d, iters=None, th2=5.991, lam=0.0):
    p = _lib.ptr
    return L.sqlm_pose_optimize(ctx, n_prob, p(d), p(d), p(d), p(off), p(d), p(d), p(d), p(iters), C.c_double(th2),
                                C.c_double(lam), p(d), p(d), p(d), p(d), None)


def test_invalid_arguments():
    L = _lib.lib()
    d = np.zeros(64)
    off = np.zeros(2, np.int64)
    p = _lib.ptr
    # no context
    assert _vision(L, None, 0, off, d) == -1
    assert _vision(L, None, 1, off, d) == -1
    assert L.sqlm_pose_refine_lidar(None, 1, p(d), p(d), p(d), p(off), p(d), p(d), p(d), p(d), p(d), p(off), p(d), p(d),
                                    p(d), p(d), p(d), None, C.c_double(5.991), C.c_double(0), p(d), p(d), p(d), p(d),
                                    None) == -1
    assert L.sqlm_pose_get_edge_chi2(None, p(d)) == -1
    assert L.sqlm_pose_get_linearization(None, p(d), p(d), None, None) == -1
    assert L.sqlm_pose_get_last_step(None, 0, p(d), p(d), p(d)) == -1


def test_python_facade():
    from sqrtlm.optimizer import Context, Optimizer
    from sqrtlm import pose, synth
    for f in (Optimizer.PoseOptimization, Context.pose_optimize, Context.pose_refine_lidar, Context.pose_edge_chi2,
              Context.pose_linearization, Context.pose_last_step, pose.pack, pose.pack_lidar):
        assert callable(f)
    prob = synth.make_pose_problem(12, seed=1)
    assert isinstance(prob, pose.PoseProblem)
    a = pose.pack([prob, synth.make_pose_problem(0), synth.make_pose_problem(5, seed=2)])
    assert a["obs_off"].tolist() == [0, 12, 12, 17] and a["obs_off"].dtype == np.int64
    assert a["pose_q"].shape == (3, 4) and a["pose_t"].shape == (3, 3) and a["intr"].shape == (3, 4)
    assert a["Xw"].shape == (17, 3) and a["uv"].shape == (17, 2) and a["info"].shape == (17,)
    l = pose.pack_lidar([pose.make_lidar_pairs(prob, 7, kinds="flat"), pose.make_lidar_pairs(prob, 0),
                         pose.make_lidar_pairs(prob, 3, kinds="corner")])
    assert l["lid_off"].tolist() == [0, 7, 7, 10] and l["lid_kind"].dtype == np.uint8
    assert l["lid_kind"].tolist() == [0] * 7 + [1] * 3 and l["lid_pc"].shape == (10, 3) and l["lid_info"].shape == (10,)
