"""The LiDAR association entry points exist at every layer: header, library,
binding, Python facade; their argument checks answer without a GPU. A context
cannot exist without a device, so here every call carries a NULL context and
each bad argument beside it; tests/test_gpu_lidar.py repeats the checks on a
live context, where INVALID_ARG and STATE can be told apart."""
import ctypes as C
import os
import re

import numpy as np

from sqrtlm import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sqlm_lidar_associate", "sqlm_set_lidar_from_clouds", "sqlm_lidar_get_exec_info"]


def test_header_binding_and_library_carry_the_names():
    hdr = open(os.path.join(ROOT, "include", "sqrtlm.h")).read()
    declared = set(re.findall(r"\b(sqlm_[A-Za-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for n in NAMES:
        assert n in declared, n
        assert n in _lib.EXPORTS, n
        assert hasattr(L, n), n
    # the section sits after the pose entry points, before the result getters
    assert hdr.index("sqlm_pose_get_last_step(") < hdr.index("sqlm_lidar_associate(") < hdr.index("int sqlm_get_poses(")


def test_signatures_are_bound():
    L = _lib.lib()
    assert len(L.sqlm_lidar_associate.argtypes) == 14
    assert len(L.sqlm_set_lidar_from_clouds.argtypes) == 13
    assert len(L.sqlm_lidar_get_exec_info.argtypes) == 2
    assert L.sqlm_lidar_associate.argtypes[8] is C.c_double and L.sqlm_lidar_associate.argtypes[5] is C.c_int64
    assert L.sqlm_set_lidar_from_clouds.argtypes[1] is C.c_int32


def _assoc(L, ctx, n_clouds, off, mxyz, mT, nq, qxyz, qT):
    p = _lib.ptr
    o = np.zeros(64, np.float32)
    return L.sqlm_lidar_associate(ctx, n_clouds, p(off), p(mxyz), p(mT), nq, p(qxyz), p(qT), 1.0, p(o), p(o), p(o), p(o),
                                  None)


def _from_clouds(L, ctx, pose, n_clouds, off, mxyz, mT, nq, qxyz, qT, nrm):
    p = _lib.ptr
    return L.sqlm_set_lidar_from_clouds(ctx, pose, n_clouds, p(off), p(mxyz), p(mT), nq, p(qxyz), p(qT), p(nrm), 1.0, 1.0,
                                        None)


def test_invalid_arguments_without_a_device():
    L = _lib.lib()
    f = np.zeros(64, np.float32)
    off = np.array([0, 4], np.int64)
    down = np.array([0, 4, 2], np.int64)
    # no context, otherwise well-formed
    assert _assoc(L, None, 1, off, f, f, 2, f, f) == -1
    assert _from_clouds(L, None, 0, 1, off, f, f, 2, f, f, f) == -1
    assert L.sqlm_lidar_get_exec_info(None, _lib.ptr(np.zeros(8, np.int32))) == -1
    # and with each bad argument: NULL required pointers, negative counts, non-monotone offsets
    for bad in ((1, None, f, f, 2, f, f), (1, off, None, f, 2, f, f), (1, off, f, f, 2, None, f), (1, off, f, f, 2, f, None),
                (-1, off, f, f, 2, f, f), (1, off, f, f, -2, f, f), (2, down, f, f, 2, f, f)):
        assert _assoc(L, None, *bad) == -1, bad
        assert _from_clouds(L, None, 0, *bad, f) == -1, bad
    assert _from_clouds(L, None, -1, 1, off, f, f, 2, f, f, f) == -1
    assert _from_clouds(L, None, 0, 1, off, f, f, 2, f, f, None) == -1


def test_lidar_error_getter_at_every_layer():
    """sqlm_get_lidar_error: declared among the result getters, bound, exported,
    wrapped; without a context it answers INVALID_ARG whatever the buffer."""
    from sqrtlm.optimizer import Context
    hdr = open(os.path.join(ROOT, "include", "sqrtlm.h")).read()
    assert re.search(r"\bint\s+sqlm_get_lidar_error\s*\(\s*sqlm_ctx\s*\*\s*ctx\s*,\s*double\s*\*\s*err\s*\)\s*;", hdr)
    assert hdr.index("int sqlm_get_edge_chi2(") < hdr.index("int sqlm_get_lidar_error(") < hdr.index("int sqlm_get_rcs_layout(")
    assert "sqlm_get_lidar_error" in _lib.EXPORTS
    L = _lib.lib()
    assert hasattr(L, "sqlm_get_lidar_error") and callable(Context.lidar_error)
    buf = np.zeros(4)
    assert L.sqlm_get_lidar_error(None, _lib.ptr(buf)) == -1
    assert L.sqlm_get_lidar_error(None, None) == -1
    assert not buf.any()


def test_python_facade():
    import inspect

    from sqrtlm import lidar, synth
    from sqrtlm.optimizer import Context, Optimizer
    for fn in (Context.lidar_associate, Context.set_lidar_from_clouds, Context.lidar_exec_info, lidar.associate,
               lidar.Twc_f32, lidar.pack_clouds, synth.make_lidar_clouds):
        assert callable(fn)
    sig = inspect.signature(Optimizer.LocalBundleAdjustment)
    assert list(sig.parameters) == ["prob", "stop_flag", "ctx", "lidar"] and sig.parameters["lidar"].default is None
    off, xyz = lidar.pack_clouds([np.zeros((3, 3)), np.zeros((0, 3)), np.ones((2, 3))])
    assert off.tolist() == [0, 3, 3, 5] and off.dtype == np.int64 and xyz.shape == (5, 3) and xyz.dtype == np.float32
    # Twc_f32: the float32 inverse of Converter::toCvMat(estimate)
    q = np.array([0.0, np.sin(0.2), 0.0, np.cos(0.2)])
    t = np.array([1.0, -2.0, 3.0])
    Twc = lidar.Twc_f32(q, t)
    assert Twc.dtype == np.float32 and Twc.shape == (4, 4)
    from sqrtlm.optimizer import pose_to_Tcw_f32
    assert np.allclose(Twc @ pose_to_Tcw_f32(q, t), np.eye(4), atol=1e-6)
    c = synth.make_lidar_clouds(np.tile(q, (3, 1)), np.tile(t, (3, 1)), [4, 5, 6], n_points=[7, 0, 9], current=2, seed=1)
    assert isinstance(c, lidar.LidarClouds) and [a.shape for a in c.xyz] == [(7, 3), (0, 3), (9, 3)]
    assert c.others == [0, 1] and c.query_xyz.shape == (9, 3) and c.pose_index.tolist() == [4, 5, 6]
    c2 = synth.make_lidar_clouds(np.tile(q, (3, 1)), np.tile(t, (3, 1)), [4, 5, 6], n_points=[7, 0, 9], current=2, seed=1)
    assert all(np.array_equal(a, b) for a, b in zip(c.xyz + c.normal, c2.xyz + c2.normal))  # seeded
