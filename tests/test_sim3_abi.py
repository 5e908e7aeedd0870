"""The Sim3-alignment entry points exist at every layer: header, library,
binding, Python facade; their argument checks answer without a GPU."""
import ctypes as C
import os
import re

import numpy as np

from sqrtlm import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sqlm_sim3_optimize", "sqlm_sim3_get_pair_chi2", "sqlm_sim3_get_linearization", "sqlm_sim3_get_last_step"]


def test_header_binding_and_library_carry_the_names():
    hdr = open(os.path.join(ROOT, "include", "sqrtlm.h")).read()
    declared = set(re.findall(r"\b(sqlm_[A-Za-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for n in NAMES:
        assert n in declared, n
        assert n in _lib.EXPORTS, n
        assert hasattr(L, n), n
    assert "sqlm_sim3_stats" in hdr


def test_stats_struct_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "sqrtlm.h")).read()
    m = re.search(r"#define SQLM_SIM3_TRACE_MAX (\d+)", hdr)
    assert m and int(m.group(1)) == _lib.SIM3_TRACE_MAX
    T = _lib.SIM3_TRACE_MAX
    # 8 ints, 6 doubles, 2 ints, 2 x 2 T doubles, 2 T ints; no padding (all 8-aligned)
    assert C.sizeof(_lib.Sim3Stats) == 8 * 4 + 6 * 8 + 2 * 4 + 4 * T * 8 + 2 * T * 4
    body = hdr[hdr.index("typedef struct sqlm_sim3_stats"):hdr.index("} sqlm_sim3_stats;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b([a-z_0-9]+)(?:\[[A-Z_0-9]+\])+[,;]|\b([a-z_0-9]+)[,;]", body)
    names = [a or b for a, b in fields]
    assert names == [f[0] for f in _lib.Sim3Stats._fields_], names


def test_invalid_arguments():
    L = _lib.lib()
    d = np.zeros(8)
    off = np.zeros(2, np.int64)
    p = _lib.ptr
    # no context
    assert L.sqlm_sim3_optimize(None, 0, None, None, None, None, None, p(off), None, None, None, None, None, None,
                                None, C.c_double(0), None, None, None, None) == -1
    assert L.sqlm_sim3_optimize(None, -1, p(d), p(d), p(d), p(d), p(d), p(off), p(d), p(d), p(d), p(d), p(d), p(d),
                                None, C.c_double(0), p(d), p(d), p(d), None) == -1
    assert L.sqlm_sim3_get_pair_chi2(None, p(d)) == -1
    assert L.sqlm_sim3_get_linearization(None, p(d), p(d)) == -1
    H = np.zeros(49)
    assert L.sqlm_sim3_get_last_step(None, 0, p(H), p(d), p(d)) == -1


def test_python_facade():
    from sqrtlm.optimizer import Context, Optimizer
    from sqrtlm import sim3, synth
    assert callable(Optimizer.OptimizeSim3) and callable(Context.sim3_optimize)
    prob = synth.make_sim3_problem(12, seed=1)
    assert isinstance(prob, sim3.Sim3Problem)
    a = sim3.pack([prob, synth.make_sim3_problem(0), synth.make_sim3_problem(5, seed=2)])
    assert a["pair_off"].tolist() == [0, 12, 12, 17] and a["X1c"].shape == (17, 3) and a["S12"].shape == (3, 8)
    assert a["th2"].tolist() == [10.0, 10.0, 10.0] and a["fix_scale"].dtype == np.uint8
