"""The cyclic reduction's superblock numbering, one against the other.

The plain band solve numbers its p superblocks 1 .. p: every level eliminates
the odd multiples of its stride, floor(p / 2) survive, and the last survivor
(the top) is the largest power of two <= p -- floor(log2 p) levels.
SQLM_CR_LO0=1 keeps the earlier numbering 0 .. p - 1 (ceil(p / 2) survive, the
top is superblock 0, ceil(log2 p) levels). Both are block eliminations of the
same SPD system in a different order, so they are compared by the rule of
tests/test_gpu_cr_fuse.py::test_legacy_factor_agrees: iteration count and
trial trace equal, chi2 within 1e-9 relative, states within 1e-9 relative.

Shapes: tracks of 2..3 keyframes with SQLM_CR_B_MIN=1 keep B = 3 (n = 32), so
p = (keyframes - 1) / 3 is what the case says: powers of two and their
neighbours (the level count does / does not drop; the top is / is not the last
superblock), plus n = 112 shapes with p = 23 and p = 93 (a wide first level).
Every run also reports the numbering, level count and top it really took
(sqlm_debug_cr_levels), which must differ as stated. On one small shape also a
rejected first trial (points far off, no kernel, a small lambda_0) and
SQLM_NO_SPEC=1. The numbering is read per plan, the other switches once per
process, hence one child process per run.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cr_levels_cases as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import json, sys, numpy as np
sys.path[:0] = [sys.argv[2], sys.argv[2] + '/sqrtlm-slam_amd']
from sqrtlm import synth
from sqrtlm.optimizer import Context
sys.path.insert(0, sys.argv[2] + '/tests')
import ctypes
import cr_levels_cases as cases
from sqrtlm import _lib
c = json.loads(sys.argv[3])
prob = cases.build(c)
ctx = Context(0)
ctx.set_problem(prob)
if c["lam0"] > 0:
    n, st = ctx.optimize(0, 3, c["lam0"])
else:
    n, st = ctx.global_ba(4)
lay = ctx.rcs_layout()
lv = (ctypes.c_int * 3)()
assert _lib.lib().sqlm_debug_cr_levels(lv) == 0
q, t = ctx.poses()
np.savez(sys.argv[1], q=q, t=t, X=ctx.points(), chi2=np.asarray(st["trace_chi2"]), n=n,
         trials=np.asarray(st["trace_trials"]), p=lay["p"], nn=lay["n"], band=lay["kind"] == "band", lv=np.asarray(list(lv)))
ctx.close()
"""


CASES = cases.CASES


def _run(tmp_path, tag, case, env_extra):
    out = str(tmp_path / f"{tag}.npz")
    env = dict(os.environ)
    for k in ("SQLM_CR_LO0", "SQLM_CR_LEGACY", "SQLM_CR_SPLIT", "SQLM_CR_B", "SQLM_NO_SPEC"):
        env.pop(k, None)
    env["SQLM_CR_B_MIN"] = "1"
    env.update(env_extra)
    subprocess.run([sys.executable, "-c", CHILD, out, ROOT, json.dumps(case)], env=env, check=True, timeout=100)
    return np.load(out)


def _rel(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


@pytest.mark.parametrize("name", list(CASES))
def test_numbering_agrees(tmp_path, name):
    case, env, _ = CASES[name]
    new = _run(tmp_path, "lo1", case, env)
    old = _run(tmp_path, "lo0", case, dict(env, SQLM_CR_LO0="1"))
    for r in (new, old):  # the shape is what the case says, on the plain band solve
        assert bool(r["band"]) and int(r["p"]) == case["p"] and int(r["nn"]) == case["n"], (r["p"], r["nn"])
    # each run really took its numbering: first superblock, level count, top
    p = case["p"]
    assert new["lv"].tolist() == [1, cases.levels(p, 1), 1 << cases.levels(p, 1)], new["lv"]
    assert old["lv"].tolist() == [0, cases.levels(p, 0), 0], old["lv"]
    print(name, "trials", new["trials"].tolist(), "chi2", new["chi2"].tolist(),
          "rel", [float(_rel(new[k], old[k])) for k in ("q", "t", "X")])
    assert int(new["n"]) == int(old["n"]) > 0
    assert np.array_equal(new["trials"], old["trials"])
    if "rejected" in name:
        assert int(new["trials"][0]) > 1, new["trials"]
    np.testing.assert_allclose(new["chi2"], old["chi2"], rtol=1e-9)
    for k in ("q", "t", "X"):
        assert _rel(new[k], old[k]) < 1e-9, k
