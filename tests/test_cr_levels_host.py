"""The cyclic reduction's level arithmetic (cr_levels, csrc/sqlm_plan.h) on a CPU.

tools/cr_levels_check is a stand-alone host program (g++, no HIP, no
libsqrtlm.so). For p = 1 .. 600 superblocks and both numberings (first real
superblock at index 0 / at index 1) it runs the function launch_cr_core sizes
its launches with against a brute-force elimination: every superblock is
eliminated exactly once or is the top, an eliminated superblock's neighbours
are alive at its level, the level count is ceil(log2 p) / floor(log2 p), the
grids match the simulated counts, and in k_cr_back_all's block -> (h, I) map
every wait targets a lower workgroup id or the top.
"""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_level_arithmetic_against_simulated_elimination():
    tools = os.path.join(ROOT, "tools")
    subprocess.run(["make", "-s", "-C", tools, "cr_levels_check"], check=True)
    r = subprocess.run([os.path.join(tools, "cr_levels_check")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])["cr_levels_check"]
    assert res == {"cases": 1200, "failures": 0}
