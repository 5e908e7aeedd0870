"""The BA setup planner (csrc/sqlm_plan.cpp) against naive references on a CPU.

tools/plan_check is a stand-alone host program (g++, no HIP, no libsqrtlm.so):
it builds its graphs itself, runs the planner's stages in prepare()'s order at
1, 3 and up to 16 host threads and checks every output -- active set, slot
order, scatter, buckets, update windows, tiles, S pattern, reduction lists,
solver plan -- against single-threaded brute-force versions. It prints one
"ok" line per graph and names the first failing check on stderr.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the paths of the planner each graph is there for
GRAPHS = ["smoke", "smoke-shuf", "border", "border-15", "dense", "two-runs", "levels-0", "levels-1", "tracks", "wide-70",
          "window-64", "window-65", "long-lists", "dup", "non-f32", "robust", "stereo", "empty", "big"]


def test_planner_against_naive_references():
    tools = os.path.join(ROOT, "tools")
    subprocess.run(["make", "-s", "-C", tools, "plan_check"], check=True)
    r = subprocess.run([os.path.join(tools, "plan_check")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.strip()]
    assert all(ln[0] == "ok" for ln in lines), r.stdout
    assert [ln[1] for ln in lines] == GRAPHS
    by = {ln[1]: ln for ln in lines}
    col = lambda name, key: by[name][by[name].index(key) + 1]
    # each graph took the path it was built for
    assert col("smoke", "solver") == "band" and col("border", "solver") == "border"
    assert col("border-15", "solver") == "border" and col("dense", "solver") == "dense"
    assert col("empty", "status") == "-7"  # SQLM_ERR_STATE: nothing to optimize
    assert col("dup", "dups") == "1" and col("non-f32", "f32") == "0"
    assert int(col("big", "nE")) >= 2 * 131072 and int(col("big", "threads").split("/")[0]) >= 1


def test_planner_on_a_shard_without_landmarks():
    """`plan_check shard`: one rank of a sharded run that owns no landmark
    (n_pt = n_obs = 0). Its free cameras come from the other ranks (prepare()
    ORs the ranks' active poses between the planner's first two stages); every
    edge list, bucket and tile list is empty and S is its diagonal."""
    tools = os.path.join(ROOT, "tools")
    subprocess.run(["make", "-s", "-C", tools, "plan_check"], check=True)
    r = subprocess.run([os.path.join(tools, "plan_check"), "shard"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.strip()]
    assert [ln[:2] for ln in lines] == [["ok", "empty-shard"]], r.stdout
    col = lambda key: lines[0][lines[0].index(key) + 1]
    assert col("status") == "0" and col("nP") == "9" and col("nL") == "0" and col("nE") == "0" and col("tiles") == "0"
