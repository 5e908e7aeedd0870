"""A/B: the same GBA on two library builds must give bitwise-equal results
(a kernel change that keeps every summation order). usage:
python scripts/ab_bits.py libsqrtlm_old.so[:VAR=V...] [scale] [--first-trial]
(the A side may carry environment settings, e.g. libsqrtlm.so:SQLM_TILE_PROD=0
compares the in-tree library against itself with that switch)
--first-trial also compares the small paths: one LM trial of every case of
tests/first_trial_cases.py at its lambda and environment (stereo, repeated
cameras, long tracks, the row kernel, every solver layout), the cases that run
on the producer / consumer tile kernel once more with SQLM_TILE_PROD=0."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FT_KEYS = ("g", "dx", "q", "t", "X", "chi")


def run(spec, scale, out, first_trial):
    lib, *var = spec.split(":") if spec else ("",)
    env = dict(os.environ, SQLM_LIB_PATH=os.path.join(ROOT, "sqrtlm-slam_amd", "sqrtlm", lib) if lib else "")
    if not lib:
        env.pop("SQLM_LIB_PATH")
    for v in var:
        k, _, x = v.partition("=")
        env[k] = x
    code = f"""
import os, sys; sys.path.insert(0, {os.path.join(ROOT, 'sqrtlm-slam_amd')!r})
import numpy as np
from sqrtlm import synth
from sqrtlm.optimizer import Context
for gen in ("band", "loop", "lba"):
    with Context(0) as c:
        if gen == "lba":  # config 2 through the three-pass local-BA schedule (small-problem paths)
            c.set_problem(synth.config2()); ran, tags, sts = c.local_ba(); st = sts[-1]
        else:
            p = synth.config4(seed=4, scale={scale}) if gen == "band" else synth.config4_loop(seed=4, scale={scale})
            c.set_problem(p); n, st = c.global_ba(5)
        q, t = c.poses()
        np.savez({out!r} + gen, q=q, t=t, X=c.points(), chi=np.array(st["trace_chi2"]))
if {first_trial!r}:
    sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})
    from first_trial_cases import CASES
    base = dict(os.environ)
    res = {{}}
    def trial(name, tag, extra):  # one trial of the case, as tests/test_gpu_first_trial.py runs it
        make, lam, env = CASES[name]
        os.environ.clear(); os.environ.update({{**base, **env, **extra}})
        with Context(0) as c:
            c.set_problem(make()); n, st = c.optimize(0, 1, user_lambda=lam)
            (g, dx), (q, t) = c.last_step(), c.poses()
            for k, v in dict(g=g, dx=dx, q=q, t=t, X=c.points(), chi=np.array(st["trace_chi2"])).items():
                res[tag + "__" + k] = v
            return c.exec_info()["tile_kernel"]
    for name in sorted(CASES):
        if trial(name, name, {{}}) == "tile_producer":
            trial(name, name + ":SQLM_TILE_PROD=0", {{"SQLM_TILE_PROD": "0"}})
    np.savez({out!r} + "ft", **res)
"""
    subprocess.run([sys.executable, "-c", code], env=env, check=True)


args = [a for a in sys.argv[1:] if a != "--first-trial"]
first_trial = "--first-trial" in sys.argv[1:]
scale = float(args[1]) if len(args) > 1 else 0.2
run(args[0], scale, "/tmp/ab_a_", first_trial)
run("", scale, "/tmp/ab_b_", first_trial)
for gen in ("band", "loop", "lba"):
    a, b = np.load(f"/tmp/ab_a_{gen}.npz"), np.load(f"/tmp/ab_b_{gen}.npz")
    same = all(np.array_equal(a[k], b[k]) for k in ("q", "t", "X", "chi"))
    print(gen, "bitwise equal" if same else f"DIFFER max dq {np.abs(a['q'] - b['q']).max():.3e} chi {a['chi'][-1]} {b['chi'][-1]}")
if first_trial:
    a, b = np.load("/tmp/ab_a_ft.npz"), np.load("/tmp/ab_b_ft.npz")
    tags = sorted({k.rsplit("__", 1)[0] for k in a.files} | {k.rsplit("__", 1)[0] for k in b.files})
    for tag in tags:
        if any(f"{tag}__{k}" not in x.files for x in (a, b) for k in FT_KEYS):
            print("first-trial", tag, "DIFFER: ran on one side only (another tile kernel)")
            continue
        diff = [k for k in FT_KEYS if not np.array_equal(a[f"{tag}__{k}"], b[f"{tag}__{k}"])]
        print("first-trial", tag, "bitwise equal" if not diff else
              "DIFFER in " + " ".join(diff) + f" max ddx {np.abs(a[tag + '__dx'] - b[tag + '__dx']).max():.3e}")
