"""The problems of tests/test_gpu_cr_levels.py: name -> (generator arguments,
environment, trial trace of the CPU oracle).

Tracks of 2..3 keyframes with SQLM_CR_B_MIN=1 keep B = 3 (n = 32), so
p = (keyframes - 1) / 3: powers of two and their neighbours, where the level
count of the two superblock numberings does and does not differ and the top
is / is not the last superblock. Tracks of 2..18 keyframes give B = 18
(n = 112): p = 23 (deep levels only) and p = 93 (47 odd superblocks: the first
level is wide, k_cr_aug<1> + k_cr_trsm, and its last superblock has no right
neighbour; the second level is not).
`p9_rejected_first_trial` starts with the points far off, no kernel and a
small lambda_0, as tests/retrial_cases.py builds its cases.

The trial traces are those of oracle.OracleGraph on the same problems;
tests/test_cr_levels_ref.py checks them on the CPU, so that a GPU run in
either numbering is compared on shapes whose accept / reject decisions the
reference takes the same way and with a wide margin.
"""
import numpy as np

from sqrtlm import synth


def _case(p, n=32, **kw):
    if n == 32:  # B = 3
        c = dict(n_kf=3 * p + 1, n_lm=40 * (3 * p + 1), k_max=3)
    else:  # B = 18, n = 112
        c = dict(n_kf=18 * p + 1, n_lm=10 * (18 * p + 1), k_max=18)
    c.update(seed=31 + p, robust=True, sigma=0.0, lam0=0.0, p=p, n=n)
    c.update(kw)
    return c


CASES = {f"p{p}": (_case(p), {}, [1, 1, 1, 1]) for p in (2, 3, 4, 5, 8, 9, 16, 17, 33)}
CASES["n112_p23"] = (_case(23, n=112), {}, [1, 1, 1, 1])
CASES["n112_p93_wide"] = (_case(93, n=112), {}, [1, 1, 1, 1])
CASES["p9_rejected_first_trial"] = (_case(9, robust=False, sigma=0.5, lam0=1e-8), {}, [8, 1, 1])
CASES["p9_no_spec"] = (_case(9), {"SQLM_NO_SPEC": "1"}, [1, 1, 1, 1])


def build(c):
    prob = synth.make_problem(c["n_kf"], c["n_lm"], k_min=2, k_max=c["k_max"], n_fixed=1, seed=c["seed"],
                              robust=c["robust"])
    if c["sigma"] > 0:  # points far off (tests/retrial_cases.py: noisy())
        prob.pt = np.ascontiguousarray(prob.pt + np.random.default_rng(5).normal(0.0, c["sigma"], prob.pt.shape))
        prob.validate()
    return prob


def levels(p, lo):
    """Elimination levels of p superblocks: ceil(log2 p) numbered from 0, floor(log2 p) from 1."""
    return (p - 1).bit_length() if lo == 0 else p.bit_length() - 1
