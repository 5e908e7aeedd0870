"""The pose graphs of tests/test_eg_gpu_retrial.py: CASES, name -> (builder,
lambda_0, trials of iteration 1). All have 60 keyframes. Every one rejects at
least three trials from its initial state before it accepts one.
tests/test_eg_retrial_ref.py checks on the CPU that the oracle takes exactly
the recorded trials, that every one of those decisions has |rho| >= 1e-3 in
the longdouble reference, and that the reference of every trial whose numbers
are compared is as well conditioned as those of tests/eg_first_trial_cases.py
(b <= 1e-14, dx <= 1e-9).

A pose graph with the drift and the measurement noise of make_pose_graph
accepts every trial at any lambda (scanned on the CPU oracle), so the initial
estimates are thrown far off: kick() left-composes a rotation of about
`rot` rad and a translation of about `tr` m onto a fraction of the vertices.
The measurements stay consistent, so the system stays well conditioned; the
Gauss-Newton-like step at a small lambda_0 overshoots and is rejected until
lambda reaches about 1e-3 .. 1e-1. The builders below were picked from such a
scan; the figures (rho of each trial of iteration 1 | of iteration 2, in the
longdouble reference; an accepted rho above 0.847 leaves the factor
1 - (2 rho - 1)^3 of the next lambda under its cap of 2/3, so that lambda
shows rho itself):

    band          -11.9 -11.6 -9.98 -3.36 0.311                     | 0.905
    band_deep     -12.2 -12.2 -12.2 -12.2 -12.2 -11.2 -0.639 0.88   | 1.03
    border3       -4.58 -4.43 -3.64 -0.698 0.838                    | 0.922
    border3_deep  -2.13 -2.13 -2.13 -2.13 -2.12 -2.09 -1.04 0.927   | 0.888
    border5       -0.645 -0.612 -0.44 0.262                         | 0.873
    info          -4.78 -4.66 -4.03 -1.21 0.822                     | 0.896
    mixed         -2.43 -2.43 -2.42 -2.28 -1.04 0.00697             | -0.192 -0.128 0.0659
    free_scale    -3.23 -3.18 -2.88 -1.18 0.832                     | -0.463 0.187

g2o's rejection rule is ``lambda *= ni; ni *= 2`` from ni = 2, so trial k
(0-based) of an iteration that started at lambda runs at
lambda 2^(k (k + 1) / 2): retrial_cases.lambda_at().

TWO_ITER: name -> (trials of iteration 1, trials of iteration 2) of
eg_optimize(2, lambda_0); both iterations end in an accepted trial.

EXHAUSTED: name -> (builder, lambda_0, whether the tenth trial is accepted):
started at 1e-16, the tenth trial runs at 2^45 1e-16 = 3.5e-3, which
border3_deep's graph still rejects (rho -0.675: nothing is accepted, the
iteration gives up) and border3's accepts (rho 0.89: accepted, and given up
all the same, levenberg.cpp:147-151).

EXPECT: graph -> exec info of the default layout, as in
eg_first_trial_cases.EXPECT.
"""
import numpy as np

import eg_first_trial_cases as ftc
from retrial_cases import lambda_at  # noqa: F401  (part of this module's interface)
from sqrtlm import synth

KICK_SEED = 5


def kick(pg, frac, rot, tr, seed=KICK_SEED):
    """A copy of pg with [quat(so3_exp(w)), t, 1], w ~ N(0, rot) per axis and
    t ~ N(0, tr), composed from the left onto S_iw of the vertices other than 0
    picked with probability frac."""
    rng = np.random.default_rng(seed)
    pick = rng.random(pg.n_kf) < frac
    pick[0] = False
    w = rng.normal(0.0, rot, (pg.n_kf, 3))
    t = rng.normal(0.0, tr, (pg.n_kf, 3))
    k = np.concatenate([synth.quat_from_mat(synth._so3_exp(w)), t, np.ones((pg.n_kf, 1))], axis=1)
    out = pg.copy()
    out.Siw[pick] = synth._sim3_compose(k[pick], pg.Siw[pick])
    return out


def state_graph(pg, Siw):
    """A copy of pg at another state: the linearization point of a later iteration."""
    out = pg.copy()
    out.Siw = np.ascontiguousarray(Siw, np.float64).reshape(-1, 8).copy()
    if out.Siw.shape != pg.Siw.shape:
        raise ValueError("state of another graph")
    return out


def _kicked(make, frac, seed=KICK_SEED):
    return lambda: kick(make(), frac, 1.5, 3.0, seed)


_BORDER3 = lambda: ftc._graph(60, 4, 3, 33)  # noqa: E731

_G = {
    # band only (no loop edge: border 0); band_deep starts it at 1e-10: seven rejections
    "band": _kicked(lambda: ftc._graph(60, 4, 0, 33), 0.3),
    # border of 2 vertices, R = 16; four rejections
    "border3": _kicked(_BORDER3, 0.3),
    # every vertex kicked, started at 1e-9: seven rejections
    "border3_deep": _kicked(_BORDER3, 1.0),
    # border of 4 vertices, R = 32
    "border5": _kicked(lambda: ftc._graph(60, 4, 5, 37), 0.3),
    # a seeded SPD information matrix per edge
    "info": _kicked(ftc._info, 0.3),
    # fixed interior vertices, reversed and duplicated edges; rejects twice inside iteration 2
    "mixed": _kicked(ftc._mixed, 0.5, 7),
    # free scale; rejects inside iteration 2
    "free_scale": _kicked(lambda: ftc._graph(60, 4, 3, 33, fix_scale=False), 1.0),
}

CASES = {
    "band": (_G["band"], 1e-6, 5),
    "band_deep": (_G["band"], 1e-10, 8),
    "border3": (_G["border3"], 1e-6, 5),
    "border3_deep": (_G["border3_deep"], 1e-9, 8),
    "border5": (_G["border5"], 1e-6, 4),
    "info": (_G["info"], 1e-6, 5),
    "mixed": (_G["mixed"], 1e-6, 6),
    "free_scale": (_G["free_scale"], 1e-6, 5),
}

TWO_ITER = {
    "band": (5, 1),
    "band_deep": (8, 1),
    "border3": (5, 1),
    "border3_deep": (8, 1),
    "border5": (4, 1),
    "info": (5, 1),
    "mixed": (6, 3),
    "free_scale": (5, 2),
}

EXHAUSTED = {
    "all_rejected": (_G["border3_deep"], 1e-16, False),
    "tenth_accepted": (_G["border3"], 1e-16, True),
}

# case -> its graph's key in EXPECT
GRAPH_OF = {"band": "band", "band_deep": "band", "border3": "border3", "border3_deep": "border3", "border5": "border5",
            "info": "info", "mixed": "mixed", "free_scale": "free_scale", "all_rejected": "border3",
            "tenth_accepted": "border3"}

EXPECT = {
    "band": dict(solve="cr", p=4, border=0, nc=112, R=16, n_last=0, info=False),
    "border3": dict(solve="cr", p=4, border=2, nc=112, R=16, n_last=16, info=False),
    "border5": dict(solve="cr", p=4, border=4, nc=112, R=32, n_last=32, info=False),
    "info": dict(solve="cr", p=4, border=2, nc=112, R=16, n_last=16, info=True),
    "mixed": dict(solve="cr", p=4, border=2, nc=112, R=16, n_last=16, info=False),
    "free_scale": dict(solve="cr", p=4, border=2, nc=112, R=16, n_last=16, info=False),
}
