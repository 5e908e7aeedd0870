"""The problems of tests/test_gpu_retrial.py: name -> (builder, lambda_0,
environment of the setup, trials of iteration 1). All small (<= 60 keyframes,
<= 4k landmarks). Every one rejects at least one trial from its initial state
before it accepts one, started at a lambda_0 too small for that state.
tests/test_retrial_ref.py checks on the CPU that the oracle takes exactly the
recorded number of trials, that every one of them is decided with a margin no
rounding can cross, and that the reference of the accepted trial is as well
conditioned as those of tests/first_trial_cases.py.

Two ways to a rejected Gauss-Newton-like step, both found by scanning on the
CPU oracle:

* gross outliers without a robust kernel (``outlier_frac`` of the generator,
  ``robust=False``): the geometry stays sane, so the reduced system stays well
  conditioned; with Huber edges the same outliers reject much more rarely
  (the pair_window layout of cr_levels does);
* N(0, sigma) on the points (noisy()), sigma <= 1: larger noise rejects more
  readily, but puts points near the cameras and the float64-vs-longdouble
  spread of dx at 1e-3, no reference to compare with.

g2o's rejection rule is ``lambda *= ni; ni *= 2`` from ni = 2
(levenberg.cpp:142-145), so trial k (0-based) of an iteration that started at
lambda runs at lambda * 2^(k (k + 1) / 2): lambda_at().

TWO_ITER: the cases of the second-iteration tests, name -> (trials of
iteration 1, trials of iteration 2) of optimize(0, 2, lambda_0); both
iterations end in an accepted trial.
"""
import numpy as np

import lidar_first_trial_cases as lidc
from sqrtlm import synth

NOISE_SEED = 5


def lambda_at(lam0, k):
    """The damping of trial k (0-based) after k rejections from lam0: the
    products g2o forms, every factor a power of two (exact in float64)."""
    lam, ni = float(lam0), 2.0
    for _ in range(k):
        lam *= ni
        ni *= 2.0
    return lam


def noisy(make, sigma, robust=None):
    """Builder of make()'s problem with N(0, sigma) added to every point;
    robust=False drops the Huber kernels (constant weights)."""
    def build():
        p = make()
        p.pt = np.ascontiguousarray(p.pt + np.random.default_rng(NOISE_SEED).normal(0.0, sigma, p.pt.shape))
        if robust is False:
            p.obs_delta = np.zeros_like(p.obs_delta)
        p.validate()
        return p
    return build


def _mid(**kw):
    # tracks of 2..18 keyframes: several tile classes in one problem (the three-stream fork / join)
    return synth.make_problem(40, 1500, seed=7, **kw)


def _cr(**kw):
    # every landmark seen by two keyframes at most 4 apart: a narrow band, >= 3 cyclic-reduction levels
    return synth.make_problem(28, 1400, pair_window=4, n_fixed=3, seed=128, **kw)


def _border():
    return synth.make_problem(60, 3000, k_min=2, k_max=10, seed=11, loop=12, n_fixed=2, robust=False)


def _rows():
    # tracks of 2..30 keyframes: one over more than 24 free cameras sends the whole problem to the row kernel
    return synth.make_problem(40, 800, k_min=2, k_max=30, seed=22, robust=False, outlier_frac=0.4)


def _stereo():
    """Every observation a stereo edge, no kernel."""
    p = synth.make_problem(30, 1000, k_min=2, k_max=12, seed=31, robust=False, outlier_frac=0.4)
    return synth.add_stereo(p, 1.0, seed=31)


LIDAR = {39: 150, 12: 40}   # LiDAR edges per pose of lidar_plain (150 = 64 + 64 + 22 lanes)


def _lidar():
    return lidc.add_lidar(_mid(), LIDAR)


def state_problem(prob, pose_q, pose_t, pt):
    """A copy of prob at another state: the linearization point of a later iteration."""
    p = prob.copy()
    p.pose_q = np.ascontiguousarray(pose_q, np.float64).copy()
    p.pose_t = np.ascontiguousarray(pose_t, np.float64).copy()
    p.pt = np.ascontiguousarray(pt, np.float64).copy()
    p.validate()
    return p


_CR = {"SQLM_CR_B_MIN": "1"}

CASES = {
    # producer tiles, several tile classes (the three-stream fork / join), constant weights, 5 rejections
    "classes_plain": (lambda: _mid(robust=False, outlier_frac=0.4), 1e-4, {}, 6),
    # band solve with >= 3 cyclic-reduction levels: Huber (stored weights) with 6 and with 8 rejections,
    # and constant weights
    "cr_huber": (lambda: _cr(outlier_frac=0.2), 1e-6, _CR, 7),
    "cr_huber_deep": (lambda: _cr(outlier_frac=0.2), 1e-12, _CR, 9),
    "cr_plain": (lambda: _cr(robust=False, outlier_frac=0.05), 1e-2, _CR, 4),
    # band + border
    "border_plain": (noisy(_border, 0.1), 1e-2, {}, 4),
    # the row kernel, dense layout
    "rows_plain": (_rows, 1e-2, {}, 3),
    # stereo tiles
    "stereo_plain": (_stereo, 1e-10, {}, 9),
    # fixed cameras inside the windows
    "fixed_plain": (lambda: synth.make_problem(24, 700, k_min=2, k_max=8, seed=26, n_fixed=3, robust=False,
                                               outlier_frac=0.2), 0.1, {}, 3),
    # LiDAR flat-point edges at level 0 on two free cameras
    "lidar_plain": (noisy(_lidar, 1.0, False), 1e-4, {}, 3),
}

TWO_ITER = {
    "cr_huber": (7, 1),
    "cr_huber_deep": (9, 5),   # rejects inside iteration 2 as well
    "cr_plain": (4, 3),        # likewise
    "classes_plain": (6, 3),   # likewise
    "fixed_plain": (3, 3),     # likewise
    "stereo_plain": (9, 1),
    "border_plain": (4, 1),
}
