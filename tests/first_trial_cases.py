"""The problems of tests/test_gpu_first_trial.py: name -> (builder, lambda,
environment of the setup). All small (<= 60 keyframes, <= 4k landmarks).
tests/test_lin_ref.py checks on the CPU that the oracle accepts the first
trial of every one of them at its lambda: the first-trial tests run accepted
first trials only. The retrial after a rejected step and the second iteration
have their own cases (tests/retrial_cases.py) and tests
(tests/test_retrial_ref.py on the CPU, tests/test_gpu_retrial.py on the GPU).
"""
import numpy as np

from sqrtlm import synth
from sqrtlm.problem import HUBER_STEREO


def _mid():
    # tracks of 2..18 keyframes: windows of every width up to the cap, several
    # tile classes in one problem (the three-stream fork / join)
    return synth.make_problem(40, 1500, seed=7)


def _track(n_kf, n_lm, k_lo, k_hi, seed, **kw):
    return synth.make_problem(n_kf, n_lm, k_min=k_lo, k_max=k_hi, seed=seed, **kw)


def _dups():
    """Every 17th observation a second time, with another measurement of the
    same keypoint (g2o keeps parallel edges: HyperGraph::addEdge does not
    look for one between the same vertices)."""
    p = _track(30, 600, 6, 9, 23)
    sel = np.arange(0, p.n_obs, 17)
    uv2 = (p.obs_uv[sel] + np.array([0.25, -0.5])).astype(np.float32).astype(np.float64)
    cat = lambda a, b: np.concatenate([a, b])
    p.obs_pose, p.obs_pt = cat(p.obs_pose, p.obs_pose[sel]), cat(p.obs_pt, p.obs_pt[sel])
    p.obs_uv, p.obs_info = cat(p.obs_uv, uv2), cat(p.obs_info, p.obs_info[sel])
    p.obs_delta, p.obs_level = cat(p.obs_delta, p.obs_delta[sel]), cat(p.obs_level, p.obs_level[sel])
    p.validate()
    return p


def _stereo(frac):
    return synth.add_stereo(synth.make_problem(30, 1000, k_min=2, k_max=12, seed=31), frac, seed=31,
                            robust_delta=HUBER_STEREO)


CASES = {
    # lambda sweep (damp_factor into S)
    "mid_lam1e-3": (_mid, 1e-3, {}),
    "mid_lam1": (_mid, 1.0, {}),
    "mid_lam1e3": (_mid, 1e3, {}),
    # one tile class each: windows of cp free cameras, NT = ceil(6 cp / 16)
    "cls3": (lambda: _track(30, 600, 2, 4, 13), 1.0, {}),
    "cls4": (lambda: _track(30, 900, 8, 9, 14), 1.0, {}),
    "cls6": (lambda: _track(30, 900, 12, 14, 16), 1.0, {}),
    "cls8": (lambda: _track(36, 900, 18, 19, 18), 1.0, {}),
    "cls9": (lambda: _track(40, 900, 22, 23, 19), 1.0, {}),
    # tracks longer than 32 (no producer kernel) over 20 fixed + 24 free keyframes
    "long_track": (lambda: _track(44, 600, 30, 40, 21, n_fixed=20), 1.0, {}),
    # tracks over more than 24 free cameras: no tiles, the row kernel
    "rows": (lambda: _track(40, 500, 26, 30, 22), 1.0, {}),
    "stereo_half": (lambda: _stereo(0.5), 1.0, {}),
    "stereo_all": (lambda: _stereo(1.0), 1.0, {}),
    # the widest stereo tiles (stereo_half / stereo_all reach classes 3, 4 and 6 only):
    # the geometry of cls8 / cls9, every second observation stereo
    "stereo_cls8": (lambda: synth.add_stereo(_track(36, 900, 18, 19, 18), 0.5, seed=18, robust_delta=HUBER_STEREO),
                    1.0, {}),
    "stereo_cls9": (lambda: synth.add_stereo(_track(40, 900, 22, 23, 19), 0.5, seed=19, robust_delta=HUBER_STEREO),
                    1.0, {}),
    "dups": (_dups, 1.0, {}),
    # 5 free cameras, 125 tiles: every S block / g row sums > 24 partials
    "long_red": (lambda: _track(6, 2000, 6, 6, 24), 1.0, {}),
    # solver layouts
    "cr_levels": (lambda: synth.make_problem(28, 1400, pair_window=4, n_fixed=3, seed=128), 1.0,
                  {"SQLM_CR_B_MIN": "1"}),
    "border": (lambda: synth.make_problem(60, 3000, k_min=2, k_max=10, seed=11, loop=12, n_fixed=2), 1.0, {}),
    # Huber on / off with fixed cameras inside the windows
    "fixed_robust": (lambda: _track(24, 700, 2, 8, 26, n_fixed=3, robust=True), 1.0, {}),
    "fixed_plain": (lambda: _track(24, 700, 2, 8, 26, n_fixed=3, robust=False), 1.0, {}),
}
