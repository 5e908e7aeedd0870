"""The problems of tests/test_gpu_first_trial_lidar.py: vision problems of
tests/first_trial_cases.py (or of their size) plus EdgeLidarFlatPoint unary
edges. name -> (builder, lambda, environment of the setup), the layout of
first_trial_cases.CASES, so the harness of tests/test_gpu_first_trial.py runs
them. All <= 60 keyframes, <= 3k landmarks. tests/test_lin_ref.py checks on
the CPU that the oracle accepts the first trial of every one at its lambda.

A problem's LiDAR levels (sqlm_set_lidar_level) travel in
``prob.meta["lid_level"]``; without the key every edge is at level 0. The
level a case optimises is LEVEL[name] (default 0).
"""
import numpy as np

from first_trial_cases import CASES as VISION
from sqrtlm import synth

# edges per pose of lid_multi: pose 0 is fixed (its 40 edges must be skipped),
# 1 / 63 / 64 / 65 sit at the 64-lane boundary of the camera pass's loop, 200
# takes four trips with a ragged tail; the free cameras between have none
MULTI = {0: 40, 5: 1, 9: 63, 14: 64, 20: 65, 29: 200}
BORDER = {59: 120, 30: 70}
ONLY_CAM = 29      # the keyframe of lid_only_cam that keeps LiDAR edges only


def add_lidar(prob, per_pose, shuffle_seed=None):
    """per_pose {pose: n}: n flat edges on each pose (its own seed each). With
    shuffle_seed the concatenated edges are permuted, so the caller's edge
    order is not grouped by pose and the device grouping is a real permutation."""
    prob.lid_pose = prob.lid_pose[:0]
    prob.lid_pc, prob.lid_pw, prob.lid_n = prob.lid_pc[:0], prob.lid_pw[:0], prob.lid_n[:0]
    prob.lid_info = prob.lid_info[:0]
    for pose, n in per_pose.items():
        synth.add_lidar_flat(prob, pose, n, seed=1000 + pose, append=True)
    if shuffle_seed is not None:
        o = np.argsort(synth.SplitMix64(shuffle_seed).uniform(prob.n_lid), kind="stable")
        for k in ("lid_pose", "lid_pc", "lid_pw", "lid_n", "lid_info"):
            setattr(prob, k, np.ascontiguousarray(getattr(prob, k)[o]))
        prob.validate()
    return prob


def _one():
    return add_lidar(synth.make_problem(30, 600, k_min=2, k_max=8, seed=41), {29: 150})


def _multi(per_pose=None):
    p = synth.make_problem(30, 600, k_min=2, k_max=8, seed=42, n_fixed=2)
    return add_lidar(p, MULTI if per_pose is None else per_pose, shuffle_seed=5)


def multi_without_fixed():
    """lid_multi without the 40 edges of the fixed pose 0, the others in the
    same relative order: must give the same bits."""
    p = _multi()
    keep = p.lid_pose != 0
    for k in ("lid_pose", "lid_pc", "lid_pw", "lid_n", "lid_info"):
        setattr(p, k, np.ascontiguousarray(getattr(p, k)[keep]))
    p.validate()
    return p


def _level():
    p = _multi()
    p.meta["lid_level"] = (np.arange(p.n_lid) % 2).astype(np.uint8)
    return p


def _only_cam():
    p = _one()
    p.obs_level = np.where(p.obs_pose == ONLY_CAM, 1, p.obs_level).astype(np.uint8)
    return p


CASES = {
    # one camera, three trips of the 64-lane loop, ragged tail (150 = 64 + 64 + 22)
    "lid_one": (_one, 1.0, {}),
    # lambda sweep on the problem with the smaller dx spread
    "lid_multi_lam1e-3": (_multi, 1e-3, {}),
    "lid_multi": (_multi, 1.0, {}),
    "lid_multi_lam1e3": (_multi, 1e3, {}),
    # every other LiDAR edge at level 1; optimised at level 0 and at level 1
    # (at level 1 no vision edge is active: LiDAR-only cameras, no landmark)
    "lid_level": (_level, 1.0, {}),
    "lid_level_l1": (_level, 1.0, {}),
    # k_camera_pass<true, true>
    "lid_stereo": (lambda: add_lidar(VISION["stereo_half"][0](), {29: 100}), 1.0, {}),
    # LiDAR diagonal blocks in a band+border layout
    "lid_border": (lambda: add_lidar(VISION["border"][0](), BORDER), 1.0, {}),
    # dense layout / row kernel
    "lid_rows": (lambda: add_lidar(VISION["rows"][0](), {39: 100}), 1.0, {}),
    # a free camera that is active through LiDAR alone
    "lid_only_cam": (_only_cam, 1.0, {}),
}
LEVEL = {"lid_level_l1": 1}
