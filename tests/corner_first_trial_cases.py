"""The problems of tests/test_gpu_first_trial_corner.py: the LiDAR windows of
tests/lidar_first_trial_cases.py (built with its add_lidar) with a kind per
edge, 0 EdgeLidarFlatPoint / 1 EdgeLidarCornerPoint. name -> (builder, lambda,
environment of the setup), the layout of lidar_first_trial_cases.CASES. A
synthetic flat pair has its map point ~0.3 m beside the current point on the
plane, so as a corner edge its error |T p_w - p_c| is a few decimetres: never
0, where the numeric Jacobian of the norm would be meaningless.

Kinds are assigned per camera in the caller's edge order after the shuffle:
that is the order the device keeps within a camera, so the 64-lane trips of
the camera pass see exactly the patterns named below.
"""
import numpy as np

import lidar_first_trial_cases as lidc
from first_trial_cases import CASES as VISION

# cor_mixed, per pose: the rule that gives edge j (caller order within the pose) its kind
MIXED = {
    29: lambda j: j >= 100,        # 100 flat then 100 corner: the kind flips inside the second 64-lane trip
    14: lambda j: j >= 0,          # 64 corner: one full trip
    20: lambda j: j % 2 == 1,      # 65 alternating: a divergent wave and a one-lane tail
    5: lambda j: j >= 0,           # one corner edge
    0: lambda j: j >= 0,           # the fixed pose: 40 corner edges, all skipped
    9: lambda j: j < 0,            # 63 flat: a flat-only camera among the mixed ones
}
ONLY_CAM = lidc.ONLY_CAM


def set_kinds(prob, rules):
    kind = np.zeros(prob.n_lid, np.uint8)
    for pose, rule in rules.items():
        e = np.nonzero(prob.lid_pose == pose)[0]
        kind[e] = [1 if rule(j) else 0 for j in range(e.size)]
    prob.lid_kind = kind
    prob.validate()
    return prob


def _one():
    p = lidc._one()
    p.lid_kind = np.ones(p.n_lid, np.uint8)
    p.validate()
    return p


def _mixed():
    return set_kinds(lidc._multi(), MIXED)


def mixed_without_fixed():
    """cor_mixed without the 40 edges of the fixed pose 0: must give the same bits."""
    p = _mixed()
    keep = p.lid_pose != 0
    for k in ("lid_kind", "lid_pose", "lid_pc", "lid_pw", "lid_n", "lid_info"):
        setattr(p, k, np.ascontiguousarray(getattr(p, k)[keep]))
    p.validate()
    return p


def _level():
    p = _mixed()
    p.meta["lid_level"] = (np.arange(p.n_lid) % 2).astype(np.uint8)
    return p


def _only_cam():
    p = lidc._only_cam()
    p.lid_kind = np.ones(p.n_lid, np.uint8)
    p.validate()
    return p


def _stereo():
    p = lidc.add_lidar(VISION["stereo_half"][0](), {29: 100})
    return set_kinds(p, {29: lambda j: j % 3 != 0})


CASES = {
    # one camera, corner edges only, three trips of the lane loop (150 = 64 + 64 + 22)
    "cor_one": (_one, 1.0, {}),
    "cor_mixed_lam1e-3": (_mixed, 1e-3, {}),
    "cor_mixed": (_mixed, 1.0, {}),
    "cor_mixed_lam1e3": (_mixed, 1e3, {}),
    # every other LiDAR edge at level 1; optimised at level 0 and at level 1
    "cor_level": (_level, 1.0, {}),
    "cor_level_l1": (_level, 1.0, {}),
    # a free camera that is active through corner edges alone
    "cor_only_cam": (_only_cam, 1.0, {}),
    # k_camera_pass<true, true>
    "cor_stereo": (_stereo, 1.0, {}),
}
LEVEL = {"cor_level_l1": 1}


def zero_kinds(prob):
    """The same problem with every edge flat: what a library that ignored the kinds would solve."""
    p = prob.copy()
    p.lid_kind = np.zeros(p.n_lid, np.uint8)
    p.validate()
    return p
