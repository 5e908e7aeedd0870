"""Cloud fixtures of tests/test_gpu_lidar_sets.py and tests/test_gpu_lba_corner.py:
the small local window of tests/lidar_cases.py (6 keyframes, pose 0 fixed, about
200 landmarks) with the planar scene as flat clouds and a scene of line
segments as corner clouds. Keyframe 5 is the current one (200 flat and 200
corner queries); keyframes 1..3 carry three map clouds of 300 points per kind.
"""
import numpy as np

import lidar_cases as LC
from sqrtlm import lidar, synth

KFS = np.array([LC.LBA_CUR, 1, 2, 3], np.int32)
CORNER_WEIGHT = 30.0  # lidarConfig::corner_optimized_weight


def lba_corner_case(seed=5):
    prob = synth.make_problem(6, 200, pair_window=3, n_fixed=1, seed=seed, robust=True)
    counts = [200, 300, 300, 300]
    clouds = synth.make_lidar_clouds(prob.pose_q[KFS], prob.pose_t[KFS], KFS, n_points=counts, current=0, seed=seed,
                                     noise=0.02, extent=3.0, dist_sq_threshold=0.04)
    clouds.corner_xyz = synth.make_lidar_corner_clouds(prob.pose_q[KFS], prob.pose_t[KFS], n_points=counts,
                                                       seed=seed + 1, noise=0.05, extent=3.0)
    clouds.corner_weight = CORNER_WEIGHT
    clouds.__post_init__()
    return prob, clouds


def cloud_sets(clouds, pose_q, pose_t):
    """The [flat, corner] sets of Context.set_lidar_from_cloud_sets at the poses (q, t) of the BA problem."""
    Twc = [lidar.Twc_f32(pose_q[p], pose_t[p]) for p in clouds.pose_index]
    return clouds.cloud_sets(Twc)


def search_args(s):
    """A set as the arguments of lidar_ref.associate / Context.lidar_associate."""
    return dict(map_clouds=s["map_clouds"], map_Twc=s["map_Twc"], query_xyz=s["query_xyz"], query_Twc=s["query_Twc"],
                thr=s["dist_sq_threshold"])
