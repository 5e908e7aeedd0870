"""What tests/test_gpu_first_trial_sharded.py runs on several ranks: the cases
of first_trial_cases / lidar_first_trial_cases it takes, their owner maps, and
the shard geometry (each rank's row range of the reduced camera system) as
upload_gather_table computes it. tests/test_lin_ref.py asserts on the CPU that
every (case, world) pair has the geometry it is there for.
"""
import functools

import numpy as np

import lidar_first_trial_cases as lidc
import lin_ref
from first_trial_cases import CASES as VISION
from sqrtlm.shard import range_owner, shard_by_owner

ALL_CASES = {**VISION, **lidc.CASES}
WORLDS = (2, 3)

# multi-rank over contiguous ranges (shard()), worlds 2 and 3
RANGE_CASES = ("mid_lam1e-3", "mid_lam1", "mid_lam1e3", "rows", "long_track", "stereo_half", "dups", "long_red",
               "cr_levels", "border", "fixed_robust", "fixed_plain", "lid_multi", "lid_border", "lid_rows",
               "lid_level_l1")
# run at user_lambda = 0 (lambda_0 through the summed pose diagonals), worlds 2
# and 3: name -> (base case, owner map). The largest diagonal entry must sit on
# a pose that more than one rank sees, or the all-reduce is not what decides
# lambda_0: with contiguous ranges that holds for mid_lam1 at both worlds, but
# at world 2 border's (pose 53) and stereo_half's (pose 9) are seen by rank 0
# alone, so these two run under the interleaved map (landmark index % world)
LAMBDA0 = {"lam0_mid_lam1": ("mid_lam1", "range"), "lam0_border": ("border", "interleaved"),
           "lam0_stereo_half": ("stereo_half", "interleaved")}
# degenerate owner maps, world 3: name -> base case
DEGENERATE = {"fixed_only_rank": "fixed_plain", "interleaved": "mid_lam1", "empty_rank": "mid_lam1"}
# no vision edge at the optimised level: every rank >= 1 holds nothing active
# there (that is what the case is for), so no two row ranges can overlap
LIDAR_ONLY = ("lid_level_l1",)


def base(name):
    """The case of first_trial_cases / lidar_first_trial_cases behind a run."""
    return LAMBDA0[name][0] if name in LAMBDA0 else DEGENERATE.get(name, name)


def level(name):
    return lidc.LEVEL.get(base(name), 0)


def user_lambda(name):
    return 0.0 if name in LAMBDA0 else ALL_CASES[base(name)][1]


def setup_env(name):
    return ALL_CASES[base(name)][2]


@functools.lru_cache(maxsize=None)
def problem(name):
    return ALL_CASES[base(name)][0]()


def fixed_only_landmarks(prob):
    """Landmarks seen by fixed cameras only."""
    fixed = prob.pose_fixed[prob.obs_pose] != 0
    n_free = np.bincount(prob.obs_pt[~fixed], minlength=prob.n_pt)
    n_fix = np.bincount(prob.obs_pt[fixed], minlength=prob.n_pt)
    return (n_free == 0) & (n_fix > 0)


def owner_map(name, world):
    """owner[n_pt] of the (case, world) pair."""
    prob = problem(name)
    if name == "fixed_only_rank":
        # rank 1: exactly the landmarks seen by fixed cameras only; the others
        # in two contiguous halves (by observations) on ranks 0 and 2
        assert world == 3
        fo = fixed_only_landmarks(prob)
        cnt = np.where(fo, 0, np.bincount(prob.obs_pt, minlength=prob.n_pt))
        half = np.cumsum(cnt) * 2 > cnt.sum()
        return np.where(fo, 1, np.where(half, 2, 0)).astype(np.int32)
    if name == "interleaved" or (name in LAMBDA0 and LAMBDA0[name][1] == "interleaved"):
        return (np.arange(prob.n_pt) % world).astype(np.int32)
    if name == "empty_rank":
        assert world == 3
        return (2 * range_owner(prob, 2)).astype(np.int32)
    return range_owner(prob, world)


def local_problem(name, world, rank):
    return shard_by_owner(problem(name), owner_map(name, world), rank)


def free_cameras(name):
    """Pose ids of the free cameras of the whole problem, hessianIndex order
    (the union over the ranks: what every rank indexes)."""
    prob, lv = problem(name), level(name)
    act = np.zeros(prob.n_pose, bool)
    act[prob.obs_pose[prob.obs_level == lv]] = True
    if prob.n_lid:
        act[prob.lid_pose[lin_ref.lidar_level(prob) == lv]] = True
    return np.nonzero(act & (prob.pose_fixed == 0))[0]


def row_range(name, world, rank):
    """[lo, hi) in free-camera indices: the cameras this rank's own active
    edges touch (rank 0: its LiDAR edges too); (0, 0) if none."""
    prob, lv = problem(name), level(name)
    loc = local_problem(name, world, rank)
    hidx = -np.ones(prob.n_pose, np.int64)
    free = free_cameras(name)
    hidx[free] = np.arange(free.size)
    h = hidx[loc.obs_pose[loc.obs_level == lv]]
    if loc.n_lid:
        h = np.concatenate([h, hidx[loc.lid_pose[lin_ref.lidar_level(loc) == lv]]])
    h = h[h >= 0]
    return (int(h.min()), int(h.max()) + 1) if h.size else (0, 0)


def overlapping_ranks(name, world):
    """Pairs of ranks whose row ranges intersect."""
    rng = [row_range(name, world, r) for r in range(world)]
    return [(a, b) for a in range(world) for b in range(a + 1, world)
            if max(rng[a][0], rng[b][0]) < min(rng[a][1], rng[b][1])]


def pairs():
    """Every (case, world) the GPU test runs on more than one rank."""
    return [(n, w) for w in WORLDS for n in RANGE_CASES + tuple(LAMBDA0)] + [(n, 3) for n in DEGENERATE]


def runs(world):
    """The run names of one world, in the order the rank processes take them."""
    return [n for n, w in pairs() if w == world]
