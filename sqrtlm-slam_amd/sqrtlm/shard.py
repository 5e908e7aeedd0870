"""Landmark sharding for multi-GPU global BA.

Every rank holds all poses and a subset of the landmarks with their
observations. `shard` gives every rank one contiguous range: landmarks are in
trajectory order (sorted by first observing keyframe, as `synth.config4` and
the reference's point ids produce them), so a contiguous range touches a
contiguous band of cameras. Ranges are balanced by observation count, the unit
of the linearisation / RCS work. `shard_by_owner` takes any assignment of
landmarks to ranks (a rank may own none). LiDAR unary pose edges go to rank 0
only (the library ignores them elsewhere as well).
"""
from __future__ import annotations

import numpy as np

from .problem import BAProblem


def landmark_ranges(prob: BAProblem, world: int) -> list[tuple[int, int]]:
    """[lo, hi) landmark ranges, one per rank, balanced by observations."""
    if world <= 1:
        return [(0, prob.n_pt)]
    counts = np.bincount(prob.obs_pt, minlength=prob.n_pt)
    cum = np.cumsum(counts)
    targets = np.linspace(0, cum[-1], world + 1)[1:-1]
    cuts = [0] + [int(np.searchsorted(cum, t)) + 1 for t in targets] + [prob.n_pt]
    cuts = np.maximum.accumulate(np.minimum(cuts, prob.n_pt))
    return [(int(cuts[r]), int(cuts[r + 1])) for r in range(world)]


def range_owner(prob: BAProblem, world: int) -> np.ndarray:
    """The owner map of `shard`: owner[l] = the rank whose range holds landmark l."""
    owner = np.zeros(prob.n_pt, np.int32)
    for r, (lo, hi) in enumerate(landmark_ranges(prob, world)):
        owner[lo:hi] = r
    return owner


def shard_by_owner(prob: BAProblem, owner, rank: int) -> BAProblem:
    """The sub-problem of rank `rank` under the owner map `owner[n_pt]` (the
    rank of every landmark): all poses, its landmarks in their original order
    (re-indexed from 0), their observations in their original relative order,
    stereo arrays carried; the LiDAR edges, their kinds and
    ``meta["lid_level"]`` on rank 0 only."""
    owner = np.asarray(owner).reshape(-1)
    if owner.shape[0] != prob.n_pt:
        raise ValueError("owner needs one rank per landmark")
    mine = owner == rank
    new_id = np.cumsum(mine) - 1
    sel = mine[prob.obs_pt]
    lid, meta = {}, {}
    if rank == 0 and prob.n_lid:
        lid = dict(lid_pose=prob.lid_pose, lid_pc=prob.lid_pc, lid_pw=prob.lid_pw, lid_n=prob.lid_n,
                   lid_info=prob.lid_info, lid_kind=prob.lid_kind)
        if prob.meta.get("lid_level") is not None:
            meta = dict(lid_level=prob.meta["lid_level"])
    stereo = {}
    if prob.obs_ur is not None:
        stereo = dict(obs_ur=prob.obs_ur[sel], pose_bf=prob.pose_bf)
    return BAProblem(pose_q=prob.pose_q, pose_t=prob.pose_t, pose_fixed=prob.pose_fixed, intr=prob.intr,
                     pt=prob.pt[mine], obs_pose=prob.obs_pose[sel], obs_pt=new_id[prob.obs_pt[sel]],
                     obs_uv=prob.obs_uv[sel], obs_info=prob.obs_info[sel], obs_delta=prob.obs_delta[sel],
                     obs_level=prob.obs_level[sel], meta=meta, **lid, **stereo)


def shard(prob: BAProblem, rank: int, world: int) -> BAProblem:
    """The sub-problem rank `rank` optimises: all poses, its landmark range
    (re-indexed from 0), the observations of those landmarks in their original
    relative order."""
    if world <= 1:
        return prob
    return shard_by_owner(prob, range_owner(prob, world), rank)
