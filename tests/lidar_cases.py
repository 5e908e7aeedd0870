"""Inputs of the LiDAR association tests (tests/lidar_ref.py is the reference):
seeded random clouds with random rigid float T_wc, the hand-built tie and
threshold cases, and the small local-BA window with a planar scene."""
import numpy as np

from sqrtlm import lidar, synth


def rigid_f32(rng):
    """A random rigid 4x4 float32 T_wc: rotation of up to pi about a random axis, translation within 5 m."""
    w = rng.normal(size=3)
    w *= rng.uniform(0.0, np.pi) / np.linalg.norm(w)
    T = np.eye(4)
    T[:3, :3] = synth._so3_exp(w[None])[0]
    T[:3, 3] = rng.uniform(-5.0, 5.0, 3)
    return T.astype(np.float32)


def random_case(sizes, n_query, *, seed=0, world=False, box=10.0, thr=1.5):
    """Clouds of ``sizes`` points uniform in a 2 box cube (sensor frame), each
    with a random T_wc (``world``: none, the clouds are in the world), and
    ``n_query`` queries with theirs. Returns the arguments of lidar_ref.associate."""
    rng = np.random.default_rng(seed)
    clouds = [rng.uniform(-box, box, (n, 3)).astype(np.float32) for n in sizes]
    Twc = None if world else np.stack([rigid_f32(rng) for _ in sizes])
    q = rng.uniform(-box, box, (n_query, 3)).astype(np.float32)
    return dict(map_clouds=clouds, map_Twc=Twc, query_xyz=q, query_Twc=rigid_f32(rng), thr=thr)


def tie_case(n_first, n_second, at_first, at_second, *, seed=3):
    """Two world clouds holding the same point (8, -3, 2.5), at index ``at_first``
    of the first and ``at_second`` of the second; the first queries sit on it
    and near it, so their nearest neighbour is that point twice at the same
    float distance. Returns (case, lower global index, the tied queries)."""
    rng = np.random.default_rng(seed)
    p = np.array([8.0, -3.0, 2.5], np.float32)
    a = rng.uniform(-6.0, 6.0, (n_first, 3)).astype(np.float32)
    b = rng.uniform(-6.0, 6.0, (n_second, 3)).astype(np.float32)
    a[at_first] = p
    b[at_second] = p
    q = rng.uniform(-6.0, 6.0, (70, 3)).astype(np.float32)
    q[0] = p
    q[1] = p + np.float32([0.125, 0.0, -0.25])
    q[2] = p + np.float32([0.0, 0.0625, 0.0])
    eye = np.eye(4, dtype=np.float32)
    return dict(map_clouds=[a, b], map_Twc=None, query_xyz=q, query_Twc=eye, thr=1.0), at_first, [0, 1, 2]


def threshold_case():
    """One world map point at the origin; axis-aligned power-of-two offsets make
    every float distance exact: query 0 is at exactly the threshold 0.3125
    (rejected: the test is strict), query 1 one step inside it, query 2 outside."""
    m = np.zeros((1, 3), np.float32)
    q = np.float32([[0.5, 0.25, 0.0], [0.5, 0.125, 0.0], [1.0, 0.0, 0.0]])
    return dict(map_clouds=[m], map_Twc=None, query_xyz=q, query_Twc=np.eye(4, dtype=np.float32), thr=0.3125)


LBA_CUR = 5  # the current keyframe of the window below (a free pose)


def lba_case(seed=5):
    """A small local window: 6 keyframes (pose 0 fixed), about 200 landmarks, and
    a planar scene seen from keyframes 1..5: keyframe 5 is the current one (200
    flat points), keyframes 1..4 carry the 4 x 300 map points. The scene is
    built from the problem's own (initial) poses."""
    prob = synth.make_problem(6, 200, pair_window=3, n_fixed=1, seed=seed, robust=True)
    kfs = np.array([5, 1, 2, 3, 4], np.int32)
    clouds = synth.make_lidar_clouds(prob.pose_q[kfs], prob.pose_t[kfs], kfs, n_points=[200, 300, 300, 300, 300],
                                     current=0, seed=seed, noise=0.02, extent=3.0, dist_sq_threshold=0.04)
    return prob, clouds


def lba_association_args(clouds, pose_q, pose_t):
    """The arguments of lidar_ref.associate for ``clouds`` at the poses (q, t) of the BA problem."""
    Twc = [lidar.Twc_f32(pose_q[p], pose_t[p]) for p in clouds.pose_index]
    oth = clouds.others
    return dict(map_clouds=[clouds.xyz[k] for k in oth], map_Twc=np.stack([Twc[k] for k in oth]),
                query_xyz=clouds.query_xyz, query_Twc=Twc[clouds.current], thr=clouds.dist_sq_threshold)
