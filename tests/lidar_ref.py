"""numpy reference of the LiDAR association (g2oOptimizer.cc:978-1073): every
float that decides a result is produced by IEEE operations in the order the
reference's libraries use, so the device result can be compared bit for bit.

* transform: pcl::transformPointCloud with an Eigen::Affine3d whose entries are
  the float entries of Twc: per coordinate (float)(((m0 x + m1 y) + m2 z) + m3)
  in float64;
* distance: FLANN L2_Simple<float>, d = query - map, ((dx dx) + dy dy) + dz dz in
  float32;
* search: exact minimum over the concatenated map, first occurrence (the lowest
  index) among equal distances;
* accept: (double)d2 < threshold, strict; pairs in query order.
"""
import numpy as np


def transform(xyz, Twc):
    """(n, 3) float32 sensor-frame points -> (n, 3) float32 world points."""
    p = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    M = np.asarray(Twc, np.float32).reshape(4, 4).astype(np.float64)
    out = np.empty((p.shape[0], 3), np.float32)
    for r in range(3):
        out[:, r] = (((M[r, 0] * p[:, 0] + M[r, 1] * p[:, 1]) + M[r, 2] * p[:, 2]) + M[r, 3]).astype(np.float32)
    return out


def world_map(map_clouds, map_Twc):
    """The concatenated world map: cloud order, then point order."""
    parts = []
    for k, c in enumerate(map_clouds):
        c = np.asarray(c, np.float32).reshape(-1, 3)
        parts.append(c.copy() if map_Twc is None else transform(c, map_Twc[k]))
    return np.concatenate(parts, axis=0) if parts else np.zeros((0, 3), np.float32)


def nearest(query_w, map_w, chunk=4096):
    """(nn_index int32, nn_sq_dist float32) of float32 world points; an empty
    map answers -1 / +inf."""
    q = np.asarray(query_w, np.float32).reshape(-1, 3)
    m = np.asarray(map_w, np.float32).reshape(-1, 3)
    n = q.shape[0]
    best_d = np.full(n, np.inf, np.float32)
    best_i = np.full(n, -1, np.int32)
    for b in range(0, m.shape[0], chunk):
        mm = m[b:b + chunk]
        dx = q[:, None, 0] - mm[None, :, 0]
        dy = q[:, None, 1] - mm[None, :, 1]
        dz = q[:, None, 2] - mm[None, :, 2]
        d2 = ((dx * dx) + dy * dy) + dz * dz
        assert d2.dtype == np.float32
        j = np.argmin(d2, axis=1)  # first occurrence = lowest index
        d = d2[np.arange(n), j]
        upd = d < best_d  # strict: an earlier chunk keeps an equal distance
        best_d[upd] = d[upd]
        best_i[upd] = (b + j[upd]).astype(np.int32)
    return best_i, best_d


def associate(map_clouds, map_Twc, query_xyz, query_Twc, thr):
    """dict(nn_index, nn_sq_dist, nn_xyz, accepted, n_pairs) as sqlm_lidar_associate returns them."""
    mw = world_map(map_clouds, map_Twc)
    qw = transform(query_xyz, query_Twc)
    idx, d2 = nearest(qw, mw)
    n = qw.shape[0]
    xyz = np.zeros((n, 3), np.float32)
    if mw.shape[0]:
        xyz[:] = mw[idx]
    acc = ((d2.astype(np.float64) < float(thr)) & (idx >= 0)).astype(np.uint8)
    return dict(nn_index=idx, nn_sq_dist=d2, nn_xyz=xyz, accepted=acc, n_pairs=int(acc.sum()), map_w=mw, query_w=qw)


def pairs(res, pose_index, query_xyz, query_normal, weight):
    """The EdgeLidarFlatPoint arrays of the accepted queries, in query order:
    (lid_pose, p_cam, p_world, normal, info) as sqlm_set_lidar takes them."""
    k = np.nonzero(res["accepted"])[0]
    q = np.asarray(query_xyz, np.float32).reshape(-1, 3)
    nm = np.asarray(query_normal, np.float32).reshape(-1, 3)
    return (np.full(k.size, pose_index, np.int32), q[k].astype(np.float64), res["nn_xyz"][k].astype(np.float64),
            nm[k].astype(np.float64), np.full(k.size, float(weight)))
