"""A naive sequential transcription of the reference's loops for the flat-point
path of Frame::lidarProcess (Frame.cc:473-642, :704-752, :797-831, :834-1239),
in pure Python: the clouds are walked arrival by arrival with the loop state the
reference keeps (halfPassed, point_state, index_num, the fill_n of the mask, the
sorted pairs, num_largest_picked and its break). It shares with the definition
(tests/lidar_feat_ref.py) only what is a function of one point or of one
candidate: the ring, the azimuth, the branch expressions and the plane fit.
tests/test_lidar_feat_ref.py compares the two: that is the check of the
definition's order-free rules."""
import math

import numpy as np

import lidar_feat_ref as R

f32, f64 = np.float32, np.float64
PI = math.pi


def _mask_rule(pc, pn):
    with np.errstate(all="ignore"):
        if f64(R.sqdiff(pc, pn)) > 0.1:
            depth, dn = R.dist(pc), R.dist(pn)
            if depth > dn:
                if f64(R.sqrtf(R.sqdiff(pn, pc, np.asarray(dn / depth))) / dn) < 0.1:
                    return 1
            elif f64(R.sqrtf(R.sqdiff(pc, pn, np.asarray(depth / dn))) / depth) < 0.1:
                return 2
    return 0


def process(xyz, P, extrinsic=None):
    xyz = np.ascontiguousarray(xyz, f32).reshape(-1, 3)
    n = len(xyz)
    ring_all = R.rings(xyz) if n else np.zeros(0, np.int32)
    cloud = [i for i in range(n) if ring_all[i] >= 0]  # removeNaNFromPointCloud, then CalculateRingAndTime
    rows, cols_n, ncr = P.row_num, P.col_num, P.num_curvature_regions_flat
    point_state = [[-3] * cols_n for _ in range(rows)]
    index = [[-1] * cols_n for _ in range(rows)]
    laser_scans = [[] for _ in range(rows)]   # the input index of every scan point
    image_index = [[] for _ in range(rows)]   # its column
    if cloud:  # PointToImage
        azis = -R.atan2f(xyz[cloud, 1], xyz[cloud, 0])
        start, end = R.oris(azis[0], azis[-1])
        index_num = [0] * rows
        half_passed = False
        for k, i in enumerate(cloud):
            azi = azis[k:k + 1]
            if not half_passed:
                a = R.unpassed(azi, start)[0]
                if f64(f32(a - start)) > PI:
                    half_passed = True
            else:
                a = R.passed(azi, end)[0]
            rel = f32(a - start)
            col = int(math.fmod(int(f64(rel) / (2.0 * PI) * cols_n) + cols_n, cols_n))
            row = int(ring_all[i])
            if col < 0 or col >= cols_n or row < 0 or row >= rows:
                continue
            if point_state[row][col] == -3:
                point_state[row][col] = 0
                index[row][col] = index_num[row]
                laser_scans[row].append(i)
                image_index[row].append(col)
                index_num[row] += 1
            else:
                k2 = index[row][col]
                if R.dist(xyz[i]) < R.dist(xyz[laser_scans[row][k2]]):
                    laser_scans[row][k2] = i
    scan_ranges, cloud_size = [], 0
    for r in range(rows):
        first = cloud_size
        cloud_size += len(laser_scans[r])
        scan_ranges.append((first, cloud_size - 1 if cloud_size > 0 else 0))
    img = np.asarray(index, np.int32).reshape(rows, cols_n)
    scans = [xyz[np.asarray(s, np.int64)] if s else np.zeros((0, 3), f32) for s in laser_scans]
    cols = [np.asarray(c, np.int32) for c in image_index]
    enabled = P.enabled()
    st = dict(mask=[], curvature=[], neighbours=[], sorted=[], reason=[])
    flat, flat_n, less, less_n, less_rc = [], [], [], [], []
    for r in range(rows):  # ExtractFeaturePoints
        scan, size = scans[r], len(scans[r])
        mask, curv, nbr = [0] * size, [f32(0)] * size, [0] * size
        srt, reason = [-1] * size, [0] * size
        start_idx, end_idx = scan_ranges[r]
        width = max(P.num_curvature_regions_flat, P.num_curvature_regions_corner)
        if end_idx > start_idx + 2 * width and enabled[r]:
            for i in range(ncr, size - ncr):  # PrepareRing_flat
                rule = _mask_rule(scan[i], scan[i + 1])
                if rule == 1:
                    for t in range(i - ncr, i + 1):
                        mask[t] = 1
                elif rule == 2:
                    for t in range(i + 1, i + 1 + ncr):
                        mask[t] = 1
            for j in range(P.num_scan_subregions):
                sp = (ncr * (P.num_scan_subregions - j) + (size - ncr) * j) // P.num_scan_subregions
                ep = (ncr * (P.num_scan_subregions - 1 - j) + (size - ncr) * (j + 1)) // P.num_scan_subregions - 1
                if ep <= sp:
                    continue
                pairs = []
                for i in range(sp, ep + 1):  # PrepareSubregion_flat
                    with np.errstate(all="ignore"):
                        q = 25.0 / f64(R.dist(scan[i])) + 0.5
                    num = int(q) + 1 if q < 1073741824.0 else ncr
                    if i < num or i + num >= size:
                        num = ncr
                    nn = 2 * num
                    d = [f32(-nn) * scan[i][k] for k in range(3)]
                    with np.errstate(all="ignore"):
                        for jj in range(1, num + 1):
                            for k in range(3):
                                d[k] = f32(d[k] + f32(scan[i + jj][k] + scan[i - jj][k]))
                        cv = f32(f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2])) / f32(nn)
                    curv[i], nbr[i] = f32(cv), num
                    pairs.append((float(cv), i))
                pairs.sort()
                for k, (_, idx) in enumerate(pairs):
                    srt[sp + k] = idx
                picked, k = 0, 0
                while k < len(pairs):
                    cv, idx = pairs[k]
                    k += 1
                    if mask[idx] != 0:
                        reason[idx] = R.MASKED
                        continue
                    if not cv < P.surf_curv_th:
                        reason[idx] = R.CURVATURE
                        continue
                    code, nrm = R.candidate(img, scans, cols, r, idx, P)
                    reason[idx] = code
                    if code != R.PICKED:
                        continue
                    if picked < P.max_surf_less_flat:
                        less.append(scan[idx])
                        less_n.append(nrm)
                        less_rc.append((r, cols[r][idx]))
                        if picked < P.max_surf_flat:
                            flat.append(scan[idx])
                            flat_n.append(nrm)
                        picked += 1
                    else:
                        reason[idx] = R.OVER_CAP
                    if picked >= P.max_surf_less_flat:
                        break
                for _, idx in pairs[k:]:  # what the break never looks at
                    reason[idx] = R.OVER_CAP
        for key, v in (("mask", mask), ("curvature", curv), ("neighbours", nbr), ("sorted", srt), ("reason", reason)):
            st[key].append(v)
    cat = lambda L, dt: np.asarray([v for row in L for v in row], dt)
    state = dict(ring=ring_all, scan_n=np.asarray([len(s) for s in laser_scans], np.int64),
                 scan_src=cat(laser_scans, np.int32), scan_col=cat(image_index, np.int32), image_index=img,
                 mask=cat(st["mask"], np.uint8), curvature=cat(st["curvature"], f32),
                 neighbours=cat(st["neighbours"], np.int32), sorted=cat(st["sorted"], np.int32),
                 reason=cat(st["reason"], np.uint8))
    pts3 = lambda L: R.transform(extrinsic, np.asarray(L, f32).reshape(-1, 3))
    return dict(flat_xyz=pts3(flat), flat_normal=pts3(flat_n), less_xyz=pts3(less), less_normal=pts3(less_n),
                less_rc=np.asarray(less_rc, np.int32).reshape(-1, 2), state=state)
