"""A naive sequential transcription of the reference's loops for the corner branch
(Frame.cc:548-642 with the point_state writes, :647-701, :756-793, :861-1037), in
pure Python: the cloud is walked arrival by arrival with the state the reference
keeps (halfPassed, point_state rewritten at every change of occupant, the fill_n
and the `continue` of the mask, the sorted (curvature, index) pairs walked from
the back, the FIFO queue, the eight-entry neighbour list with its two repeated
offsets, lineCountFlag, labelCount, num_largest_picked and its break).

It shares with the definition (tests/lidar_corner_ref.py) only functions of one
point or of one pair of points: the ring, the azimuth branch expressions, the
squared differences and the edge angle. The flat branch the reference interleaves
per ring reads point_state only as != -3 and writes none of what is used here, so
it is left out. tests/test_lidar_corner_ref.py compares the two on every case:
that is the check of the definition's order-free rules."""
import math

import numpy as np

import lidar_corner_ref as CR
import lidar_feat_ref as R

f32, f64 = np.float32, np.float64
PI = math.pi
NEIGHBOR = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (0, -1), (0, 1))  # :930-938


def _sq(a, b, wb=None):
    with np.errstate(all="ignore"):
        return R.sqdiff(a, b) if wb is None else R.sqdiff(a, b, np.asarray(wb))


def process(xyz, P, CP, extrinsic=None):
    xyz = np.ascontiguousarray(xyz, f32).reshape(-1, 3)
    n = len(xyz)
    ring_all = R.rings(xyz) if n else np.zeros(0, np.int32)
    cloud = [i for i in range(n) if ring_all[i] >= 0]
    rows, cols_n = P.row_num, P.col_num
    point_state = [[-3] * cols_n for _ in range(rows)]
    index = [[-1] * cols_n for _ in range(rows)]
    laser_scans = [[] for _ in range(rows)]
    image_index = [[] for _ in range(rows)]
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
            ground = f64(xyz[i, 2]) < CP.ground_z_bound
            if point_state[row][col] == -3:
                point_state[row][col] = -1 if ground else 0
                index[row][col] = index_num[row]
                laser_scans[row].append(i)
                image_index[row].append(col)
                index_num[row] += 1
            else:
                k2 = index[row][col]
                if R.dist(xyz[i]) < R.dist(xyz[laser_scans[row][k2]]):
                    point_state[row][col] = -1 if ground else 0
                    laser_scans[row][k2] = i
    state0 = np.asarray(point_state, np.int32).reshape(rows, cols_n)
    scans = [xyz[np.asarray(s, np.int64)] if s else np.zeros((0, 3), f32) for s in laser_scans]
    enabled = CP.enabled()
    c, n_sub = P.num_curvature_regions_corner, P.num_scan_subregions
    width = max(P.num_curvature_regions_flat, c)
    st = dict(mask=[], curvature=[], sorted=[], reason=[])
    sharp, less, less_label, less_rc = [], [], [], []
    angle_cache = {}

    def angle(a, b):
        key = (a, b) if a < b else (b, a)  # the predicate is symmetric bit for bit (tested on its own)
        if key not in angle_cache:
            pa = scans[a[0]][index[a[0]][a[1]]]
            pb = scans[b[0]][index[b[0]][b[1]]]
            angle_cache[key] = CR.angle(pa[None], pb[None])[0]
        return angle_cache[key]

    label_count = 1
    first, cloud_size = 0, 0
    for i in range(rows):  # ExtractFeaturePoints
        scan, size = scans[i], len(scans[i])
        start_idx = cloud_size
        cloud_size += size
        end_idx = cloud_size - 1 if cloud_size > 0 else 0
        mask, curv = [0] * size, [f32(0)] * size
        srt, reason = [-1] * size, [0] * size
        if end_idx > start_idx + 2 * width and enabled[i]:
            for k in range(c, size - c):  # PrepareRing_corner
                pp, pc, pn = scan[k - 1], scan[k], scan[k + 1]
                diff_next2 = _sq(pc, pn)
                with np.errstate(all="ignore"):
                    if f64(diff_next2) > 0.1:
                        depth, dn = R.dist(pc), R.dist(pn)
                        if depth > dn:
                            if f64(R.sqrtf(_sq(pn, pc, dn / depth)) / dn) < 0.1:
                                for t in range(k - c, k + 1):
                                    mask[t] = 1
                                continue
                        elif f64(R.sqrtf(_sq(pc, pn, depth / dn)) / depth) < 0.1:
                            for t in range(k + 1, k + 1 + c):
                                mask[t] = 1
                            continue
                    diff_prev2 = _sq(pc, pp)
                    dis2 = f32(f32(f32(pc[0] * pc[0]) + f32(pc[1] * pc[1])) + f32(pc[2] * pc[2]))
                    if f64(diff_next2) > 0.0002 * f64(dis2) and f64(diff_prev2) > 0.0002 * f64(dis2):
                        mask[k] = 1
            for j in range(n_sub):
                sp = (c * (n_sub - j) + (size - c) * j) // n_sub
                ep = (c * (n_sub - 1 - j) + (size - c) * (j + 1)) // n_sub - 1
                if ep <= sp:
                    continue
                pairs = []
                for k in range(sp, ep + 1):  # PrepareSubregion_corner
                    nn = 2 * c
                    with np.errstate(all="ignore"):
                        d = [f32(-nn) * scan[k][q] for q in range(3)]
                        for jj in range(1, c + 1):
                            for q in range(3):
                                d[q] = f32(d[q] + f32(scan[k + jj][q] + scan[k - jj][q]))
                        cv = f32(f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2])) / f32(nn)
                    curv[k] = f32(cv)
                    pairs.append((float(cv), k))
                pairs.sort()
                for k, (_, idx) in enumerate(pairs):
                    srt[sp + k] = idx
                num, k = 0, len(pairs)
                while k > 0:
                    cv, idx = pairs[k - 1]
                    k -= 1
                    col = image_index[i][idx]
                    if point_state[i][col] == -1:
                        reason[idx] = CR.GROUND
                        continue
                    if not (mask[idx] == 0 and cv > CP.sharp_curv_th):
                        reason[idx] = CR.MASKED if mask[idx] != 0 else CR.CURVATURE
                        continue
                    if point_state[i][col] == 0:
                        line_flag = [False] * rows
                        queue = [(i, col)]
                        q_start = 0
                        while q_start < len(queue):
                            fx, fy = queue[q_start]
                            q_start += 1
                            point_state[fx][fy] = label_count
                            for dr, dc in NEIGHBOR:
                                tx, ty = fx + dr, fy + dc
                                if tx < 0 or tx >= rows:
                                    continue
                                if ty < 0:
                                    ty = cols_n - 1
                                if ty >= cols_n:
                                    ty = 0
                                if point_state[tx][ty] != 0:
                                    continue
                                if angle((fx, fy), (tx, ty)) > f32(1.0):
                                    queue.append((tx, ty))
                                    point_state[tx][ty] = label_count
                                    line_flag[tx] = True
                        if sum(line_flag) >= 3:
                            label_count += 1
                        else:
                            for qx, qy in queue:
                                point_state[qx][qy] = -2
                    if point_state[i][col] < 1:
                        reason[idx] = CR.UNSTABLE
                        continue
                    if num < CP.max_corner_less_sharp:
                        reason[idx] = CR.PICKED
                        less.append(scan[idx])
                        less_label.append(point_state[i][col])
                        less_rc.append((i, col))
                        if num < CP.max_corner_sharp:
                            sharp.append(scan[idx])
                        num += 1
                    else:
                        reason[idx] = CR.OVER_CAP
                    if num >= CP.max_corner_less_sharp:
                        break
                for _, idx in pairs[:k]:  # what the break never looks at
                    reason[idx] = CR.OVER_CAP
        for key, v in (("mask", mask), ("curvature", curv), ("sorted", srt), ("reason", reason)):
            st[key].append(v)
    cat = lambda L, dt: np.asarray([v for row in L for v in row], dt)
    cstate = dict(cell_state=np.asarray(point_state, np.int32).reshape(rows, cols_n), initial_state=state0,
                  mask=cat(st["mask"], np.uint8), curvature=cat(st["curvature"], f32), sorted=cat(st["sorted"], np.int32),
                  reason=cat(st["reason"], np.uint8))
    pts3 = lambda L: R.transform(extrinsic, np.asarray(L, f32).reshape(-1, 3))
    return dict(sharp_xyz=pts3(sharp), less_sharp_xyz=pts3(less), less_sharp_label=np.asarray(less_label, np.int32),
                less_sharp_rc=np.asarray(less_rc, np.int32).reshape(-1, 2), corner_state=cstate)
