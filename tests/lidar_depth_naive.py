"""A naive sequential transcription of the reference's loops for the LiDAR
depth image and the keypoint depth association (Frame.cc:290-313, :333-408,
:1710-1723) in pure Python: the overwrite loop over the points, the two `break`
loops of min_v, the dx / dy scan with its strict `<` on sqrt values, the
push_back and the sort of depthrange. C++'s conversions are spelled out: int()
of a double truncates and gives INT_MIN where x86-64's cvttsd2si does, the uchar
read is that conversion's low byte. It shares nothing with the definition
(tests/lidar_depth_ref.py); tests/test_lidar_depth_ref.py compares the two:
that is the check of the definition's order-free rules.

One deliberate difference from the reference is kept here as in the
definition: a patch cell outside the image is skipped where the reference
reads out of bounds."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
INT_MIN = -2 ** 31


def c_int(q):
    """int(double) as gcc compiles it on x86-64."""
    q = float(q)
    if q != q or q in (math.inf, -math.inf) or not (-2147483649.0 < q < 2147483648.0):
        return INT_MIN
    return int(q)  # toward zero


def uchar(d):
    return c_int(d) & 255


def matmul34(a, b):
    M = [[0.0] * 4 for _ in range(3)]
    for r in range(3):
        for c in range(4):
            M[r][c] = ((a[r][0] * b[0][c] + a[r][1] * b[1][c]) + a[r][2] * b[2][c]) + a[r][3] * b[3][c]
    return M


def apply(row, P):
    with np.errstate(all="ignore"):
        return float(((f64(row[0]) * f64(P[0]) + f64(row[1]) * f64(P[1])) + f64(row[2]) * f64(P[2])) + f64(row[3]))


def divide(a, b):
    with np.errstate(all="ignore"):
        return float(f64(a) / f64(b))


def process(xyz, keys, rows, cols, intrinsic, extrinsic, keys_un=None, cam=None):
    xyz = np.ascontiguousarray(xyz, f32).reshape(-1, 3)
    keys = np.ascontiguousarray(keys, f32).reshape(-1, 2)
    K = np.asarray(intrinsic, f64).reshape(3, 4).tolist()
    E = np.asarray(extrinsic, f64).reshape(4, 4).tolist()
    M = matmul34(K, E)
    img = [[0.0] * cols for _ in range(rows)]             # Depthimg_, :290
    written = [[0] * cols for _ in range(rows)]
    pixel = [-1] * len(xyz)
    depthpixel_num = 0
    for i in range(len(xyz)):                             # :293
        x, y, z = xyz[i]
        if x < f32(1):                                    # :295
            continue
        P = (float(x), float(y), float(z))
        zP = [apply(M[r], P) for r in range(3)]           # :301
        u, v = c_int(divide(zP[0], zP[2])), c_int(divide(zP[1], zP[2]))  # :302
        if u >= 0 and v >= 0 and u <= cols - 1 and v <= rows - 1:        # :304
            if x > f32(1):                                # :308
                img[v][u] = apply(E[2], P)                # :309, overwriting
                written[v][u] = i + 1
                pixel[i] = v * cols + u
                depthpixel_num += 1
    min_v = 0                                             # :341-353
    for v in range(rows):
        break_flag = False
        for u in range(cols):
            if img[v][u] > 0:
                min_v = v
                break_flag = True
                break
        if break_flag:
            break
    m = len(keys)
    class_id, mv_depth, nearest = [0] * m, [f32(-1.0)] * m, [(-1, -1)] * m
    for i in range(m):                                    # :355
        ptx, pty = keys[i]
        with np.errstate(invalid="ignore"):
            is_below = bool(pty < f32(min_v))             # the int converts to float
        if is_below:
            class_id[i] = 0
            continue
        min_pixel_distance = 100000.0
        nearest_pixel = None
        exist_nearest = False
        depthrange = []
        for dx in range(-4, 4):
            for dy in range(-7, 7):
                with np.errstate(all="ignore"):
                    r, c = c_int(pty + f32(dy)), c_int(ptx + f32(dx))   # float add, then at<double>(int, int)
                if not (0 <= r < rows and 0 <= c < cols):
                    continue                              # the reference reads out of bounds here
                if uchar(img[r][c]) == 0:                 # :366-367
                    continue
                depth = img[r][c]
                depthrange.append(depth)
                pixel_distance = math.sqrt(dy * dy + dx * dx)
                if pixel_distance < min_pixel_distance:   # :373
                    min_pixel_distance = pixel_distance
                    exist_nearest = True
                    nearest_pixel = (c, r)
        if exist_nearest:
            depthrange.sort()
            nearest[i] = nearest_pixel
            if depthrange[-1] - depthrange[0] > 2:
                class_id[i] = 2
            else:
                class_id[i] = 1
                mv_depth[i] = f32(img[nearest_pixel[1]][nearest_pixel[0]])
        else:
            class_id[i] = 0
    existdepth = sum(1 for d in mv_depth if d > 0)        # :404-408
    occupied = sum(1 for row in written for w in row if w)
    out = dict(class_id=np.asarray(class_id, np.int32).reshape(m), depth=np.asarray(mv_depth, f32).reshape(m),
               nearest_uv=np.asarray(nearest, np.int32).reshape(m, 2),
               stats=np.array([min_v, depthpixel_num, occupied, existdepth], np.int32),
               image=np.asarray(img, f64).reshape(rows, cols), pixel=np.asarray(pixel, np.int32).reshape(len(xyz)),
               winner=np.asarray(written, np.int32).reshape(rows, cols))
    if keys_un is not None and cam is not None:           # UnprojectStereo, :1710-1723
        un = np.ascontiguousarray(keys_un, f32).reshape(-1, 2)
        fx, fy, cx, cy = (f32(c) for c in np.asarray(cam, f32))
        invfx, invfy = f32(1.0) / fx, f32(1.0) / fy
        pts = np.zeros((m, 3), f32)
        for i in range(m):
            zf = mv_depth[i]
            if zf > 0:
                with np.errstate(all="ignore"):
                    pts[i] = ((un[i, 0] - cx) * zf * invfx, (un[i, 1] - cy) * zf * invfy, zf)
        out["xyz_cam"] = pts
    return out
