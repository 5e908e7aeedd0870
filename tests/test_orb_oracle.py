"""Pins of the ORB oracle (oracle/orb_ref.c) by independent restatements.

OpenCV is absent here and the reference ships no ORB fixtures, so the
OpenCV-implemented stages (resize, GaussianBlur, FAST) are parity UNPINNED
against the reference binary (oracle/orb_ref.h); they are pinned below by
their defining properties (FAST: the 9-of-16 arc definition and the score as
the largest threshold that keeps the corner; resize / blur: within one grey
level of the exact bilinear / Gaussian filter). The stages the reference
implements itself (IC_Angle, steered BRIEF, Hamming distance, quadtree,
SearchForInitialization) are checked against direct numpy / Python
transliterations of the reference source, and the whole extractor output is
frozen in tests/golden/orb/orb_golden.npz."""
import math
import os

import numpy as np
import pytest

from orb_translit import (_py_area, _py_bow_kf_frame, _py_bow_kf_kf, _py_fuse, _py_grid, _py_sbp_kf, _py_sbp_last,
                          _py_sbp_local, _py_sbp_sim3, _py_search_by_sim3, _py_search_for_init, _py_triangulation)
from sqrtlm import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "orb", "orb_golden.npz")
CIRCLE = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2),
          (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]


@pytest.fixture(scope="module")
def OB(oracle):
    from oracle import orb
    return orb


def test_level_geometry(OB):
    lw, lh, nf, sc = OB.levels(OB.params(), 1241, 376)
    assert list(lw) == [1241, 1034, 862, 718, 598, 499, 416, 346]
    assert list(lh) == [376, 313, 261, 218, 181, 151, 126, 105]
    assert nf.sum() == 2000 and list(nf[:3]) == [434, 362, 302]
    np.testing.assert_allclose(sc, 1.2 ** np.arange(8), rtol=1e-6)


def test_gauss_kernel(OB):
    k = OB.gauss_kernel()  # getGaussianKernel(7, 2) x 256: 18 34 49 55 49 34 18
    assert list(k) == [18, 34, 49, 55, 49, 34, 18]


def test_hamming_matches_popcount(OB):
    rng = np.random.default_rng(0)
    for _ in range(50):
        a, b = rng.integers(0, 256, (2, 32), dtype=np.uint8)
        assert OB.hamming(a, b) == int(np.unpackbits(a ^ b).sum())


def _brute_fast(img, th):
    """9-contiguous-of-16 definition; score = max over arcs of min |d| - 1."""
    h, w = img.shape
    I = img.astype(int)
    score = np.zeros((h, w), int)
    for y in range(3, h - 3):
        for x in range(3, w - 3):
            v = I[y, x]
            d = np.array([v - I[y + dy, x + dx] for dx, dy in CIRCLE])
            best = -1
            for s in range(16):
                arc = d[[(s + k) % 16 for k in range(9)]]
                best = max(best, arc.min() - 1, (-arc).min() - 1)
            if best >= th:
                score[y, x] = best
    return score


def test_fast_against_definition(OB):
    img, _ = synth.make_image_pair(90, 70, seed=2)
    for th in (7, 20):
        kps = OB.fast(img, th)
        score = _brute_fast(img, th)
        exp = []
        h, w = img.shape
        for y in range(3, h - 3):
            for x in range(3, w - 3):
                s = score[y, x]
                if s and all(s > score[y + dy, x + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx):
                    exp.append((x, y, s))
        got = [(int(k["x"]), int(k["y"]), int(k["response"])) for k in kps]
        assert got == exp and len(got) > 5


def test_resize_close_to_bilinear(OB):
    img, _ = synth.make_image_pair(300, 200, seed=3)
    out = OB.resize(img, 250, 167)
    sx, sy = 300 / 250, 200 / 167
    fx = (np.arange(250) + 0.5) * sx - 0.5
    fy = (np.arange(167) + 0.5) * sy - 0.5
    x0 = np.clip(np.floor(fx).astype(int), 0, 298)
    y0 = np.clip(np.floor(fy).astype(int), 0, 198)
    ax = np.clip(fx - x0, 0, 1)[None, :]
    ay = np.clip(fy - y0, 0, 1)[:, None]
    I = img.astype(float)
    ref = ((1 - ay) * ((1 - ax) * I[y0][:, x0] + ax * I[y0][:, x0 + 1]) +
           ay * ((1 - ax) * I[y0 + 1][:, x0] + ax * I[y0 + 1][:, x0 + 1]))
    assert np.abs(out.astype(float) - ref).max() <= 1.0


def test_blur_close_to_gaussian(OB):
    img, _ = synth.make_image_pair(120, 90, seed=4)
    out = OB.blur(img)
    x = np.arange(7) - 3.0
    g = np.exp(-x * x / 8.0)
    g /= g.sum()
    P = np.pad(img.astype(float), 3, mode="reflect")  # numpy "reflect" = BORDER_REFLECT_101
    R = sum(g[i] * P[:, i:i + 120] for i in range(7))
    ref = sum(g[i] * R[i:i + 90, :] for i in range(7))
    assert np.abs(out.astype(float) - ref).max() <= 2.5  # the x256 integer taps sum to 257
    # exactly the integer-tap filter, rounded to nearest (ties either way)
    ik = OB.gauss_kernel().astype(np.int64)
    Pi = np.pad(img.astype(np.int64), 3, mode="reflect")
    Ri = sum(ik[i] * Pi[:, i:i + 120] for i in range(7))
    N = sum(ik[i] * Ri[i:i + 90, :] for i in range(7))
    assert np.abs(out.astype(float) - np.minimum(N / 65536.0, 255.0)).max() <= 0.5


def _umax():
    import math
    umax = [0] * 16
    vmax = math.floor(15 * math.sqrt(2) / 2 + 1)
    vmin = math.ceil(15 * math.sqrt(2) / 2)
    for v in range(vmax + 1):
        umax[v] = int(np.rint(math.sqrt(225 - v * v)))
    v0 = 0
    for v in range(15, vmin - 1, -1):
        while umax[v0] == umax[v0 + 1]:
            v0 += 1
        umax[v] = v0
        v0 += 1
    return umax


def test_ic_angle_is_intensity_centroid(OB):
    img, _ = synth.make_image_pair(200, 120, seed=5)
    umax = _umax()
    I = img.astype(np.int64)
    for (x, y) in [(40, 40), (100, 60), (150, 80), (77, 33)]:
        m10 = m01 = 0
        for v in range(-15, 16):
            d = umax[abs(v)]
            for u in range(-d, d + 1):
                m10 += u * I[y + v, x + u]
                m01 += v * I[y + v, x + u]
        ang = OB.ic_angle(img, x, y)
        exact = np.degrees(np.arctan2(m01, m10)) % 360.0
        diff = abs((ang - exact + 180.0) % 360.0 - 180.0)
        assert diff < 0.02  # fastAtan2 polynomial accuracy


def test_fast_atan2_quadrants(OB):
    for y, x in [(1, 1), (1, -1), (-1, -1), (-1, 1), (0, 1), (1, 0), (3, 7), (-7, 3)]:
        ref = np.degrees(np.arctan2(y, x)) % 360.0
        assert abs((OB.fast_atan2(y, x) - ref + 180) % 360 - 180) < 0.02


def _pattern():
    import re
    txt = open(os.path.join(os.path.dirname(GOLDEN), "..", "..", "..", "oracle", "orb_pattern.h")).read()
    body = txt[txt.index("{") + 1:txt.index("};")]
    vals = [int(v) for v in re.findall(r"-?\d+", body)]
    assert len(vals) == 1024
    return vals


def test_descriptor_matches_steered_brief(OB):
    pattern = _pattern()
    img, _ = synth.make_image_pair(160, 120, seed=6)
    I = img.astype(int)
    for (x, y, ang) in [(50, 50, 0.0), (80, 60, 37.5), (100, 70, 211.25), (60, 40, 359.0)]:
        kp = np.zeros(1, OB.KP_DTYPE)
        kp["x"], kp["y"], kp["angle"] = x, y, ang
        d = OB.describe(img, kp)
        angle = np.float32(np.float32(ang) * np.float32(np.pi / 180.0))
        a, b = np.float32(np.cos(np.float64(angle))), np.float32(np.sin(np.float64(angle)))
        bits = []
        for i in range(256):
            x0, y0, x1, y1 = (np.float32(v) for v in pattern[4 * i:4 * i + 4])
            t0 = I[y + int(np.rint(x0 * b + y0 * a)), x + int(np.rint(x0 * a - y0 * b))]
            t1 = I[y + int(np.rint(x1 * b + y1 * a)), x + int(np.rint(x1 * a - y1 * b))]
            bits.append(int(t0 < t1))
        exp = np.packbits(np.array(bits, np.uint8).reshape(32, 8), axis=1, bitorder="little").ravel()
        np.testing.assert_array_equal(d, exp)


def test_distribute_invariants(OB):
    rng = np.random.default_rng(7)
    n = 3000
    keys = np.zeros(n, OB.KP_DTYPE)
    keys["x"] = rng.integers(0, 1209, n)
    keys["y"] = rng.integers(0, 344, n)
    keys["response"] = rng.integers(7, 120, n)
    for N in (50, 434, 2000):
        out = OB.distribute(keys, 16, 1225, 16, 360, N)
        assert N <= len(out) <= N + 3 * 64 or len(out) == n
        src = set(zip(keys["x"].tolist(), keys["y"].tolist(), keys["response"].tolist()))
        assert all((k["x"], k["y"], k["response"]) in src for k in out)
    out = OB.distribute(keys[:1], 16, 1225, 16, 360, 10)
    assert len(out) == 1
    assert len(OB.distribute(keys[:0], 16, 1225, 16, 360, 10)) == 0


@pytest.mark.parametrize("check_ori", [True, False])
def test_search_for_init_matches_transliteration(OB, check_ori):
    a, b = synth.make_image_pair(640, 300, seed=12, shift=(5.0, 2.0))
    p = OB.params(800)
    k1, d1 = OB.extract(p, a)
    k2, d2 = OB.extract(p, b)
    prev = np.ascontiguousarray(np.stack([k1["x"], k1["y"]], 1), np.float32)
    grid = (0.0, 640.0, 0.0, 300.0)
    n, m12, pr = OB.search_for_init(k1, d1, k2, d2, grid, prev, 100, 0.9, check_ori)
    n_py, m_py = _py_search_for_init(k1, d1, k2, d2, grid, prev, 100, 0.9, check_ori)
    assert n == n_py and n > 20
    np.testing.assert_array_equal(m12, m_py)
    ok = m12 >= 0
    np.testing.assert_array_equal(pr[ok, 0], k2["x"][m12[ok]])


def test_golden_extract_and_match(OB):
    g = np.load(GOLDEN)
    a, b = synth.make_image_pair(640, 300, seed=int(g["seed"]), shift=tuple(g["shift"]))
    p = OB.params(800)
    k1, d1 = OB.extract(p, a)
    k2, d2 = OB.extract(p, b)
    np.testing.assert_array_equal(np.asarray(a), g["img1"])
    for f in OB.KP_DTYPE.names:
        np.testing.assert_array_equal(k1[f], g["k1_" + f])
    np.testing.assert_array_equal(d1, g["d1"])
    np.testing.assert_array_equal(d2, g["d2"])
    prev = np.ascontiguousarray(np.stack([k1["x"], k1["y"]], 1), np.float32)
    n, m12, _ = OB.search_for_init(k1, d1, k2, d2, (0.0, 640.0, 0.0, 300.0), prev, 100, 0.9, True)
    assert n == int(g["n_matches"])
    np.testing.assert_array_equal(m12, g["m12"])


# ---- projection searches: the C oracle vs a second, pure-Python transliteration ----
@pytest.fixture(scope="module")
def proj_scene(OB):
    from sqrtlm import orb_scene as S
    a, b = synth.make_image_pair(640, 300, seed=21, shift=(6.0, -2.0))
    p = OB.params(800)
    k1, d1 = OB.extract(p, a)
    k2, d2 = OB.extract(p, b)
    return S, k1, d1, k2, d2, (0.0, 640.0, 0.0, 300.0)


def test_features_in_area_matches_transliteration(OB, proj_scene):
    S, k1, d1, k2, d2, bounds = proj_scene
    G = _py_grid(k2, bounds)
    rng = np.random.default_rng(3)
    for _ in range(60):
        x, y = rng.uniform(-20, 660), rng.uniform(-20, 320)
        r = float(rng.choice([2.5, 4.0, 7.2, 30.0]))
        lv = [(-1, -1), (0, -1), (2, -1), (-1, 0), (0, 3), (1, 1), (3, 5)][rng.integers(7)]
        got = OB.features_in_area(k2, bounds, x, y, r, *lv)
        assert list(got) == _py_area(G, k2, x, y, r, *lv)
    assert len(OB.features_in_area(k2, bounds, 320, 150, 40)) > 0


@pytest.mark.parametrize("stereo,th", [(False, 1.0), (True, 1.0), (True, 3.0)])
def test_search_by_projection_local_matches_transliteration(OB, proj_scene, stereo, th):
    S, k1, d1, k2, d2, bounds = proj_scene
    mps, md = S.local_points(k1, d1, (6.0, -2.0), seed=5, stereo=stereo)
    ur, sm, so = S.current_slots(k2, 5, stereo)
    sf = S.scale_factors()
    n, m, o = OB.search_by_projection_local(k2, d2, bounds, sf, ur, sm, so, mps, md, th, 0.8)
    n_py, m_py, o_py = _py_sbp_local(k2, d2, bounds, sf, ur, sm, so, mps, md, th, 0.8)
    assert n == n_py and n > 30
    np.testing.assert_array_equal(m, m_py)
    np.testing.assert_array_equal(o, o_py)


@pytest.mark.parametrize("stereo,mono,tz,th,check_ori", [(False, True, 0.0, 7.0, True), (True, False, 1.0, 7.0, True),
                                                         (True, False, -1.0, 15.0, False),
                                                         (True, False, 0.0, 7.0, True)])
def test_search_by_projection_last_matches_transliteration(OB, proj_scene, stereo, mono, tz, th, check_ori):
    S, k1, d1, k2, d2, bounds = proj_scene
    Tcw, Tlw, lp, ld = S.last_frame(k1, d1, (6.0, -2.0), 640, 300, seed=9, tz=tz)
    ur, sm, so = S.current_slots(k2, 9, stereo)
    sf, cam = S.scale_factors(), S.camera(640, 300)
    n, m, o = OB.search_by_projection_last(k2, d2, bounds, sf, cam, ur, sm, so, Tcw, Tlw, lp, ld, th, mono, check_ori)
    n_py, m_py, o_py = _py_sbp_last(k2, d2, bounds, sf, cam, ur, sm, so, Tcw, Tlw, lp, ld, th, mono, check_ori)
    assert n == n_py and n > 20
    np.testing.assert_array_equal(m, m_py)
    np.testing.assert_array_equal(o, o_py)


# ---- keyframe projection and BoW searches vs pure-Python transliterations ----
@pytest.fixture(scope="module")
def kf_scene(OB, proj_scene):
    S, k1, d1, k2, d2, bounds = proj_scene
    cam = S.camera(640, 300)
    mps, md = S.map_points(k1, d1, 640, 300, seed=2)
    return S, k1, d1, k2, d2, bounds, cam, mps, md


@pytest.mark.parametrize("s,th", [(1.0, 10), (1.3, 10), (0.8, 4)])
def test_search_by_projection_sim3_matches_transliteration(OB, kf_scene, s, th):
    S, k1, d1, k2, d2, bounds, cam, mps, md = kf_scene
    Scw = S.sim3_of(S.keyframe_pose((6.0, -2.0), 640, 300, (0.02, 0.0, 0.1)), s)
    _, sm, _ = S.current_slots(k2, 2, False)
    sf = S.scale_factors()
    n, m = OB.search_by_projection_sim3(k2, d2, bounds, sf, cam, sm, Scw, mps, md, th)
    n_py, m_py = _py_sbp_sim3(k2, d2, bounds, sf, cam, sm, Scw, mps, md, th)
    assert n == n_py and n > 20
    np.testing.assert_array_equal(m, m_py)


@pytest.mark.parametrize("sim3,stereo,th", [(False, False, 3.0), (False, True, 5.0), (True, False, 4.0)])
def test_fuse_matches_transliteration(OB, kf_scene, sim3, stereo, th):
    S, k1, d1, k2, d2, bounds, cam, mps, md = kf_scene
    T = S.keyframe_pose((6.0, -2.0), 640, 300, (0.0, 0.01, 0.05))
    if sim3:
        T = S.sim3_of(T, 1.2)
    ur, _, _ = S.current_slots(k2, 3, stereo)
    sf = S.scale_factors()
    n, idx = OB.fuse(k2, d2, bounds, sf, cam, ur, T, sim3, mps, md, th)
    n_py, idx_py = _py_fuse(k2, d2, bounds, sf, cam, ur, T, sim3, mps, md, th)
    assert n == n_py and n > 10
    np.testing.assert_array_equal(idx, idx_py)


@pytest.mark.parametrize("th,orb_dist,check_ori", [(10.0, 100, True), (3.0, 64, False)])
def test_search_by_projection_kf_matches_transliteration(OB, kf_scene, th, orb_dist, check_ori):
    S, k1, d1, k2, d2, bounds, cam, mps, md = kf_scene
    Tcw = S.keyframe_pose((6.0, -2.0), 640, 300, (0.01, 0.0, -0.1))
    _, sm, _ = S.current_slots(k2, 4, False)
    sf = S.scale_factors()
    n, m = OB.search_by_projection_kf(k2, d2, bounds, sf, cam, sm, Tcw, mps, md, k1["angle"], th, orb_dist,
                                      check_ori)
    n_py, m_py = _py_sbp_kf(k2, d2, bounds, sf, cam, sm, Tcw, mps, md, k1["angle"], th, orb_dist, check_ori)
    assert n == n_py and n > 20
    np.testing.assert_array_equal(m, m_py)


@pytest.mark.parametrize("check_ori", [True, False])
def test_search_by_bow_matches_transliteration(OB, proj_scene, check_ori):
    S, k1, d1, k2, d2, bounds = proj_scene
    n1, n2 = S.bow_nodes(d1, 1), S.bow_nodes(d2, 2)
    mp1, bad1 = S.bow_points(len(k1), 1)
    mp2, bad2 = S.bow_points(len(k2), 2, base=10000)
    a = (k1, d1, n1, mp1, bad1)
    n, out = OB.search_by_bow_kf_frame(a, (k2, d2, n2, mp2), 0.7, check_ori)
    n_py, out_py = _py_bow_kf_frame(a, (k2, d2, n2), 0.7, check_ori)
    assert n == n_py and n > 20
    np.testing.assert_array_equal(out, out_py)
    b = (k2, d2, n2, mp2, bad2)
    n, out = OB.search_by_bow_kf_kf(a, b, 0.75, check_ori)
    n_py, out_py = _py_bow_kf_kf(a, b, 0.75, check_ori)
    assert n == n_py and n > 20
    np.testing.assert_array_equal(out, out_py)


@pytest.mark.parametrize("stereo,only_stereo,check_ori", [(False, False, False), (True, False, True),
                                                          (True, True, False)])
def test_search_for_triangulation_matches_transliteration(OB, proj_scene, stereo, only_stereo, check_ori):
    S, k1, d1, k2, d2, bounds = proj_scene
    cam = S.camera(640, 300)
    T1 = S.keyframe_pose((0.0, 0.0), 640, 300)
    T2 = S.keyframe_pose((6.0, -2.0), 640, 300, (0.3, 0.0, 0.05))
    F12 = S.fundamental_12(T1, T2, cam, cam)
    n1, n2 = S.bow_nodes(d1, 5), S.bow_nodes(d2, 6)
    mp1, _ = S.bow_points(len(k1), 5, frac=0.3)
    mp2, _ = S.bow_points(len(k2), 6, frac=0.3)
    ur1, _, _ = S.current_slots(k1, 5, stereo)
    ur2, _, _ = S.current_slots(k2, 6, stereo)
    C1 = np.zeros(3, np.float32)
    a = (k1, d1, n1, mp1, None, ur1)
    b = (k2, d2, n2, mp2, None, ur2)
    sf = S.scale_factors()
    n, m12 = OB.search_for_triangulation(a, b, C1, T2, cam[:4], sf, F12, only_stereo, check_ori)
    n_py, m_py = _py_triangulation(a, b, C1, T2, cam[:4], sf, F12, only_stereo, check_ori)
    assert n == n_py and n > 5
    np.testing.assert_array_equal(m12, m_py)


@pytest.mark.parametrize("s12,th", [(1.0, 7.5), (1.03, 10.0)])
def test_search_by_sim3_matches_transliteration(OB, proj_scene, s12, th):
    S, k1, d1, k2, d2, bounds = proj_scene
    cam = S.camera(640, 300)
    T1, T2, mp1, md1, mp2, md2, R12, t12, m12 = S.sim3_scene(k1, d1, k2, d2, (6.0, -2.0), 640, 300, 3)
    sf = S.scale_factors()
    n, m = OB.search_by_sim3(k1, d1, k2, d2, bounds, sf, cam, T1, T2, mp1, md1, mp2, md2, s12, R12, t12, th, m12)
    n_py, m_py = _py_search_by_sim3(k1, d1, k2, d2, bounds, sf, cam, T1, T2, mp1, md1, mp2, md2, s12, R12, t12, th,
                                    m12)
    assert n == n_py and n > 20
    np.testing.assert_array_equal(m, m_py)
