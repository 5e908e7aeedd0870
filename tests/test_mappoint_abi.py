"""The host side of sqlm_triangulate_pairs and sqlm_map_points_update without a
GPU: the kernels' shared text compiled for the CPU (the *_host twins) equals
the numpy definition bit for bit on every case, NaN for NaN; the Jacobi sweep
count; the halves of the refresh; argument errors."""
import ctypes as C

import numpy as np
import pytest

import mappoint_cases as MC
import mappoint_ref as R
from sqrtlm import mappoint as M
from sqrtlm._lib import lib, ptr

INVALID, UNSUPPORTED = -1, -8


@pytest.fixture(scope="module")
def host_tri():
    return M.triangulate_pairs_host(list(MC.tri_pairs().values()))


@pytest.mark.parametrize("name", MC.tri_names())
def test_triangulation_host_equals_the_definition_bit_for_bit(name, host_tri):
    names = list(MC.tri_pairs())
    k = names.index(name)
    lo, hi = int(host_tri["off"][k]), int(host_tri["off"][k + 1])
    s = MC.tri_slice(name)
    assert MC.same(host_tri["x3d"][lo:hi], s["x3d"])
    assert MC.same(host_tri["reason"][lo:hi], s["reason"])
    assert host_tri["n_new"][k] == s["n_new"][0]
    alone = M.triangulate_pairs_host([MC.tri_pairs()[name]])
    assert MC.same(alone["x3d"], s["x3d"]) and MC.same(alone["reason"], s["reason"])


def test_sweep_count_is_converged_with_two_to_spare():
    """The library's sweep count is two more than the count from which on every count gives the same stored
    bits on every match of the cases: two sweeps fewer already equal twice as many. One fewer than that does not
    (the rank-2 A of "zero_dist", where the sign of an exact zero still turns)."""
    pairs = list(MC.tri_pairs().values())
    lib_sw = M.triangulate_info()["sweeps"]
    assert lib_sw == R.SWEEPS
    a = M.triangulate_pairs_host(pairs, sweeps=lib_sw - 2)
    b = M.triangulate_pairs_host(pairs, sweeps=2 * lib_sw)
    c = M.triangulate_pairs_host(pairs)
    for k in ("x3d", "reason", "n_new"):
        assert MC.same(a[k], b[k]) and MC.same(a[k], c[k]), k
    few = M.triangulate_pairs_host(pairs, sweeps=lib_sw - 3)
    assert not MC.same(few["x3d"], b["x3d"])
    # every match of full rank is converged after three sweeps
    names = list(MC.tri_pairs())
    k = names.index("zero_dist")
    three = M.triangulate_pairs_host(pairs[:k] + pairs[k + 1:], sweeps=3)
    full = M.triangulate_pairs_host(pairs[:k] + pairs[k + 1:])
    assert MC.same(three["x3d"], full["x3d"]) and MC.same(three["reason"], full["reason"])


def test_refresh_host_equals_the_definition_and_its_halves_the_whole():
    b, r = MC.mp_batch(), MC.mp_reference()
    o = M.map_points_update_host(b)
    for k in ("best_idx", "best_median", "normal", "max_dist", "min_dist"):
        assert MC.same(o[k], r[k]), k
    d = M.map_points_update_host(b.halves(normal=False))
    n = M.map_points_update_host(b.halves(desc=False))
    assert set(d) == {"best_idx", "best_median"} and set(n) == {"normal", "max_dist", "min_dist"}
    for k in d:
        assert MC.same(d[k], r[k]), k
    for k in n:
        assert MC.same(n[k], r[k]), k
    # a point alone and the batch reversed
    for idx in ([3], list(range(b.n_pt))[::-1]):
        s = M.map_points_update_host(b.select(idx))
        for k in r:
            assert MC.same(s[k], r[k][idx]), (idx[:1], k)


def _tri_args(pairs):
    arr, off, m = M._pack_pairs(pairs)
    n = max(int(off[-1]), 1)
    return arr, off, m, np.zeros((n, 3), np.float32), np.zeros(n, np.uint8), np.zeros(len(pairs), np.int32)


def _tri_host(pairs, mutate=None, null=()):
    arr, off, m, x, r, nn = _tri_args(pairs)
    if mutate:
        mutate(arr, off, m)
    a = dict(pairs=arr, off=ptr(off), m=ptr(m), x=ptr(x), r=ptr(r), nn=ptr(nn))
    a.update({k: None for k in null})
    return lib().sqlm_triangulate_pairs_host(len(pairs), a["pairs"], a["off"], a["m"], 0, a["x"], a["r"], a["nn"])


def test_triangulation_argument_errors():
    L = lib()
    p = MC.tri_pairs()["n63"]
    assert _tri_host([p]) == 0
    assert _tri_host([]) == 0
    for k in ("pairs", "off", "m", "x", "r", "nn"):
        assert _tri_host([p], null=(k,)) == INVALID, k
    assert L.sqlm_triangulate_pairs_host(-1, None, None, None, 0, None, None, None) == INVALID
    assert L.sqlm_triangulate_pairs(None, 0, None, None, None, None, None, None) == INVALID
    assert L.sqlm_triangulate_info(None) == INVALID

    def set_m(i, j, v):
        return lambda arr, off, m: m.__setitem__((i, j), v)

    assert _tri_host([p], set_m(5, 0, -1)) == INVALID
    assert _tri_host([p], set_m(5, 0, p.kf1.N)) == INVALID
    assert _tri_host([p], set_m(62, 1, p.kf2.N)) == INVALID
    assert _tri_host([p], lambda arr, off, m: off.__setitem__(0, 1)) == INVALID
    assert _tri_host([p, p], lambda arr, off, m: off.__setitem__(1, 200)) == INVALID
    # an octave outside the keyframe's tables
    for bad in (-1, 8):
        q = M.TriPair(M.TriKeyFrame(p.kf1.mvKeysUn, p.kf1.mvScaleFactors, p.kf1.Tcw, *p.kf1.cam[:4]), p.kf2, p.matches)
        q.kf1.mvKeysUn["octave"][int(p.matches[7, 0])] = bad
        assert _tri_host([q]) == INVALID
    # negative sweeps
    arr, off, m, x, r, nn = _tri_args([p])
    assert L.sqlm_triangulate_pairs_host(1, arr, ptr(off), ptr(m), -1, ptr(x), ptr(r), ptr(nn)) == INVALID


def test_stereo_keypoints_are_refused():
    p = MC.tri_pairs()["n63"]
    ur = np.full(p.kf1.N, -1.0, np.float32)
    mono = M.TriPair(M.TriKeyFrame(p.kf1.mvKeysUn, p.kf1.mvScaleFactors, p.kf1.Tcw, *p.kf1.cam[:4], mvuRight=ur),
                     p.kf2, p.matches)
    o = M.triangulate_pairs_host([mono])     # mvuRight = -1 everywhere is this fork's monocular frame
    assert MC.same(o["x3d"], MC.tri_slice("n63")["x3d"])
    for side in (1, 2):
        ur = np.full(p.kf1.N, -1.0, np.float32)
        ur[int(p.matches[11, side - 1])] = 0.0
        kf = (p.kf1, p.kf2)[side - 1]
        st = M.TriKeyFrame(kf.mvKeysUn, kf.mvScaleFactors, kf.Tcw, *kf.cam[:4], mvuRight=ur)
        q = M.TriPair(st, p.kf2, p.matches) if side == 1 else M.TriPair(p.kf1, st, p.matches)
        assert _tri_host([q]) == UNSUPPORTED
        # an unmatched stereo keypoint is not read
        q.matches = np.delete(p.matches, 11, axis=0)
        assert _tri_host([q]) == 0


def test_refresh_argument_errors():
    L = lib()
    b = MC.mp_batch()
    n = b.n_pt
    out = [np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, 3), np.float32), np.zeros(n, np.float32),
           np.zeros(n, np.float32)]
    ins = [b.obs_off, b.obs_desc, b.obs_center, b.pos, b.ref_center, b.level_scale, b.max_scale]

    def call(ins, out, n=n):
        return L.sqlm_map_points_update_host(n, *[ptr(a) for a in ins], *[ptr(a) for a in out])

    assert call(ins, out) == 0
    assert call(ins, out, n=-1) == INVALID
    assert call([None] + ins[1:], out) == INVALID
    bad = b.obs_off.copy()
    bad[0] = 1
    assert call([bad] + ins[1:], out) == INVALID
    bad = b.obs_off.copy()
    bad[3] = bad[2] - 1
    assert call([bad] + ins[1:], out) == INVALID
    for i in range(3, 7):     # the normal half needs every per-point input
        assert call(ins[:i] + [None] + ins[i + 1:], out) == INVALID, i
    for i in range(2):
        assert call(ins, out[:i] + [None] + out[i + 1:]) == INVALID
        assert call(ins[:1] + [None] + ins[2:], out[:i] + [None] + out[i + 1:]) == 0   # descriptor half off
    for i in range(2, 5):
        assert call(ins, out[:i] + [None] + out[i + 1:]) == INVALID
    assert call(ins[:2] + [None] * 5, out[:2] + [None] * 3) == 0                        # normal half off
    assert L.sqlm_map_points_update(None, 0, ptr(b.obs_off), *[None] * 11) == INVALID
    assert L.sqlm_map_points_update_info(None, None) == INVALID
    assert call([np.zeros(1, np.int64)] + [None] * 6, [None] * 5, n=0) == 0
