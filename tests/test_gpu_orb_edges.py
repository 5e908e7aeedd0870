"""The ORB kernels (sqlm_orb.hip) at the shapes the one KITTI frame pair of
tests/test_orb_gpu.py misses, against the CPU oracle (oracle/orb_ref.c) on the
inputs of tests/orb_edge_cases.py; tests/test_orb_edge_ref.py asserts, on the
oracle alone, that those inputs reach the paths named here. Every comparison
is bit-equality.

- k_area_list: grid cells of 64, 70 and 150 keypoints (one, two and three
  ballots of the 64-wide loop, the `run` offset between them, the write order
  of `pairs`), bounds that are non-zero and non-integer on all sides,
  keypoints outside the grid, windows beside the grid and over all of it,
  frames of 0, 1, 3 and 5 keypoints -- through all eleven ORBmatcher searches;
- k_orb_scan: 1, 3, 1023, 1024, 1025 and 2049 queries (chunk 1 -> 2 -> 3);
- k_cand_dist: BoW node runs of 1, 63, 64, 65, 128, 129 and 140 features;
- k_orb_bf: the 256-row tile boundary on either side, duplicates across it,
  every descriptor equal;
- sqlm_orb_extract: the smallest accepted image and the 4096-px limit (with
  the rejections beside them), 1, 3 and 12 levels, scale factors 2.0 and 1.1,
  nfeatures 0, 1 and 50000, a saturated 0 / 255 image, corners along every
  border, level widths of every residue mod 4, the ABI's `stride` and `cap`
  contracts, and one engine going through geometry A, B, A and A with other
  levels (the cached cell table).

Deliberately wrong scratch builds (nothing of them is committed), each run
against this file and against the unchanged tests/test_orb_gpu.py:

(a) k_area_list reads only the first 64 entries of a cell: 24 of the 70 tests
    here fail -- test_search_crowd for all 20 cases of the nine searches that
    go through the area search (every case of init, local, last, proj_sim3,
    fuse, fuse_sim3, proj_kf, sim3) and test_local_query_counts at 1023, 1024,
    1025 and 2049 queries. The BoW searches and SearchForTriangulation take no
    area list and pass, as do the tiny frames. tests/test_orb_gpu.py: all 37
    pass.
(b) area_search and k_area_list use 0 for min_x: 23 fail -- the same tests
    as under (a) except last-(True, False, 1.0, 7.0, True), whose 122 matches
    happen to survive the shifted grid. The tiny frames and the windows
    beside the grid still pass.
    tests/test_orb_gpu.py: all 37 pass (its bounds start at 0).
(c) extract uploads with pitch w in place of stride: the four
    test_extract_stride cases fail, nothing else. tests/test_orb_gpu.py: all
    37 pass (stride == w everywhere).

The product build passes all 70 tests here and all 37 of tests/test_orb_gpu.py.

Wall time of this file on an MI355X: 1.2 s for the 70 tests (pytest's total);
the slowest, test_extract_geometry_sequence with its four contexts, takes
0.13 s, the 4096 x 240 image 0.11 s.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import orb_edge_cases as E
from sqrtlm import synth

pytestmark = pytest.mark.gpu

KP_FIELDS = ("x", "y", "size", "angle", "response", "octave")


@pytest.fixture(scope="module")
def OB(oracle):
    from oracle import orb as OB
    return OB


def _same(got, ref, what):
    assert len(got) == len(ref), what
    assert got[0] == ref[0], (what, got[0], ref[0])
    for i, (a, b) in enumerate(zip(got[1:], ref[1:])):
        np.testing.assert_array_equal(a, b, err_msg=f"{what}: output {i}")


# ---- the eleven searches ---------------------------------------------------------------
@pytest.mark.parametrize("search,params", E.CASES, ids=[f"{s}-{p}" for s, p in E.CASES])
def test_search_crowd(gpu_ctx, OB, search, params):
    ref = E.run_oracle(OB, "crowd", search, params)
    assert ref[0] >= 30
    _same(E.run_gpu(gpu_ctx, "crowd", search, params), ref, f"{search} {params}")


@pytest.mark.parametrize("pair", E.TINY_PAIRS, ids=[f"{a}x{b}" for a, b in E.TINY_PAIRS])
def test_search_tiny(gpu_ctx, OB, pair):
    for search, params in E.CASES:
        _same(E.run_gpu(gpu_ctx, pair, search, params), E.run_oracle(OB, pair, search, params),
              f"{pair} {search} {params}")


@pytest.mark.parametrize("m", E.QUERY_COUNTS)
def test_local_query_counts(gpu_ctx, OB, m):
    from sqrtlm.orb import ORBmatcher
    F, Q = E.crowd(), E.local_queries(m)
    _, th, nnratio = E.LOCAL_Q_PARAMS
    n_r, m_r, o_r = OB.search_by_projection_local(F.k2, F.d2, F.bounds, E.SF, Q["ur"], Q["sm"], Q["so"], Q["mps"],
                                                  Q["md"], th, nnratio)
    G = E.gpu_frame(F, Q)
    n_g = ORBmatcher(nnratio, ctx=gpu_ctx).SearchByProjection(G, Q["mps"], Q["md"], th)
    assert n_g == n_r and n_r >= min(m, 100)
    np.testing.assert_array_equal(G.mvpMapPoints, m_r)
    np.testing.assert_array_equal(G.slot_obs, o_r)


@pytest.mark.parametrize("n2", [1, 3, 5])
def test_area_search_bounds(gpu_ctx, OB, n2):
    from sqrtlm.orb import ORBmatcher
    F = E.tiny(n2, n2)
    mps, md, th = E.area_bound_points(F)
    I = dict(ur=None, sm=np.full(n2, -1, np.int32), so=np.zeros(n2, np.uint8))
    lists = [OB.features_in_area(F.k2, F.bounds, p["proj_x"], p["proj_y"], 4.0 * th, -1, 0) for p in mps]
    assert [len(v) for v in lists] == [0, 0, 0, 0, n2, 0]
    n_r, m_r, o_r = OB.search_by_projection_local(F.k2, F.d2, F.bounds, E.SF, None, I["sm"], I["so"], mps, md, th, 0.9)
    G = E.gpu_frame(F, I)
    n_g = ORBmatcher(0.9, ctx=gpu_ctx).SearchByProjection(G, mps, md, th)
    assert n_g == n_r == 1  # the one window over the grid takes the keypoint whose descriptor it carries
    np.testing.assert_array_equal(G.mvpMapPoints, m_r)
    np.testing.assert_array_equal(G.slot_obs, o_r)


# ---- brute force ----------------------------------------------------------------------
@pytest.mark.parametrize("nq,nt,kind", E.BF_CASES)
def test_match_bf_sizes(gpu_ctx, nq, nt, kind):
    from sqrtlm.orb import ORBmatcher
    q, t, planted = E.bf_case(nq, nt, kind)
    bi, bd, bd2 = ORBmatcher(ctx=gpu_ctx).match_bf(q, t)
    D = np.unpackbits(q[:, None, :] ^ t[None, :, :], axis=2).sum(axis=2)
    np.testing.assert_array_equal(bd, D.min(axis=1))
    np.testing.assert_array_equal(bi, D.argmin(axis=1))
    second = np.sort(D, axis=1)[:, 1] if nt > 1 else np.full(nq, 2 ** 31 - 1)
    np.testing.assert_array_equal(bd2, second)
    for qi, a, b in planted:  # a tie: the first index wins, the second best is the same distance
        assert bi[qi] == a and bd[qi] == 0 and bd2[qi] == 0
    if kind == "equal":
        assert (bi == 0).all() and (bd == 0).all() and (bd2 == 0).all()


# ---- extractor ------------------------------------------------------------------------
def _extractor(ctx, prm):
    from sqrtlm.orb import ORBextractor
    return ORBextractor(*prm, ctx=ctx)


def _cmp_extract(got, ref, what):
    (kg, dg), (kr, dr) = got, ref
    assert len(kg) == len(kr), what
    for f in KP_FIELDS:
        np.testing.assert_array_equal(kg[f], kr[f], err_msg=f"{what}: {f}")
    np.testing.assert_array_equal(dg, dr, err_msg=what)


def _cmp_pyramid(got, ref, what):
    assert len(got) == len(ref), what
    for lvl, (a, b) in enumerate(zip(got, ref)):
        np.testing.assert_array_equal(a, b, err_msg=f"{what}: level {lvl}")


@functools.lru_cache(maxsize=None)
def _oracle_extract(name):
    from oracle import orb as OB
    kr, dr, pyr = OB.extract(OB.params(*E.EXTRACT_CASES[name][1]), E.extract_image(name), with_levels=True)
    return kr, dr, pyr


@pytest.mark.parametrize("name", list(E.EXTRACT_CASES))
def test_extract_cases(gpu_ctx, OB, name):
    prm = E.EXTRACT_CASES[name][1]
    kr, dr, pyr = _oracle_extract(name)
    ex = _extractor(gpu_ctx, prm)
    _cmp_extract(ex(E.extract_image(name)), (kr, dr), name)
    if prm[2] > 1:
        _cmp_pyramid(ex.image_pyramid(), pyr, name)
    assert len(kr) >= (400 if prm[0] >= 500 else 1)


def test_extract_smallest_and_largest(gpu_ctx, OB):
    from sqrtlm._lib import SqlmError
    w, h = E.min_size(OB)
    img, _ = synth.make_image_pair(w, h, seed=12)
    prm = (2000, 1.2, 8, 20, 7)
    ex = _extractor(gpu_ctx, prm)
    kr, dr, pyr = OB.extract(OB.params(*prm), img, with_levels=True)
    _cmp_extract(ex(img), (kr, dr), f"{w}x{h}")
    _cmp_pyramid(ex.image_pyramid(), pyr, f"{w}x{h}")
    assert len(kr) >= 20 and kr["octave"].max() == 7
    for bad in ((w - 1, h), (w, h - 1), (4097, 240), (240, 4097)):
        with pytest.raises(SqlmError):
            ex(np.zeros((bad[1], bad[0]), np.uint8))
    # the engine still serves the accepted size after the rejections
    _cmp_extract(ex(img), (kr, dr), f"{w}x{h} again")


@pytest.mark.parametrize("fill", [255, "noise"])
@pytest.mark.parametrize("pad", ["w+13", "64"])
def test_extract_stride(gpu_ctx, pad, fill):
    img = E.extract_image("synth643")
    h, w = img.shape
    stride = w + 13 if pad == "w+13" else (w + 63) // 64 * 64
    view = E.strided(img, stride, fill, seed=3)
    assert view.strides == (stride, 1) and not view.flags.c_contiguous and stride > w
    ex = _extractor(gpu_ctx, E.EXTRACT_CASES["synth643"][1])
    ref = ex(img)
    pyr = ex.image_pyramid()
    _cmp_extract(ex(view), ref, f"stride {stride}")
    _cmp_pyramid(ex.image_pyramid(), pyr, f"stride {stride}")
    assert len(ref[0]) > 1000


def test_extract_cap(gpu_ctx):
    """n_out > cap: n_out is the full count, the first cap entries are the full run's, nothing is written past cap."""
    from sqrtlm import _lib
    from sqrtlm.orb import KP_DTYPE, OrbParams
    img = E.extract_image("synth486")
    h, w = img.shape
    prm = OrbParams(*E.EXTRACT_CASES["synth486"][1])
    kf, df = _extractor(gpu_ctx, E.EXTRACT_CASES["synth486"][1])(img)
    n = len(kf)
    assert n > 1000
    for cap in (n - 1, 1):
        kps = np.full(n * KP_DTYPE.itemsize, 0xA5, np.uint8)
        desc = np.full((n, 32), 0xA5, np.uint8)
        n_out = C.c_int(-1)
        rc = _lib.lib().sqlm_orb_extract(gpu_ctx._h, C.byref(prm), _lib.ptr(img), w, h, w, _lib.ptr(kps),
                                         _lib.ptr(desc), cap, C.byref(n_out))
        assert rc == 0 and n_out.value == n
        np.testing.assert_array_equal(kps[:cap * KP_DTYPE.itemsize], kf[:cap].view(np.uint8))
        np.testing.assert_array_equal(desc[:cap], df[:cap])
        assert (kps[cap * KP_DTYPE.itemsize:] == 0xA5).all() and (desc[cap:] == 0xA5).all()


def test_extract_geometry_sequence(OB):
    """One engine through geometry A, B, A, A with 5 levels, A: every result equals a fresh context's."""
    from sqrtlm.optimizer import Context
    A, B = E.EXTRACT_CASES["synth643"][1], E.EXTRACT_CASES["synth486"][1]
    A5 = (A[0], A[1], 5, A[3], A[4])
    steps = [("synth643", A), ("synth486", B), ("synth643", A), ("synth643", A5), ("synth643", A)]

    def run(ctx, name, prm):
        ex = _extractor(ctx, prm)
        k, d = ex(E.extract_image(name))
        return k, d, ex.image_pyramid()

    fresh = {}
    for step in dict.fromkeys(steps):
        with Context(0) as ctx:
            fresh[step] = run(ctx, *step)
    with Context(0) as one:
        for i, step in enumerate(steps):
            k, d, pyr = run(one, *step)
            _cmp_extract((k, d), fresh[step][:2], f"step {i} {step}")
            _cmp_pyramid(pyr, fresh[step][2], f"step {i} {step}")
    # and the fresh results are the oracle's
    kr, dr, _ = _oracle_extract("synth643")
    _cmp_extract(fresh[steps[0]][:2], (kr, dr), "fresh A")
    kr, dr = OB.extract(OB.params(*A5), E.extract_image("synth643"))
    _cmp_extract(fresh[steps[3]][:2], (kr, dr), "fresh A, 5 levels")
