"""sqlm_triangulate_pairs and sqlm_map_points_update on the GPU against the
numpy definition (tests/mappoint_ref.py) on the cases of
tests/mappoint_cases.py: everything the device stores is identical, NaN for
NaN; results do not depend on the batch (a case alone, in the full batch, in
the reversed batch, and after a larger call that grew the staging buffers);
each half of the refresh alone equals the combined call; both descriptor paths
ran; argument errors reach the caller before the device is touched."""
import numpy as np
import pytest

import mappoint_cases as MC
from sqrtlm import mappoint as M
from sqrtlm._lib import SqlmError

pytestmark = pytest.mark.gpu


def _check_tri(o, names):
    assert len(o["n_new"]) == len(names)
    for k, name in enumerate(names):
        lo, hi = int(o["off"][k]), int(o["off"][k + 1])
        s = MC.tri_slice(name)
        assert MC.same(o["x3d"][lo:hi], s["x3d"]), name
        assert MC.same(o["reason"][lo:hi], s["reason"]), name
        assert o["n_new"][k] == s["n_new"][0], name


def test_triangulation_full_batch_equals_the_definition(gpu_ctx):
    names = list(MC.tri_pairs())
    _check_tri(gpu_ctx.triangulate_pairs([MC.tri_pairs()[n] for n in names]), names)


def test_triangulation_does_not_depend_on_the_batch(gpu_ctx):
    pairs = MC.tri_pairs()
    names = list(pairs)
    # after a larger call: the staging buffers have grown and hold another call's data
    big = [M.make_two_view(700, seed=s) for s in (1, 2)]
    gpu_ctx.triangulate_pairs(big)
    for name in names:
        _check_tri(gpu_ctx.triangulate_pairs([pairs[name]]), [name])
    rev = names[::-1]
    _check_tri(gpu_ctx.triangulate_pairs([pairs[n] for n in rev]), rev)
    _check_tri(gpu_ctx.triangulate_pairs([pairs[n] for n in names]), names)


def test_create_new_map_points_mirror(gpu_ctx):
    p = MC.tri_pairs()["n65"]
    q = MC.tri_pairs()["reproj1"]
    created, nnew = M.CreateNewMapPoints(gpu_ctx, [p, q])
    assert nnew == 65 and len(created[0]) == 65 and created[1] == []
    for (i1, i2, X), m, want in zip(created[0], p.matches, MC.tri_slice("n65")["x3d"]):
        assert (i1, i2) == (int(m[0]), int(m[1])) and MC.same(X, want)


def _check_mp(o, idx, keys=("best_idx", "best_median", "normal", "max_dist", "min_dist")):
    r = MC.mp_reference()
    assert set(o) == set(keys)
    for k in keys:
        assert MC.same(o[k], r[k][idx]), k


def test_refresh_equals_the_definition_and_takes_both_descriptor_paths(gpu_ctx):
    b = MC.mp_batch()
    _check_mp(gpu_ctx.map_points_update(b), list(range(b.n_pt)))
    info = gpu_ctx.map_points_update_info()
    cnt = np.diff(b.obs_off)
    assert info["n_global"] == int((cnt > info["lds_max"]).sum()) == 1
    assert info["n_lds"] == b.n_pt - 1 and info["n_launch"] == 2


def test_refresh_halves_equal_the_combined_call(gpu_ctx):
    b = MC.mp_batch()
    idx = list(range(b.n_pt))
    _check_mp(gpu_ctx.map_points_update(b.halves(normal=False)), idx, ("best_idx", "best_median"))
    assert gpu_ctx.map_points_update_info()["n_launch"] == 1
    _check_mp(gpu_ctx.map_points_update(b.halves(desc=False)), idx, ("normal", "max_dist", "min_dist"))
    info = gpu_ctx.map_points_update_info()
    assert info["n_launch"] == 1 and info["n_lds"] == info["n_global"] == 0


def test_refresh_does_not_depend_on_the_batch(gpu_ctx):
    b = MC.mp_batch()
    gpu_ctx.map_points_update(M.make_tracks([40] * 300 + [300], seed=9))   # a larger call first
    for j in range(b.n_pt):
        _check_mp(gpu_ctx.map_points_update(b.select([j])), [j])
    rev = list(range(b.n_pt))[::-1]
    _check_mp(gpu_ctx.map_points_update(b.select(rev)), rev)
    _check_mp(gpu_ctx.map_points_update(b), list(range(b.n_pt)))


def test_update_map_points_mirror(gpu_ctx):
    b, r = MC.mp_batch(), MC.mp_reference()
    keep = np.full((b.n_pt, 32), 7, np.uint8)
    d, normal, mx, mn = M.UpdateMapPoints(gpu_ctx, b, keep)
    assert (d[0] == 7).all()    # no observation: mDescriptor stays
    for j in range(1, b.n_pt):
        assert (d[j] == b.obs_desc[b.obs_off[j] + r["best_idx"][j]]).all()
    assert MC.same(normal, r["normal"]) and MC.same(mx, r["max_dist"]) and MC.same(mn, r["min_dist"])


def test_argument_errors_and_empty_batches(gpu_ctx):
    p = MC.tri_pairs()["n63"]
    o = gpu_ctx.triangulate_pairs([])
    assert len(o["reason"]) == 0
    o = gpu_ctx.triangulate_pairs([MC.tri_pairs()["empty"]])
    assert o["n_new"].tolist() == [0]
    bad = M.TriPair(p.kf1, p.kf2, p.matches.copy())
    bad.matches[3, 1] = p.kf2.N
    with pytest.raises(SqlmError) as e:
        gpu_ctx.triangulate_pairs([p, bad])
    assert e.value.status == -1
    ur = np.full(p.kf2.N, -1.0, np.float32)
    ur[int(p.matches[0, 1])] = 12.5
    st = M.TriKeyFrame(p.kf2.mvKeysUn, p.kf2.mvScaleFactors, p.kf2.Tcw, *p.kf2.cam[:4], mvuRight=ur)
    with pytest.raises(SqlmError) as e:
        gpu_ctx.triangulate_pairs([M.TriPair(p.kf1, st, p.matches)])
    assert e.value.status == -8
    b = MC.mp_batch()
    assert gpu_ctx.map_points_update(b.select([])) is not None
    off = b.obs_off.copy()
    off[2] = off[1] - 1
    with pytest.raises(SqlmError):
        gpu_ctx.map_points_update(M.MapPointBatch(off, b.obs_desc, None))
