"""The numpy definition of the LiDAR flat-feature extraction
(tests/lidar_feat_ref.py) against a naive sequential transcription of the
reference's loops (tests/lidar_feat_naive.py) on the small cases: every stored
value is identical, which is the check of the order-free rules (halfPassed as a
minimum, the cell's occupant and index, the mask as an OR, the sort, the pick
without the break). The cases hit what they are built for. The restated atan /
atan2 stay within one ulp of numpy's."""
import numpy as np
import pytest

import lidar_feat_cases as LC
import lidar_feat_naive as N
import lidar_feat_ref as R


@pytest.mark.parametrize("name", LC.names(full=False))
def test_definition_equals_the_sequential_transcription(name):
    cloud, P, ext = LC.cases()[name]
    assert LC.differences(N.process(cloud, P, ext), LC.reference(name)) == []


def test_ring_limits():
    cloud, want = LC.ring_limit_points()
    assert np.array_equal(R.rings(cloud), want)
    assert np.array_equal(LC.reference("ring_limits")["state"]["ring"], want)


def _reasons(name):
    return np.bincount(LC.reference(name)["state"]["reason"], minlength=8)


def test_cases_hit_what_they_are_built_for():
    ref = LC.reference
    # filtering and empty sweeps
    assert (ref("non_finite")["state"]["ring"] == -1).sum() >= 2
    for n in ("empty", "dropped_only"):
        assert ref(n)["state"]["scan_n"].sum() == 0 and len(ref(n)["less_xyz"]) == 0
    full = ref("rows_above_row_num")["state"]
    assert (full["ring"] >= 6).any() and len(full["scan_n"]) == 6
    # collisions: fewer scan points than claiming points, and the occupant is not always the first arrival
    cloud, P, _ = LC.cases()["collisions"]
    st = ref("collisions")["state"]
    assert st["scan_n"].sum() < (st["ring"] >= 0).sum()
    # of the five late points only the nearest of the three in one cell became an occupant
    assert set(st["scan_src"][st["scan_src"] >= len(cloud) - 5].tolist()) == {len(cloud) - 2}
    # arrival order is not column order
    st = ref("shuffled")["state"]
    off = np.concatenate([[0], np.cumsum(st["scan_n"])])
    assert any(np.any(np.diff(st["scan_col"][off[r]:off[r + 1]]) < 0) for r in range(6))
    ev = st["reason"] >= R.FEW_SEARCH
    assert st["scan_col"][ev].min() == 0 and st["scan_col"][ev].max() == 95  # the gather meets both image edges
    # short rings: 10 and 11 scan points are skipped, 12 are not
    for m, n_cand in ((10, 0), (11, 0), (12, 2), (13, 3)):
        st = ref(f"short_ring_{m}")["state"]
        assert st["scan_n"][2] == m
        o = int(st["scan_n"][:2].sum())
        assert (st["reason"][o:o + m] != 0).sum() == n_cand, m
    st = ref("short_ring_24_sub8")["state"]
    o = int(st["scan_n"][:2].sum())
    assert 0 < (st["sorted"][o:o + 24] >= 0).sum() < 14  # some subregions of one point were skipped
    st = ref("corner_wider_than_flat")["state"]
    o = int(st["scan_n"][:2].sum())
    assert st["scan_n"][2] == 16 and not st["reason"][o:o + 16].any()  # 16 - 1 <= 2 * 7
    # region sizes, equal curvatures ordered by index, neighbourhoods wider than the default and the fallback
    for size in (63, 64, 65, 129):
        r = ref(f"region_{size}")
        st, o = r["state"], int(r["state"]["scan_n"][:6].sum())
        srt = st["sorted"][o:o + size + 10]
        assert np.array_equal(srt[5:size + 5], np.arange(5, size + 5)) and (srt[:5] == -1).all()
        assert not st["curvature"][o:o + size + 10].any() and len(r["less_xyz"]) == 6 and len(r["flat_xyz"]) == 2
        nb = st["neighbours"][o + 5:o + size + 5]
        assert nb.max() > 5 and nb[0] == 5 and nb[-1] == 5
    # both mask branches
    cloud, P, _ = LC.cases()["mask_both"]
    assert {1, 2} <= set(R.mask_rules(cloud[32:64], 5).tolist())
    assert _reasons("mask_both")[R.MASKED] > 0
    assert {1, 2} <= set(np.concatenate([R.mask_rules(s, 5) for s in
                                         R.image_of(*LC.cases()["start_0"][:2])[4]]).tolist())
    # fit rejections
    assert _reasons("few_search")[R.FEW_SEARCH] == 30
    for n in ("few_near", "collinear_zero_column", "collinear_proportional_columns"):
        assert _reasons(n)[R.DEGENERATE] == 30, n
    assert _reasons("outlier")[R.PLANE_INVALID] > 0 and _reasons("outlier")[R.PICKED] > 0
    # caps
    for k in (0, 1, 2, 3, 6, 7):
        for cf, cl in ((2, 6), (6, 6), (2, 2)):
            r = ref(f"caps_{k}valid_{cf}_{cl}")
            assert len(r["less_xyz"]) == min(k, cl) and len(r["flat_xyz"]) == min(k, cl, cf), (k, cf, cl)
            assert (_reasons(f"caps_{k}valid_{cf}_{cl}")[R.OVER_CAP] > 0) == (k >= cl)
    z = _reasons("caps_zero")
    assert z[R.PICKED] == 0 and z[R.OVER_CAP] > 0 and len(ref("caps_flat_zero")["flat_xyz"]) == 0
    assert len(ref("caps_flat_zero")["less_xyz"]) == 3
    # first and last ring, a moved start, the extrinsic, the full size
    for n in ("start_0", "start_100", "start_170", "start_m100_ring", "start_179_ring"):
        rc = ref(n)["less_rc"]
        assert {0, 5} <= set(rc[:, 0].tolist()), n
    e, b = ref("extrinsic"), R.process(*LC.cases()["extrinsic"][:2])
    assert len(e["less_xyz"]) > 50 and np.array_equal(e["less_rc"], b["less_rc"])
    assert not np.allclose(e["less_normal"], b["less_normal"])
    cloud, P, _ = LC.cases()["full_size"]
    assert 100000 < len(cloud) <= 130000 and (P.row_num, P.col_num) == (64, 1800)
    assert len(ref("full_size")["less_xyz"]) > 1000


def test_ring_enabled_follows_the_four_ranges():
    from sqrtlm import lidar_feat as LF
    e = LF.Params().enabled()
    assert e[4:50].all() and not e[:4].any() and not e[50:].any()
    # the fourth range is tested against its lower bound at both ends
    e = LF.Params(ring_x_rot=(1, 0), ring_y_rot=(1, 0), ring_z_trans=(1, 0), ring_z_rot_xy_trans=(7, 50)).enabled()
    assert e.sum() == 1 and e[6]


def _ulp_err(got, want):
    return np.max(np.abs(got - want) / np.spacing(np.abs(want)))


def test_restated_atan_and_atan2_stay_within_one_ulp_of_numpy():
    x = np.concatenate([np.linspace(-40.0, 40.0, 400001), np.logspace(-12, 12, 20001), -np.logspace(-12, 12, 20001),
                        [0.4375, 0.6875, 1.1875, 2.4375, 1.0]])
    err = _ulp_err(R.atan(x), np.arctan(x))
    print("atan: largest deviation from numpy %.3f ulp" % err)
    assert err <= 1.0
    rng = np.random.default_rng(1)
    th = np.concatenate([np.linspace(-np.pi, np.pi, 200001), rng.uniform(-np.pi, np.pi, 100000)])
    r = np.concatenate([np.ones(200001), 10.0 ** rng.uniform(-3, 3, 100000)])
    y, xx = r * np.sin(th), r * np.cos(th)
    err = _ulp_err(R.atan2(y, xx), np.arctan2(y, xx))
    print("atan2: largest deviation from numpy %.3f ulp" % err)
    assert err <= 1.0
    # the axes and the signed zeros
    ys = np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0, 2.0, -3.0])
    xs = np.array([1.0, 1.0, -1.0, -1.0, 0.0, 0.0, 1.0, 1.0])
    assert np.array_equal(R.atan2(ys, xs), np.arctan2(ys, xs))
    assert np.array_equal(np.signbit(R.atan2(ys, xs)), np.signbit(np.arctan2(ys, xs)))
