"""The order-free numpy definition of sqlm_lidar_depth (tests/lidar_depth_ref.py)
against the naive sequential transcription of the reference's loops
(tests/lidar_depth_naive.py) on every small case of tests/lidar_depth_cases.py,
every stored value identical; and what each case is there to show (its
``expect``) holds for the definition."""
import numpy as np
import pytest

import lidar_depth_cases as LC
import lidar_depth_naive as N
import lidar_depth_ref as R

STAT = {"min_v": 0, "n_written": 1, "n_occupied": 2, "n_with_depth": 3}


@pytest.mark.parametrize("name", LC.names(full=False))
def test_definition_equals_the_naive_transcription(name):
    c = LC.cases()[name]
    want = N.process(c.xyz, c.keys, c.cfg.rows, c.cfg.cols, c.cfg.intrinsic, c.cfg.extrinsic, c.keys_un, c.cfg.cam)
    assert LC.differences(LC.reference(name), want) == []


@pytest.mark.parametrize("name", [n for n in LC.names() if LC.cases()[n].expect])
def test_each_case_shows_what_it_is_there_for(name):
    got = LC.reference(name)
    for k, v in LC.cases()[name].expect.items():
        if k in STAT:
            assert got["stats"][STAT[k]] == v, k
        elif k == "depth":
            assert LC.same(got[k], np.asarray(v, np.float32)), k
        else:
            assert np.array_equal(got[k], np.asarray(v)), (k, got[k])


def test_the_uchar_rule_on_its_eight_depths():
    assert list(R.seen(LC.UCHAR_DEPTHS)) == LC.UCHAR_SEEN
    got, c = LC.reference("uchar"), LC.cases()["uchar"]
    # a seen return is the keypoint's depth, negative ones included; its camera point is zeros then
    dep = (c.xyz[:, 0].astype(np.float64) - 10.0).astype(np.float32)
    assert LC.same(got["depth"], np.where(LC.UCHAR_SEEN, dep, np.float32(-1.0)).astype(np.float32))
    assert got["depth"][7] < 0 and got["class_id"][7] == 1 and not got["xyz_cam"][7].any()
    assert got["xyz_cam"][1].all() and got["stats"][3] == 4
    # beyond int32, the infinities and NaN read as INT_MIN: unseen
    assert not R.seen([2.0 ** 31, -2.0 ** 31 - 1, np.inf, -np.inf, np.nan, 3e300]).any()
    assert R.seen([2.0 ** 31 - 1, -2.0 ** 31 + 1, 511.5, -255.0]).all() and not R.seen([512.9, -256.0, -0.99]).any()


def test_the_cases_cover_collisions_and_counts():
    for n in (63, 64, 65, 257, 4097):
        got = LC.reference(f"collide_{n}")
        assert got["stats"][1] == n and got["stats"][2] == 3
        w = got["winner"]
        last_b = n // 2 if (n // 2) % 2 else n // 2 - 1  # B takes the odd indices up to the middle
        assert (w[2, 3], w[9, 12], w[9, 13]) == (1, last_b + 1, n)  # the winner is the index plus one
    assert LC.reference("scattered_16")["stats"][1] > LC.reference("scattered_16")["stats"][2]
    assert sorted(len(LC.cases()[f"keys_{m}"].keys) for m in (0, 1, 63, 64, 65, 2049)) == [0, 1, 63, 64, 65, 2049]
    # every class occurs among the scattered keypoints
    assert set(LC.reference("keys_2049")["class_id"]) == {0, 1, 2}
    full = LC.reference("full_size")
    assert full["stats"][1] > 10000 and full["stats"][3] > 500 and set(full["class_id"]) == {0, 1, 2}


def test_product_matches_a_plain_matrix_product_closely():
    from sqrtlm import lidar_depth as LD
    M = R.product(LD.KITTI_INTRINSIC, LD.VELO_TO_CAM)
    assert np.allclose(M, LD.KITTI_INTRINSIC @ LD.VELO_TO_CAM, rtol=1e-15, atol=0)
