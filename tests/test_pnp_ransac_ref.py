"""What the cases of tests/pnp_ransac_cases.py are there for, asserted on the
numpy definition (tests/pnp_ransac_ref.py) alone: no library, no GPU."""
import numpy as np
import pytest

import pnp_ransac_cases as PC
import pnp_ransac_ref as R


def _refine_sizes(name):
    r = PC.reference(name)
    return {h: int(r["count"][h]) for h in r["refined"]}


def test_shapes_cover_the_kernel_paths():
    pairs = sorted({PC.case(n)["problem"].n_pair for n in PC.NAMES})
    assert {4, 15, 63, 64, 65, 129, 300} <= set(pairs)
    hyps = {PC.case(n)["n_hyp"] for n in PC.NAMES}
    assert {0, 1, 3, 4, 5, 300} <= hyps                      # a workgroup takes 4 hypotheses
    sizes = set()
    for n in PC.NAMES:
        sizes |= set(_refine_sizes(n).values())
    assert {4, 10, 63, 64, 65} <= sizes and max(sizes) >= 129
    assert PC.NAMES.index("n8_lt_min") not in (0, len(PC.NAMES) - 1)   # in the middle of the batch
    assert len({tuple(PC.case(n)["problem"].intr) for n in PC.NAMES}) == 2
    assert len(set(np.concatenate([PC.case(n)["problem"].sigma2 for n in PC.NAMES]).tolist())) == 8


def test_min_inliers_equal_to_n():
    c, r = PC.case("n4_h1_min_eq_n"), PC.reference("n4_h1_min_eq_n")
    assert c["min_inliers"] == c["problem"].n_pair == 4
    assert r["count"].tolist() == [4] and r["flags"].tolist() == [3]     # a record whose refine cannot exceed 4
    assert (r["first_return"], r["best"]) == (-1, 0)


def test_refine_on_exactly_ten_fails_the_strict_comparison():
    r = PC.reference("n15_h5_refine10")
    assert r["count"][3] == 10 and int(r["refined"][3]["count"][0]) == 10
    assert r["flags"].tolist() == [0, 0, 0, 3, 0] and r["first_return"] == -1 and r["best"] == 3
    assert r["count"][1] < 10                                            # the mismatch spoils hypothesis 1


@pytest.mark.parametrize("name,size", [("n63_h3_k2", 63), ("n64_h4", 64), ("n65_h5", 65)])
def test_refine_sizes_around_the_wavefront(name, size):
    r = PC.reference(name)
    h = r["first_return"]
    assert h >= 0 and r["count"][h] == size and int(r["refined"][h]["count"][0]) > PC.case(name)["min_inliers"]


def test_many_hypotheses_and_large_refines():
    r = PC.reference("n129_h300")
    assert (r["flags"] & 1).sum() > 10 and min(_refine_sizes("n129_h300").values()) > 64
    assert (r["count"] == 0).any() and r["first_return"] >= 0
    assert max(_refine_sizes("n300_h5").values()) >= 129
    assert np.isfinite(r["R"]).all()


def test_no_hypothesis_qualifies():
    r = PC.reference("n129_never")
    assert r["count"].max() >= 80 and r["count"].max() < PC.case("n129_never")["min_inliers"]
    assert not r["flags"].any() and (r["first_return"], r["best"]) == (-1, -1) and not r["refined"]
    assert PC.case("n8_lt_min")["n_hyp"] == 0 and PC.case("n8_lt_min")["problem"].n_pair < PC.case("n8_lt_min")["min_inliers"]


def test_coplanar_points_zero_the_third_row_of_the_inverse():
    r = PC.reference("n20_coplanar")
    assert (r["cci"][:, 2, :] == 0.0).all() and (r["cci"][:, :2, :] != 0.0).any()
    assert r["count"][0] == 20 and (r["refined"][0]["cci"][0, 2] == 0.0).all()
    # EPnP without a planar branch (the reference has none): the control point that spans nothing leaves three
    # more null vectors in M^T M, and the refine on all 20 coplanar pairs does not find the pose
    assert int(r["refined"][0]["count"][0]) <= PC.case("n20_coplanar")["min_inliers"] and r["flags"][0] == 3


def test_two_coinciding_points():
    c, r = PC.case("n20_same"), PC.reference("n20_same")
    p = c["problem"]
    assert r["idx"][0, :2].tolist() == [0, 1] and (p.Xw[0] == p.Xw[1]).all() and (p.uv[0] == p.uv[1]).all()
    assert r["count"][0] >= 0 and r["flags"][3] & 1                       # nothing faults; a later hypothesis is fine


def test_point_behind_the_camera():
    c, r = PC.case("n20_behind"), PC.reference("n20_behind")
    p = c["problem"]
    j = int(r["idx"][0, 0])
    depth = p.meta["Rcw"][2] @ p.Xw[j].astype(np.float64) + p.meta["tcw"][2]
    assert depth < 0
    assert r["count"][0] < c["min_inliers"] <= r["count"][1]      # solve_for_sign takes it for a point in front


def test_failed_refine_then_a_successful_one():
    r = PC.reference("n30_fail_then_ok")
    assert r["count"].tolist()[1:3] == [10, 20] and r["flags"].tolist() == [0, 3, 7, 0]
    assert int(r["refined"][1]["count"][0]) == 10 and int(r["refined"][2]["count"][0]) == 20
    assert (r["first_return"], r["best"]) == (2, 2)


def test_index_mapping_against_the_literal_vector():
    for n in (4, 5, 6):
        all_draws = [(a, b, c, d) for a in range(n) for b in range(n - 1) for c in range(n - 2) for d in range(n - 3)]
        got = R.indices(n, np.array(all_draws))
        for q, g in zip(all_draws, got):
            assert g.tolist() == R.indices_literal(n, q)


def test_max_its_below_five():
    c, r = PC.case("n20_its4"), PC.reference("n20_its4")
    assert R.max_its(20, 0.99, 18, 300, 4, 0.5) == (PC.MAX_ITS["n20_its4"], c["min_inliers"]) == (4, 18)
    assert c["n_hyp"] >= 5 + 4
    # 18 planted inliers: the good hypotheses qualify with exactly 18, their refine cannot exceed it, nothing returns,
    # and the first iterate(5) runs five hypotheses, one past mRansacMaxIts, and ends with the best
    assert r["count"][1] == 18 and r["flags"][1] == 3 and r["first_return"] == -1
    s = R.LiteralSolver(r["count"], lambda h: int(r["refined"][h]["count"][0]), 20, 18, 4)
    assert s.iterate(5) == ("best", 1, True) and s.mnIterations == 5
    assert s.iterate(5) == ("best", 1, True) and s.mnIterations == 10
