"""The numpy definition (tests/mappoint_ref.py) on the cases
(tests/mappoint_cases.py): every case does what it is there for, so that the
bit-for-bit tests of the host twins and of the kernels do not pass on vacuous
inputs."""
import numpy as np
import pytest

import mappoint_cases as MC
import mappoint_ref as R
from sqrtlm import mappoint as M


def test_every_reason_code_occurs_where_it_was_planted():
    seen = set()
    for name in MC.REASON_NAMES:
        want = MC.reason_pairs()[name][1]
        got = MC.tri_slice(name)["reason"]
        assert len(got) >= 1
        if want is not None:
            assert (got == want).all(), (name, got)
        seen |= set(int(v) for v in got)
    assert seen >= set(range(9)), seen


def test_reason_cases_fail_for_the_reason_they_name():
    """Beyond the code: the quantity the case aims at is what decides."""
    s = MC.tri_slice("parallax")
    assert (s["x3d"] == 0).all()
    for name, row, sign in (("z1", "kf1", -1), ("z2", "kf2", -1)):
        p, s = MC.reason_pairs()[name][0], MC.tri_slice(name)
        T = getattr(p, row).Tcw.astype(float)
        z = s["x3d"].astype(float) @ T[2, :3] + T[2, 3]
        assert (z < 0).all()
        np.testing.assert_allclose(s["x3d"], p.meta["X"], rtol=1e-5)   # the point behind the camera is recovered
    # the two sides of the ratio test (:623)
    p, s = MC.reason_pairs()["scale"][0], MC.tri_slice("scale")
    sides = []
    for i in range(2):
        X = s["x3d"][i]
        d1 = np.float32(np.linalg.norm(X - R.center(p.kf1.Tcw)))
        d2 = np.float32(np.linalg.norm(X - R.center(p.kf2.Tcw)))
        ro = (p.kf1.mvScaleFactors[p.kf1.mvKeysUn["octave"][i]] / p.kf2.mvScaleFactors[p.kf2.mvKeysUn["octave"][i]])
        rd, rf = d2 / d1, np.float32(p.ratio_factor)
        sides.append((bool(rd * rf < ro), bool(rd > ro * rf)))
    assert sides == [(True, False), (False, True)]
    # w == 0 and the zero distance are exact
    assert (MC.tri_slice("w_zero")["x3d"] == 0).all()
    p, s = MC.reason_pairs()["zero_dist"][0], MC.tri_slice("zero_dist")
    assert (s["x3d"][0] == R.center(p.kf1.Tcw)).all() and s["x3d"][0, 2] != 0
    # NaN and Inf reject
    for name in ("nan_keypoint", "inf_translation", "inf_rotation", "same_pose"):
        assert (MC.tri_slice(name)["reason"] != 0).all(), name


def test_planted_pairs_create_their_points_and_straddle_the_kernel_shapes():
    info = M.triangulate_info()
    sizes = set(MC.SIZES)
    assert {info["wave"] - 1, info["wave"], info["wave"] + 1, info["block"] + 1, 1} <= sizes
    names = list(MC.tri_pairs())
    assert 0 < names.index("empty") < len(MC.SIZES) and len(MC.tri_pairs()["empty"].matches) == 0
    for n in MC.SIZES:
        s = MC.tri_slice(f"n{n}")
        assert len(s["reason"]) == n and s["n_new"][0] == n and (s["reason"] == 0).all()
        p = MC.tri_pairs()[f"n{n}"]
        # 0.5 px of noise at 4 to 12 m with a 1 m baseline: centimetres to decimetres
        assert np.abs(s["x3d"] - p.meta["X"]).max() < 0.5
    assert MC.tri_reference()["off"][-1] < 600   # the whole batch stays small


def test_the_library_reports_the_definitions_constants():
    assert M.triangulate_info()["sweeps"] == R.SWEEPS
    assert M.map_points_update_info()["lds_max"] == R.LDS_MAX


def test_refresh_cases_do_what_they_are_there_for():
    b, r = MC.mp_batch(), MC.mp_reference()
    cnt = np.diff(b.obs_off)
    names = list(MC.MP_NAMES)
    assert list(cnt[:len(MC.MP_COUNTS)]) == list(MC.MP_COUNTS)
    lds = M.map_points_update_info()["lds_max"]
    assert cnt.max() == lds + 1 and sorted(cnt)[-2] <= lds    # exactly one point past the threshold, by one
    assert r["best_idx"][0] == -1 and (r["normal"][0] == 0).all()
    # all descriptors equal: every median 0, the first row wins
    j = names.index("all_equal")
    assert r["best_idx"][j] == 0 and r["best_median"][j] == 0 and cnt[j] > 1
    # the tie is a tie: rows 0 and 1 share the least median, row 2 is worse
    j, k = names.index("tie"), names.index("tie_permuted")
    D = np.sort(R.hamming_matrix(b.obs_desc[b.obs_off[j]:b.obs_off[j + 1]]), axis=1)
    med = D[:, int(0.5 * (cnt[j] - 1))]
    assert med[0] == med[1] < med[2] and r["best_idx"][j] == 0
    # permuted: the other of the tied rows wins, which is another descriptor; nothing else changes
    perm = list(MC.TIE_PERM)
    assert r["best_idx"][k] == 1 and perm[1] == 1 and perm[0] == 2
    dj = b.obs_desc[b.obs_off[j] + r["best_idx"][j]]
    dk = b.obs_desc[b.obs_off[k] + r["best_idx"][k]]
    assert (dj != dk).any() and r["best_median"][j] == r["best_median"][k]
    assert r["max_dist"][j] == r["max_dist"][k] and r["min_dist"][j] == r["min_dist"][k]
    np.testing.assert_allclose(r["normal"][j], r["normal"][k], rtol=0, atol=4 * np.finfo(np.float32).eps)
    # a camera centre equal to the point: IEEE's NaN
    j = names.index("at_center")
    assert np.isnan(r["normal"][j]).all() and np.isfinite(r["max_dist"][j])
    assert np.isfinite(r["normal"][:j]).all()


def test_distinctive_descriptor_equals_the_literal_transcription():
    b, r = MC.mp_batch(), MC.mp_reference()
    for j in range(b.n_pt):
        d = b.obs_desc[b.obs_off[j]:b.obs_off[j + 1]]
        if len(d) == 0:
            continue
        assert R.distinctive_literal(d) == (r["best_idx"][j], r["best_median"][j]), j


def test_normal_and_depth_agree_with_double_arithmetic():
    b, r = MC.mp_batch(), MC.mp_reference()
    for j in range(1, b.n_pt - 1):
        c = b.obs_center[b.obs_off[j]:b.obs_off[j + 1]].astype(float)
        v = b.pos[j].astype(float) - c
        n = (v / np.linalg.norm(v, axis=1, keepdims=True)).mean(0)
        np.testing.assert_allclose(r["normal"][j], n, atol=1e-5)
        dist = np.linalg.norm(b.pos[j].astype(float) - b.ref_center[j])
        np.testing.assert_allclose(r["max_dist"][j], dist * b.level_scale[j], rtol=1e-6)
        np.testing.assert_allclose(r["min_dist"][j], dist * b.level_scale[j] / b.max_scale[j], rtol=1e-6)
