"""The corner branch on the CPU: the order-free definition (tests/lidar_corner_ref.py)
against the naive transcription of the reference's loops, the host twin
(sqlm_lidar_features_all_host) against the definition bit for bit, what the new
entry point owes the old one, and the library's acos / sin / cos."""
import numpy as np
import pytest

import lidar_corner_cases as CC
import lidar_corner_naive as NV
import lidar_corner_ref as CR
import lidar_feat_cases as FC
from sqrtlm import lidar_feat as LF
from sqrtlm._lib import SqlmError

SMALL = CC.names(full=False)


@pytest.mark.parametrize("name", CC.names())
def test_case_hits_its_rule(name):
    CC.witness(name)


@pytest.mark.parametrize("name", SMALL)
def test_definition_equals_naive_transcription(name):
    cloud, P, CP, ext, _ = CC.cases()[name]
    want, got = NV.process(cloud, P, CP, ext), CC.reference(name)
    bad = [k for k in CC.OUT_KEYS if not CC.same(got[k], want[k])]
    bad += [k for k in ("cell_state", "initial_state", "mask", "curvature", "sorted", "reason")
            if not CC.same(got["corner_state"][k], want["corner_state"][k])]
    assert not bad, bad


def test_seed_order_changes_the_result():
    a, b = CC.reference("diag_seed_upper_first"), CC.reference("diag_seed_lower_first")
    sa, sb = a["corner_state"]["cell_state"], b["corner_state"]["cell_state"]
    assert sa[2, 19] == 1 and sb[2, 19] == -2 and sb[1, 20] == 0


@pytest.mark.parametrize("name", CC.names())
def test_host_twin_equals_definition(name):
    cloud, P, CP, ext, _ = CC.cases()[name]
    got = LF.features_all_host([cloud], P, CP, ext, state=True)
    assert not CC.differences(CC.slice_of(got, 0, P), CC.reference(name))


def test_host_twin_batches_restart_labels():
    for P, CP, names in CC.batches():
        if len(names) < 2:
            continue
        got = LF.features_all_host([CC.cases()[n][0] for n in names], P, CP, state=True)
        for k, n in enumerate(names):
            assert not CC.differences(CC.slice_of(got, k, P), CC.reference(n)), n
    caps = [CC.cases()["caps_3_0"][0]] * 2
    P, CP = CC.cases()["caps_3_0"][1:3]
    got = LF.features_all_host(caps, P, CP)
    lab = got["less_sharp_label"]
    o = got["less_sharp_off"]
    assert list(lab[o[0]:o[1]]) == list(lab[o[1]:o[2]]) == [1, 2, 3]


@pytest.mark.parametrize("name", FC.names(full=False))
def test_without_corner_equals_the_flat_entry_point(name):
    cloud, P, ext = FC.cases()[name]
    want = LF.features_host([cloud], P, ext, state=True)
    got = LF.features_all_host([cloud], P, None, ext, state=True)
    assert all(FC.same(got[k], want[k]) for k in FC.OUT_KEYS + ("flat_off", "less_off"))
    assert all(FC.same(got["state"][k], want["state"][k]) for k in FC.STATE_KEYS + ("scan_off",))


def _flat_independent(cloud, P, CP, ext):
    off = LF.features_all_host([cloud], P, None, ext, state=True)
    on = LF.features_all_host([cloud], P, CP, ext, state=True)
    assert all(FC.same(on[k], off[k]) for k in FC.OUT_KEYS + ("flat_off", "less_off"))
    assert all(FC.same(on["state"][k], off["state"][k]) for k in FC.STATE_KEYS)
    alone = LF.features_all_host([cloud], P, CP, ext, flat=False)
    assert all(CC.same(alone[k], on[k]) for k in CC.OUT_KEYS)


@pytest.mark.parametrize("name", [n for n in FC.names(full=False) if FC.cases()[n][1].num_curvature_regions_corner >= 1])
def test_flat_outputs_do_not_depend_on_the_corner_branch_flat_cases(name):
    cloud, P, ext = FC.cases()[name]
    _flat_independent(cloud, P, LF.CornerParams(sharp_curv_th=0.05, ground_z_bound=-1.0, ring_enabled=CC.ALL), ext)


@pytest.mark.parametrize("name", SMALL)
def test_flat_outputs_do_not_depend_on_the_corner_branch(name):
    cloud, P, CP, ext, _ = CC.cases()[name]
    _flat_independent(cloud, P, CP, ext)


def test_argument_errors():
    cloud, P, CP, _, _ = CC.cases()["caps_2_1"]

    def status(P=P, CP=CP, **kw):
        with pytest.raises(SqlmError) as e:
            LF.features_all_host([cloud], P, CP, **kw)
        return e.value.status

    from dataclasses import replace
    inv, unsupported = -1, -8  # SQLM_ERR_INVALID_ARG, SQLM_ERR_UNSUPPORTED
    assert status(P=replace(P, num_curvature_regions_corner=0)) == inv
    assert status(CP=replace(CP, max_corner_sharp=-1)) == inv
    assert status(CP=replace(CP, max_corner_less_sharp=-1)) == inv
    assert status(CP=replace(CP, sharp_curv_th=float("nan"))) == inv
    assert status(CP=replace(CP, sharp_curv_th=float("inf"))) == inv
    assert status(CP=replace(CP, ground_z_bound=float("-inf"))) == inv
    assert status(P=replace(P, row_num=129)) == unsupported
    # the width check applies to the corner stage only
    LF.features_all_host([cloud], replace(P, num_curvature_regions_corner=0), None)
    # using_sharp_point is ignored here and still refused by the old entry point
    LF.features_all_host([cloud], replace(P, using_sharp_point=1), CP)
    with pytest.raises(SqlmError) as e:
        LF.features_host([cloud], replace(P, using_sharp_point=1))
    assert e.value.status == unsupported


def test_edge_predicate_is_bit_symmetric_and_parallel_rays_give_no_edge():
    rng = np.random.default_rng(5)
    p1 = (rng.normal(size=(20000, 3)) * 8).astype(np.float32)
    p2 = (p1 * rng.uniform(0.5, 2.0, (20000, 1)) + rng.normal(size=(20000, 3)) * 0.3).astype(np.float32)
    a, b = LF.corner_angle_probe(p1, p2), LF.corner_angle_probe(p2, p1)
    assert CC.same(a, b) and CC.same(a, CR.angle(p1, p2)) and (a > 1).any() and (a <= 1).any()
    # exactly parallel rays: the acos argument is exactly 1 (angle 0) or, found by this search, rounds
    # above 1 (NaN); neither is an edge and the definition agrees on which is which
    q = LF.corner_angle_probe(p1, p1 * np.float32(2.0))
    want = CR.angle(p1, p1 * np.float32(2.0))
    assert np.isnan(q).any() and (q[~np.isnan(q)] < 1e-3).all() and not (q > 1).any()
    assert np.array_equal(np.isnan(q), np.isnan(want)) and CC.same(q[~np.isnan(q)], want[~np.isnan(want)])
    # far-apart cells: opposite directions, huge range ratio
    far = LF.corner_angle_probe(p1, -p1 * np.float32(1000.0))
    assert not (far > 1).any()


def test_edge_masks_are_symmetric_where_the_offsets_are():
    for name in ("wall", "linecount", "full_size"):
        st = CC.reference(name)["corner_state"]
        e, ang = st["edge"], st["angle"]
        down, up = ang[:-1, :, 1], ang[1:, :, 0]
        assert CC.same(down, up)
        right, left = ang[:, :, 3], np.roll(ang[:, :, 2], -1, axis=1)
        assert CC.same(right, left)
        assert np.array_equal(e[:-1] >> 1 & 1, e[1:] & 1)


def test_library_trig_within_one_ulp_of_numpy():
    worst = {}
    for which, f, x in (("acos", np.arccos, np.linspace(-1.0, 1.0, 400001)),
                        ("sin", np.sin, np.linspace(0.0, np.pi, 400001)),
                        ("cos", np.cos, np.linspace(0.0, np.pi, 400001))):
        got, want = LF.corner_trig_probe(which, x), f(x)
        ulp = np.abs(got - want) / np.spacing(np.maximum(np.abs(want), np.finfo(np.float64).tiny))
        worst[which] = float(ulp.max())  # the whole sweep, the zeros of the functions included
        assert CC.same(got, getattr(CR, which)(x))
    print("worst ulp against numpy:", worst)
    assert max(worst.values()) <= 1.0
