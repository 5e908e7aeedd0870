"""sqlm_lidar_features_all on the GPU against the numpy definition
(tests/lidar_corner_ref.py) on the cases of tests/lidar_corner_cases.py: the
corner outputs, the final cell state, the corner mask, curvature, sorted order
and reasons, the edge masks and the angles are identical bit for bit, alone and
in a batch; results do not depend on the batch; without a corner stage the call
equals sqlm_lidar_features on the same context; the info counters show the large
growths and the ungrown candidates of a cap stop; the flat and the less-sharp
clouds go on to local BA pass 3."""
import numpy as np
import pytest

import lidar_corner_cases as CC
import lidar_feat_cases as FC
from sqrtlm import lidar_feat as LF
from sqrtlm._lib import SqlmError

pytestmark = pytest.mark.gpu


def _run(ctx, clouds, P, CP, ext=None):
    o = LF.features_all(ctx, clouds, P, CP, ext)
    o.update(LF.features_all_state(ctx))
    return o


def _check_batch(ctx, P, CP, group, reverse=False):
    filler = CC.cases()["caps_2_1"][0][: 40] if P.col_num == 256 else np.zeros((0, 3), np.float32)
    clouds = [filler] + [CC.cases()[n][0] for n in group] + [filler]
    order = list(range(len(clouds)))[::-1] if reverse else list(range(len(clouds)))
    o = _run(ctx, [clouds[k] for k in order], P, CP)
    for j, n in enumerate(group):
        assert CC.differences(CC.slice_of(o, order.index(j + 1), P), CC.reference(n)) == [], n


def test_every_case_alone_equals_the_definition(gpu_ctx):
    for name in CC.names():
        cloud, P, CP, ext, _ = CC.cases()[name]
        o = _run(gpu_ctx, [cloud], P, CP, ext)
        assert CC.differences(CC.slice_of(o, 0, P), CC.reference(name)) == [], name
        # the flat outputs beside them are those of the host twin
        host = LF.features_all_host([cloud], P, CP, ext)
        assert all(FC.same(o[k], host[k]) for k in FC.OUT_KEYS), name


def test_every_case_in_its_batch_equals_the_definition(gpu_ctx):
    for P, CP, group in CC.batches():
        _check_batch(gpu_ctx, P, CP, group)


def test_results_do_not_depend_on_the_batch(gpu_ctx):
    cloud, P, CP, ext, _ = CC.cases()["full_size"]
    LF.features_all(gpu_ctx, [cloud, cloud[::2]], P, CP, ext)  # the buffers grow and hold another call's data
    for name in ("diag_seed_upper_first", "linecount", "snake"):
        cloud, P, CP, ext, _ = CC.cases()[name]
        o = _run(gpu_ctx, [cloud], P, CP, ext)
        assert CC.differences(CC.slice_of(o, 0, P), CC.reference(name)) == [], name
    for P, CP, group in CC.batches():
        _check_batch(gpu_ctx, P, CP, group, reverse=True)
    # labels restart at 1 in every sweep of a batch
    cloud, P, CP, _, _ = CC.cases()["caps_3_0"]
    o = LF.features_all(gpu_ctx, [cloud, cloud], P, CP)
    off, lab = o["less_sharp_off"], o["less_sharp_label"]
    assert list(lab[off[0]:off[1]]) == list(lab[off[1]:off[2]]) == [1, 2, 3]


def test_without_corner_equals_the_flat_entry_point(gpu_ctx):
    for name in ("start_100", "collisions", "caps_3valid_2_6", "extrinsic"):
        cloud, P, ext = FC.cases()[name]
        want = LF.features(gpu_ctx, [cloud], P, ext)
        want_state = LF.features_state(gpu_ctx)
        got = LF.features_all(gpu_ctx, [cloud], P, None, ext)
        got_state = LF.features_all_state(gpu_ctx)["state"]
        assert all(FC.same(got[k], want[k]) for k in FC.OUT_KEYS + ("flat_off", "less_off")), name
        assert all(FC.same(got_state[k], want_state[k]) for k in FC.STATE_KEYS), name
        assert LF.features_info(gpu_ctx)["launches"] == 7
    # the old entry point still refuses the corner branch
    with pytest.raises(SqlmError) as e:
        LF.features(gpu_ctx, [cloud], FC.small(using_sharp_point=1))
    assert e.value.status == -8


def test_info_counters(gpu_ctx):
    for name in ("wall", "snake", "caps_2_1", "caps_0_0"):
        cloud, P, CP, ext, _ = CC.cases()[name]
        o = LF.features_all(gpu_ctx, [cloud], P, CP, ext)
        info, st = LF.features_all_info(gpu_ctx), CC.reference(name)["stats"]
        assert info["launches"] == 13
        for k in ("seeds_grown", "cells_labelled", "cells_unstable", "largest_segment", "most_levels"):
            assert info[k] == st[k], (name, k)
        assert info["less_sharp"] == len(o["less_sharp_xyz"]) and info["sharp"] == len(o["sharp_xyz"])
    # a segment larger than the workgroup (one level's chunk of 256 lanes), and a growth of more than 64 levels
    LF.features_all(gpu_ctx, [CC.cases()["wall"][0]], *CC.cases()["wall"][1:3])
    assert LF.features_all_info(gpu_ctx)["largest_segment"] == 1536
    LF.features_all(gpu_ctx, [CC.cases()["snake"][0]], *CC.cases()["snake"][1:3])
    assert LF.features_all_info(gpu_ctx)["most_levels"] == 90
    # the cap stop left candidates ungrown: 5 feasible seeds, 2 grown (and the partner between them)
    # (the device shows the 3 growths; that the 7 skipped candidates' cells stayed 0 is the definition's
    # counter, and the device's final cell state equals the definition's in the tests above)
    LF.features_all(gpu_ctx, [CC.cases()["caps_2_1"][0]], *CC.cases()["caps_2_1"][1:3])
    assert LF.features_all_info(gpu_ctx)["seeds_grown"] == 3 and CC.reference("caps_2_1")["stats"]["ungrown_passing"] == 7
    # an empty batch launches nothing
    LF.features_all(gpu_ctx, [np.zeros((0, 3), np.float32)], *CC.cases()["wall"][1:3])
    assert LF.features_all_info(gpu_ctx)["launches"] == 0


def test_argument_errors_reach_the_caller_before_the_device(gpu_ctx):
    from dataclasses import replace
    cloud, P, CP, _, _ = CC.cases()["caps_2_1"]
    for kw, status in ((dict(P=replace(P, num_curvature_regions_corner=0)), -1),
                       (dict(CP=replace(CP, max_corner_less_sharp=-1)), -1),
                       (dict(CP=replace(CP, sharp_curv_th=float("nan"))), -1),
                       (dict(P=replace(P, col_num=4097)), -8)):
        with pytest.raises(SqlmError) as e:
            LF.features_all(gpu_ctx, [cloud], kw.get("P", P), kw.get("CP", CP))
        assert e.value.status == status, kw
    o = _run(gpu_ctx, [cloud], P, CP)
    assert CC.differences(CC.slice_of(o, 0, P), CC.reference("caps_2_1")) == []


def test_hand_off_to_local_ba_pass_3(gpu_ctx):
    """Two small generated sweeps with poles: the flat and the less-sharp clouds
    become a flat and a corner set of pose 5's LiDAR edges, and one optimize runs."""
    P = LF.Params(row_num=64, col_num=900)
    CP = LF.CornerParams(sharp_curv_th=1.0)
    poses = [(np.eye(3), np.array([0.0, 0.0, 0.0])), (np.eye(3), np.array([0.3, 0.1, 0.0]))]
    clouds = [LF.make_sweep(60, n_az=900, order="azimuth", pose=p, n_poles=12) for p in poses]  # one scene, two poses
    Twc = []
    for R_, t in poses:
        T = np.eye(4, dtype=np.float32)
        T[:3, :3], T[:3, 3] = R_, t
        Twc.append(T)
    dev, host = LF.features_all(gpu_ctx, clouds, P, CP), LF.features_all_host(clouds, P, CP)
    for k in FC.OUT_KEYS + CC.OUT_KEYS + ("less_off", "less_sharp_off", "sharp_off"):
        assert CC.same(dev[k], host[k]), k
    from sqrtlm import synth
    gpu_ctx.set_problem(synth.make_problem(8, 120, pair_window=3, n_fixed=2, seed=7, robust=True))
    n_flat, n_corner = LF.set_lidar_edge_sets(gpu_ctx, 5, dev, Twc, query=1, info=50.0, dist_sq_threshold=1.0)
    assert n_flat > 0 and n_corner > 0, (n_flat, n_corner)
    n_it, st = gpu_ctx.optimize(0, 3)
    assert n_it >= 1 and np.isfinite(st["chi2_end"])
    # the mirror of the reference interface
    out = LF.lidarProcess(gpu_ctx, clouds[0], P, corner=CP)
    assert len(out) == 7 and CC.same(out[5], dev["less_sharp_xyz"][:dev["less_sharp_off"][1]])
    assert CC.same(out[4], dev["sharp_xyz"][:dev["sharp_off"][1]])
