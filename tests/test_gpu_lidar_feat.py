"""sqlm_lidar_features on the GPU against the numpy definition
(tests/lidar_feat_ref.py) on the cases of tests/lidar_feat_cases.py: the
outputs, the per-point rings, the scans, the range image, the mask, the
curvature, the sorted orders and the reason codes are identical, NaN for NaN;
results do not depend on the batch (a case alone, in its batch, in the reversed
batch, and after the full-size sweep has grown the staging buffers); info
reports the launches and that the early stop ran; argument errors reach the
caller before the device is touched; the less-flat clouds of three sweeps go
through sqlm_lidar_associate as the host twin's do."""
import numpy as np
import pytest

import lidar_feat_cases as LC
from sqrtlm import lidar_feat as LF
from sqrtlm._lib import SqlmError

pytestmark = pytest.mark.gpu


def _run(ctx, clouds, P, ext):
    o = LF.features(ctx, clouds, P, ext)
    o["state"] = LF.features_state(ctx)
    return o, np.concatenate([[0], np.cumsum([len(c) for c in clouds])])


def _check_batch(ctx, P, ext, group, reverse=False):
    fill = LC.fillers(P)
    clouds = [fill[0]] + [LC.cases()[n][0] for n in group] + [fill[1]]
    order = list(range(len(clouds)))[::-1] if reverse else list(range(len(clouds)))
    o, off = _run(ctx, [clouds[k] for k in order], P, ext)
    for j, n in enumerate(group):
        assert LC.differences(LC.slice_of(o, order.index(j + 1), off, P), LC.reference(n)) == [], n


def test_full_size_sweep_equals_the_definition(gpu_ctx):
    cloud, P, ext = LC.cases()["full_size"]
    o, off = _run(gpu_ctx, [cloud], P, ext)
    assert LC.differences(LC.slice_of(o, 0, off, P), LC.reference("full_size")) == []
    info, st = LF.features_info(gpu_ctx), LC.reference("full_size")["stats"]
    assert info["launches"] == 7
    assert info["largest_subregion"] == st["largest_subregion"] and info["candidates"] == st["candidates"]
    assert info["picked"] == st["picked"] == len(o["less_xyz"])
    assert info["evaluated"] < info["candidates"]  # the caps stopped most subregions early


def test_every_case_in_its_batch_equals_the_definition(gpu_ctx):
    for P, ext, group in LC.batches():
        _check_batch(gpu_ctx, P, ext, group)


def test_results_do_not_depend_on_the_batch(gpu_ctx):
    cloud, P, ext = LC.cases()["full_size"]
    LF.features(gpu_ctx, [cloud, cloud[::2]], P, ext)  # the staging buffers grow and hold another call's data
    for name in LC.names(full=False):
        cloud, P, ext = LC.cases()[name]
        o, off = _run(gpu_ctx, [cloud], P, ext)
        assert LC.differences(LC.slice_of(o, 0, off, P), LC.reference(name)) == [], name
    for P, ext, group in LC.batches():
        _check_batch(gpu_ctx, P, ext, group, reverse=True)


def test_the_early_stop_ran_on_the_cap_case(gpu_ctx):
    cloud, P, ext = LC.cases()["region_129"]
    o = LF.features(gpu_ctx, [cloud], P, ext)
    info = LF.features_info(gpu_ctx)
    assert info["launches"] == 7 and info["largest_subregion"] == 129 and info["candidates"] == 129
    assert info["evaluated"] == 64 and info["picked"] == 6 == len(o["less_xyz"])
    # an empty batch launches nothing
    LF.features(gpu_ctx, [np.zeros((0, 3), np.float32)], P, ext)
    assert LF.features_info(gpu_ctx)["launches"] == 0
    assert LF.features_state(gpu_ctx)["scan_off"][-1] == 0


def test_argument_errors_reach_the_caller_before_the_device(gpu_ctx):
    cloud = LC.cases()["start_0"][0]
    for bad, status in ((dict(using_sharp_point=1), -8), (dict(rows=129), -8), (dict(cols=4097), -8),
                        (dict(num_scan_subregions=0), -1), (dict(deg_diff=0.0), -1)):
        with pytest.raises(SqlmError) as e:
            LF.features(gpu_ctx, [cloud], LC.small(**bad))
        assert e.value.status == status, bad
    # the context still works
    name = "start_100"
    cloud, P, ext = LC.cases()[name]
    o, off = _run(gpu_ctx, [cloud], P, ext)
    assert LC.differences(LC.slice_of(o, 0, off, P), LC.reference(name)) == []


def test_hand_off_to_the_lidar_association(gpu_ctx):
    """Three generated sweeps at known poses: the device's less-flat clouds fed
    to sqlm_lidar_associate give the pairs the host twin's clouds give."""
    P = LF.Params(row_num=64, col_num=600)
    poses = [(np.eye(3), np.array([0.0, 0.0, 0.0])), (np.eye(3), np.array([0.4, 0.1, 0.0])),
             (np.eye(3), np.array([0.8, -0.1, 0.0]))]
    clouds = [LF.make_sweep(50 + k, n_az=600, order="azimuth", pose=p) for k, p in enumerate(poses)]
    Twc = []
    for R_, t in poses:
        T = np.eye(4, dtype=np.float32)
        T[:3, :3], T[:3, 3] = R_, t
        Twc.append(T)
    dev, host = LF.features(gpu_ctx, clouds, P), LF.features_host(clouds, P)
    for k in LC.OUT_KEYS + ("less_off", "flat_off"):
        assert LC.same(dev[k], host[k]), k
    res = []
    for f in (dev, host):
        off = f["less_off"]
        maps = [f["less_xyz"][off[k]:off[k + 1]] for k in (0, 1)]
        idx, d2, xyz, acc = gpu_ctx.lidar_associate(maps, Twc[:2], f["less_xyz"][off[2]:off[3]], Twc[2], 1.0)
        res.append((idx, acc, gpu_ctx.lidar_n_pairs))
    assert res[0][2] == res[1][2] > 0
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    # the helper onto the optimizer's existing cloud path builds the same number of LiDAR edges
    from sqrtlm import synth
    gpu_ctx.set_problem(synth.make_problem(8, 120, pair_window=3, n_fixed=2, seed=7, robust=True))
    assert LF.set_lidar_edges(gpu_ctx, 5, dev, Twc, query=2, info=50.0, dist_sq_threshold=1.0) == res[0][2]
    # the mirror of the reference interface
    flat, less, less_n, less_rc = LF.lidarProcess(gpu_ctx, clouds[0], P)
    assert LC.same(less, dev["less_xyz"][:dev["less_off"][1]]) and len(less_n) == len(less_rc) == len(less)
    assert LC.same(flat, dev["flat_xyz"][:dev["flat_off"][1]])
