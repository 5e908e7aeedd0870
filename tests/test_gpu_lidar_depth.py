"""sqlm_lidar_depth on the GPU against the numpy definition
(tests/lidar_depth_ref.py) on the cases of tests/lidar_depth_cases.py: the
per-keypoint class, depth, nearest pixel and camera point, the stats, the
per-point pixel, the winner image and the depth image (downloaded, and read back
as state) are identical bit for bit; results do not depend on the batch (a case
alone, in its batch, in the reversed batch, and after the full-size frame has
grown the staging buffers); info reports a constant number of launches, 0 for
an empty call; argument errors reach the caller before the device is touched."""
import numpy as np
import pytest

import lidar_depth_cases as LC
from sqrtlm import lidar_depth as LD
from sqrtlm._lib import SqlmError, lib

pytestmark = pytest.mark.gpu

LAUNCHES = 3


def _run(ctx, frames, image=True):
    o = LD.depth(ctx, **LC.call_args(frames), image=image)
    o["state"] = LD.depth_state(ctx)
    return o


def _check_batch(ctx, cfg, group, reverse=False):
    fill = LC.fillers(cfg)
    frames = [fill[0]] + [LC.cases()[n] for n in group] + [fill[1]]
    order = list(range(len(frames)))[::-1] if reverse else list(range(len(frames)))
    o = _run(ctx, [frames[k] for k in order])
    assert LD.depth_info(ctx)["launches"] == LAUNCHES
    for j, n in enumerate(group):
        assert LC.differences(LC.slice_of(o, order.index(j + 1)), LC.reference(n)) == [], n


def test_full_size_frame_equals_the_definition(gpu_ctx):
    o = _run(gpu_ctx, [LC.cases()["full_size"]])
    assert LC.differences(LC.slice_of(o, 0), LC.reference("full_size")) == []
    info = LD.depth_info(gpu_ctx)
    assert info["launches"] == LAUNCHES and info["keypoints"] == 2000
    assert info["points"] == len(LC.cases()["full_size"].xyz)
    # the mirror of what the constructor leaves behind
    c = LC.cases()["full_size"]
    cls, mv_depth, img = LD.frame_depth(gpu_ctx, c.xyz, c.keys)
    want = LC.reference("full_size")
    assert LC.same(cls, want["class_id"]) and LC.same(mv_depth, want["depth"]) and LC.same(img, want["image"])


def test_every_case_in_its_batch_equals_the_definition(gpu_ctx):
    for cfg, group in LC.batches():
        _check_batch(gpu_ctx, cfg, group)


def test_results_do_not_depend_on_the_batch(gpu_ctx):
    full = LC.cases()["full_size"]
    half = LC.Case(full.cfg, full.xyz[::2], full.keys[::2], full.keys_un[::2])
    LD.depth(gpu_ctx, **LC.call_args([full, half]))  # the staging buffers grow and hold another call's data
    for name in LC.names(full=False):
        o = _run(gpu_ctx, [LC.cases()[name]])
        assert LC.differences(LC.slice_of(o, 0), LC.reference(name)) == [], name
    for cfg, group in LC.batches():
        _check_batch(gpu_ctx, cfg, group, reverse=True)


def test_launch_counts_and_the_optional_arrays(gpu_ctx):
    for name in ("collide_1", "collide_4097", "keys_2049", "empty_sweep", "empty_keys"):
        _run(gpu_ctx, [LC.cases()[name]])
        assert LD.depth_info(gpu_ctx)["launches"] == LAUNCHES, name
    # nothing reaches the device: no launch, zero images, zero stats
    for frames in ([LC.cases()["empty_both"]], [LC.cases()["empty_both"]] * 3):
        o = _run(gpu_ctx, frames)
        assert LD.depth_info(gpu_ctx)["launches"] == 0
        assert not o["image"].any() and not o["stats"].any() and not o["state"]["winner"].any()
    o = LD.depth(gpu_ctx, [], [], 16, 24, LC.UNIT_K, LC.axes(), image=True)
    assert LD.depth_info(gpu_ctx)["launches"] == 0 and o["stats"].shape == (0, 4)
    # without the image, the undistorted keypoints and the camera the other outputs are the same
    c = LC.cases()["truncation_37"]
    a = LC.call_args([c])
    plain = LD.depth(gpu_ctx, **dict(a, keys_un=None, cam=None), image=False)
    want = LC.reference("truncation_37")
    assert "xyz_cam" not in plain and "image" not in plain
    for k in ("class_id", "depth", "nearest_uv"):
        assert LC.same(plain[k], want[k]), k
    assert LC.same(plain["stats"][0], want["stats"])
    assert LC.same(LD.depth_state(gpu_ctx)["image"][0], want["image"])


def test_state_before_any_call_and_argument_errors_before_the_device():
    from sqrtlm.optimizer import Context
    with Context(0) as ctx:
        assert lib().sqlm_lidar_depth_get_state(ctx._h, None, None, None) == -7
        c = LC.cases()["keys_1"]
        a = LC.call_args([c])
        E = LC.axes()
        E[0, 0] = np.nan
        for bad, status in ((dict(rows=4097), -8), (dict(cols=4097), -8), (dict(rows=0), -1), (dict(extrinsic=E), -1)):
            with pytest.raises(SqlmError) as e:
                LD.depth(ctx, **dict(a, **bad))
            assert e.value.status == status, bad
        with pytest.raises(SqlmError) as e:  # the cell count of the batch
            LD.depth(ctx, [c.xyz] * 3, [c.keys] * 3, 4096, 4096, c.cfg.intrinsic, c.cfg.extrinsic)
        assert e.value.status == -8
        # none of them reached the device or left a state behind
        assert LD.depth_info(ctx)["launches"] == 0
        assert lib().sqlm_lidar_depth_get_state(ctx._h, None, None, None) == -7
        # the context still works
        o = _run(ctx, [c])
        assert LC.differences(LC.slice_of(o, 0), LC.reference("keys_1")) == []
