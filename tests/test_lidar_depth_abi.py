"""sqlm_lidar_depth_host, the kernels' shared text compiled for the CPU, without
a GPU: it equals the numpy definition (tests/lidar_depth_ref.py) bit for bit on
every case: the outputs, the stats, the state (per-point pixel, winner image)
and the depth image; a case alone equals the same case inside a batch and inside
the reversed batch; every argument error and limit returns its status."""
import numpy as np
import pytest

import lidar_depth_cases as LC
from sqrtlm import _lib
from sqrtlm import lidar_depth as LD
from sqrtlm._lib import SqlmError, lib, ptr

INVALID, UNSUPPORTED, STATE = -1, -8, -7


def test_the_library_exports_the_calls():
    for s in ("sqlm_lidar_depth", "sqlm_lidar_depth_host", "sqlm_lidar_depth_get_state", "sqlm_lidar_depth_info"):
        assert s in _lib.EXPORTS and hasattr(lib(), s)
    info = LD.depth_info()
    assert (info["max_dim"], info["max_cells"], info["launches"]) == (LD.MAX_DIM, LD.MAX_CELLS, 0)
    assert (info["half_w"], info["half_h"], info["lanes_per_keypoint"]) == (LD.HALF_W, LD.HALF_H, 8)
    assert lib().sqlm_lidar_depth_get_state(None, None, None, None) == INVALID


@pytest.mark.parametrize("name", LC.names())
def test_host_twin_equals_the_definition_bit_for_bit(name):
    o = LD.depth_host(**LC.call_args([LC.cases()[name]]), image=True, state=True)
    assert LC.differences(LC.slice_of(o, 0), LC.reference(name)) == []


@pytest.mark.parametrize("k", range(len(LC.batches())))
def test_a_case_in_a_batch_equals_the_case_alone(k):
    cfg, group = LC.batches()[k]
    fill = LC.fillers(cfg)
    frames = [fill[0]] + [LC.cases()[n] for n in group] + [fill[1]]
    o = LD.depth_host(**LC.call_args(frames), image=True, state=True)
    for j, n in enumerate(group):
        assert LC.differences(LC.slice_of(o, j + 1), LC.reference(n)) == [], n
    rev = LD.depth_host(**LC.call_args(frames[::-1]), image=True, state=True)
    for j, n in enumerate(group):
        assert LC.differences(LC.slice_of(rev, len(frames) - 2 - j), LC.reference(n)) == [], n


def test_without_the_optional_arrays():
    c = LC.cases()["truncation_37"]
    a = LC.call_args([c])
    full = LD.depth_host(**a, image=True)
    plain = LD.depth_host(**dict(a, keys_un=None, cam=None), image=False)
    assert "xyz_cam" in full and "xyz_cam" not in plain and "image" not in plain
    for k in ("class_id", "depth", "nearest_uv", "stats"):
        assert LC.same(full[k], plain[k]), k


def _raw(n_frame=1, soff=(0, 3), koff=(0, 2), rows=16, cols=24, null=(), intrinsic=None, extrinsic=None, want_cam=False):
    """sqlm_lidar_depth_host with explicit (possibly NULL) pointers on tiny arrays; returns the status."""
    a = dict(sweep_off=np.asarray(soff, np.int64), xyz=np.full((4, 3), 5.0, np.float32), key_off=np.asarray(koff, np.int64),
             key_xy=np.full((4, 2), 5.0, np.float32), key_un_xy=np.full((4, 2), 5.0, np.float32),
             intrinsic=np.ascontiguousarray(LC.UNIT_K if intrinsic is None else intrinsic, np.float64),
             extrinsic=np.ascontiguousarray(LC.axes() if extrinsic is None else extrinsic, np.float64),
             cam=np.ones(4, np.float32), class_id=np.zeros(4, np.int32), depth=np.zeros(4, np.float32),
             nearest_uv=np.zeros((4, 2), np.int32), xyz_cam=np.zeros((4, 3), np.float32) if want_cam else None,
             stats=np.zeros((max(n_frame, 1), 4), np.int32))
    p = {k: (None if k in null else ptr(v)) for k, v in a.items()}
    return lib().sqlm_lidar_depth_host(n_frame, p["sweep_off"], p["xyz"], p["key_off"], p["key_xy"], p["key_un_xy"], rows, cols,
                                       p["intrinsic"], p["extrinsic"], p["cam"], p["class_id"], p["depth"], p["nearest_uv"],
                                       p["xyz_cam"], p["stats"], None, None, None)


def test_argument_errors():
    assert _raw() == 0
    assert _raw(want_cam=True) == 0
    for k in ("sweep_off", "xyz", "key_off", "key_xy", "intrinsic", "extrinsic", "class_id", "depth", "nearest_uv", "stats"):
        assert _raw(null=(k,)) == INVALID, k
    assert _raw(null=("key_un_xy", "cam")) == 0                 # optional without xyz_cam
    assert _raw(null=("cam",), want_cam=True) == INVALID        # xyz_cam needs both
    assert _raw(null=("key_un_xy",), want_cam=True) == INVALID
    assert _raw(n_frame=-1) == INVALID
    assert _raw(n_frame=2, soff=(0, 3, 2), koff=(0, 1, 2)) == INVALID   # decreasing offsets
    assert _raw(n_frame=2, soff=(0, 1, 2), koff=(0, 2, 1)) == INVALID
    assert _raw(soff=(1, 3)) == INVALID and _raw(koff=(1, 2)) == INVALID
    assert _raw(soff=(0, 2 ** 31)) == INVALID                           # a sweep of 2^31 points: before xyz is read
    assert _raw(soff=(0, 2 ** 31 - 1)) == INVALID
    assert _raw(rows=0) == INVALID and _raw(cols=0) == INVALID and _raw(rows=-3) == INVALID
    for bad in (np.nan, np.inf, -np.inf):
        K, E = LC.UNIT_K.copy(), LC.axes()
        K[1, 2] = bad
        E[3, 0] = bad
        assert _raw(intrinsic=K) == INVALID and _raw(extrinsic=E) == INVALID, bad
    # empty inputs need no arrays
    assert _raw(soff=(0, 0), null=("xyz",)) == 0
    assert _raw(koff=(0, 0), null=("key_xy", "class_id", "depth", "nearest_uv", "key_un_xy")) == 0
    assert _raw(n_frame=0, soff=(0,), koff=(0,), null=("xyz", "key_xy", "stats")) == 0


def test_limits():
    assert _raw(rows=4097) == UNSUPPORTED and _raw(cols=4097) == UNSUPPORTED
    # the cell count of the batch, before any array is touched
    assert _raw(n_frame=2, soff=(0, 1, 3), koff=(0, 1, 2), rows=4096, cols=4096) == 0
    assert _raw(n_frame=3, soff=(0, 1, 2, 3), koff=(0, 1, 2, 2), rows=4096, cols=4096) == UNSUPPORTED
    # 2^31 points or 2^27 keypoints in the batch
    assert _raw(n_frame=2, soff=(0, 2 ** 30, 2 ** 31), koff=(0, 1, 2)) == UNSUPPORTED
    assert _raw(koff=(0, 2 ** 27)) == UNSUPPORTED
    with pytest.raises(SqlmError) as e:
        LD.depth_host([np.zeros((0, 3), np.float32)], [np.zeros((0, 2), np.float32)], 4097, 10)
    assert e.value.status == UNSUPPORTED


def test_degenerate_batches_are_fine():
    o = LD.depth_host([], [], 16, 24, LC.UNIT_K, LC.axes())
    assert o["stats"].shape == (0, 4) and len(o["class_id"]) == 0 and o["image"].shape == (0, 16, 24)
    group = [LC.cases()[n] for n in ("empty_sweep", "empty_keys", "empty_both", "keys_1")]
    o = LD.depth_host(**LC.call_args(group), image=True, state=True)
    for j, n in enumerate(("empty_sweep", "empty_keys", "empty_both", "keys_1")):
        assert LC.differences(LC.slice_of(o, j), LC.reference(n)) == [], n
    assert not o["image"][0].any() and not o["image"][2].any() and o["image"][1].any()
