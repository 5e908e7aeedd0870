"""sqlm_lidar_features_host, the kernels' shared text compiled for the CPU,
without a GPU: it equals the numpy definition (tests/lidar_feat_ref.py) bit for
bit on every case, all outputs and all of the intermediate state; a case alone
equals the same case inside a batch; sqlm_atan / sqlm_atan2 as the library
compiled them equal the numpy restatement bit for bit; argument errors."""
import ctypes as C

import numpy as np
import pytest

import lidar_feat_cases as LC
import lidar_feat_ref as R
from sqrtlm import _lib
from sqrtlm import lidar_feat as LF
from sqrtlm._lib import SqlmError, lib

INVALID, UNSUPPORTED = -1, -8


def test_the_library_exports_the_calls():
    for s in ("sqlm_lidar_features", "sqlm_lidar_features_host", "sqlm_lidar_features_get_state",
              "sqlm_lidar_features_info", "sqlm_lidar_feat_trig_probe"):
        assert s in _lib.EXPORTS and hasattr(lib(), s)
    info = LF.features_info()
    assert (info["max_rows"], info["max_cols"], info["launches"]) == (128, 4096, 0)


@pytest.mark.parametrize("name", LC.names())
def test_host_twin_equals_the_definition_bit_for_bit(name):
    cloud, P, ext = LC.cases()[name]
    o = LF.features_host([cloud], P, ext, state=True)
    assert LC.differences(LC.slice_of(o, 0, np.array([0, len(cloud)]), P), LC.reference(name)) == []


@pytest.mark.parametrize("k", range(len(LC.batches())))
def test_a_case_in_a_batch_equals_the_case_alone(k):
    P, ext, group = LC.batches()[k]
    fill = LC.fillers(P)
    clouds = [fill[0]] + [LC.cases()[n][0] for n in group] + [fill[1]]
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    o = LF.features_host(clouds, P, ext, state=True)
    for j, n in enumerate(group):
        assert LC.differences(LC.slice_of(o, j + 1, off, P), LC.reference(n)) == [], n
    rev = LF.features_host(clouds[::-1], P, ext, state=True)
    roff = np.concatenate([[0], np.cumsum([len(c) for c in clouds[::-1]])])
    for j, n in enumerate(group):
        assert LC.differences(LC.slice_of(rev, len(clouds) - 2 - j, roff, P), LC.reference(n)) == [], n


def test_library_atan_and_atan2_equal_the_numpy_restatement():
    rng = np.random.default_rng(3)
    x = np.concatenate([np.linspace(-40.0, 40.0, 200001), np.logspace(-12, 25, 5001), -np.logspace(-12, 25, 5001),
                        [0.0, -0.0, 0.4375, 0.6875, 1.1875, 2.4375, np.inf, -np.inf, np.nan]])
    assert LC.same(LF.trig_probe(x).view(np.uint64), R.atan(x).view(np.uint64))
    th = rng.uniform(-np.pi, np.pi, 200000)
    r = 10.0 ** rng.uniform(-3, 3, 200000)
    y = np.concatenate([r * np.sin(th), [0.0, -0.0, 0.0, -0.0, 1.0, -1.0, 1e-300, 1e300, np.nan, 1.0, 3.0]])
    xx = np.concatenate([r * np.cos(th), [1.0, 1.0, -1.0, -1.0, 0.0, 0.0, 1e300, 1e-300, 1.0, np.nan, 1.0]])
    assert LC.same(LF.trig_probe(y, xx).view(np.uint64), R.atan2(y, xx).view(np.uint64))
    # the float azimuths of a sweep, as the extraction takes them
    c = LC.cases()["full_size"][0][::7].astype(np.float64)
    assert LC.same(LF.trig_probe(c[:, 1], c[:, 0]).view(np.uint64), R.atan2(c[:, 1], c[:, 0]).view(np.uint64))


def _raw(n_sweep, off, xyz, P, outs=None, params_null=False):
    """sqlm_lidar_features_host with explicit (possibly NULL) pointers; returns the status."""
    n = max(len(xyz), 1) if xyz is not None else 1
    bufs = [np.zeros(n_sweep + 1 if k in (0, 3) else 3 * n, np.int64 if k in (0, 3) else np.float32) for k in range(7)]
    ptrs = [b.ctypes.data for b in bufs]
    for k in (outs or ()):
        ptrs[k] = None
    pc = P.as_c()
    return lib().sqlm_lidar_features_host(
        n_sweep, None if off is None else off.ctypes.data, None if xyz is None else xyz.ctypes.data,
        None if params_null else C.addressof(pc), None, *ptrs, None)


def test_argument_errors():
    cloud = np.ascontiguousarray(LC.cases()["start_0"][0])
    P = LC.small()
    off = np.array([0, len(cloud)], np.int64)
    assert _raw(1, off, cloud, P) == 0
    assert _raw(1, None, cloud, P) == INVALID
    assert _raw(1, off, None, P) == INVALID
    assert _raw(1, off, cloud, P, params_null=True) == INVALID
    assert _raw(-1, off, cloud, P) == INVALID
    for k in range(7):
        assert _raw(1, off, cloud, P, outs=[k]) == INVALID, k
    assert _raw(2, np.array([0, 10, 5], np.int64), cloud, P) == INVALID   # offsets not ascending
    assert _raw(1, np.array([1, len(cloud)], np.int64), cloud, P) == INVALID
    for bad in (dict(num_scan_subregions=0), dict(num_curvature_regions_flat=0), dict(num_curvature_regions_corner=-1),
                dict(max_surf_flat=-1), dict(max_surf_less_flat=-1), dict(deg_diff=0.0), dict(deg_diff=float("nan"))):
        assert _raw(1, off, cloud, LC.small(**bad)) == INVALID, bad
    assert _raw(1, off, cloud, LC.small(rows=0)) == INVALID
    assert _raw(1, off, cloud, LC.small(cols=0)) == INVALID
    # the limits and the corner branch
    assert _raw(1, off, cloud, LC.small(rows=128, cols=4096)) == 0
    assert _raw(1, off, cloud, LC.small(rows=129)) == UNSUPPORTED
    assert _raw(1, off, cloud, LC.small(cols=4097)) == UNSUPPORTED
    assert _raw(1, off, cloud, LC.small(using_sharp_point=1)) == UNSUPPORTED
    assert _raw(1, off, cloud, LC.small(deg_diff=0.08)) == 0            # half-width 7 + 1
    assert _raw(1, off, cloud, LC.small(deg_diff=0.07)) == UNSUPPORTED  # half-width 8 + 1
    with pytest.raises(SqlmError) as e:
        LF.features_host([cloud], LC.small(using_sharp_point=1))
    assert e.value.status == UNSUPPORTED
    # an empty batch and an empty sweep are fine
    o = LF.features_host([], P)
    assert list(o["less_off"]) == [0] and len(o["less_xyz"]) == 0
    o = LF.features_host([np.zeros((0, 3), np.float32), cloud], P)
    assert o["less_off"][1] == 0 and o["less_off"][2] == len(LC.reference("start_0")["less_xyz"])
