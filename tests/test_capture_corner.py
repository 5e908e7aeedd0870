"""The per-edge LiDAR kind in capture files (optional section "LIDK", one byte
per pair): round trip, files without the section (the committed fixtures among
them) reading as all flat, a value above 1 rejected. GPU: a replay with kinds
is the library's local BA on the same graph with sqlm_set_lidar_kind.
"""
import os

import numpy as np
import pytest

from sqrtlm import capture, synth

HERE = os.path.dirname(os.path.abspath(__file__))


def _capture(oracle, kinds=True):
    from capture_util import problem_to_capture
    prob = synth.add_lidar_flat(synth.make_problem(6, 50, pair_window=3, seed=1), 5, 40)
    c = problem_to_capture(prob, capture.LBA, oracle)
    if kinds:
        c.lid_kind = (np.arange(c.n_lid) % 3 == 1).astype(np.uint8)
    return c


def test_roundtrip_with_kinds(tmp_path, oracle):
    c = _capture(oracle)
    p = tmp_path / "k.sqcap"
    capture.write(p, c)
    b = capture.read(p)
    assert b.lid_kind is not None and b.lid_kind.dtype == np.uint8 and np.array_equal(b.lid_kind, c.lid_kind)
    assert b.lid_kind.any() and not b.lid_kind.all()
    for name in ("lid_pose", "lid_pc", "lid_pw", "lid_n", "lid_info"):
        assert np.array_equal(getattr(b, name), getattr(c, name)), name


def test_absent_section_reads_as_all_flat(tmp_path, oracle):
    c = _capture(oracle, kinds=False)
    p = tmp_path / "f.sqcap"
    capture.write(p, c)
    blob = p.read_bytes()
    assert b"LIDK" not in blob and b"LIDI" in blob
    assert capture.read(p).lid_kind is None
    # the committed fixtures predate the section
    for name in ("lba_capture.sqcap", "gba_stereo_capture.sqcap"):
        assert b"LIDK" not in open(os.path.join(HERE, "golden", name), "rb").read()
        assert capture.read(os.path.join(HERE, "golden", name)).lid_kind is None
    # with kinds the file is the same file plus one section of 16 + n_lid bytes
    k = _capture(oracle)
    capture.write(p, k)
    assert len(p.read_bytes()) == len(blob) + 16 + k.n_lid


def test_reader_rejects_a_kind_above_one(tmp_path, oracle):
    from sqrtlm._lib import SqlmError
    c = _capture(oracle)
    c.lid_kind = c.lid_kind.copy()
    c.lid_kind[2] = 2
    p = tmp_path / "bad.sqcap"
    capture.write(p, c)
    with pytest.raises(SqlmError):
        capture.read(p)


@pytest.mark.gpu
def test_replay_applies_the_kinds(gpu_ctx, oracle, tmp_path):
    from capture_util import capture_to_problem
    c = _capture(oracle)
    p = tmp_path / "k.sqcap"
    capture.write(p, c)
    cap = capture.read(p)
    out = capture.replay(gpu_ctx, cap)
    prob, edge_of, pt_src = capture_to_problem(cap, oracle)
    prob.lid_kind = cap.lid_kind
    prob.validate()
    gpu_ctx.set_problem(prob)
    ran, outl, st = gpu_ctx.local_ba()
    assert ran and out["ran"]
    assert np.array_equal(out["chi2"][edge_of], gpu_ctx.edge_chi2()) and np.array_equal(out["outlier"][edge_of], outl)
    assert [s["trials"] for s in out["stats"]] == [s["trials"] for s in st]
    assert out["stats"][2]["chi2_end"] == st[2]["chi2_end"]
    flat = capture.replay(gpu_ctx, _capture(oracle, kinds=False))
    assert flat["stats"][2]["chi2_end"] != out["stats"][2]["chi2_end"]
