"""bench.py's command line: a plain run times the steps and prints the headline
line only, `--full` adds the rest, `--dump-outputs DIR` writes what the timed
steps computed (bounded in size, the same sample on every run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("kernel_ms_per_step", "roofline", "roofline_secondary", "final_rmse_px", "end_to_end", "cpu_baseline",
             "cpu_baseline_multithread", "extra_workloads")


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--scale", "0.002",
                        "--steps", "3", "--warmup", "1", *args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_dump_outputs_small_arrays_whole(tmp_path):
    a = np.arange(12, dtype=np.float64).reshape(4, 3)
    bench.dump_outputs(str(tmp_path / "d"), {"a": a, "n": np.array([3], dtype=np.int32)})
    assert np.array_equal(np.load(tmp_path / "d" / "a.npy"), a)
    n = np.load(tmp_path / "d" / "n.npy")
    assert n.dtype == np.float32 and n.tolist() == [3.0]


def test_dump_outputs_bounded_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4096)
    big = np.arange(3000, dtype=np.float64).reshape(1000, 3)
    small = np.ones(5, dtype=np.float32)
    for d in ("x", "y"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    x, y = np.load(tmp_path / "x" / "big.npy"), np.load(tmp_path / "y" / "big.npy")
    assert np.array_equal(x, y) and x.dtype == np.float64 and 0 < len(x) < 1000
    assert x.nbytes + small.nbytes <= 4096
    assert np.array_equal(x[:, 1], x[:, 0] + 1) and np.all(np.diff(x[:, 0]) > 0)  # whole rows, in order
    assert np.array_equal(np.load(tmp_path / "x" / "small.npy"), small)


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_outputs(tmp_path):
    d = tmp_path / "out"
    line = _bench("--dump-outputs", str(d))
    for k in HEADLINE:
        assert k in line, k
    assert not [k for k in FULL_ONLY if k in line]
    assert line["steps"] == 3 and line["warmup"] == 1 and line["dtype"] == "f64"
    assert np.isclose(line["value"], 1000.0 / line["ms_per_step"])
    n_pose, n_pt = line["config"]["n_pose"], line["config"]["n_landmark"]
    q, t, X = (np.load(d / f"{n}.npy") for n in ("pose_q", "pose_t", "points"))
    assert q.shape == (n_pose, 4) and t.shape == (n_pose, 3) and X.shape == (n_pt, 3)
    assert q.dtype == t.dtype == X.dtype == np.float64
    assert np.allclose(np.linalg.norm(q, axis=1), 1.0, atol=1e-9) and np.all(np.isfinite(X))
    assert np.load(d / "chi2_end.npy").tolist() == [line["chi2_last"]]


@pytest.mark.gpu
def test_full_run_keeps_the_other_figures():
    line = _bench("--full")
    for k in HEADLINE + ("kernel_ms_per_step", "roofline", "roofline_secondary", "final_rmse_px", "end_to_end",
                         "cpu_baseline", "cpu_baseline_multithread"):
        assert k in line, k
    assert "k_rcs_tile" in line["kernel_ms_per_step"] and line["final_rmse_px"] > 0
