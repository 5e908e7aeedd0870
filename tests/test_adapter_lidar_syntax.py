"""adapter/hipOptimizer.cc hands the pass-3 LiDAR association to the library:
no PCL kd-tree or cloud transform is left in the LBA adapter, and its call of
sqlm_set_lidar_from_clouds is a real compile against include/sqrtlm.h (the
stand-ins of tests/adapter_syntax/ need no overlay for it)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUBS = os.path.join(ROOT, "tests", "adapter_syntax")
INCLUDES = ["", "data_structure", "utils", "backend"]
SRC = os.path.join(ROOT, "adapter", "hipOptimizer.cc")


def test_lba_adapter_is_free_of_the_kd_tree():
    text = open(SRC).read()
    for gone in ("KdTreeFLANN", "transformPointCloud", "kdtree_flann.h", "nearestKSearch"):
        assert gone not in text, gone
    assert "sqlm_set_lidar_from_clouds(ctx, g.kf_index.at(pKF)" in text
    assert "cv::Mat(4, 4, CV_32F, T).inv()" in text  # the float pose path stays OpenCV's


def test_a_wrong_call_is_rejected():
    """Dropping the normals from the call fails the compile."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    text = open(SRC).read()
    broken = text.replace("cur_Twc, nrm.data(), cfg->flat_optimized_weight,", "cur_Twc, cfg->flat_optimized_weight,", 1)
    assert broken != text
    cmd = [cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-x", "c++"]
    cmd += ["-I" + os.path.join(STUBS, d) for d in INCLUDES] + ["-I" + os.path.join(ROOT, "include"), "-"]
    ok = subprocess.run(cmd, input=text, capture_output=True, text=True, timeout=120)
    assert ok.returncode == 0, ok.stderr
    bad = subprocess.run(cmd, input=broken, capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0
