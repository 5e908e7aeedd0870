"""adapter/hipOptimizerLidar.cc (LocalBundleAdjustment pass 3 with
using_sharp_point: the flat and the corner search as one
sqlm_set_lidar_from_cloud_sets call) compiles against the reference's
declarations: `g++ -fsyntax-only -Wall -Wextra -Werror` with the overlay
stand-ins of tests/adapter_syntax_lidar/ (KeyFrame::corner_points_less_sharp_,
lidarConfig::corner_optimized_weight) searched before the base stand-ins of
tests/adapter_syntax/. Nothing is linked. The g2o fallback of
hipOptimizer::LocalBundleAdjustment is gone."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OVERLAY = os.path.join(ROOT, "tests", "adapter_syntax_lidar")
STUBS = os.path.join(ROOT, "tests", "adapter_syntax")
INCLUDES = ["", "data_structure", "utils", "backend"]
SRC = os.path.join(ROOT, "adapter", "hipOptimizerLidar.cc")


def _cmd(src, extra=()):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    cmd = [cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", *extra]
    for base in (OVERLAY, STUBS):
        cmd += ["-I" + os.path.join(base, d) for d in INCLUDES]
    return cmd + ["-I" + os.path.join(ROOT, "include"), src]


def test_lidar_adapter_compiles_against_reference_declarations():
    r = subprocess.run(_cmd(SRC), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


def test_main_adapter_compiles_against_the_overlay_too():
    r = subprocess.run(_cmd(os.path.join(ROOT, "adapter", "hipOptimizer.cc")), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


def test_a_wrong_call_is_rejected():
    """The check is a real compile: the corner set without its weight fails it."""
    text = open(SRC).read()
    broken = text.replace("corner_q, nullptr, cfg->corner_optimized_weight);", "corner_q, nullptr);", 1)
    assert broken != text
    r = subprocess.run(_cmd("-", ("-x", "c++", "-I" + os.path.join(ROOT, "adapter"))), input=broken, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode != 0


def test_no_g2o_fallback_for_corner_points():
    lba = open(os.path.join(ROOT, "adapter", "hipOptimizer.cc")).read()
    assert "g2oOptimizer::" not in lba and "g2oOptimizer.h" not in lba
    assert "not implemented by libsqrtlm" not in lba
    assert "hipOptimizer::LidarCloudSets(ctx, pKF, map_kfs, g.kf_index.at(pKF)" in lba
    src = open(SRC).read()
    assert "g2oOptimizer::" not in src and len(re.findall(r"sqlm_set_lidar_from_cloud_sets\(", src)) == 1
    hdr = open(os.path.join(ROOT, "adapter", "hipOptimizer.h")).read()
    assert "static void CaptureLidarCorner(const Eigen::Vector3d& curr_point, const Eigen::Vector3d& near_point," in hdr
