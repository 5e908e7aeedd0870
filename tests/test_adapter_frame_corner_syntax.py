"""adapter/hipFrameLidarCorner.cc (both branches of Frame::ExtractFeaturePoints
on one sqlm_lidar_features_all call) compiles against the reference's
declarations: `g++ -fsyntax-only -Wall -Wextra -Werror` with the overlay
stand-ins of tests/adapter_syntax_frame_corner/ (Frame with its corner clouds,
lidarConfig with its corner fields) searched before the base stand-ins of
tests/adapter_syntax/. hipFrameLidar.cc, which defines the helpers both files
share, compiles against the same overlay. Nothing is linked."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OVERLAY = os.path.join(ROOT, "tests", "adapter_syntax_frame_corner")
STUBS = os.path.join(ROOT, "tests", "adapter_syntax")
INCLUDES = ["", "data_structure", "utils"]


def _cmd(src):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    cmd = [cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror"]
    for base in (OVERLAY, STUBS):
        cmd += ["-I" + os.path.join(base, d) for d in INCLUDES]
    return cmd + ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "adapter"), src]


@pytest.mark.parametrize("name", ["hipFrameLidarCorner.cc", "hipFrameLidar.cc"])
def test_adapter_compiles_against_reference_declarations(name):
    r = subprocess.run(_cmd(os.path.join(ROOT, "adapter", name)), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


def test_header_declares_the_entry_points():
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "adapter", "hipFrameLidar.h")).read())
    assert "static bool ExtractFeatures(Frame* pF);" in hdr
    assert "static bool ExtractFeatures(Frame* pF, const Eigen::Matrix<double, 4, 4>& extrinsicMatrix);" in hdr


def test_adapter_makes_one_call_and_fills_the_ring_range_as_the_python_params_do():
    src = open(os.path.join(ROOT, "adapter", "hipFrameLidarCorner.cc")).read()
    assert len(re.findall(r"sqlm_lidar_features_all\(", src)) == 1 and "sqlm_lidar_features(" not in src
    assert "c.lower_ring_num_sharp_point <= i + 1 && i < c.upper_ring_num_sharp_point" in src
    # the flat entry point is unchanged: it still declines using_sharp_point
    flat = open(os.path.join(ROOT, "adapter", "hipFrameLidar.cc")).read()
    assert "if (cfg.using_sharp_point) return false;" in flat
