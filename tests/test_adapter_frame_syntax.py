"""adapter/hipFrameLidar.cc (Frame::lidarProcess's flat-point path on
sqlm_lidar_features) compiles against the reference's declarations: `g++
-fsyntax-only -Wall -Wextra -Werror` with the overlay stand-ins of
tests/adapter_syntax_frame/ (Frame, lidarConfig) searched before the base
stand-ins of tests/adapter_syntax/ (the PCL cloud types, Eigen). Nothing is
linked."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OVERLAY = os.path.join(ROOT, "tests", "adapter_syntax_frame")
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


def test_frame_adapter_compiles_against_reference_declarations():
    r = subprocess.run(_cmd(os.path.join(ROOT, "adapter", "hipFrameLidar.cc")), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr


def test_header_declares_the_entry_point():
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "adapter", "hipFrameLidar.h")).read())
    assert "static bool ExtractFlatFeatures(Frame* pF);" in hdr
    assert "static bool ExtractFlatFeatures(Frame* pF, const Eigen::Matrix<double, 4, 4>& extrinsicMatrix);" in hdr


def test_adapter_fills_the_ring_ranges_as_the_python_params_do():
    """The fourth range's `lower <= i + 1 <= lower` is kept in both places."""
    src = open(os.path.join(ROOT, "adapter", "hipFrameLidar.cc")).read()
    assert "c.lower_ring_num_z_rot_xy_trans <= r && r <= c.lower_ring_num_z_rot_xy_trans" in src
