"""adapter/hipFrameDepth.cc (the LiDAR depth image and keypoint depth
association of the Frame constructor on sqlm_lidar_depth) compiles against the
reference's declarations: `g++ -fsyntax-only -Wall -Wextra -Werror` with the
overlay stand-ins of tests/adapter_syntax_depth/ (Frame, a minimal cv::Mat /
cv::KeyPoint) searched before the base stand-ins of tests/adapter_syntax/ (the
PCL cloud types, Eigen). Nothing is linked or run."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OVERLAY = os.path.join(ROOT, "tests", "adapter_syntax_depth")
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


def test_depth_adapter_compiles_against_reference_declarations():
    r = subprocess.run(_cmd(os.path.join(ROOT, "adapter", "hipFrameDepth.cc")), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr


def test_header_declares_the_entry_points():
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "adapter", "hipFrameDepth.h")).read())
    assert ("static bool AssociateDepth(Frame* pF, const Eigen::Matrix<double, 3, 4>& intrinsicMatrix, "
            "const Eigen::Matrix<double, 4, 4>& extrinsicMatrix);") in hdr
    assert "static bool UnprojectAll(Frame* pF," in hdr and "std::vector<cv::Point3f>& vP3Dc);" in hdr


def test_adapter_fills_the_members_the_constructor_fills():
    src = open(os.path.join(ROOT, "adapter", "hipFrameDepth.cc")).read()
    for member in ("pF->mvKeys[i].class_id = cls[i];", "pF->mvDepth[i] = depth[i];", "img.ptr<double>(0)"):
        assert member in src, member
    # the library call comes before any write to the frame: a failure leaves it untouched
    assert src.index("sqlm_lidar_depth(ctx") < src.index("pF->mvKeys[i].class_id =")
    assert src.index("return false;\n  }\n  if (!image.empty())") < src.index("pF->mvDepth[i] =")
