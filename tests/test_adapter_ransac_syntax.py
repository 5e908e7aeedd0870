"""adapter/hipSim3Solver.cc (the reference's Sim3Solver interface on
sqlm_sim3_ransac) compiles against the reference's declarations:
`g++ -fsyntax-only -Wall -Wextra -Werror` with the overlay stand-ins of
tests/adapter_syntax_ransac/ (KeyFrame::mvLevelSigma2 and mK,
MapPoint::GetIndexInKeyFrame, DUtils::Random) searched before the base
stand-ins of tests/adapter_syntax/. Nothing is linked."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OVERLAY = os.path.join(ROOT, "tests", "adapter_syntax_ransac")
STUBS = os.path.join(ROOT, "tests", "adapter_syntax")
INCLUDES = ["", "data_structure", "utils", "backend"]


def _cmd(src, extra=()):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    cmd = [cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", *extra]
    for base in (OVERLAY, STUBS):
        cmd += ["-I" + os.path.join(base, d) for d in INCLUDES]
    return cmd + ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "adapter"), src]


def test_ransac_adapter_compiles_against_reference_declarations():
    r = subprocess.run(_cmd(os.path.join(ROOT, "adapter", "hipSim3Solver.cc")), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr


def test_header_declares_the_reference_interface():
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "adapter", "hipSim3Solver.h")).read())
    for decl in (
            "hipSim3Solver(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<MapPoint*>& vpMatched12, "
            "const bool bFixScale = true);",
            "void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300);",
            "cv::Mat find(std::vector<bool>& vbInliers12, int& nInliers);",
            "cv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers);",
            "cv::Mat GetEstimatedRotation();", "cv::Mat GetEstimatedTranslation();", "float GetEstimatedScale();",
            "static bool SolveBatch(const std::vector<hipSim3Solver*>& vpSolvers);"):
        assert decl in hdr, decl
