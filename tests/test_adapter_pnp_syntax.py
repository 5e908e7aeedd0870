"""adapter/hipPnPsolver.cc (the reference's PnPsolver interface on
sqlm_pnp_ransac) compiles against the reference's declarations:
`g++ -fsyntax-only -Wall -Wextra -Werror` with the overlay stand-ins of
tests/adapter_syntax_pnp/ (Frame::mvKeysUn, mvLevelSigma2, fx .. cy,
DUtils::Random) searched before the base stand-ins of tests/adapter_syntax/.
Nothing is linked."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OVERLAY = os.path.join(ROOT, "tests", "adapter_syntax_pnp")
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


def test_pnp_adapter_compiles_against_reference_declarations():
    r = subprocess.run(_cmd(os.path.join(ROOT, "adapter", "hipPnPsolver.cc")), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr


def test_header_declares_the_reference_interface():
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "adapter", "hipPnPsolver.h")).read())
    for decl in (
            "hipPnPsolver(const Frame& F, const std::vector<MapPoint*>& vpMapPointMatches);",
            "void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, "
            "int minSet = 4, float epsilon = 0.4, float th2 = 5.991);",
            "cv::Mat find(std::vector<bool>& vbInliers, int& nInliers);",
            "cv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers);",
            "static bool SolveBatch(const std::vector<hipPnPsolver*>& vpSolvers);"):
        assert decl in hdr, decl
