"""adapter/hipOptimizerSim3.cc (hipOptimizer::OptimizeSim3 and the
Optimizer::OptimizeSim3 dispatch) compiles against the reference's
declarations: `g++ -fsyntax-only -Wall -Wextra -Werror` with the overlay
stand-ins of tests/adapter_syntax_sim3/ (KeyFrame::mK,
MapPoint::GetIndexInKeyFrame, the OptimizeSim3 declarations) searched before
the base stand-ins of tests/adapter_syntax/. Nothing is linked."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OVERLAY = os.path.join(ROOT, "tests", "adapter_syntax_sim3")
STUBS = os.path.join(ROOT, "tests", "adapter_syntax")
INCLUDES = ["", "data_structure", "utils", "backend"]


def _cmd(src, extra=()):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    cmd = [cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", *extra]
    for base in (OVERLAY, STUBS):
        cmd += ["-I" + os.path.join(base, d) for d in INCLUDES]
    return cmd + ["-I" + os.path.join(ROOT, "include"), src]


def test_sim3_adapter_compiles_against_reference_declarations():
    r = subprocess.run(_cmd(os.path.join(ROOT, "adapter", "hipOptimizerSim3.cc")), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr


def test_header_declares_the_reference_signature():
    hdr = open(os.path.join(ROOT, "adapter", "hipOptimizer.h")).read()
    assert "static int OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches1," in hdr
    assert "g2o::Sim3& g2oS12, const float th2, const bool bFixScale);" in hdr
