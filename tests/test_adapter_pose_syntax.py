"""adapter/hipOptimizerPose.cc (hipOptimizer::PoseOptimization and the
Optimizer::PoseOptimization dispatch) compiles against the reference's
declarations: `g++ -fsyntax-only -Wall -Wextra -Werror` with the overlay
stand-ins of tests/adapter_syntax_pose/ (Frame, KdTreeFLANN::Ptr,
lidarConfig::corner_optimized_weight, the PoseOptimization declarations)
searched before the base stand-ins of tests/adapter_syntax/. Nothing is linked."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OVERLAY = os.path.join(ROOT, "tests", "adapter_syntax_pose")
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


def test_pose_adapter_compiles_against_reference_declarations():
    r = subprocess.run(_cmd(os.path.join(ROOT, "adapter", "hipOptimizerPose.cc")), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr


def test_header_declares_the_reference_signature():
    hdr = open(os.path.join(ROOT, "adapter", "hipOptimizer.h")).read()
    assert "static int PoseOptimization(Frame* pFrame, PointICloudPtr local_lidarmap_cloud_ptr," in hdr
    assert "typename Tree::Ptr kdtree_local_map, const lidarConfig* lidarconfig);" in hdr
    assert "template <typename Tree = pcl::KdTreeFLANN<PointI> >" in hdr


def test_a_wrong_call_is_rejected():
    """The check is a real compile: a call with a wrong argument fails it."""
    src = os.path.join(ROOT, "adapter", "hipOptimizerPose.cc")
    text = open(src).read().replace("th2, 0.0, q_out,\n", "th2, \"x\", q_out,\n", 1)
    assert text != open(src).read()
    r = subprocess.run(_cmd("-", ("-x", "c++", "-I" + os.path.join(ROOT, "adapter"))), input=text, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode != 0
