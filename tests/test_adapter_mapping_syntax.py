"""adapter/hipLocalMapping.cc (the match loop of CreateNewMapPoints on
sqlm_triangulate_pairs, the map-point refresh on sqlm_map_points_update)
compiles against the reference's declarations: `g++ -fsyntax-only -Wall -Wextra
-Werror` with the overlay stand-ins of tests/adapter_syntax_mapping/ (KeyFrame,
MapPoint with the two added setters, Map, cv::Mat::row) searched before the
base stand-ins of tests/adapter_syntax/. Nothing is linked."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OVERLAY = os.path.join(ROOT, "tests", "adapter_syntax_mapping")
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


def test_mapping_adapter_compiles_against_reference_declarations():
    r = subprocess.run(_cmd(os.path.join(ROOT, "adapter", "hipLocalMapping.cc")), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr


def test_header_declares_the_two_entry_points():
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "adapter", "hipLocalMapping.h")).read())
    for decl in (
            "static int TriangulateMatches(KeyFrame* pKF1, KeyFrame* pKF2, "
            "const std::vector<std::pair<size_t, size_t> >& vMatchedIndices, float ratioFactor, Map* pMap, "
            "std::vector<MapPoint*>& vpNewMapPoints);",
            "static bool UpdateMapPoints(const std::vector<MapPoint*>& vpMapPoints);"):
        assert decl in hdr, decl
