"""The host text of the LiDAR depth association (csrc/lidar_depth_dev.h) under
AddressSanitizer and UndefinedBehaviorSanitizer: tools/depth_check.cpp is a
stand-alone program (its own main, plain g++, neither HIP nor libsqrtlm.so) that
runs one frame on heap blocks of exactly the promised sizes. It is built here
with -fsanitize=address,undefined and run on the border, truncation, zw and
non-finite cases from files this test writes; its output equals the numpy
definition bit for bit and the sanitizers report nothing. Nothing is loaded into
Python under a sanitizer. Skips, with the reason, where the sanitizer runtime is
not installed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import lidar_depth_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
NAMES = ["borders_16", "borders_37", "truncation_16", "truncation_37", "zw", "one_by_one", "fractional", "uchar", "offsets",
         "x_thresholds", "min_v_half_top", "collide_65", "scattered_16", "keys_65", "empty_sweep", "empty_keys", "empty_both"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("depth_check")
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    why = ""
    for extra in (["-static-libasan", "-static-libubsan"], []):  # a static runtime starts beside any preloaded library
        r = subprocess.run([cxx] + SAN + extra + ["-o", str(d / "probe"), str(probe)], capture_output=True, text=True,
                           timeout=120)
        if r.returncode == 0:
            r = subprocess.run([str(d / "probe")], capture_output=True, text=True, timeout=60, env=ENV)
        if r.returncode == 0:
            break
        why = r.stderr.strip()[-200:]
    else:
        pytest.skip("the AddressSanitizer / UBSan runtime is not installed or does not start here: " + why)
    exe = d / "depth_check_san"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + SAN + extra
    cmd += ["-o", str(exe), os.path.join(ROOT, "tools", "depth_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe), d


def _write(path, c):
    un = c.cfg.cam is not None
    with open(path, "wb") as f:
        np.array([c.cfg.rows, c.cfg.cols, len(c.xyz), len(c.keys), int(un)], np.int32).tofile(f)
        np.ascontiguousarray(c.cfg.intrinsic, np.float64).tofile(f)
        np.ascontiguousarray(c.cfg.extrinsic, np.float64).tofile(f)
        np.asarray(c.cfg.cam if un else (0, 0, 0, 0), np.float32).tofile(f)
        np.ascontiguousarray(c.xyz, np.float32).tofile(f)
        np.ascontiguousarray(c.keys, np.float32).tofile(f)
        if un:
            np.ascontiguousarray(c.keys_un, np.float32).tofile(f)


def _read(path, c):
    un = c.cfg.cam is not None
    n, m, rows, cols = len(c.xyz), len(c.keys), c.cfg.rows, c.cfg.cols
    with open(path, "rb") as f:
        take = lambda dt, k: np.fromfile(f, dt, k)
        status = int(take(np.int32, 1)[0])
        o = dict(class_id=take(np.int32, m), depth=take(np.float32, m), nearest_uv=take(np.int32, 2 * m).reshape(m, 2))
        if un:
            o["xyz_cam"] = take(np.float32, 3 * m).reshape(m, 3)
        o.update(stats=take(np.int32, 4), pixel=take(np.int32, n), winner=take(np.int32, rows * cols).reshape(rows, cols),
                 image=take(np.float64, rows * cols).reshape(rows, cols))
        assert f.read() == b""
    return status, o


@pytest.mark.parametrize("name", NAMES)
def test_checked_host_text_equals_the_definition(program, name):
    exe, d = program
    c = LC.cases()[name]
    src, dst = str(d / (name + ".in")), str(d / (name + ".out"))
    _write(src, c)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    assert r.stdout.split()[:3] == ["ok", "status", "0"], r.stdout
    status, got = _read(dst, c)
    assert status == 0 and LC.differences(got, LC.reference(name)) == []


def test_the_checked_program_reports_argument_errors(program):
    exe, d = program
    c = LC.cases()["keys_1"]
    bad = LC.Case(LC.Cfg(c.cfg.rows, 4097, c.cfg.extrinsic, c.cfg.intrinsic, c.cfg.cam), c.xyz, c.keys, c.keys_un)
    src, dst = str(d / "bad.in"), str(d / "bad.out")
    _write(src, bad)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    assert np.fromfile(dst, np.int32).tolist() == [-8]
