"""The host text of the LiDAR flat- and corner-feature extraction
(csrc/lidar_feat_host.h) under AddressSanitizer and UndefinedBehaviorSanitizer:
tools/corner_check.cpp is a stand-alone program (its own main, plain g++,
neither HIP nor libsqrtlm.so) that runs one sweep on heap blocks of exactly the
promised sizes. It is built here with -fsanitize=address,undefined and run on
the wrap, large-segment, cap and empty cases from files this test writes; its
output equals the numpy definition bit for bit and the sanitizers report
nothing. Nothing is loaded into Python under a sanitizer. Skips, with the
reason, where the sanitizer runtime is not installed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import lidar_corner_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
NAMES = ["column_wrap", "wall", "snake", "caps_1_1", "caps_2_5", "caps_3_0", "caps_0_0", "extrinsic", "empty"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("corner_check")
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
    exe = d / "corner_check_san"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + SAN + extra
    cmd += ["-o", str(exe), os.path.join(ROOT, "tools", "corner_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe), d


def _write(path, cloud, P, CP, ext):
    cloud = np.ascontiguousarray(cloud, np.float32).reshape(-1, 3)
    with open(path, "wb") as f:
        np.array([P.row_num, P.col_num, P.num_scan_subregions, P.num_curvature_regions_flat, P.num_curvature_regions_corner,
                  P.max_surf_flat, P.max_surf_less_flat, CP.max_corner_sharp, CP.max_corner_less_sharp, len(cloud),
                  int(ext is not None)], np.int32).tofile(f)
        np.array([P.surf_curv_th, P.max_sq_dis, P.deg_diff, CP.sharp_curv_th, CP.ground_z_bound], np.float64).tofile(f)
        np.ascontiguousarray(np.eye(4) if ext is None else ext, np.float64).tofile(f)
        P.enabled().astype(np.uint8).tofile(f)
        CP.enabled().astype(np.uint8).tofile(f)
        cloud.tofile(f)


def _read(path, n, P):
    S, C = P.row_num, P.col_num
    with open(path, "rb") as f:
        take = lambda dt, k: np.fromfile(f, dt, k)
        status = int(take(np.int32, 1)[0])
        if status != 0:
            assert f.read() == b""
            return status, None
        offs = [take(np.int64, 2) for _ in range(4)]
        kf, kl, ks, kc = (int(o[1]) for o in offs)
        full = dict(flat_xyz=take(np.float32, 3 * n).reshape(n, 3)[:kf], flat_normal=take(np.float32, 3 * n).reshape(n, 3)[:kf],
                    less_xyz=take(np.float32, 3 * n).reshape(n, 3)[:kl], less_normal=take(np.float32, 3 * n).reshape(n, 3)[:kl],
                    less_rc=take(np.int32, 2 * n).reshape(n, 2)[:kl], sharp_xyz=take(np.float32, 3 * n).reshape(n, 3)[:ks],
                    less_sharp_xyz=take(np.float32, 3 * n).reshape(n, 3)[:kc], less_sharp_label=take(np.int32, n)[:kc],
                    less_sharp_rc=take(np.int32, 2 * n).reshape(n, 2)[:kc])
        ns = int(take(np.int64, S + 1)[-1])
        full["corner_state"] = dict(cell_state=take(np.int32, S * C).reshape(S, C), mask=take(np.uint8, n)[:ns],
                                    curvature=take(np.float32, n)[:ns], sorted=take(np.int32, n)[:ns],
                                    reason=take(np.uint8, n)[:ns], edge=take(np.uint8, S * C).reshape(S, C),
                                    angle=take(np.float32, S * C * 6).reshape(S, C, 6))
        assert f.read() == b""
    return status, full


@pytest.mark.parametrize("name", NAMES)
def test_checked_host_text_equals_the_definition(program, name):
    exe, d = program
    cloud, P, CP, ext, _ = CC.cases()[name]
    src, dst = str(d / (name + ".in")), str(d / (name + ".out"))
    _write(src, cloud, P, CP, ext)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    assert r.stdout.split()[:3] == ["ok", "status", "0"], r.stdout
    status, got = _read(dst, len(cloud), P)
    assert status == 0 and CC.differences(got, CC.reference(name)) == []
    from sqrtlm import lidar_feat as LF
    import lidar_feat_cases as FC
    host = LF.features_all_host([cloud], P, CP, ext)
    assert all(FC.same(got[k], host[k]) for k in FC.OUT_KEYS)


def test_the_checked_program_reports_argument_errors(program):
    from dataclasses import replace
    exe, d = program
    cloud, P, CP, ext, _ = CC.cases()["caps_1_1"]
    src, dst = str(d / "bad.in"), str(d / "bad.out")
    for bad_p, bad_cp, want in ((replace(P, col_num=4097), CP, -8), (P, replace(CP, max_corner_sharp=-1), -1)):
        _write(src, cloud, bad_p, bad_cp, ext)
        r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120, env=ENV)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
        assert np.fromfile(dst, np.int32).tolist() == [want]
