"""The float edge angle of the corner branch against a longdouble evaluation.

Three generated scenes (random occupancy of an 8 x 256 image at three range
levels with 0.02 % jitter, seeds with partners as in tests/lidar_corner_cases.py):
the angle of every candidate edge is evaluated in np.longdouble from the same
float points, the largest |float angle - longdouble angle| is printed, and the
margin is 100 times that measured value, the project's usual factor over a
reference's own rounding spread; it is measured against the longdouble
evaluation, not against the library. The scenes are chosen (and checked here)
so that no edge has its longdouble angle within the margin of 1: equal ranges
give angles near pi/2, range jumps angles near the angular step. Then the edge
bits, the segments and the picked sets of the definition equal those of the
longdouble evaluation exactly, nothing excluded, and the host twin equals both."""
import numpy as np
import pytest

import lidar_corner_cases as CC
import lidar_corner_ref as CR
import lidar_feat_ref as R
from sqrtlm import lidar_feat as LF

ld = np.longdouble
SEEDS = (1, 2, 3)


def angle_ld(p1, p2):
    a, b = np.asarray(p1, np.float32).astype(ld), np.asarray(p2, np.float32).astype(ld)
    n1 = np.sqrt((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2])
    n2 = np.sqrt((b[..., 0] * b[..., 0] + b[..., 1] * b[..., 1]) + b[..., 2] * b[..., 2])
    dot = (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    d1, d2 = np.maximum(n1, n2), np.minimum(n1, n2)
    alpha = np.arccos(np.clip(dot / (n1 * n2), -1, 1))
    return np.arctan2(d2 * np.sin(alpha), d1 - d2 * np.cos(alpha))


def scene(seed):
    rng = np.random.default_rng(seed)
    g = CC.Grid(8, 256)
    seeds = {1: (16, 48, 80, 112), 3: (32, 64, 96, 128)}
    reserved = {(r, c + dc) for r, cs in seeds.items() for c in cs for dc in (0, 1, 2)}
    reserved |= {(r + dr, c + 2) for r, cs in seeds.items() for c in cs for dr in (-1, 1)}
    for r, cs in seeds.items():
        g.pad(r, 200)
        for k, c in enumerate(cs):
            g.seed(r, c, 206 + 6 * k)
        g.pad(r, 250)
    levels = (CC.BASE, CC.FAR, CC.FILL)
    for r in range(8):
        for c in range(0, 180):
            if (r, c) in reserved or (r, c) in g.cells or rng.random() < 0.35:
                continue
            g.add(r, c, levels[int(rng.integers(0, 3 if rng.random() < 0.3 else 1))] * (1.0 + rng.uniform(-0.0002, 0.0002)))
    return g.cloud(), CC.P_small(8, 256), CC.CP_open()


@pytest.fixture(scope="module")
def evaluated():
    out = []
    for seed in SEEDS:
        cloud, P, CP = scene(seed)
        image = R.image_of(cloud, P)
        seen = {}

        def both(p1, p2):
            x = angle_ld(p1, p2)
            seen.setdefault("ld", []).append(x)
            seen.setdefault("f32", []).append(CR.angle(p1, p2))
            return x

        exact = CR.process(cloud, P, CP, angle_fn=both, image=image)
        out.append((cloud, P, CP, image, exact, np.concatenate(seen["ld"]), np.concatenate(seen["f32"])))
    return out


def test_float_angle_decides_every_edge_as_the_longdouble_angle(evaluated):
    err = max(float(np.nanmax(np.abs(f.astype(ld) - l))) for *_, l, f in evaluated)
    margin = 100.0 * err
    print(f"largest |float angle - longdouble angle| {err:.3e}, margin {margin:.3e}")
    assert 0.0 < margin < 0.05
    for cloud, P, CP, image, exact, l, f in evaluated:
        assert len(l) > 3000 and (l > 1).sum() > 500 and (l < 1).sum() > 100
        nearest = float(np.nanmin(np.abs(l - 1)))
        print(f"edges {len(l)}, nearest longdouble angle to 1: {nearest:.3e}")
        assert nearest > margin  # the condition: no edge of the chosen scenes within the margin of 1
        got = CR.process(cloud, P, CP, image=image)
        assert exact["stats"]["cells_labelled"] > 0 and exact["stats"]["cells_unstable"] > 0
        for k in CC.OUT_KEYS:
            assert CC.same(got[k], exact[k]), k
        for k in ("edge", "cell_state", "reason", "sorted", "mask"):
            assert CC.same(got["corner_state"][k], exact["corner_state"][k]), k
        host = LF.features_all_host([cloud], P, CP, state=True)
        assert not CC.differences(CC.slice_of(host, 0, P), got)
