"""How far the plane fit of the LiDAR flat-feature extraction is from the exact
least-squares plane. On generated scenes with planted planes (a ground plane,
walls, boxes) the less-flat normals of the host twin are compared with a
np.longdouble solve of A n = -1 on the same near points (the definition's
Householder steps in extended precision), and the picked set with the set the
longdouble evaluation picks.

Measured on these scenes: the largest deviation of a stored normal component is
2.98e-08, half an ulp of a float near 1: the stored normal is the float nearest
to the extended-precision one or its neighbour. The double QR itself is within
3.71e-12 of the extended one before the rounding to float (the near points lie 4 to
60 m from the origin on patches under a metre wide: A's condition number is about 1e4). The test's bounds are
these figures times 100, as for the first-trial tests: the result sits on a
different rounding path, not a different formula."""
import numpy as np

import lidar_feat_ref as R
from sqrtlm import lidar_feat as LF

LD = np.longdouble
MEASURED_STORED = 2.98e-08   # |float normal - longdouble normal|, largest component
MEASURED_DOUBLE = 3.71e-12   # |double normal - longdouble normal| before the rounding to float
MARGIN = 100.0
SEEDS = (61, 62, 63)
COLS = 600


def _ld_plane(near):
    """(unit normal, worst residual) of the near points in longdouble; None when degenerate."""
    A = [[LD(v) for v in r] for r in near]
    x = R.qr_solve(A, [LD(-1.0)] * len(A), sqrt=np.sqrt)
    if x is None:
        return None
    x = np.array(x, LD)
    nrm = np.sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2])
    n, d0 = x / nrm, LD(1.0) / nrm
    res = max(abs(n[0] * r[0] + n[1] * r[1] + n[2] * r[2] + d0) for r in A)
    return n, res


def _double_plane(near):
    A = [[float(v) for v in r] for r in near]
    x = R.qr_solve(A, [-1.0] * len(A))
    nrm = np.sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2])
    return np.array([x[0] / nrm, x[1] / nrm, x[2] / nrm])


def _evaluate(seed):
    cloud = LF.make_sweep(seed, n_az=COLS, order="azimuth", start_deg=11.0 * seed)
    P = LF.Params(col_num=COLS)
    o = LF.features_host([cloud], P, state=True)
    st = o["state"]
    ring, image_index, src, cols, scans = R.image_of(cloud, P)
    off = st["scan_off"]
    assert np.array_equal(np.diff(off), [len(s) for s in scans])
    got = {(int(r), int(c)): n for (r, c), n in zip(o["less_rc"], o["less_normal"])}
    dev_stored = dev_double = 0.0
    n_cand = n_left = 0
    want_picked, got_picked, excluded = set(), set(got), set()
    ncr = P.num_curvature_regions_flat
    for r in range(P.row_num):
        m = len(scans[r])
        if not P.enabled()[r] or m <= R.min_scan(P):
            continue
        base = int(off[r])
        for j in range(P.num_scan_subregions):
            sp, ep = R.region(m, ncr, P.num_scan_subregions, j)
            if ep <= sp:
                continue
            order = st["sorted"][base + sp:base + ep + 1]
            picked = 0
            for k, idx in enumerate(order):
                idx = int(idx)
                n_cand += 1
                if st["mask"][base + idx]:
                    continue
                cv = float(st["curvature"][base + idx])
                if abs(cv - P.surf_curv_th) <= 1e-4 * P.surf_curv_th:
                    n_left += len(order) - k   # the walk may part ways here: the rest of the subregion is left out
                    break
                if not cv < P.surf_curv_th:
                    continue
                n_search, near = R.near_points(image_index, scans, cols, r, idx, P)
                if n_search < 5 or len(near) < 3:
                    continue
                fit = _ld_plane(near)
                if fit is None:
                    continue
                n, res = fit
                if abs(res - LD(0.1)) <= LD(1e-4) * LD(0.1):
                    n_left += len(order) - k
                    break
                if res > LD(0.1):
                    continue
                key = (r, int(cols[r][idx]))
                want_picked.add(key)
                if key in got:
                    dev_stored = max(dev_stored, float(np.max(np.abs(got[key].astype(LD) - n))))
                    dev_double = max(dev_double, float(np.max(np.abs(_double_plane(near).astype(LD) - n))))
                picked += 1
                if picked >= P.max_surf_less_flat:
                    break
            else:
                continue
            if picked < P.max_surf_less_flat:  # the walk ended at a borderline candidate: the subregion is not compared
                excluded |= {(r, int(cols[r][int(i)])) for i in order}
    want_picked, got_picked = want_picked - excluded, got_picked - excluded
    return dict(dev_stored=dev_stored, dev_double=dev_double, n_cand=n_cand, n_left=n_left, want=want_picked,
                got=got_picked, n_less=len(got))


def test_less_flat_normals_against_a_longdouble_least_squares_plane():
    worst_stored = worst_double = 0.0
    for seed in SEEDS:
        e = _evaluate(seed)
        print("seed %d: %d less-flat points, %d candidates, %d left out, deviation stored %.3e double %.3e"
              % (seed, e["n_less"], e["n_cand"], e["n_left"], e["dev_stored"], e["dev_double"]))
        assert e["n_less"] > 300
        assert e["n_left"] <= 0.05 * e["n_cand"]
        assert e["want"] == e["got"]
        worst_stored, worst_double = max(worst_stored, e["dev_stored"]), max(worst_double, e["dev_double"])
    print("largest deviation: stored %.3e, double %.3e" % (worst_stored, worst_double))
    assert worst_stored <= MARGIN * MEASURED_STORED
    assert worst_double <= MARGIN * MEASURED_DOUBLE
