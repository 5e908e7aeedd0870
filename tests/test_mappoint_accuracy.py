"""The triangulation of sqlm_triangulate_pairs against independent mathematics
(CPU). The library defines cv::SVD::compute of the 4x4 A as a fixed-sweep
one-sided Jacobi SVD; here x3D of every match of the cases that passes the
parallax test is compared with the null vector numpy.linalg.svd (LAPACK) finds
for the same float A, taken through the same float division by w.

Bound: K x spread with K = 100, the project's constant
(tests/test_pnp_ransac_accuracy.py). The spread of a match is the definition's
own largest movement under eight seeded +-1-ulp perturbations of A's float
entries, floored at 4 eps32; both relative to |x3D|. A with a non-finite entry
("inf_translation") has no SVD to compare with and is left out; "w_zero" stores
no point. Planted noise-free points must be recovered within the same bound of
the truth. Largest measured ratios: DESIGN.md 8h.
"""
import numpy as np
import pytest

import mappoint_cases as MC
import mappoint_ref as R
from sqrtlm import mappoint as M

K = 100.0
EPS32 = float(np.finfo(np.float32).eps)


def _x3d(A):
    x4, _ = R.null_vector(A)
    return R.divide_w(x4).astype(np.float64)


def _spread(A, X, seed):
    rng = np.random.default_rng(seed)
    scale = np.linalg.norm(X)
    s = 4 * EPS32
    for _ in range(8):
        S = rng.choice([-1.0, 1.0], 16).astype(np.float32)
        Ap = (A + S * np.spacing(np.abs(A))).astype(np.float32)
        s = max(s, float(np.linalg.norm(_x3d(Ap) - X) / scale))
    return s


def _svd_x3d(A):
    vt = np.linalg.svd(A.astype(np.float64).reshape(4, 4))[2]
    return R.divide_w(vt[3].astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("name", MC.tri_names())
def test_x3d_equals_the_lapack_null_vector_within_the_spread(name):
    s = MC.tri_slice(name)
    worst = 0.0
    for i, A in enumerate(s["A"]):
        if A is None or s["reason"][i] == 2 or not np.isfinite(A).all():
            continue
        X = s["x3d"][i].astype(np.float64)
        assert np.array_equal(X, _x3d(A))
        spread = _spread(A, X, 1000 + i)
        err = float(np.linalg.norm(_svd_x3d(A) - X) / np.linalg.norm(X))
        worst = max(worst, err / spread)
        assert err <= K * spread, (name, i, err, spread)
    print(f"{name}: largest error / spread {worst:.3g}")


def test_noise_free_points_are_recovered_within_the_spread():
    worst = 0.0
    for seed, n in ((1, 40), (2, 40)):
        p = M.make_two_view(n, seed=seed, pixel_noise=0.0)
        r = R.triangulate_pairs([p], keep_A=True)
        assert (r["reason"] == 0).all()
        for i in range(n):
            X, truth = r["x3d"][i].astype(np.float64), p.meta["X"][i]
            spread = _spread(r["A"][i], X, 2000 + i)
            err = float(np.linalg.norm(truth - X) / np.linalg.norm(X))
            worst = max(worst, err / spread)
            assert err <= K * spread, (seed, i, err, spread)
    print(f"noise-free: largest error / spread {worst:.3g}")
