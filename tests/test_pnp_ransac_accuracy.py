"""The library's EPnP against independent mathematics, on the CPU (the kernels'
text compiled for the host; the GPU equals it bit for bit,
tests/test_gpu_pnp_ransac.py). Three stages.

Eigen stage.

For every hypothesis and every refine of every case: the 12 eigenvalues the
library stores against numpy.linalg.eigvalsh(M^T M), the residuals
|M^T M v - lambda v| of its 12 eigenvectors and |V^T V - I|. The bound is
K x spread with K = 100, the project's constant (tests/test_gpu_first_trial.py).
The spread is the larger of eigvalsh's own largest change under eight seeded
+-1-ulp perturbations of M^T M and 4 eps64 lambda_max; |V^T V - I| is
dimensionless and is held to that bound divided by lambda_max. The eigenvectors
themselves are not compared: in the null space of a 4-point M^T M (dimension 4
or more) they are an arbitrary basis, which is why the library defines its own.

Downstream of the library's own ut. Betas, R, t and the reprojection errors of
every hypothesis and refine against the longdouble restatement
(pnp_ransac_ref.downstream in longdouble) from the same ut, control points and
inputs. Bound K x spread, the rule of tests/test_gpu_sim3_ransac.py: the spread
is the larger of the float64 definition's own distance from the longdouble
result and the longdouble result's largest change under eight seeded +-1-ulp
perturbations of its inputs, floored at 4 eps64; each quantity relative to its
own largest entry. No hypothesis is left out. Where a perturbation flips a
branch (a sign rule, the candidate choice, a NaN) the spread of that hypothesis
is large or not finite and the bound holds by construction; bit-equality with
the definition pins those.

Where EPnP is unique: the refine on 10 or more planted inliers in general
position against an independent EPnP written here from the algorithm with
numpy.linalg.eigh, lstsq and svd. R and t, each relative to its own largest
entry, within K x that independent solver's own spread under eight seeded
+-1-ulp perturbations of its inputs, floored at 4 eps64.
"""
import numpy as np
import pytest

import pnp_ransac_cases as PC
import pnp_ransac_ref as R
from sqrtlm import pnp

K = 100.0
EPS = float(np.finfo(np.float64).eps)


def _mtm(p, who):
    pw, uv = p.Xw[who][None].astype(np.float64), p.uv[who][None].astype(np.float64)
    with np.errstate(all="ignore"):
        cws, cci = R.control_points(pw)
        return R.mtm(pw, uv, np.asarray(p.intr, np.float64), cws, cci)[0]


def _check(A, ut, eig, what):
    ref = np.linalg.eigvalsh(A)[::-1]
    rng = np.random.default_rng(11)
    spread = 4 * EPS * abs(ref[0])
    for _ in range(8):
        S = rng.choice([-1.0, 1.0], A.shape)
        S = np.triu(S) + np.triu(S, 1).T                 # the perturbed matrix stays symmetric
        spread = max(spread, float(np.abs(np.linalg.eigvalsh(A + S * np.spacing(np.abs(A)))[::-1] - ref).max()))
    bound = K * spread
    assert np.abs(eig - ref).max() <= bound, (what, "eigenvalues", np.abs(eig - ref).max() / spread)
    res = np.linalg.norm(A @ ut.T - ut.T * eig[None, :], axis=0).max()
    assert res <= bound, (what, "residual", res / spread)
    orth = np.abs(ut @ ut.T - np.eye(12)).max()
    assert orth <= bound / abs(ref[0]), (what, "orthogonality", orth * abs(ref[0]) / spread)


@pytest.mark.parametrize("name", PC.NAMES)
def test_eigen_stage_against_eigvalsh(name):
    c, r = PC.case(name), PC.reference(name)
    p = c["problem"]
    for h in range(c["n_hyp"]):
        o = pnp.hypothesis_host(p, c["draws"][h])
        _check(_mtm(p, o["idx"]), o["ut"], o["eig"], (name, "hypothesis", h))
    for h in r["refined"]:
        o = pnp.refine_host(p, r["mask"][h])
        _check(_mtm(p, np.flatnonzero(r["mask"][h])), o["ut"], o["eig"], (name, "refine", h))


LD = np.longdouble
_QUANT = ("betas", "R", "t", "rep")


def _pick(d, chosen):
    """betas (H,3,4), R, t of the given candidate, rep (H,3) of a downstream result."""
    hh = np.arange(d["rep"].shape[0])
    return dict(betas=d["betas"], R=d["Rs"][hh, chosen], t=d["ts"][hh, chosen], rep=d["rep"])


def _rel(a, b, scale):
    """max |a - b| per hypothesis over the trailing axes, relative to scale; inf where either is not finite."""
    with np.errstate(all="ignore"):
        e = np.abs(a.astype(LD) - b.astype(LD)).reshape(a.shape[0], -1).max(axis=1) / scale
    return np.where(np.isfinite(e), e, np.inf).astype(np.float64)


def _downstream_check(r, pw32, uv32, K_, lib, what):
    """lib: the library's betas, R, t, rep (H leading) and chosen; r: the float64 definition of the same solves."""
    chosen = lib["chosen"]
    ld = _pick(R.downstream_ld(r, pw32, uv32, K_), chosen)
    f64 = _pick(r, chosen)
    rng = np.random.default_rng(13)
    pert = [_pick(R.downstream_ld(r, pw32, uv32, K_, perturb=lambda a: (
        rng.choice([-1.0, 1.0], a.shape) * np.spacing(np.abs(a.astype(np.float64)))).astype(LD)), chosen)
        for _ in range(8)]
    for q in _QUANT:
        with np.errstate(all="ignore"):
            scale = np.abs(ld[q]).reshape(ld[q].shape[0], -1).max(axis=1)
            scale = np.where(np.isfinite(scale) & (scale > 0), scale, 1.0)
        spread = np.maximum(_rel(f64[q], ld[q], scale), 4 * EPS)
        for p_ in pert:
            spread = np.maximum(spread, _rel(p_[q], ld[q], scale))
        err = _rel(lib[q], ld[q], scale)
        ok = (err <= K * spread) | ~np.isfinite(spread)
        assert ok.all(), (what, q, np.flatnonzero(~ok)[:5], err[~ok][:5], spread[~ok][:5])


@pytest.mark.parametrize("name", PC.NAMES)
def test_downstream_of_ut_against_longdouble(name):
    c, r = PC.case(name), PC.reference(name)
    p = c["problem"]
    if c["n_hyp"]:
        outs = [pnp.hypothesis_host(p, c["draws"][h]) for h in range(c["n_hyp"])]
        lib = dict(betas=np.array([o["betas"] for o in outs]), R=np.array([o["R"] for o in outs]),
                   t=np.array([o["t"] for o in outs]), rep=np.array([o["rep_err"] for o in outs]),
                   chosen=np.array([o["chosen"] for o in outs]))
        _downstream_check(r, p.Xw[r["idx"]], p.uv[r["idx"]], p.intr, lib, (name, "hypotheses"))
    for h, v in r["refined"].items():
        o = pnp.refine_host(p, r["mask"][h])
        who = np.flatnonzero(r["mask"][h])
        lib = dict(betas=o["betas"][None], R=o["R"][None], t=o["t"][None], rep=o["rep_err"][None],
                   chosen=np.array([o["chosen"]]))
        _downstream_check(v, p.Xw[who][None], p.uv[who][None], p.intr, lib, (name, "refine", h))


def _epnp_independent(Xw, uv, K_, signs=(1, 1, 1)):
    """EPnP from the algorithm (Lepetit, Moreno-Noguer, Fua 2009) with numpy's solvers: (R, t). ``signs``: the
    orientation of the three principal axes the control points lie on."""
    n = Xw.shape[0]
    c0 = Xw.mean(axis=0)
    lam, vec = np.linalg.eigh((Xw - c0).T @ (Xw - c0))
    cws = np.vstack([c0] + [c0 + sg * np.sqrt(lam[i] / n) * vec[:, i] for sg, i in zip(signs, (2, 1, 0))])
    al = np.linalg.solve((cws[1:] - cws[0]).T, (Xw - c0).T).T
    al = np.hstack([1.0 - al.sum(axis=1, keepdims=True), al])
    M = np.zeros((2 * n, 12))
    for j in range(4):
        M[0::2, 3 * j], M[0::2, 3 * j + 2] = al[:, j] * K_[0], al[:, j] * (K_[2] - uv[:, 0])
        M[1::2, 3 * j + 1], M[1::2, 3 * j + 2] = al[:, j] * K_[1], al[:, j] * (K_[3] - uv[:, 1])
    v = np.linalg.eigh(M.T @ M)[1][:, :4].T.reshape(4, 4, 3)       # the four smallest, smallest first
    pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    dv = np.array([[v[i, a] - v[i, b] for a, b in pairs] for i in range(4)])     # (4, 6, 3)
    terms = [(0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 2), (0, 3), (1, 3), (2, 3), (3, 3)]
    L = np.array([[(1 if x == y else 2) * dv[x, i] @ dv[y, i] for x, y in terms] for i in range(6)])
    rho = np.array([np.sum((cws[a] - cws[b]) ** 2) for a, b in pairs])

    def gn(b):
        for _ in range(5):
            bb = np.array([b[x] * b[y] for x, y in terms])
            J = np.zeros((6, 4))
            for k, (x, y) in enumerate(terms):
                J[:, x] += L[:, k] * b[y]
                J[:, y] += L[:, k] * b[x]
            b = b + np.linalg.lstsq(J, rho - L @ bb, rcond=None)[0]
        return b

    def pose(b):
        cc = np.tensordot(b, v, axes=(0, 0))
        pc = al @ cc
        if pc[0, 2] < 0:
            pc = -pc
        pc0, pw0 = pc.mean(axis=0), Xw.mean(axis=0)
        U, _, Vt = np.linalg.svd((pc - pc0).T @ (Xw - pw0))
        Rm = U @ Vt
        if np.linalg.det(Rm) < 0:
            Rm[2] = -Rm[2]
        tm = pc0 - Rm @ pw0
        Xc = Xw @ Rm.T + tm
        err = np.hypot(uv[:, 0] - (K_[2] + K_[0] * Xc[:, 0] / Xc[:, 2]), uv[:, 1] - (K_[3] + K_[1] * Xc[:, 1] / Xc[:, 2]))
        return err.mean(), Rm, tm

    inits = []
    x = np.linalg.lstsq(L[:, [0, 1, 3, 6]], rho, rcond=None)[0]
    x = -x if x[0] < 0 else x
    inits.append(np.array([np.sqrt(x[0]), x[1] / np.sqrt(x[0]), x[2] / np.sqrt(x[0]), x[3] / np.sqrt(x[0])]))
    for cols in ([0, 1, 2], [0, 1, 2, 3, 4]):
        x = np.linalg.lstsq(L[:, cols], rho, rcond=None)[0]
        b0 = np.sqrt(abs(x[0]))
        b1 = np.sqrt(abs(x[2])) if (x[2] < 0) == (x[0] < 0) and x[2] != 0 else 0.0
        b0 = -b0 if x[1] < 0 else b0
        inits.append(np.array([b0, b1, x[3] / b0 if len(cols) == 5 else 0.0, 0.0]))
    return min((pose(gn(b)) for b in inits), key=lambda e: e[0])[1:]


def test_refine_against_an_independent_epnp():
    """With noisy keypoints EPnP's pose depends on which way the principal axes point: min |M x| over |x| = 1 is
    not invariant under mirroring a control point through the centroid (measured here: 1e-4 on R at 0.1 px of
    noise, against 1e-15 between two eigen solvers on the same control points). An eigenvector's sign is the
    eigen solver's own, so the independent solver is run for all eight orientations and the library's pose must
    be one of them, within K x the spread of that orientation."""
    import itertools
    checked = 0
    for name in PC.NAMES:
        if name == "n20_coplanar":      # not in general position
            continue
        c, r = PC.case(name), PC.reference(name)
        p = c["problem"]
        for h in r["refined"]:
            who = np.flatnonzero(r["mask"][h])
            if len(who) < 10:
                continue
            o = pnp.refine_host(p, r["mask"][h])
            Xw, uv, K_ = p.Xw[who].astype(np.float64), p.uv[who].astype(np.float64), np.asarray(p.intr, np.float64)
            best = None
            for signs in itertools.product((1, -1), repeat=3):
                Ri, ti = _epnp_independent(Xw, uv, K_, signs)
                rng = np.random.default_rng(17)
                sR = st = 4 * EPS
                for _ in range(8):
                    args = [a + rng.choice([-1.0, 1.0], a.shape) * np.spacing(np.abs(a)) for a in (Xw, uv, K_)]
                    Rp, tp = _epnp_independent(*args, signs)
                    sR = max(sR, np.abs(Rp - Ri).max() / np.abs(Ri).max())
                    st = max(st, np.abs(tp - ti).max() / np.abs(ti).max())
                eR, et = np.abs(o["R"] - Ri).max() / np.abs(Ri).max(), np.abs(o["t"] - ti).max() / np.abs(ti).max()
                if best is None or max(eR / sR, et / st) < max(best[0] / best[1], best[2] / best[3]):
                    best = (eR, sR, et, st, signs)
            eR, sR, et, st, signs = best
            print(f"{name} refine of {h} on {len(who)}, axes {signs}: R {eR:.2e} / spread {sR:.2e}, "
                  f"t {et:.2e} / spread {st:.2e}")
            assert eR <= K * sR and et <= K * st, (name, h, eR / sR, et / st)
            checked += 1
    assert checked >= 8
