"""PnP RANSAC of relocalization candidates: the reference's ``PnPsolver``
(src/algorithm/PnPsolver.cc) over ``sqlm_pnp_ransac``.

``PnPProblem`` holds what the reference's constructor keeps of a frame and its
map point matches, ``make_pnp_problem`` plants one with mismatches, ``pack``
lays a list of them out as the C ABI's batch, ``pnp_max_its`` is
``SetRansacParameters`` and ``PnPsolver`` mirrors the reference's
``SetRansacParameters / iterate / find`` by replaying the per-hypothesis flags
the library returns, the ``||`` of iterate's loop condition included.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from .sim3 import orb_level_sigma2

TH2 = np.float32(5.991)


@dataclass
class PnPProblem:
    intr: np.ndarray      # (4,) float64 fu fv uc vc, float values
    Xw: np.ndarray        # (N, 3) float32 mvP3Dw
    uv: np.ndarray        # (N, 2) float32 mvP2D
    sigma2: np.ndarray    # (N,) float32 mvSigma2
    meta: dict = field(default_factory=dict)

    @property
    def n_pair(self) -> int:
        return int(self.Xw.shape[0])

    def max_err(self, th2=TH2) -> np.ndarray:
        """mvMaxError as stored (:226): the float product sigma2 * th2."""
        return (self.sigma2.astype(np.float32) * np.float32(th2)).astype(np.float32)


def _rot(w):
    th = float(np.linalg.norm(w))
    if th == 0.0:
        return np.eye(3)
    k = np.asarray(w, float) / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def make_pnp_problem(n: int = 100, *, seed: int = 0, outlier_frac: float = 0.3, pixel_noise: float = 0.5,
                     coplanar: bool = False, intr=(718.856, 718.856, 607.1928, 185.2157), n_levels: int = 8,
                     levels=None, behind: int = 0) -> PnPProblem:
    """A relocalization candidate: ``n`` world points 4-25 m in front of a
    camera with the known pose ``meta['Rcw'], meta['tcw']`` (``coplanar``: all
    on one plane), their projections plus ``pixel_noise`` px, stored as float32
    like the reference's constructor stores them. ``round(outlier_frac * n)``
    pairs (``meta['outlier']``) are mismatches: their keypoints are permuted
    cyclically among themselves. Each keypoint has an octave (``levels`` or
    random below ``n_levels``) and with it a sigma2. ``behind``: that many
    further pairs are appended whose world point lies behind the camera."""
    rng = np.random.default_rng([seed, 0x9E9])
    K = np.array(intr, np.float32).astype(np.float64)
    R = _rot(np.array([0.08, -0.15, 0.04]) + 0.03 * rng.normal(size=3))
    t = np.array([0.4, -0.2, 0.7]) + 0.2 * rng.normal(size=3)
    n = int(n)
    z = rng.uniform(4.0, 25.0, n)
    if coplanar:   # the world plane z = 0 exactly, seen obliquely from 12 m
        Xw = np.stack([rng.uniform(-6.0, 6.0, n), rng.uniform(-3.0, 3.0, n), np.zeros(n)], axis=1).astype(np.float32)
        t = np.array([0.3, -0.2, 12.0]) + 0.2 * rng.normal(size=3)
        R = _rot(np.array([0.5, -0.3, 0.1]) + 0.03 * rng.normal(size=3))
        Xc = Xw.astype(np.float64) @ R.T + t
    else:
        Xc = np.stack([rng.uniform(-0.8, 0.8, n) * z, rng.uniform(-0.25, 0.25, n) * z, z], axis=1)
    if behind:
        zb = -rng.uniform(4.0, 25.0, behind)
        Xc = np.concatenate([Xc, np.stack([rng.uniform(-0.8, 0.8, behind) * zb,
                                           rng.uniform(-0.25, 0.25, behind) * zb, zb], axis=1)])
        n += behind
    Xw = ((Xc - t) @ R).astype(np.float32)   # R^T (Xc - t)
    Xc = Xw.astype(np.float64) @ R.T + t
    uv = np.stack([K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]], axis=1)
    uv = uv + pixel_noise * rng.normal(size=(n, 2))
    n_out = int(round(outlier_frac * n))
    outlier = np.zeros(n, bool)
    if n_out >= 2:
        who = np.sort(rng.permutation(n)[:n_out])
        outlier[who] = True
        uv[who] = uv[np.roll(who, 1)]
    lv = rng.integers(0, n_levels, n) if levels is None else np.asarray(levels, np.int64).reshape(n)
    sig2 = orb_level_sigma2(n_levels)[lv].astype(np.float32)
    return PnPProblem(intr=K, Xw=Xw, uv=uv.astype(np.float32), sigma2=sig2,
                      meta=dict(Rcw=R, tcw=t, outlier=outlier, levels=lv, seed=seed))


def pack(problems, draws, min_inliers, max_err=None):
    """The batch arrays of ``sqlm_pnp_ransac``: ``draws`` a list of (n_hyp, 4)
    arrays of raw RandomInt values, ``min_inliers`` an int or one per problem,
    ``max_err`` a list of (N,) float32 arrays (default: each problem's own)."""
    P = len(problems)
    if len(draws) != P:
        raise ValueError("one draws array per problem")
    c = lambda xs, w, t: (np.concatenate([np.asarray(x, t).reshape(-1, w) for x in xs], axis=0)
                          if xs else np.zeros((0, w), t))
    poff, hoff = np.zeros(P + 1, np.int64), np.zeros(P + 1, np.int64)
    poff[1:] = np.cumsum([p.n_pair for p in problems])
    draws = [np.asarray(d, np.int32).reshape(-1, 4) for d in draws]
    hoff[1:] = np.cumsum([d.shape[0] for d in draws])
    me = [p.max_err() for p in problems] if max_err is None else max_err
    return dict(intr=c([p.intr for p in problems], 4, np.float64),
                min_inliers=np.broadcast_to(np.asarray(min_inliers, np.int32), (P,)).copy(), pair_off=poff,
                Xw=c([p.Xw for p in problems], 3, np.float32), uv=c([p.uv for p in problems], 2, np.float32),
                max_err=c(me, 1, np.float32).reshape(-1), hyp_off=hoff, draws=c(draws, 4, np.int32))


def pnp_max_its(n_pair: int, probability: float = 0.99, min_inliers: int = 10, max_iterations: int = 300,
                min_set: int = 4, epsilon: float = 0.5):
    """sqlm_pnp_ransac_max_its: ``(mRansacMaxIts, mRansacMinInliers)`` after
    SetRansacParameters; mRansacMaxIts is 0 where iterate gives up at once (host only, no GPU)."""
    import ctypes as C
    from ._lib import lib
    out = C.c_int(0)
    its = lib().sqlm_pnp_ransac_max_its(int(n_pair), float(probability), int(min_inliers), int(max_iterations),
                                        int(min_set), float(epsilon), C.byref(out))
    return int(its), int(out.value)


def draw(rng, n_pair: int, n_hyp: int) -> np.ndarray:
    """(n_hyp, 4) raw RandomInt values in iterate's order: draw i of a hypothesis is in [0, N-1-i]."""
    if n_hyp <= 0:
        return np.zeros((0, 4), np.int32)
    return np.stack([rng.integers(0, n_pair - i, n_hyp) for i in range(4)], axis=1).astype(np.int32)


def _host_out(n):
    return dict(R=np.zeros((3, 3)), t=np.zeros(3), mask=np.zeros(max(n, 1), np.uint8), cnt=np.zeros(1, np.int32),
                ut=np.zeros((12, 12)), eig=np.zeros(12), betas=np.zeros((3, 4)), rep_err=np.zeros(3),
                chosen=np.zeros(1, np.int32))


def _host_done(o, n):
    o.update(mask=o["mask"][:n], n_inliers=int(o.pop("cnt")[0]), chosen=int(o["chosen"][0]))
    return o


def hypothesis_host(problem: PnPProblem, draws4, max_err=None, sweeps=None):
    """sqlm_pnp_ransac_hypothesis_host: one hypothesis on the CPU from the kernels' source text. A dict of idx,
    R, t, mask, n_inliers, ut, eig, betas, rep_err, chosen. ``sweeps``: (3,) Jacobi sweep counts, 0 = the library's."""
    from ._lib import lib, ptr, check
    n = problem.n_pair
    me = np.ascontiguousarray(problem.max_err() if max_err is None else max_err, np.float32)
    o, idx = _host_out(n), np.zeros(4, np.int32)
    dr = np.ascontiguousarray(draws4, np.int32).reshape(4)
    sw = None if sweeps is None else np.ascontiguousarray(sweeps, np.int32).reshape(3)
    Xw, uv = np.ascontiguousarray(problem.Xw, np.float32), np.ascontiguousarray(problem.uv, np.float32)
    check(lib().sqlm_pnp_ransac_hypothesis_host(n, ptr(problem.intr), ptr(Xw), ptr(uv), ptr(me), ptr(dr), ptr(sw),
                                                ptr(idx), ptr(o["R"]), ptr(o["t"]), ptr(o["mask"]), ptr(o["cnt"]),
                                                ptr(o["ut"]), ptr(o["eig"]), ptr(o["betas"]), ptr(o["rep_err"]),
                                                ptr(o["chosen"])), "sqlm_pnp_ransac_hypothesis_host")
    o["idx"] = idx
    return _host_done(o, n)


def refine_host(problem: PnPProblem, in_mask, max_err=None, sweeps=None):
    """sqlm_pnp_ransac_refine_host: EPnP on the pairs of ``in_mask`` and the inlier test, on the CPU."""
    from ._lib import lib, ptr, check
    n = problem.n_pair
    me = np.ascontiguousarray(problem.max_err() if max_err is None else max_err, np.float32)
    o = _host_out(n)
    im = np.ascontiguousarray(in_mask, np.uint8).reshape(n)
    sw = None if sweeps is None else np.ascontiguousarray(sweeps, np.int32).reshape(3)
    Xw, uv = np.ascontiguousarray(problem.Xw, np.float32), np.ascontiguousarray(problem.uv, np.float32)
    check(lib().sqlm_pnp_ransac_refine_host(n, ptr(problem.intr), ptr(Xw), ptr(uv), ptr(me), ptr(im), ptr(sw),
                                            ptr(o["R"]), ptr(o["t"]), ptr(o["mask"]), ptr(o["cnt"]), ptr(o["ut"]),
                                            ptr(o["eig"]), ptr(o["betas"]), ptr(o["rep_err"]), ptr(o["chosen"])),
          "sqlm_pnp_ransac_refine_host")
    return _host_done(o, n)


def scan(counts, refined, min_inliers):
    """sqlm_pnp_ransac_scan: (flags (H,), first_return, best, n_record) of iterate's bookkeeping on the counts."""
    from ._lib import lib, ptr, check
    c = np.ascontiguousarray(counts, np.int32)
    rf = None if refined is None else np.ascontiguousarray(refined, np.int32)
    flags, o = np.zeros(max(c.shape[0], 1), np.uint8), np.zeros(3, np.int64)
    check(lib().sqlm_pnp_ransac_scan(c.shape[0], ptr(c), ptr(rf), 0 if rf is None else rf.shape[0], int(min_inliers),
                                     ptr(flags), o[0:1].ctypes.data, o[1:2].ctypes.data, o[2:3].ctypes.data),
          "sqlm_pnp_ransac_scan")
    return flags[:c.shape[0]], int(o[0]), int(o[1]), int(o[2])


class PnPsolver:
    """The reference's PnPsolver on the GPU.

    Constructed from a PnPProblem and a numpy ``Generator`` (``rng``) or given
    ``draws`` (``(>= max(mRansacMaxIts, 5), 4)`` raw RandomInt values). The
    hypotheses are evaluated in one GPU call, made lazily by the first
    ``iterate`` / ``find`` (or by ``solve_batch`` for several solvers at once).
    A call after an early return can run past the evaluated hypotheses; the
    solver then draws ``max(nIterations, 5)`` more and resubmits the problem
    with all draws, whose prefix reproduces. ``keypoint_indices`` / ``n_matches``
    are mvKeyPointIndices and the size of vpMapPointMatches."""

    def __init__(self, problem: PnPProblem, rng=None, draws=None, keypoint_indices=None, n_matches=None, ctx=None):
        self.problem = problem
        self.N = problem.n_pair
        self.keypoint_indices = (np.arange(self.N) if keypoint_indices is None
                                 else np.asarray(keypoint_indices, np.int64).reshape(self.N))
        self.n_matches = self.N if n_matches is None else int(n_matches)
        self._rng, self._given, self._ctx = rng, draws, ctx
        if rng is None and draws is None:
            raise ValueError("give a numpy Generator (rng) or explicit draws")
        self.SetRansacParameters()

    def SetRansacParameters(self, probability: float = 0.99, minInliers: int = 8, maxIterations: int = 300,
                            minSet: int = 4, epsilon: float = 0.4, th2: float = 5.991):
        self.mRansacMaxIts, self.mRansacMinInliers = pnp_max_its(self.N, probability, minInliers, maxIterations,
                                                                 minSet, epsilon)
        self.max_err = self.problem.max_err(th2)
        self.mnIterations = 0
        self.mnBestInliers = 0
        self._best = -1
        self._res = None
        self._draws = None

    @property
    def draws(self):
        if self._draws is None:
            self._draws = self._more(np.zeros((0, 4), np.int32), max(self.mRansacMaxIts, 5) if self.mRansacMaxIts else 0)
        return self._draws

    def _more(self, have, n_more):
        H = have.shape[0] + n_more
        if self._given is not None:
            d = np.asarray(self._given, np.int32).reshape(-1, 4)
            if d.shape[0] < H:
                raise ValueError(f"{H} hypotheses need {H} draw quadruples, {d.shape[0]} given")
            return d[:H].copy()
        return np.concatenate([have, draw(self._rng, self.N, n_more)])

    @classmethod
    def solve_batch(cls, solvers, ctx=None):
        """Evaluate every hypothesis of every solver in one sqlm_pnp_ransac call."""
        solvers = [s for s in solvers if s.mRansacMaxIts > 0]
        if not solvers:
            return
        own = None
        if ctx is None:
            ctx = next((s._ctx for s in solvers if s._ctx is not None), None)
        if ctx is None:
            from .optimizer import Context
            ctx = own = Context(0)
        try:
            res = ctx.pnp_ransac([s.problem for s in solvers], [s.draws for s in solvers],
                                 [s.mRansacMinInliers for s in solvers], [s.max_err for s in solvers])
            for k, s in enumerate(solvers):
                r = res[k]
                rec = [int(h) for h in np.flatnonzero(r["flags"] & 2)]
                r["mask"] = {h: ctx.pnp_ransac_inliers(k, h).astype(bool) for h in rec}
                r["refined"] = {h: ctx.pnp_ransac_refined(k, h) for h in rec}
                s._res = r
        finally:
            if own is not None:
                own.close()

    def _results(self, n_hyp, n_more):
        if self._res is None or self._res["n_inliers"].shape[0] < n_hyp:
            if self._res is not None:
                self._draws = self._more(self._draws, max(n_more, 5))
            type(self).solve_batch([self], self._ctx)
        return self._res

    @staticmethod
    def _T(R, t):
        T = np.eye(4, dtype=np.float32)
        T[:3, :3], T[:3, 3] = np.asarray(R, np.float32), np.asarray(t, np.float32)
        return T

    def _vb(self, mask):
        vb = np.zeros(self.n_matches, bool)
        vb[self.keypoint_indices[mask]] = True
        return vb

    def iterate(self, nIterations: int):
        """(Tcw (4,4) float32 or None, bNoMore, vbInliers (n_matches,) bool, nInliers): PnPsolver.cc:247-370."""
        empty = np.zeros(0, bool)
        if self.N < self.mRansacMinInliers or self.mRansacMaxIts == 0:
            return None, True, empty, 0
        cur = 0
        while self.mnIterations < self.mRansacMaxIts or cur < nIterations:
            cur += 1
            h = self.mnIterations
            self.mnIterations += 1
            r = self._results(h + 1, nIterations)
            f = int(r["flags"][h])
            if f & 1:
                if f & 2:
                    self._best, self.mnBestInliers = h, int(r["n_inliers"][h])
                if f & 4:
                    ref = r["refined"][self._best]
                    return self._T(ref["R"], ref["t"]), False, self._vb(ref["mask"].astype(bool)), int(ref["n_inliers"])
        if self.mnIterations >= self.mRansacMaxIts:
            if self.mnBestInliers >= self.mRansacMinInliers:
                r = self._res
                return (self._T(r["R"][self._best], r["t"][self._best]), True, self._vb(r["mask"][self._best]),
                        self.mnBestInliers)
            return None, True, empty, 0
        return None, False, empty, 0

    def find(self):
        """(Tcw or None, vbInliers, nInliers): iterate(mRansacMaxIts) without its flag (:231-235)."""
        T, _, vb, n = self.iterate(self.mRansacMaxIts)
        return T, vb, n
