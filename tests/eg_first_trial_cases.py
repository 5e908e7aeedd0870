"""The pose graphs of tests/test_eg_gpu_first_trial.py: name -> (builder,
lambda). All have at most 300 keyframes. tests/test_eg_lin_ref.py checks on
the CPU that the oracle accepts the first trial of every one of them at its
lambda and that the reference's own rounding on it is small (b <= 1e-14,
dx <= 1e-9), so the GPU comparison is neither skipped nor vacuous.

EXPECT holds what each graph is there for, as sqlm_eg_get_exec_info reports
it without any environment switch: solve path, band blocks p, border
vertices, nc (padded order of the border complement), R (padded count of
cyclic-reduction right-hand sides, 7 border + 1), n_last (rows factored in
the complement's last block), information flag.
"""
import numpy as np

from sqrtlm import synth


def _graph(n_kf, window, n_loops, seed, **kw):
    kw.setdefault("fix_scale", True)
    kw.setdefault("rot_noise", 3e-4)
    kw.setdefault("trans_noise", 5e-4)
    return synth.make_pose_graph(n_kf, window=window, n_loops=n_loops, seed=seed, **kw)


def _append(pg, ei, ej, Sji, info=None):
    """pg with further edges after its own (g2o keeps insertion order, and
    parallel edges: HyperGraph::addEdge does not look for one between the
    same vertices)."""
    if (pg.info is None) != (info is None):
        raise ValueError("information for all edges or for none")
    return synth.PoseGraph(Siw=pg.Siw, fixed=pg.fixed, fix_scale=pg.fix_scale,
                           ei=np.concatenate([pg.ei, np.asarray(ei, np.int32)]),
                           ej=np.concatenate([pg.ej, np.asarray(ej, np.int32)]),
                           Sji=np.concatenate([pg.Sji, np.asarray(Sji, np.float64).reshape(-1, 8)]),
                           info=None if info is None else np.concatenate([pg.info, info]), meta=pg.meta)


def _long_edges(pg, pairs):
    """Edges (i, j) measuring the ground-truth relative Sim3 S_j S_i^-1."""
    gt = pg.meta["gt"]
    ei = np.array([p[0] for p in pairs], np.int32)
    ej = np.array([p[1] for p in pairs], np.int32)
    return _append(pg, ei, ej, synth._sim3_compose(gt[ej], synth._sim3_inv(gt[ei])))


def _border_wide():
    # 76 long edges with 152 distinct ends: 76 border vertices, 7 * 76 + 1 > 512 right-hand sides
    return _long_edges(_graph(300, 6, 0, 41), [(298 - 2 * k, 1 + k) for k in range(76)])


def _dense_auto():
    # 16 long edges (span 22 > 16) with distinct ends among 39 free vertices: 3 * 16 > 39
    return _long_edges(_graph(40, 6, 0, 42), [(23 + k, 1 + k) for k in range(16)])


def _info():
    """border3's shape, a seeded random SPD information per edge (eigenvalues
    in about 0.5 .. 4, exactly symmetric)."""
    pg = _graph(60, 4, 3, 33)
    R = np.random.default_rng(43).normal(size=(pg.n_edge, 7, 7))
    M = R @ R.transpose(0, 2, 1) / 7.0 + 0.5 * np.eye(7)
    pg.info = np.ascontiguousarray(0.5 * (M + M.transpose(0, 2, 1)))
    return pg


def _mixed():
    """Vertices 7, 8 and 20 fixed besides 0 (edge 8 -> 7 is inactive); every
    ninth edge again in the other direction (vertex 0 < vertex 1, the inverse
    measurement); five edges twice, with another measurement."""
    pg = _graph(60, 4, 3, 34)
    pg.fixed[[7, 8, 20]] = 1
    rev = np.arange(0, pg.n_edge, 9)
    dup = np.array([3, 40, 77, 150, pg.n_edge - 1])  # the last: a loop edge, an off-band block
    S2 = pg.Sji[dup].copy()
    S2[:, 4:7] += 1e-3
    pg = _append(pg, pg.ej[rev], pg.ei[rev], synth._sim3_inv(pg.Sji[rev]))
    return _append(pg, pg.ei[dup], pg.ej[dup], S2)


def _free_scale():
    # Free scale makes H ill-conditioned (entries up to 1e8 .. 1e12 against 1e6
    # with the scale fixed: the erratic update of tests/test_eg_gpu.py's
    # docstring). Measured on the CPU, float64-vs-longdouble spread of dx and
    # longdouble residual |(H + lam I) dx - b| / |b| (bounds 1e-9 and 1e-17):
    #   default drift 0.01, noise-free, lam 1:     4.9e-10, 1.5e-17 (residual too large)
    #   default drift 0.01, noise-free, lam 1000:  1.9e-11, 9.2e-19
    #   drift 0.003, noise-free, lam 1:            5.9e-6 (cap broken)
    #   drift 0.003, noisy, lam 1:                 7.1e-12, 5.7e-18 (under 2x of margin)
    #   drift 0.003, noisy, lam 10 / 100:          first trial rejected
    #   drift 0.003, noisy, lam 1000:              5.9e-13, 1.8e-19  <- this one
    return _graph(60, 4, 3, 3, fix_scale=False, drift=0.003, scale_noise=1e-3)


_G = {
    "band1": lambda: _graph(12, 6, 0, 31),
    "band_p3": lambda: _graph(40, 6, 0, 32),
    "border3": lambda: _graph(60, 4, 3, 33),
    "border5": lambda: _graph(60, 4, 5, 37),
    "border16": lambda: _graph(200, 6, 17, 35),
    "border17": lambda: _graph(200, 6, 18, 36),
    "border_wide": _border_wide,
    "dense_auto": _dense_auto,
    "info": _info,
    "mixed": _mixed,
    "free_scale": _free_scale,
}

_LAMBDAS = {
    "band1": (1e-16, 1.0),
    "band_p3": (1e-16, 1e-3, 1.0, 1e3),
    "border3": (1e-16, 1.0),
    "border5": (1.0,),
    "border16": (1.0,),
    "border17": (1.0,),
    "border_wide": (1.0,),
    "dense_auto": (1.0,),
    "info": (1e-16, 1.0),
    "mixed": (1e-16, 1.0),
    "free_scale": (1e3,),
}

# graph -> exec info of the default layout. A loop edge onto the fixed keyframe 0
# is not long, so n_loops gives n_loops - 1 border vertices: border3 has 2 and
# R = 16 like a borderless graph; border5 is there for R = 32.
EXPECT = {
    "band1": dict(solve="cr", p=1, border=0, nc=112, R=16, n_last=0, info=False),
    "band_p3": dict(solve="cr", p=3, border=0, nc=112, R=16, n_last=0, info=False),
    "border3": dict(solve="cr", p=4, border=2, nc=112, R=16, n_last=16, info=False),
    "border5": dict(solve="cr", p=4, border=4, nc=112, R=32, n_last=32, info=False),
    "border16": dict(solve="cr", p=12, border=16, nc=112, R=128, n_last=112, info=False),
    "border17": dict(solve="cr", p=12, border=17, nc=224, R=128, n_last=16, info=False),
    "border_wide": dict(solve="arrow_cholesky", p=14, border=76, nc=0, R=0, n_last=0, info=False),
    "dense_auto": dict(solve="dense", p=0, border=0, nc=0, R=0, n_last=0, info=False),
    "info": dict(solve="cr", p=4, border=2, nc=112, R=16, n_last=16, info=True),
    "mixed": dict(solve="cr", p=4, border=2, nc=112, R=16, n_last=16, info=False),
    "free_scale": dict(solve="cr", p=4, border=2, nc=112, R=16, n_last=16, info=False),
}


def _lam_name(lam):
    return f"{lam:g}"


# name -> (builder, lambda); GRAPH_OF[name] is the graph's key in EXPECT
CASES, GRAPH_OF = {}, {}
for _g, _lams in _LAMBDAS.items():
    for _lam in _lams:
        _name = _g if len(_lams) == 1 else f"{_g}_lam{_lam_name(_lam)}"
        CASES[_name] = (_G[_g], _lam)
        GRAPH_OF[_name] = _g
