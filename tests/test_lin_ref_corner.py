"""tests/lin_ref_corner.py (lin_ref with EdgeLidarCornerPoint edges) against
lin_ref, against the unmodified oracle through a flat twin, and against a
reference that ignores the kinds. No GPU.

(b) The oracle has no corner edge, but a corner edge with d = T p_w - p_c and a
flat edge with the normal n = d / |d| have the same error and, to first order,
the same derivative. The twin's normal is evaluated in longdouble at the
initial poses and rounded to float64. Errors agree within 8 eps relative. The
Jacobian rows are central differences of errors with delta = 1e-9: the
symmetric difference cancels the second-order term of the norm, what is left
is the rounding of the error evaluations, a few eps of the magnitudes that
enter d, divided by the step: 64 eps (|p_w| + |t| + |p_c|) / delta per entry.
Observed (test_corner_matches_flat_twin prints them): largest row-entry
difference / bound 1.2e-4 on cor_one (150 corner edges) and 1.9e-4 on cor_mixed
(197), with bounds of 5e-4 .. 1.8e-3 against entries up to 31; largest error
difference 0.22 and 0.17 of the 8 eps.
"""
import functools

import numpy as np
import pytest

import corner_first_trial_cases as corc
import lidar_first_trial_cases as lidc
import lin_ref
import lin_ref_corner as LRC

EPS = float(np.finfo(np.float64).eps)
LD = lin_ref.LD
K = 100.0           # the project's bound on GPU error / reference spread (tests/test_gpu_first_trial.py)
FLOOR = 4 * EPS
DELTA = 1e-9


@functools.lru_cache(maxsize=None)
def _problem(name):
    return corc.CASES[name][0]()


def _same_trial(a, b):
    for f in ("free", "lms", "Hpp", "bp", "Hll", "bl", "S", "g", "dx", "dl"):
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and np.array_equal(x, y), f
    assert a.chi2_0 == b.chi2_0 and a.refine_steps == b.refine_steps


def test_all_flat_is_lin_ref_bit_for_bit():
    prob = lidc.CASES["lid_multi"][0]()
    assert prob.n_lid and not prob.lid_kind.any()
    for T in (np.float64, LD):
        a, b = LRC.lidar_edges(prob, T), lin_ref.lidar_edges(prob, T)
        for f in ("eid", "pose", "e", "J", "info", "chi2"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
        assert LRC.chi2(prob, dtype=T) == lin_ref.chi2(prob, dtype=T)
    eid = np.arange(prob.n_lid)
    assert np.array_equal(LRC.lidar_jacobians(prob, eid), lin_ref.lidar_jacobians(prob, eid))
    sa, ra, fa = LRC.spreads(prob, 1.0)
    sb, rb, fb = lin_ref.spreads(prob, 1.0)
    assert sa == sb
    _same_trial(ra, rb)
    _same_trial(fa, fb)
    _same_trial(LRC.first_trial(prob, 1.0, np.float64), lin_ref.first_trial(prob, 1.0, np.float64))
    sa, ra, fa = LRC.spreads_lambda_init(prob)
    sb, rb, fb = lin_ref.spreads_lambda_init(prob)
    assert sa == sb
    _same_trial(ra, rb)
    assert LRC.chi2_spread(prob, prob.pose_q, prob.pose_t, prob.pt) == lin_ref.chi2_spread(prob, prob.pose_q,
                                                                                          prob.pose_t, prob.pt)
    assert lin_ref.lidar_edges.__module__ == "lin_ref"      # the wrapper put lin_ref's own function back


@pytest.mark.parametrize("name", ["cor_one", "cor_mixed"])
def test_corner_matches_flat_twin(oracle, name):
    prob = _problem(name)
    cor = np.nonzero(prob.lid_kind == 1)[0]
    assert cor.size >= 150
    p = prob.lid_pose[cor]
    d = (lin_ref._rotate(prob.pose_q[p].astype(LD), prob.lid_pw[cor].astype(LD)) + prob.pose_t[p].astype(LD)) \
        - prob.lid_pc[cor].astype(LD)
    nrm = np.sqrt((d * d).sum(axis=1))
    twin = prob.copy()
    twin.lid_n[cor] = (d / nrm[:, None]).astype(np.float64)
    twin.lid_kind = np.zeros(prob.n_lid, np.uint8)
    twin.validate()
    free = prob.pose_fixed[prob.lid_pose] == 0
    mine = LRC.lidar_edges(prob, np.float64)
    assert np.array_equal(mine.eid, np.nonzero(free)[0])
    sel = np.nonzero(prob.lid_kind[mine.eid] == 1)[0]           # corner edges among the active ones
    e_twin = np.array([oracle.lidar_error(twin.pose_q[twin.lid_pose[e]], twin.pose_t[twin.lid_pose[e]], twin.lid_pc[e],
                                          twin.lid_pw[e], twin.lid_n[e]) for e in mine.eid[sel]])
    J_twin = lin_ref.lidar_jacobians(twin, mine.eid[sel])        # orc_lidar_jacobian, the unmodified oracle
    e_rel = np.abs(mine.e[sel] - e_twin) / np.abs(e_twin)
    pe = prob.lid_pose[mine.eid[sel]]
    bound = 64 * EPS * (np.linalg.norm(prob.lid_pw[mine.eid[sel]], axis=1) + np.linalg.norm(prob.pose_t[pe], axis=1)
                        + np.linalg.norm(prob.lid_pc[mine.eid[sel]], axis=1)) / DELTA
    ratio = np.abs(mine.J[sel] - J_twin) / bound[:, None]
    print(f"{name}: {sel.size} corner edges, error diff {e_rel.max() / (8 * EPS):.3g} of 8 eps relative, "
          f"largest Jacobian entry diff / bound {ratio.max():.3g} (bound {bound.min():.2e}..{bound.max():.2e}, "
          f"|J| up to {np.abs(J_twin).max():.3g})")
    assert np.all(mine.e[sel] > 0) and sel.size > 0
    assert e_rel.max() <= 8 * EPS
    assert ratio.max() <= 1.0
    # the flat edges of the same problem are lin_ref's own, bit for bit
    fl = np.nonzero(prob.lid_kind[mine.eid] == 0)[0]
    ref = lin_ref.lidar_edges(twin, np.float64)
    assert np.array_equal(mine.e[fl], ref.e[fl]) and np.array_equal(mine.J[fl], ref.J[fl])


@pytest.mark.parametrize("name", sorted(corc.CASES))
def test_ignoring_the_kinds_cannot_pass(name):
    """The reference with every kind zeroed is more than 1e6 x K spreads away
    from the corner reference in g and in dx: a kernel that accepted the kinds
    and ignored them would fail the GPU test by six orders of magnitude."""
    prob, lam, level = _problem(name), corc.CASES[name][1], corc.LEVEL.get(name, 0)
    assert prob.lid_kind.any()
    sp, ref, f64 = LRC.spreads(prob, lam, level=level)
    flat = LRC.first_trial(corc.zero_kinds(prob), lam, np.float64, level)
    assert np.array_equal(flat.free, ref.free)
    for k in ("g", "dx"):
        diff = lin_ref._rel(getattr(flat, k), getattr(ref, k))
        need = 1e6 * K * max(sp[k], FLOOR)
        print(f"{name}: {k} flat-vs-corner {diff:.3g}, spread {sp[k]:.3g}, 1e6 K spread {need:.3g}")
        assert diff > need, (name, k, diff, need)
    # the sanity bounds of tests/test_lin_ref.py on the reference itself
    assert 0 < sp["g"] < 1e-13 and 0 < sp["dx"] < (1e-8 if lam < 1 else 1e-11), sp
    assert np.abs(ref.S @ ref.dx - ref.g).max() <= 1e-17 * np.abs(ref.g).max()


@pytest.mark.parametrize("name", sorted(corc.CASES))
def test_first_trial_reduces_chi2(oracle, name):
    """The trial the GPU test runs is an accepted one: chi2 falls with margin."""
    prob, lam, level = _problem(name), corc.CASES[name][1], corc.LEVEL.get(name, 0)
    tr = LRC.first_trial(prob, lam, np.float64, level)
    q, t = lin_ref.oplus_poses(oracle, prob, tr.free, tr.dx)
    chi = LRC.chi2(prob, q, t, prob.pt + tr.dl, np.float64, level)
    print(f"{name}: chi2 {float(tr.chi2_0):.6g} -> {float(chi):.6g}")
    assert chi < tr.chi2_0 * (1 - 1e-3)


def test_case_layout():
    p = _problem("cor_mixed")
    free = p.pose_fixed[p.lid_pose] == 0
    k29 = p.lid_kind[p.lid_pose == 29]
    assert k29.size == 200 and not k29[:100].any() and k29[100:].all()
    assert p.lid_kind[p.lid_pose == 14].all() and (p.lid_pose == 14).sum() == 64
    k20 = p.lid_kind[p.lid_pose == 20]
    assert k20.size == 65 and np.array_equal(k20, np.arange(65) % 2)
    assert p.lid_kind[p.lid_pose == 5].tolist() == [1]
    assert p.pose_fixed[0] and p.lid_kind[p.lid_pose == 0].all() and (p.lid_pose == 0).sum() == 40
    assert np.any(np.diff(p.lid_pose) < 0) and free.any()
    q = _problem("cor_level")
    l1 = (q.meta["lid_level"] == 1) & (q.pose_fixed[q.lid_pose] == 0)
    assert q.lid_kind[l1].any() and not q.lid_kind[l1].all()
    c = _problem("cor_only_cam")
    assert not np.any((c.obs_pose == corc.ONLY_CAM) & (c.obs_level == 0)) and c.lid_kind.all()
    assert _problem("cor_stereo").has_stereo and _problem("cor_one").lid_kind.all()
