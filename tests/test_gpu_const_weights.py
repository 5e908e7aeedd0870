"""Constant weights are written once: with no robust
kernel on any active edge the stored weight sqrt(rho' info) is sqrt(info) at
every state, so k_linearize writes it at iteration 0, the speculative pass of
the landmark update does not store it again and obs_s_nx is obs_s itself. One
edge with a Huber delta keeps the stored-weight path. SQLM_TRIAL_STORES=1
(separate arrays, stored every trial) is the reference: bitwise equal."""
import numpy as np
import pytest

from sqrtlm import synth

pytestmark = pytest.mark.gpu

TOL = 1e-6
_DROP = {"ms_total", "ms_setup", "ms_linearize", "ms_trials"}


def _run(ctx, prob, iters, monkeypatch, stores):
    if stores:
        monkeypatch.setenv("SQLM_TRIAL_STORES", "1")
    else:
        monkeypatch.delenv("SQLM_TRIAL_STORES", raising=False)
    ctx.set_problem(prob)
    n, st = ctx.optimize(0, iters)
    q, t = ctx.poses()
    st = {k: v for k, v in st.items() if k not in _DROP}
    return n, st, q.copy(), t.copy(), ctx.points().copy(), ctx.edge_chi2().copy()


def _assert_same(a, b):
    assert a[0] == b[0] and a[1] == b[1]
    for x, y in zip(a[2:], b[2:]):
        assert np.array_equal(x, y)


def _rejecting_problem():
    """A problem without a robust kernel whose LM run rejects trials: the CPU
    oracle's trace_trials of make_problem(14, 400, seed=s, robust=False,
    outlier_frac=0.1), optimize(0, 20), has entries above 1 for s = 1, 2, 4
    and 7; s = 7 gives [1, 1, 1, 1, 1, 1, 2, 3, 1, 1, 2, 1, 1, 2, 1, 1]."""
    return synth.make_problem(14, 400, seed=7, robust=False, outlier_frac=0.1)


def test_no_robust_edge_with_rejected_trials(gpu_ctx, monkeypatch):
    prob = _rejecting_problem()
    assert not (prob.obs_delta > 0).any()
    a = _run(gpu_ctx, prob, 20, monkeypatch, False)
    b = _run(gpu_ctx, prob, 20, monkeypatch, True)
    _assert_same(a, b)
    tr = a[1]["trace_trials"][:a[0]]
    assert max(tr) > 1 and tr[-1] == 1  # rejected trials, and accepted ones after them


def test_one_robust_edge_keeps_stored_weights(gpu_ctx, oracle, monkeypatch):
    prob = _rejecting_problem()
    prob.obs_delta[7] = np.float32(np.sqrt(5.991))
    assert np.count_nonzero(prob.obs_delta > 0) == 1
    a = _run(gpu_ctx, prob, 10, monkeypatch, False)
    b = _run(gpu_ctx, prob, 10, monkeypatch, True)
    _assert_same(a, b)
    ref = oracle.OracleGraph(prob)
    nr, sr = ref.optimize(0, 10)
    n, st, q, t, X, chi = a
    assert n == nr and st["trace_trials"] == sr["trace_trials"]
    assert max(st["trace_trials"][:n]) > 1
    np.testing.assert_allclose(st["trace_chi2"], sr["trace_chi2"], rtol=TOL)
    np.testing.assert_allclose(st["trace_lambda"], sr["trace_lambda"], rtol=TOL)
    assert np.abs(q - ref.pose_q).max() < TOL
    assert np.abs(t - ref.pose_t).max() / max(1.0, np.abs(ref.pose_t).max()) < TOL
    assert np.abs(X - ref.pt).max() / max(1.0, np.abs(ref.pt).max()) < TOL
    np.testing.assert_allclose(chi, ref.edge_chi2(), rtol=1e-6, atol=1e-9)


def test_double_inputs_without_robust_kernel(gpu_ctx, monkeypatch):
    """The double input arrays (one information value off float32 by one
    ulp), no robust kernel."""
    prob = synth.make_problem(14, 400, pair_window=4, n_fixed=3, seed=5, robust=False)
    prob.obs_info[11] = np.nextafter(prob.obs_info[11], np.inf)
    assert not (prob.obs_delta > 0).any()
    a = _run(gpu_ctx, prob, 10, monkeypatch, False)
    assert gpu_ctx.exec_info()["obs_f32"] is False
    b = _run(gpu_ctx, prob, 10, monkeypatch, True)
    assert gpu_ctx.exec_info()["obs_f32"] is False
    _assert_same(a, b)
