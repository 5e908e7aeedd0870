"""The CPU oracle on the shapes of tests/test_gpu_cr_levels.py.

That test compares two orders of the same block elimination by iteration
count, trial trace and 1e-9 on chi2 and the states. The rule only means
something on problems whose accept / reject decisions do not hang on the last
bits of the step, so every shape is run through oracle.OracleGraph here: it
must take the recorded trials, and each decision must be a clear one -- an
accepted trial lowers chi2 by more than 1 % of it, a rejected first trial is
followed by an accepted one that does.
"""
import pytest

import cr_levels_cases as cases
from oracle import oracle as O


@pytest.mark.parametrize("name", list(cases.CASES))
def test_oracle_takes_the_recorded_trials(name):
    c, _, trials = cases.CASES[name]
    g = O.OracleGraph(cases.build(c))
    if c["lam0"] > 0:
        n, st = g.optimize(0, 3, user_lambda=c["lam0"])
    else:
        n, st = g.global_ba(4)
    assert n == len(trials) and list(st["trace_trials"][:n]) == trials, st["trace_trials"][:n]
    chi = [st["chi2_begin"]] + list(st["trace_chi2"][:n])
    for a, b in zip(chi, chi[1:]):  # every iteration ends in an accepted trial with a clear gain
        assert b < 0.99 * a, chi
