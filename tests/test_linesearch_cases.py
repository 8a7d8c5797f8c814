"""CPU tier of the line-search cases (tests/linesearch_cases.py): what the device assertions of tests/test_gpu_linesearch.py rest on, shown on the oracle.

For every case: no decision of the oracle lies within DECISION_MARGIN of its threshold (so "the same step size" can be asserted of an implementation
that sums in another order), the seeds are the smallest that achieve this, and the oracle's record shows the trial counts the case exists for."""
import numpy as np
import pytest

from tests import linesearch_cases as lc

BRANCHES = [n for n in lc.CASES if n.startswith("branches-")]


@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_no_decision_sits_on_its_threshold(name):
    c, prob, warm = lc.case_inputs(name)
    assert len(warm) == c["batch"] and min(lc.margin(name)) >= lc.DECISION_MARGIN, lc.margin(name)
    for (x, u), (xo, uo, _, rec) in zip(warm, lc.oracle_solves(name)):
        assert len(lc.ran(rec)) >= 1 and x.shape[0] == xo.shape[0] <= c["max_nodes"] + 1
    if c["d"]:
        assert np.abs(prob["x0"] - np.array([x[0] for x, _ in warm])).max() > 0.1 * c["d"]         # the measured state is far from the iterate's first node


def test_seeds_are_the_smallest_and_few():
    assert set(lc.SEEDS) <= set(lc.CASES)
    for name, seeds in lc.SEEDS.items():
        assert len(seeds) == lc.CASES[name]["batch"] and 3 * sum(1 for k in seeds if k) <= len(seeds)
        for b, k in enumerate(seeds):
            for smaller in range(k):
                trial = tuple(smaller if i == b else s for i, s in enumerate(seeds))
                c = lc.CASES[name]
                prob = lc.problem(c["robot"], c["batch"], c["n_intervals"], c["gait"])
                x, u = lc.warm_start(c["robot"], c["batch"], c["n_intervals"], c["gait"], trial)[b]
                rec = lc._oracle_solve(c, dict(prob, x0=lc.measured_state(prob["x0"], c["d"])), b, x, u, c["iterations"])[3]
                assert min(r[11] for r in lc.ran(rec)) < lc.DECISION_MARGIN, (name, b, smaller)


def test_branch_cases_reach_what_they_exist_for():
    """Deep back-tracking, a search that gives up after all 14 trials, one that accepts at trial 13 or 14, and steps that differ between the default
    and the Armijo settings (the branch changes the decision, not only the path to it)."""
    assert len(BRANCHES) == 12
    every = [t for n in BRANCHES for per_problem in lc.trials(n) for t in per_problem]
    assert max(every) == 14 and sum(1 for t in every if t >= 8) >= 4
    gave_up = accepted_late = 0
    for n in BRANCHES:
        for _, _, _, rec in lc.oracle_solves(n):
            for r in lc.ran(rec):
                gave_up += r[10] == 14 and r[3] == 0.0
                accepted_late += r[10] in (13, 14) and r[3] > 0.0
    assert gave_up >= 1 and accepted_late >= 1
    a3, d3 = lc.oracle_solves("branches-armijo-d1-it3"), lc.oracle_solves("branches-defaults-d1-it3")
    assert [int(r[10]) for r in lc.ran(a3[3][3])] == [8, 13, 14] and a3[3][3][2][3] == 0.0 and a3[3][3][1][3] == 2.0 ** -12
    assert lc.trials("branches-armijo-d1-it1") == [[3], [6], [3], [8], [9], [3]] and lc.trials("branches-armijo-d0.5-it1") == [[3], [5], [2], [7], [8], [2]]
    for d in ("d0.5", "d1"):
        differ = [b for b in range(6) if lc.oracle_solves("branches-armijo-%s-it1" % d)[b][3][0][3] != lc.oracle_solves("branches-defaults-%s-it1" % d)[b][3][0][3]]
        assert differ == [1, 3, 4], differ
    assert any(len(lc.ran(rec)) == 3 and rec[2][3] == 0.0 for _, _, _, rec in a3)          # the give-up is in iteration 3: iterations 1 and 2 moved the iterate


def test_stagger_case_stops_at_different_iterations():
    its = [len(t) for t in lc.trials("stagger")]
    assert its == [3, 2, 3, 2, 3, 3] and lc.CASES["stagger"]["iterations"] == 5


def test_horizon_cases():
    for name, nodes in (("horizon121", 121), ("horizon290", 290)):
        for s in ("defaults", "armijo"):
            assert lc.oracle_solves("%s-%s" % (name, s))[0][0].shape[0] == nodes + 1
        assert max(t[0] for s in ("defaults", "armijo") for t in lc.trials("%s-%s" % (name, s))) >= 4
    assert lc.trials("horizon121-armijo") == [[7], [3], [5]] and lc.trials("horizon290-armijo") == [[4], [5]] and lc.trials("horizon290-defaults") == [[4], [3]]
    assert max(t[0] for t in lc.trials("horizon121-defaults")) == 3        # the 121-node batch under the defaults back-tracks twice at most: its 4 trials come from the Armijo settings
    for n in (1, 2, 3):
        for s in ("armijo", "defaults"):
            name = "short%d-%s" % (n, s)
            assert lc.oracle_solves(name)[0][0].shape[0] == n + 1 and max(t[0] for t in lc.trials(name)) >= 2, name
        assert max(t[0] for t in lc.trials("short%d-armijo" % n)) >= 7


def test_nx24_cases_back_track_five_times():
    for robot in ("g1", "openloong"):
        assert lc.oracle_solves(robot)[0][0].shape[1] == 24 and max(t[0] for t in lc.trials(robot)) >= 5


def test_settings_cases():
    for name, count in (("reject_all", 14), ("reject_all_9", 9), ("reject_all_9_edge", 10)):
        assert lc.trials(name) == [[count]] * 6
        for (x, u), (xo, uo, _, rec) in zip(lc.case_inputs(name)[2], lc.oracle_solves(name)):
            assert rec[0][3] == 0.0 and np.array_equal(x, xo) and np.array_equal(u, uo)
    t = [t[0] for t in lc.trials("armijo_0.9")]
    assert min(t) == 3 and max(t) == 12 and min(lc.margin("armijo_0.9")) >= 1e-5
