"""GPU tier: the WBC's active-set QP (csrc/kernels/wbc.h) at its cap of 20 working-set changes, at singular working sets and at the threshold of
its equality-consistency test, against oracle/wbc_py.py on the populations of tests/wbc_stress_cases.py (labels A - E and "decisive" there;
tests/test_wbc_stress_cases.py asserts on the CPU that the populations contain what is relied on here).  Every launch is 32 robots with a row per
robot set through setParams, after a benign tick under the task.info rows that seeds the handle's last solutions (a fallback is then
distinguishable from zeros).

  every status 0   the vector satisfies the ORACLE's full QP by the tolerances of test_hip_wbc_matches_oracle (equalities, inequalities 1e-7,
                   stationarity on its tight set 1e-6 max(1, |g|)) and - new - the least-squares multipliers of its tight inequality rows are
                   >= -1e-6 max(1, |g|) (wbc_stress_cases.assert_kkt, which also says what is done where those multipliers are not unique)
  A                status 0, the oracle's objective to 1e-9; decisive robots: the oracle's tight set, iteration count and final working set;
                   five joints per leg (H1, Hunter): the oracle's vector to 1e-8
  B, D             status 1, reason 3 (change budget), 21 KKT solves, the previous solution bit for bit
  C                status 1, reason 2 (singular KKT system) or 3, the previous solution bit for bit
  boundary         the decisive robots of a model with exactly 21 and exactly 22 iterations in one batch: the former solved, the latter fall back
  mixed            successes and fallbacks interleaved: every robot as alone on a max_batch = 1 handle, bit for bit; a benign tick recovers the
                   robots that fell back; a second failing tick returns the latest successful vector, not the seed
  equalities       H1 double stance, measured velocity blended between consistent and not: status 0 where the oracle's residual is <= 1e-11,
                   status 1 / reason 1 where it is >= 1e-4, nothing asserted between

A non-decisive robot keeps every statement except the equality of iteration counts, working sets and tight sets.

Hunter's pull population has a seed per robot, chosen on the CPU so that every robot is decisive (tests/wbc_stress_cases.py).  With one stream
for the population 7 of its 32 robots were non-decisive, and the device showed what that means at the budget: it resolved a tie between the
lateral pyramid rows of heel and toe the other way and took another path - one robot with 22 oracle iterations was solved in 20 KKT solves, to
the oracle's minimum (KKT statement, objective 1e-9, vector 1e-8), and one with 20 oracle iterations ran out of budget after 21.  Neither is a
wrong answer; for a non-decisive robot the count, and with it the label A or B, is not the oracle's to fix.

Measured on an MI355X (pytest -s prints the figures):
  singularity test   `gmax > 1e-14` of the KKT elimination, class C robots.  H1: 21 robots, 17 ended singular (reason 2), 4 by the change budget
                     (the oracle meets their inconsistent working set after its 21st iteration); rejected pivots 0 .. 1.06e-17; smallest pivot
                     accepted 1.8e-11 on the way of a class C robot, 7.7e-07 among solved robots.  G1: 6 robots, all singular; rejected pivots
                     4.4e-18 .. 6.96e-16; smallest accepted 9.3e-12 (class C), 5.2e-07 (solved).  The threshold lies a factor 14 above the
                     largest pivot it rejected and 900 below the smallest it accepted.  No class C robot of any model returned status 0 and
                     every status 0 vector passed the KKT statement: no singular system slipped through, the kernel was left as it was.
  vector, class A    largest relative difference from the oracle: H1 2.5e-09 (lowtau; pull 3.0e-10), Hunter 1.2e-11: the existing 1e-8 holds
                     and no wider tolerance was needed (the two float64 CPU solves of the issue differ by up to 3.5e-09 on H1 lowtau).  Six
                     joints per leg, where only gauge-free statements are asserted: G1 2.3e-07, OpenLoong 5.5e-08.
  equalities         the device accepts up to an oracle residual of 6.4e-09 (eps 1e-2) and refuses from 6.4e-08 (eps 3.2e-2) on; the oracle's own
                     test flips at 1e-8, between the two.
  change budget      every decisive robot took the oracle's number of KKT solves and ended with its working set; H1 [22, 21, 21] and G1
                     [21, 22, 22, 21, 21] iterations in one batch: the 21s solved, the 22s fell back after 21 solves.
"""
import functools

import numpy as np
import pytest

from tests import wbc_params_cases as wc
from tests import wbc_stress_cases as sc

pytestmark = pytest.mark.gpu

ROBOT_POPS = [(r, n) for r, names in sc.ROBOT_POPULATIONS.items() for n in names]


def _unpack(d, nv):
    o = nv * nv + nv + 12 * nv
    nwork = int(d[o + 20])
    return dict(rank=int(d[o + 18]), iters=int(d[o + 19]), reason=int(d[o + 21]), minpiv=float(d[o + 22]), rejpiv=float(d[o + 23]),
                work=sorted(int(i) for i in d[o + 24:o + 24 + nwork]))


def _update(wbc, cases, modes, debug=False):
    return wbc.update([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], modes, debug=debug)


def _seeded(robot, max_batch=sc.B):
    """a handle whose last solutions are those of the benign tick 0 under the task.info rows: (handle, their values)"""
    import bipedal_control_amd as bp
    from bipedal_control_amd import scenarios
    wbc = bp.WeightedWbc(scenarios.interface(robot), max_batch=max_batch)
    cases = sc.benign_cases(robot, 0)
    sol0, st0 = _update(wbc, cases[:max_batch], sc.MODES[:max_batch])
    assert np.all(st0 == 0) and all(np.abs(s).max() > 0.0 for s in sol0)
    return wbc, sol0


@functools.lru_cache(maxsize=None)
def _run(robot, name):
    """one stressed tick of a population on a seeded handle: (seed solutions, solutions, statuses, debug records)"""
    pop = sc.population(robot, name)
    wbc, sol0 = _seeded(robot)
    wbc.setParams(pop["rows"])
    sol, status, dbg = _update(wbc, pop["cases"], pop["modes"], debug=True)
    nv = 6 + pop["m"]["nj"]
    return sol0, sol, status, [_unpack(d, nv) for d in dbg]


def _rel(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


_tight, _assert_kkt = sc.tight, sc.assert_kkt


def _objective(p, x):
    return 0.5 * x @ p["H"] @ x + p["g"] @ x


def _assert_robot(robot, s, prev, x, status, d, tag):
    """the statements of the module docstring for one robot: s its oracle record, prev its last solution, (x, status, d) what the device returned"""
    p = s["p"]
    if status == 0:
        _assert_kkt(p, x, tag)
    if s["label"] == "A":
        assert status == 0 and d["reason"] == 0, (tag, status, d)
        assert abs(_objective(p, x) - _objective(p, s["x"])) < 1e-9 * max(1.0, abs(_objective(p, s["x"]))), tag
        if s["decisive"]:
            assert _tight(p["D"], p["f"], x) == _tight(p["D"], p["f"], s["x"]), tag
            assert d["iters"] == s["iters"] and d["work"] == s["work"], (tag, d, s["iters"], s["work"])
        if robot in ("h1", "hunter"):            # five joints per leg: the minimiser is unique (see test_hip_wbc_matches_oracle)
            assert _rel(x, s["x"]) < 1e-8, (tag, _rel(x, s["x"]))
    elif s["label"] in "BD":
        assert status == 1 and d["reason"] == 3 and d["iters"] == sc.CAP, (tag, status, d)
        assert np.array_equal(x, prev), tag
    else:
        assert s["label"] == "C", tag
        assert status == 1 and d["reason"] in (2, 3), (tag, status, d)
        assert np.array_equal(x, prev), tag


@pytest.mark.parametrize("robot,name", ROBOT_POPS)
def test_population_against_the_oracle(robot, name):
    pop = sc.population(robot, name)
    sol0, sol, status, dbg = _run(robot, name)
    worst, missed = 0.0, []
    for b, s in enumerate(pop["sols"]):
        try:                                     # every robot is examined; the robots that miss a statement are reported together
            _assert_robot(robot, s, sol0[b], sol[b], status[b], dbg[b], (robot, name, b, s["label"], s["iters"]))
        except AssertionError as e:
            missed.append((b, s["label"], s["iters"], s["decisive"], int(status[b]), dbg[b]["reason"], dbg[b]["iters"], str(e).split("\n")[0][:120]))
        if s["x"] is not None and status[b] == 0:
            worst = max(worst, _rel(sol[b], s["x"]))
    print(robot, name, "labels", "".join(s["label"] for s in pop["sols"]), "status", "".join(map(str, status)), "reasons", "".join(str(d["reason"]) for d in dbg),
          "max vector difference of the solved robots %.2e" % worst)
    assert not missed, missed


@pytest.mark.parametrize("robot", ["h1", "g1"])
def test_pivot_margins_of_the_singularity_test(robot):
    """What the absolute test gmax > 1e-14 of the KKT elimination met: the rejected pivots of class C robots against the smallest pivots it accepted
    (of solved robots: regular systems).  The figures are printed; asserted is only what the threshold itself implies."""
    rejected, accepted_solved, accepted_c, reasons = [], [], [], []
    for name in sc.ROBOT_POPULATIONS[robot]:
        pop = sc.population(robot, name)
        _, _, status, dbg = _run(robot, name)
        for s, st, d in zip(pop["sols"], status, dbg):
            if st == 0:
                accepted_solved.append(d["minpiv"])
            if s["label"] == "C":
                reasons.append(d["reason"])
                accepted_c.append(d["minpiv"])
                if d["reason"] == 2:
                    rejected.append(d["rejpiv"])
    print(robot, "class C: %d robots, %d ended singular, %d by the change budget" % (len(reasons), reasons.count(2), reasons.count(3)))
    print(robot, "rejected pivots: largest %.3e smallest %.3e" % (max(rejected, default=0.0), min(rejected, default=0.0)))
    print(robot, "smallest accepted pivot: solved robots %.3e, class C robots %.3e" % (min(accepted_solved), min(accepted_c, default=np.inf)))
    assert all(0.0 <= r <= 1e-14 for r in rejected) and min(accepted_solved) > 1e-14


@pytest.mark.parametrize("robot", ["h1", "g1"])
def test_boundary_of_the_change_budget(robot):
    picked = [(pop, b) for pop in (sc.population(robot, n) for n in sc.MIXED_ORDER) for b, s in enumerate(pop["sols"])
              if s["decisive"] and s["label"] in "AB" and s["iters"] in (sc.CAP, sc.CAP + 1)][:sc.B]
    iters = [pop["sols"][b]["iters"] for pop, b in picked]
    assert sc.CAP in iters and sc.CAP + 1 in iters
    wbc, sol0 = _seeded(robot)
    n = len(picked)
    # robot k of the batch was seeded with benign case k
    wbc.setParams(np.array([pop["rows"][b] for pop, b in picked]).reshape(n, 32), mask=np.ones(n, np.int32))
    sol, status, dbg = _update(wbc, [pop["cases"][b] for pop, b in picked], [pop["modes"][b] for pop, b in picked], debug=True)
    nv = 6 + picked[0][0]["m"]["nj"]
    for k, (pop, b) in enumerate(picked):
        s, d = pop["sols"][b], _unpack(dbg[k], nv)
        _assert_robot(robot, s, sol0[k], sol[k], status[k], d, (robot, pop["name"], b, s["iters"]))
        assert (status[k] == 0) == (s["iters"] == sc.CAP) and d["iters"] == sc.CAP
    print(robot, "boundary batch: oracle iterations", iters, "status", status.tolist())


@pytest.mark.parametrize("robot", ["h1", "g1"])
def test_mixed_batch_isolation_recovery_and_latest_fallback(robot):
    import bipedal_control_amd as bp
    from bipedal_control_amd import scenarios
    pop = sc.population(robot, "mixed")
    m, rows, modes = pop["m"], pop["rows"], pop["modes"]
    default = wc.default_row(robot)
    wbc, sol0 = _seeded(robot)
    wbc.setParams(rows)
    sol1, st1, dbg1 = _update(wbc, pop["cases"], modes, debug=True)
    nv = 6 + m["nj"]
    for b, s in enumerate(pop["sols"]):
        _assert_robot(robot, s, sol0[b], sol1[b], st1[b], _unpack(dbg1[b], nv), (robot, "mixed", b, s["label"], s["iters"]))
    fell = np.nonzero(st1 == 1)[0]
    assert len(fell) >= 4 and len(fell) <= sc.B - 4 and sum(st1[b] != st1[b + 1] for b in range(sc.B - 1)) >= 4      # interleaved
    # every robot alone, from the same previous solution
    one = bp.WeightedWbc(scenarios.interface(robot), max_batch=1)
    seeds = sc.benign_cases(robot, 0)
    for b in range(sc.B):
        one.setParams(default)
        s0, t0 = _update(one, [seeds[b]], [modes[b]])
        assert t0[0] == 0 and np.array_equal(s0[0], sol0[b]), b
        one.setParams(rows[b])
        s1, t1 = _update(one, [pop["cases"][b]], [modes[b]])
        assert t1[0] == st1[b] and np.array_equal(s1[0], sol1[b]), (b, t1[0], st1[b])
    # a benign tick: the robots that fell back recover
    cases2, sols2 = sc.benign(robot, 1)
    wbc.setParams(np.tile(default, (sc.B, 1)))
    sol2, st2 = _update(wbc, cases2, modes)
    assert np.all(st2 == 0)
    for b in fell:
        s = sols2[b]
        assert s["label"] == "A"
        _assert_kkt(s["p"], sol2[b], (robot, "recovery", b))
        assert abs(_objective(s["p"], sol2[b]) - _objective(s["p"], s["x"])) < 1e-9 * max(1.0, abs(_objective(s["p"], s["x"])))
        if robot == "h1":
            assert _rel(sol2[b], s["x"]) < 1e-8, (b, _rel(sol2[b], s["x"]))
        assert not np.array_equal(sol2[b], sol0[b])
    # the failing tick again: the latest successful vector, not the seed
    wbc.setParams(rows)
    sol3, st3 = _update(wbc, pop["cases"], modes)
    assert np.array_equal(st3, st1)
    for b in range(sc.B):
        assert np.array_equal(sol3[b], sol2[b] if st1[b] else sol1[b]), b


def test_equality_consistency_threshold():
    """The device compares the unpivoted rows of its eliminated right-hand side with 10 * 1e-8 * its scale, the oracle the minimum-norm residual with
    1e-8 max(1, |d|): different measures, so between 1e-11 and 1e-4 of the oracle's nothing is asserted and the flip is printed."""
    cases, eps, res = sc.equality_blend()
    n = len(cases)
    assert n <= sc.B and (res <= 1e-11).sum() >= 4 and (res >= 1e-4).sum() >= 4
    wbc, sol0 = _seeded("h1", max_batch=n)
    sol, status, dbg = _update(wbc, cases, 3, debug=True)
    reasons = [_unpack(d, 16)["reason"] for d in dbg]
    for k in range(n):
        print("eps %.1e  oracle residual %.3e  status %d  reason %d" % (eps[k], res[k], status[k], reasons[k]))
        if res[k] <= 1e-11:
            assert status[k] == 0 and reasons[k] == 0, (eps[k], res[k])
        if res[k] >= 1e-4:
            assert status[k] == 1 and reasons[k] == 1 and np.array_equal(sol[k], sol0[k]), (eps[k], res[k])
        if status[k] == 1:
            assert reasons[k] == 1
    ok, bad = res[status == 0], res[status == 1]
    print("largest oracle residual the device accepts %.3e, smallest it refuses %.3e (the oracle flips at 1e-8)" % (ok.max(), bad.min()))
