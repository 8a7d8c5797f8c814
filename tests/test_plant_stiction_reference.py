"""CPU tier of the plant's stick-slip contacts (include/bpmpc.h "Plant"): properties of the numpy restatement tests/plant_stiction_reference.py that
tests/test_gpu_plant_stiction.py compares k_plant_stick_step against, and the scenario the two files share.
  kt = 0        the restatement returns exactly what plant_reference.substep returns, on the five robots of test_gpu_plant._cases, H1 and G1
  scenario      the five robots of test_gpu_plant._cases with kt = kn over three launches: 20 substeps; 2 substeps with the ground under the left
                foot of robot 2 lowered by 5 cm (its two points open); 2 substeps with the first ground again (they close and anchor afresh).  The
                restatement alone shows that the population holds sticking points, slipping points, points that open, points that re-close and
                re-anchor elsewhere, and an airborne robot, and that no decision is left to rounding: |d_i| > 1e-6, |n_i - contact_threshold| > 1e-6
                and, for every point that came into the substep anchored, |phi - cap| > 1e-6 max(1, cap).  (A point that anchors in the substep has
                s = a - p = 0 exactly and sticks whatever the cap: there is no decision.)
  invariants    over those 24 substeps: kt |a - p| <= mu n after the clamp; the anchor of a sticking point does not change; an open point has no
                anchor; A is symmetric positive definite.
The clamp's inequality holds in exact arithmetic.  In doubles a = p + s cap / phi is rounded at the magnitude of p (the contact points lie within a
metre of the origin) and s = a - p is formed again from it, so kt |a - p| may pass the cap by kt times a few units in the last place of |p|: the
bound asserted is cap + 8 eps kt max(1, |p|) (9e-11 N at kt = 5e4 N/m), the rounding of that one subtraction and nothing wider."""
import functools

import numpy as np

from tests import oracle_bridge as ob
from tests import plant_reference as pr
from tests import plant_stiction_reference as sr

KT = pr.DEFAULT_ROW[0]                      # kt = kn
LAUNCHES = (20, 2, 2)                       # substeps of the three launches
H = 0.0005                                  # substep length (test_gpu_plant.H)


def _base(robot):
    from tests import test_gpu_plant as tp
    assert tp.H == H
    return tp._cases(robot), tp._limits(robot)


def grounds(robot):
    """the ground heights [5, 4] of the three launches"""
    (_, _, _, _, ground), _ = _base(robot)
    low = ground.copy()
    low[2, :2] = -0.05
    return ground, low, ground


@functools.lru_cache(maxsize=None)
def stiction_reference(robot, launches=LAUNCHES):
    """The restatement over the launches with kt = kn: per robot the list of substep dicts (every launch's substeps in sequence); the restatement's
    own floor as test_gpu_plant._reference measures it (v+ of numpy.linalg.solve against a Cholesky solve of the same system, relative to
    max(1, |v+|)); and the same floor for the contact forces, f - D J v+ formed from the two solutions, relative to max(1, |force|) - D reaches
    mu n / v_eps, some 1e4 N s/m, so the forces carry the solvers' difference a hundred times larger than v+ does.  Computed once per robot and
    launch plan; every decision is checked to be decisive."""
    m = ob.model(robot)
    (q, v, cmd, force, _), lim = _base(robot)
    steps, floor, floor_force = [], 0.0, 0.0
    for b in range(q.shape[0]):
        qb, vb, rows = q[b], v[b], []
        anchor, anchored = sr.no_anchors()
        cb = {k: a[b] for k, a in cmd.items()}
        for n, ground in zip(launches, grounds(robot)):
            for _ in range(n):
                s = sr.substep(m, qb, vb, cb, H, KT, anchor, anchored, ground=ground[b], w_ext=force[b], torque_limits=lim)
                assert np.abs(s["d"]).min() > 1e-6, (robot, b, s["d"])
                assert np.abs(s["n"] - pr.DEFAULT_ROW[5]).min() > 1e-6, (robot, b, s["n"])
                decided = (anchored != 0) & s["closed"]
                assert np.all(np.abs(s["phi"] - s["cap"])[decided] > 1e-6 * np.maximum(1.0, s["cap"][decided])), (robot, b, s["phi"], s["cap"])
                s["anchored_before"], s["anchor_before"] = anchored.copy(), anchor.copy()
                sol = pr.cholesky_solve(s["A"], s["rhs"])
                floor = max(floor, float((np.abs(sol - s["v"]) / np.maximum(1.0, np.abs(s["v"]))).max()))
                spread = (s["D"] * (s["J"] @ (sol - s["v"]))).reshape(sr.NC, 3)
                spread[~s["closed"]] = 0.0
                floor_force = max(floor_force, float((np.abs(spread) / np.maximum(1.0, np.abs(s["force"]))).max()))
                rows.append(s)
                qb, vb, anchor, anchored = s["q"], s["v"], s["anchor"], s["anchored"]
        steps.append(rows)
    return steps, floor, floor_force


def test_kt_zero_is_the_plant_without_stiction():
    from tests import test_gpu_plant as tp
    for robot in ("h1", "g1"):
        m = ob.model(robot)
        (q, v, cmd, force, ground), lim = _base(robot)
        for b in range(tp.B5):
            cb = {k: a[b] for k, a in cmd.items()}
            ref = pr.substep(m, q[b], v[b], cb, H, ground=ground[b], w_ext=force[b], torque_limits=lim)
            new = sr.substep(m, q[b], v[b], cb, H, 0.0, *sr.no_anchors(), ground=ground[b], w_ext=force[b], torque_limits=lim)
            for k, val in ref.items():
                assert np.array_equal(np.asarray(val), np.asarray(new[k])), (robot, b, k)
            assert not new["anchored"].any() and not new["anchor"].any() and np.all(new["stick"] == -1)


def test_the_population_holds_every_kind():
    steps, _, _ = stiction_reference("h1")
    stick = np.array([[s["stick"] for s in rows] for rows in steps])                 # [robot, substep, point]
    anchored = np.array([[s["anchored"] for s in rows] for rows in steps])
    closed = np.array([[s["closed"] for s in rows] for rows in steps])
    n1, n2 = LAUNCHES[0], LAUNCHES[0] + LAUNCHES[1]
    kept = np.array([[s["anchored_before"] for s in rows] for rows in steps]) != 0
    print("sticking decisions", int(((stick == 1) & kept).sum()), "slipping", int((stick == 0).sum()), "open", int((stick == -1).sum()))
    assert ((stick == 1) & kept).any() and (stick == 0).any()                          # sticking on an older anchor, slipping
    assert not closed[0].any() and not anchored[0].any()                               # the airborne robot
    assert (closed[:, 0] & ~closed[:, n1 - 1]).any()                                   # a point that opens within the first launch
    # robot 2's left foot: anchored through the first launch, open in the second, closed and anchored elsewhere in the third
    assert anchored[2, n1 - 1, :2].all() and not anchored[2, n1:n2, :2].any() and anchored[2, n2:, :2].all()
    first, again = steps[2][n1 - 1]["anchor"][:2], steps[2][n2]["anchor"][:2]
    assert np.all(np.abs(again - first).max(axis=1) > 1e-6), (first, again)
    assert np.array_equal(again, steps[2][n2]["p"][:2, :2])                            # a fresh anchor is the point itself


def test_invariants_over_the_scenario():
    steps, _, _ = stiction_reference("h1")
    assert sum(LAUNCHES) == len(steps[0]) == 24
    eps = np.finfo(float).eps
    worst = 0.0
    for rows in steps:
        for s in rows:
            on = s["anchored"] != 0
            assert np.array_equal(on, s["closed"])                                      # closed points are anchored, open points are not
            pull = KT * np.linalg.norm(s["anchor"] - s["p"][:, :2], axis=1)
            cap = pr.DEFAULT_ROW[3] * s["n"]
            slack = 8 * eps * KT * np.maximum(1.0, np.abs(s["p"][:, :2]).max(axis=1))
            worst = max(worst, float((pull - cap)[on].max(initial=-np.inf)))
            assert np.all(pull[on] <= (cap + slack)[on]), (pull, cap)
            held = (s["stick"] == 1) & (s["anchored_before"] != 0)
            assert np.array_equal(s["anchor"][held], s["anchor_before"][held])
            A = s["A"]
            assert np.abs(A - A.T).max() <= 1e-12 * np.abs(A).max()
            assert np.linalg.eigvalsh(0.5 * (A + A.T)).min() > 0.0
            np.linalg.cholesky(A)
    print("largest kt |a - p| - mu n over the scenario", worst)
