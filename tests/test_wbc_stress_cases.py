"""CPU tier: the populations of tests/wbc_stress_cases.py contain what tests/test_gpu_wbc_stress.py relies on, by the oracle alone; and the optional
trace of oracle/wbc_py.py:solve_qp changes no result.

Counts found with the committed seeds (A solved within the device's 21 KKT solves, B solved with more, C working set inconsistent, D cycling;
"21" / "22": decisive robots with exactly that many iterations; "A12": decisive A robots with 12 iterations or more; "nd": non-decisive robots):
  COUNTS below, asserted entry for entry.  Per model: H1 34 A12, two robots at 21, one at 22, 8 B, 21 C; G1 35 A12, three at 21, two at 22,
  13 B, 6 C.  Cycling robots (D) occur with other seeds (H1 pull 3, lowtau 3; G1 pull 1 and 2, both 2; Hunter both 0, 1, 4); the committed seeds
  pass them over because each costs 400 oracle iterations.

Hunter's pull population has a seed per robot (tests/wbc_stress_cases.py says why): with one stream for the population, seeds 0 .. 67 give
between 7 and 12 non-decisive robots of 32, because the lateral pyramid rows of the heel and toe points of a Hunter foot, which lie on one line,
tie to 1e-13 (e.g. 1.8743182418323778 against 1.8743182418322553) and rounding picks the row that is added."""
import numpy as np
import pytest

from oracle import wbc_py as wp
from tests import oracle_bridge as ob
from tests import wbc_stress_cases as sc
from tests.test_wbc import _case, _task

# (robot, population) -> (A, B, C, D, A12, exactly 21, exactly 22, non-decisive)
COUNTS = {("h1", "pull"): (26, 6, 0, 0, 11, 1, 1, 0), ("h1", "both"): (26, 0, 6, 0, 9, 1, 0, 0), ("h1", "zeroF"): (22, 2, 8, 0, 7, 0, 0, 0),
          ("h1", "lowtau"): (25, 0, 7, 0, 2, 0, 0, 0),
          ("g1", "pull"): (26, 6, 0, 0, 6, 0, 0, 0), ("g1", "both"): (31, 0, 1, 0, 15, 0, 0, 0), ("g1", "zeroF"): (27, 5, 0, 0, 13, 2, 2, 0),
          ("g1", "lowtau"): (25, 2, 5, 0, 1, 1, 0, 0),
          ("hunter", "both"): (22, 2, 8, 0, 8, 1, 0, 0), ("hunter", "pull"): (31, 1, 0, 0, 13, 0, 1, 0),
          ("openloong", "both"): (27, 2, 3, 0, 16, 1, 0, 0), ("openloong", "pull"): (29, 3, 0, 0, 6, 1, 0, 0)}


@pytest.mark.parametrize("mode", [3, 1])
def test_trace_changes_no_result(mode):
    m = ob.model("h1")
    st = sc.wc.settings_from_row(sc.stress_row("h1", "both"), m["nj"])
    x, u, rbd, q, v = _case(m, mode, np.random.default_rng(20 + mode), speed=1.0)
    p = wp.formulate(m, st, x, u, rbd, mode)
    H, g = p["Aw"].T @ p["Aw"], -p["Aw"].T @ p["bw"]
    plain = wp.solve_qp(H, g, p["Aeq"], p["beq"], p["D"], p["f"])
    trace = []
    traced = wp.solve_qp(H, g, p["Aeq"], p["beq"], p["D"], p["f"], trace=trace)
    assert np.array_equal(plain[0], traced[0]) and np.array_equal(plain[1], traced[1]) and plain[2:] == traced[2:]
    assert len(trace) == plain[3] > 1 and trace[-1]["decision"] == "done" and all(e["decision"] in ("add", "drop") for e in trace[:-1])
    # the trace replays: the working set of every iteration follows from the decisions before it
    work = []
    for e in trace:
        assert e["work"] == work
        if e["decision"] == "add":
            assert e["index"] not in work and e["viol"] > 1e-9 and e["viol"] >= e["viol_second"]
            work.append(e["index"])
        elif e["decision"] == "drop":
            assert e["viol"] <= 1e-9 and e["mu"] < -1e-9 and e["mu"] <= e["mu_second"]
            work.pop(e["index"])
    assert e["viol"] <= 1e-9 and e["mu"] >= -1e-9


def test_decisive_rule():
    base = dict(work=[], index=0, residual=0.0)
    add = lambda v, v2: dict(base, decision="add", viol=v, viol_second=v2, mu=np.inf, mu_second=np.inf)           # noqa: E731
    drop = lambda mu, mu2, v=-1.0: dict(base, decision="drop", viol=v, viol_second=v, mu=mu, mu_second=mu2)       # noqa: E731
    done = lambda v, mu: dict(base, decision="done", viol=v, viol_second=v, mu=mu, mu_second=mu)                  # noqa: E731
    assert sc.decisive([add(1.0, 0.5), drop(-1.0, -0.5), done(-1.0, 0.1)])
    assert not sc.decisive([add(1.0, 1.0 - 1e-7)]) and sc.decisive([add(1.0, 1.0 - 1e-5)])                       # a win by 1e-6 max(1, |value|)
    assert not sc.decisive([add(100.0, 100.0 - 1e-5)])
    assert not sc.decisive([add(5e-8, -1.0)]) and not sc.decisive([done(5e-11, 1.0)]) and sc.decisive([done(5e-12, 1.0)])     # within 100 of tol
    assert not sc.decisive([drop(-1.0, -1.0 + 1e-7)]) and not sc.decisive([drop(-5e-8, 1.0)]) and not sc.decisive([done(-1.0, -5e-11)])
    assert sc.decisive([done(-1.0, -5e-12)]) and sc.decisive([done(-np.inf, np.inf)])


@pytest.mark.parametrize("robot,name", sorted(COUNTS))
def test_population_counts_and_share_of_nondecisive_robots(robot, name):
    pop = sc.population(robot, name)
    assert len(pop["cases"]) == len(pop["sols"]) == sc.B and pop["rows"].shape == (sc.B, 32) and pop["modes"] == [3, 1, 2, 0] * 8
    c = sc.counts(pop)
    got = (c["A"], c["B"], c["C"], c["D"], c["A12"], c["at21"], c["at22"], c["nondecisive"])
    print(robot, name, got, " ".join("%s%d%s" % (s["label"], s["iters"], "" if s["decisive"] else "?") for s in pop["sols"]))
    assert c["E"] == 0                                         # the equalities themselves are consistent: every fallback is the iteration's
    assert got == COUNTS[(robot, name)], (robot, name, got)
    seed = sc.SEEDS[(robot, name)]
    again = sc._cases(robot, name, seed)                       # deterministic by seed
    assert all(np.array_equal(a, b) for ca, cb in zip(again, pop["cases"]) for a, b in zip(ca, cb))
    assert c["nondecisive"] <= 0.1 * sc.B, (robot, name, c["nondecisive"])
    if isinstance(seed, tuple):                                # a seed per robot: 100 b + k, and every k before the one taken gives a non-decisive robot
        assert len(seed) == sc.B and all(100 * b <= s < 100 * (b + 1) for b, s in enumerate(seed))
        st = sc.wc.settings_from_row(sc.stress_row(robot, name), pop["m"]["nj"])
        for b, s in enumerate(seed):
            for earlier in range(100 * b, s):
                trial = list(seed); trial[b] = earlier
                assert not sc.solve(pop["m"], st, sc._cases(robot, name, tuple(trial))[b], sc.MODES[b])["decisive"], (b, earlier)


@pytest.mark.parametrize("robot", ["h1", "g1"])
def test_a_model_has_every_class_the_boundary_and_a_mixed_batch(robot):
    assert set(sc.ROBOT_POPULATIONS) == {r for r, _ in COUNTS} and all(set(v) == {n for r, n in COUNTS if r == k} for k, v in sc.ROBOT_POPULATIONS.items())
    A, Bc, C, D, A12, at21, at22, nd = np.sum([sc_ for (r, n), sc_ in COUNTS.items() if r == robot], axis=0)      # asserted entry for entry above
    assert A12 >= 8 and at21 >= 1 and at22 >= 1 and Bc >= 4 and C >= 4
    mixed = sc.population(robot, "mixed")
    labels = [s["label"] for s in mixed["sols"]]
    fail = [lb != "A" for lb in labels]
    assert 4 <= sum(fail) <= sc.B - 4 and sum(a != b for a, b in zip(fail[:-1], fail[1:])) >= 4, labels
    for b in range(sc.B):
        src = sc.population(robot, sc.MIXED_ORDER[(b // 4) % 4])
        assert mixed["sols"][b] is src["sols"][b] and np.array_equal(mixed["rows"][b], src["rows"][b]) and mixed["cases"][b] is src["cases"][b]
    assert len({tuple(r) for r in mixed["rows"]}) == 4
    for which in (0, 1):                                       # the seeding tick and the recovery tick are solved by every robot
        assert all(s["label"] == "A" for s in sc.benign(robot, which)[1])


def test_equality_blend_has_both_sides():
    cases, eps, res = sc.equality_blend()
    assert len(cases) <= sc.B and (res <= 1e-11).sum() >= 4 and (res >= 1e-4).sum() >= 4
    assert res[0] <= 1e-11 and res[-1] >= 1e-4
    m = ob.model("h1")
    st = wp.load_settings(_task("h1"), 10)
    for k in (0, len(cases) - 1):                              # the ends behave as the fallback test of tests/test_wbc.py says
        assert wp.update(m, st, cases[k][0], cases[k][1], cases[k][2], 3)[1]["status"] == (0 if k == 0 else 1)


def test_kkt_statement_accepts_the_oracle_and_refuses_a_negative_multiplier():
    # a point that is stationary on its tight set with a NEGATIVE multiplier (the plain least-squares stationarity check accepts it):
    # min 1/2 |x|^2 - (1, 1) x  s.t. x_0 <= 2  at x = (2, 1); the minimiser (1, 1) passes
    p = dict(Aeq=np.zeros((0, 2)), beq=np.zeros(0), D=np.array([[1.0, 0.0]]), f=np.array([2.0]), H=np.eye(2), g=-np.ones(2))
    sc.assert_kkt(p, np.array([1.0, 1.0]), "minimiser")
    with pytest.raises(AssertionError):
        sc.assert_kkt(p, np.array([2.0, 1.0]), "negative multiplier")
    # dependent tight rows: the apex of a pyramid.  min 1/2 |x - (-1, 0, -1)|^2 over the cone {x_2 >= 0, |x_0|, |x_1| <= x_2} is its apex
    pyr = np.array([[0, 0, -1], [1, 0, -1], [-1, 0, -1], [0, 1, -1], [0, -1, -1]], float)
    cone = dict(Aeq=np.zeros((0, 3)), beq=np.zeros(0), D=pyr, f=np.zeros(5), H=np.eye(3), g=np.array([1.0, 0.0, 1.0]))
    assert sc.assert_kkt(cone, np.zeros(3), "apex")[1] >= 0.0
    cone["g"] = np.array([1.0, 0.0, -2.0])                     # now the apex is not the minimiser ((-0.5, 0, 0.5) ... is better): refused
    with pytest.raises(AssertionError):
        sc.assert_kkt(cone, np.zeros(3), "apex, not optimal")
    # the oracle's own solutions of two stressed populations, degenerate ones included
    seen_degenerate = 0
    for name in ("pull", "both"):
        for s in sc.population("h1", name)["sols"]:
            if s["x"] is not None:
                sc.assert_kkt(s["p"], s["x"], ("h1", name))
                E, e, D, f = sc.split_rows(s["p"])
                Ga = np.vstack([E, D[sorted(sc.tight(D, f, s["x"]))]])
                seen_degenerate += np.linalg.matrix_rank(Ga) < len(Ga)
    assert seen_degenerate >= 4
