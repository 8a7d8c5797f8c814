"""CPU tier of the value function (include/bpmpc.h "Value function"): the numpy restatement tests/value_function_reference.py held to the oracle's QP
(oracle_py.OracleModel.node_lq / qp_step) on a trot case of 21 intervals with one event node inside the grid, a perturbed iterate and dx0 != 0.
Tolerances: 1e-12 relative for the identities, 1e-9 for the finite differences.  No device."""
import functools

import numpy as np
import pytest

from oracle import reference_py as rp
from tests import oracle_bridge as ob
from tests import value_function_reference as vf

IDENTITY_TOL, FD_TOL, FD_STEP = 1e-12, 1e-9, 1e-4


class Case:
    """One problem: the oracle's nodes, an iterate off the cold start, a start state off the iterate's, the oracle's QP step and the value function."""

    def __init__(self, robot):
        from bipedal_control_amd import scenarios as sc
        itf = sc.interface(robot)
        prob = sc.trot_problem(itf, batch=1, n_intervals=20)
        self.om, self.nodes = ob.oracle(robot), ob.oracle_nodes(prob, 0, robot=robot)
        self.n, self.kind = int(self.nodes["N"]), np.asarray(self.nodes["kind"])
        rng = np.random.default_rng(7)
        x, u = rp.cold_start(ob.model(robot), self.nodes, prob["x0"][0])
        self.x = x + 0.01 * rng.uniform(-1, 1, x.shape)
        self.u = u + 0.5 * rng.uniform(-1, 1, u.shape)
        self.x0 = self.x[0] + 0.02 * rng.uniform(-1, 1, x.shape[1])
        self.lq = vf.oracle_lq(self.om, self.nodes, self.x, self.u)
        self.dx, self.du, self.K = self.om.qp_step(self.nodes, self.x0, self.x, self.u)
        self.S, self.s, self.v = vf.value_recursion(self.lq, self.K, self.dx, self.du, self.kind)

    def optimum(self, x0):
        dx, du, _ = self.om.qp_step(self.nodes, x0, self.x, self.u)
        return vf.tail_costs(self.lq, dx, du, self.kind)[0]


@functools.lru_cache(maxsize=None)
def _case(robot):
    return Case(robot)


@pytest.fixture(scope="module", params=["h1", "g1"])
def case(request):
    return _case(request.param)


def test_case_has_an_event_node_inside_the_grid_and_a_start_off_the_iterate(case):
    events = np.nonzero(case.kind)[0]
    assert len(events) >= 1 and 0 < events[0] < case.n - 1
    assert case.n - len(events) >= 20
    assert np.abs(case.dx[0]).max() > 1e-3


def test_tail_cost_identity_at_every_node(case):
    tails = vf.tail_costs(case.lq, case.dx, case.du, case.kind)
    scale = np.abs(tails).max()
    for k in range(case.n + 1):
        assert abs(vf.value_at(case.S, case.s, case.v, k, case.dx[k]) - tails[k]) <= IDENTITY_TOL * scale, k


def test_v0_is_the_optimum_of_the_qp_from_other_start_states(case):
    rng = np.random.default_rng(11)
    for _ in range(4):
        x0 = case.x[0] + 0.05 * rng.uniform(-1, 1, case.x.shape[1])
        want = case.optimum(x0)
        got = vf.value_at(case.S, case.s, case.v, 0, x0 - case.x[0])
        assert abs(got - want) <= IDENTITY_TOL * abs(want)


def test_gradient_against_central_differences():
    case = _case("h1")                      # G1 repeats the identities; the finite differences are taken on H1
    grad = case.s[0] + case.S[0] @ case.dx[0]
    fd = np.zeros_like(grad)
    for i in range(len(grad)):
        e = np.zeros_like(grad)
        e[i] = FD_STEP
        fd[i] = (case.optimum(case.x0 + e) - case.optimum(case.x0 - e)) / (2 * FD_STEP)
    assert np.abs(fd - grad).max() <= FD_TOL * np.abs(grad).max()


def test_symmetry_and_definiteness(case):
    for k in range(case.n + 1):
        assert np.array_equal(case.S[k], case.S[k].T), k
    for k in range(case.n):
        assert np.linalg.eigvalsh(case.S[k]).min() > 0, k
    assert not case.S[case.n].any() and not case.s[case.n].any() and case.v[case.n] == 0


def test_an_event_node_passes_S_through_unchanged(case):
    for k in np.nonzero(case.kind)[0]:
        assert np.array_equal(case.S[k], case.S[k + 1])


def test_double_agrees_with_extended_precision(case):
    """The recursion in double against the same text in np.longdouble, per node relative to the node's largest entry: what the GPU tier calls r."""
    Se, se, ve = vf.value_recursion(case.lq, case.K, case.dx, case.du, case.kind, np.longdouble)
    assert vf.relative_distance(case.S, Se) < 1e-14
    assert vf.relative_distance(case.s, se) < 1e-13
    assert vf.relative_distance(case.v, ve) < 1e-13


def test_query_interpolates_between_nodes_and_clamps(case):
    times = np.asarray(case.nodes["times"])
    x = case.x0
    f, g, H = vf.query(times, case.S, case.s, case.v, case.x, times[3], x)
    assert np.isclose(f, vf.value_at(case.S, case.s, case.v, 3, x - case.x[3]), rtol=1e-13)
    assert np.array_equal(H, case.S[3])
    f_lo = vf.query(times, case.S, case.s, case.v, case.x, times[0] - 1.0, x)[0]
    assert f_lo == vf.query(times, case.S, case.s, case.v, case.x, times[0], x)[0]
    f_hi, g_hi, H_hi = vf.query(times, case.S, case.s, case.v, case.x, times[-1] + 1.0, x)
    assert f_hi == 0 and not g_hi.any() and not H_hi.any()
    tm = 0.5 * (times[4] + times[5])
    H_mid = vf.query(times, case.S, case.s, case.v, case.x, tm, x)[2]
    assert np.allclose(H_mid, 0.5 * (case.S[4] + case.S[5]), rtol=1e-12, atol=0)
