"""CPU tier of the plan geometry (include/bpmpc.h "Plan geometry"): bpmpc_plan_rows_host, which is compiled from the text the kernels are compiled
from (csrc/kernels/plan_geometry.h), against the numpy restatement tests/plan_geometry_reference.py.
  rows, footholds, summary   H1 and G1, 70 nodes (the 64 accumulators of the summary wrap), five events of which two in a row; 1e-12 absolute -
                             the bound tests/test_gpu_telemetry.py holds the same kinematics to; modes, kinds, masks and flags exactly
  the foothold rule          hand-made tables: an event at the first node and one at the last node (both excluded), two events in a row, a foot that
                             lifts (no entry) and one that lands (two entries, points in order), 9 landings (count 18, 16 stored), n_nodes = 1
  closed forms               the centre of pressure of equal forces is the mean of the points; a plan without inputs; a state that is not finite
Every comparison prints its maximum before it asserts (pytest -s)."""
import numpy as np
import pytest

from tests import oracle_bridge as ob
from tests import plan_geometry_reference as pr

TOL = 1e-12
FLY, LF, RF, STANCE = 0, 1, 2, 3


def _itf(robot):
    from bipedal_control_amd import scenarios as sc
    return sc.interface(robot)


def _host(robot, t, x, mode, kind, u=None):
    import bipedal_control_amd as bp
    return bp.PlanGeometry.rows_host(_itf(robot), t, x, mode, kind, u)


def table(phases, per=2, dt=0.1, t0=0.0, event_first=False, event_last=False):
    """(t [n + 1], mode [n], kind [n]) of a grid with `per` intermediate nodes per phase and a pre-event node between two phases; the pre-event
    node carries the mode of the phase it ends and the time of the node behind it"""
    mode, kind = [], []
    for p, md in enumerate(phases):
        mode += [md] * per
        kind += [0] * per
        if p + 1 < len(phases):
            mode.append(md)
            kind.append(1)
    if event_first:
        mode.insert(0, phases[0]); kind.insert(0, 1)
    if event_last:
        mode.append(phases[-1]); kind.append(1)
    t = [t0]
    for kd in kind:
        t.append(t[-1] + (0.0 if kd == 1 else dt))
    return np.array(t), np.array(mode, np.int32), np.array(kind, np.int32)


def random_states(m, count, rng):
    """[count, nx] in the ranges of tests/test_gpu_telemetry.py _episode: joints within 0.5 rad of the default joint state, base height 0.6 .. 1.1,
    pitch and roll up to 1.2, any yaw"""
    nj = m["nj"]
    q0 = np.array(m["initial_state"], float)[12:]
    x = np.zeros((count, 12 + nj))
    x[:, 0:6] = rng.standard_normal((count, 6))
    x[:, 6:8] = rng.uniform(-2.0, 2.0, (count, 2))
    x[:, 8] = rng.uniform(0.6, 1.1, count)
    x[:, 9] = rng.uniform(-3.0, 3.0, count)
    x[:, 10:12] = rng.uniform(-1.2, 1.2, (count, 2))
    x[:, 12:] = q0 + rng.uniform(-0.5, 0.5, (count, nj))
    return x


def random_inputs(m, count, rng, zero_forces=False):
    """[count, nu]: f_z in 50 .. 400 N (or all contact forces 0), everything else of order 1"""
    u = rng.standard_normal((count, 12 + m["nj"]))
    for i in range(4):
        u[:, 3 * i + 2] = rng.uniform(50.0, 400.0, count)
    if zero_forces:
        u[:, :12] = 0.0
    return u


def random_plan(m, n, rng, events=(), zero_forces=False, gait=(STANCE, LF, STANCE, RF)):
    """(t, x, mode, kind, u) of n nodes whose pre-event nodes are `events`"""
    kind = np.zeros(n, np.int32)
    kind[list(events)] = 1
    mode, t, phase = np.zeros(n, np.int32), np.zeros(n + 1), 0
    for k in range(n):
        mode[k] = gait[phase % len(gait)]
        t[k + 1] = t[k] + (0.0 if kind[k] else 0.015)
        phase += int(kind[k])
    return t, random_states(m, n + 1, rng), mode, kind, random_inputs(m, n, rng, zero_forces)


def compare(got, want, what):
    """the asserts of one robot's (rows, footholds, count, summary) against the restatement's; returns the largest differences it printed"""
    rows, foot, count, summ = got
    rw, entries, cnt, sm = want
    n = len(rw) - 1
    ok = rw[:, pr.BAD] == 0.0
    d_rows = np.abs(rows[ok][:, :pr.TIME] - rw[ok][:, :pr.TIME]).max() if ok.any() else 0.0
    stored = min(cnt, pr.MAX_FOOTHOLDS)
    d_foot = np.abs(foot[:stored, 2:5] - entries[:stored, 2:5]).max() if stored else 0.0
    d_path = abs(summ[pr.S_PATH] - sm[pr.S_PATH])
    d_max = np.abs(summ[pr.S_APEX:pr.S_MIN_SUM_Z + 1] - sm[pr.S_APEX:pr.S_MIN_SUM_Z + 1]).max()
    print("plan geometry %s: rows %.3e, footholds %.3e (count %d), path length %.3e over %d terms, maxima %.3e" % (what, d_rows, d_foot, cnt, d_path, n, d_max))
    assert d_rows <= TOL
    assert np.array_equal(rows[:, pr.TIME:], rw[:, pr.TIME:])      # t, mode, kind, sum_z (three additions in the stated order), mask, flag
    assert count == cnt
    assert np.array_equal(foot[:stored][:, [0, 1, 5]], entries[:stored][:, [0, 1, 5]]) and d_foot <= TOL
    assert d_path <= TOL * max(n, 1) and d_max <= TOL
    assert np.array_equal(summ[[pr.S_NODES, pr.S_FOOTHOLDS, pr.S_BAD]], sm[[pr.S_NODES, pr.S_FOOTHOLDS, pr.S_BAD]]) and np.all(summ[13:] == 0.0)
    return d_rows, d_foot, d_path, d_max


@pytest.mark.parametrize("robot", ["h1", "g1"])
def test_rows_host_against_restatement(robot):
    m = ob.model(robot)
    t, x, mode, kind, u = random_plan(m, 70, np.random.default_rng(5), events=(5, 11, 12, 30, 66))
    got = _host(robot, t, x, mode, kind, u)
    want = pr.plan(m, t, x, mode, kind, u)
    compare(got, want, robot + " host")
    assert got[2] >= 4 and got[3][pr.S_PATH] > 10.0 and got[3][pr.S_MIN_SUM_Z] >= 200.0
    # the copies are the inputs' bits
    assert np.array_equal(got[0][:, 0:3], x[:, 6:9]) and np.array_equal(got[0][:, pr.TIME], t)
    assert got[0][-1, pr.MODE] == -1 and got[0][-1, pr.KIND] == -1 and np.all(got[0][-1, [15, 16, 17, 21, 22]] == 0.0)


def _nominal(m, n):
    return np.tile(np.array(m["initial_state"], float), (n + 1, 1))


def _footholds(robot, t, mode, kind):
    m = ob.model(robot)
    n = len(mode)
    x = _nominal(m, n)
    x[:, 6] = np.linspace(0.0, 1.0, n + 1)          # the base moves forward, so every node has contact points of its own
    got = _host(robot, t, x, mode, kind)
    compare(got, pr.plan(m, t, x, mode, kind), "%s table of %d nodes" % (robot, n))
    return got


def test_events_at_the_first_and_the_last_node_are_excluded():
    t, mode, kind = table([LF, STANCE], event_first=True, event_last=True)
    assert kind[0] == 1 and kind[-1] == 1 and t[0] == t[1] and t[-1] == t[-2]
    rows, foot, count, summ = _footholds("h1", t, mode, kind)
    assert count == 2 and foot[:2, 1].tolist() == [2.0, 3.0]                  # the landing between the two phases, and nothing at either end
    t, mode, kind = table([LF], event_first=True, event_last=True)
    assert _footholds("h1", t, mode, kind)[2] == 0


def test_two_events_in_a_row():
    """both pre-event nodes see LF before and STANCE behind them: each gives the right foot's two points, from its own post-event node"""
    t = np.array([0.0, 0.1, 0.2, 0.2, 0.2, 0.3, 0.4])
    mode = np.array([LF, LF, LF, LF, STANCE, STANCE], np.int32)
    kind = np.array([0, 0, 1, 1, 0, 0], np.int32)
    rows, foot, count, summ = _footholds("h1", t, mode, kind)
    assert count == 4 and foot[:4, 1].tolist() == [2.0, 3.0, 2.0, 3.0] and foot[:4, 5].tolist() == [3.0, 3.0, 4.0, 4.0]
    assert np.array_equal(foot[0, 2:5], rows[3, 9:12]) and np.array_equal(foot[3, 2:5], rows[4, 12:15])


def test_a_lifting_foot_gives_nothing_and_a_landing_foot_two_entries():
    t, mode, kind = table([STANCE, LF])                                       # the right foot lifts
    assert _footholds("g1", t, mode, kind)[2] == 0
    t, mode, kind = table([RF, STANCE])                                       # the left foot lands
    rows, foot, count, summ = _footholds("g1", t, mode, kind)
    assert count == 2 and foot[:2, 1].tolist() == [0.0, 1.0] and foot[:2, 5].tolist() == [3.0, 3.0] and foot[0, 0] == t[3]
    assert np.array_equal(foot[0, 2:5], rows[3, 3:6]) and np.array_equal(foot[1, 2:5], rows[3, 6:9]) and np.all(foot[2:] == 0.0)
    t, mode, kind = table([FLY, STANCE])                                      # both land: four entries in the order of the points
    assert _footholds("g1", t, mode, kind)[1][:4, 1].tolist() == [0.0, 1.0, 2.0, 3.0]


def test_nine_landings_count_eighteen_and_store_sixteen():
    phases = [LF]
    for p in range(9):
        phases += [STANCE, RF if p % 2 == 0 else LF]
    t, mode, kind = table(phases)
    rows, foot, count, summ = _footholds("h1", t, mode, kind)
    assert count == 18 and summ[pr.S_FOOTHOLDS] == 18.0 and len(t) - 1 > 48
    assert np.all(np.diff(foot[:, 5]) >= 0) and foot[:, 1].tolist() == [2.0, 3.0, 0.0, 1.0] * 4


def test_a_plan_of_one_node():
    m = ob.model("h1")
    x = _nominal(m, 1)
    x[1, 6:9] += [0.3, 0.0, 0.4]
    t, mode, kind = np.array([1.0, 1.1]), np.array([STANCE], np.int32), np.array([0], np.int32)
    u = np.zeros((1, 22))
    u[0, [2, 5, 8, 11]] = 100.0
    got = _host("h1", t, x, mode, kind, u)
    compare(got, pr.plan(m, t, x, mode, kind, u), "h1 one node")
    rows, foot, count, summ = got
    assert count == 0 and summ[pr.S_NODES] == 1.0 and abs(summ[pr.S_PATH] - 0.5) <= 1e-15 and summ[pr.S_MIN_SUM_Z] == 400.0
    assert np.all(summ[pr.S_DRIFT:pr.S_DRIFT + 4] == 0.0)                      # the last node has no mode: no pair in contact
    # equal forces: the centre of pressure is the mean of the four points
    assert np.abs(rows[0, 15:18] - rows[0, 3:15].reshape(4, 3).mean(axis=0)).max() <= 1e-15


def test_without_inputs_and_with_a_state_that_is_not_finite():
    m = ob.model("h1")
    t, x, mode, kind, u = random_plan(m, 9, np.random.default_rng(2), events=(4,))
    rows, foot, count, summ = _host("h1", t, x, mode, kind)
    assert np.all(rows[:, [15, 16, 17, 21]] == 0.0) and summ[pr.S_MIN_SUM_Z] == 0.0
    x[3, 14] = np.nan
    x[7, 2] = np.inf                                                           # a momentum entry counts too
    got = _host("h1", t, x, mode, kind, u)
    assert got[0][:, pr.BAD].tolist() == [0, 0, 0, 1, 0, 0, 0, 1, 0, 0] and got[3][pr.S_BAD] == 2.0
    compare(got, pr.plan(m, t, x, mode, kind, u), "h1 with two rows that are not finite")


def test_refusals():
    import ctypes as C
    from bipedal_control_amd import load_library
    lib = load_library()
    itf = _itf("h1")
    d, i = (C.c_double * 64)(), (C.c_int * 4)()
    assert lib.bpmpc_plan_rows_host(None, 1, d, d, d, i, i, None, None, None, None) == -1 and b"bpmpc_plan_rows_host" in lib.bpmpc_last_error()
    assert lib.bpmpc_plan_rows_host(itf.handle, 1, d, None, d, i, i, None, None, None, None) == -1 and b"null" in lib.bpmpc_last_error()
    assert lib.bpmpc_plan_rows_host(itf.handle, 0, d, d, d, i, i, None, None, None, None) == -1 and b"n_nodes" in lib.bpmpc_last_error()
    assert lib.bpmpc_plan_rows_host(itf.handle, 1, d, d, None, i, i, None, None, None, None) == 0      # every output is nullable
