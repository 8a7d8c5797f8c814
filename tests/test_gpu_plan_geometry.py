"""GPU tier: the plan geometry (include/bpmpc.h "Plan geometry"; kernels/plan_geometry.h k_plan_fused, k_plan_nodes, k_plan_reduce) against the
numpy restatement tests/plan_geometry_reference.py, whose kinematics are oracle/wbc_py.py fk / contact_points.
  arrays       H1 batch 3 in a handle of 4, N = 40, n_nodes (16, 17, 1): a full tile, a tile plus one node, a single node; G1 batch 2, n_nodes
               (33, 5); both ways to launch.  States in the ranges of tests/test_gpu_telemetry.py _episode, f_z 50 .. 400 N, one robot with all
               forces 0.  Node rows 1e-12 absolute - the bound the telemetry holds the same kinematics to (seen there 4.4e-16; seen here
               6.7e-16); times, modes, kinds, sum_z, masks and flags exactly; footholds exactly in (t, i, node) and 1e-12 in position; the path
               length 1e-12 times its number of terms, maxima and minimum 1e-12.  Rows beyond n_nodes, robots beyond the batch and foothold slots
               behind the count keep a sentinel.  Host arrays and device pointers, one launch and two: the same bits.  A NaN joint flags its row
               and no other and leaves the other robots bit-identical.
  solver       H1 batch 2, a trot, horizon 0.6 s, t0 = (0, 0.1): two grids.  update(solver) against the restatement fed fetch and read; the
               foothold times and feet against the landings of the mode schedule, computed here from the schedule; x, u and stats after run +
               update bit-identical to a run alone.
  policy       publish, adopt, update_from_policy: optimized, footholds and summary bit for bit those of update(solver), the desired block keeps
               its sentinel; refused before the first adoption.
  refusals     a batch above max_batch, a solver with more nodes than the handle, an update before a setup, a solver of another robot, a host
               n_nodes outside 1 .. N.
Every comparison prints its maximum before it asserts (pytest -s)."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (torch's own HIP runtime sees the GPU only when it is loaded before the library's runtime initialises)

from tests import oracle_bridge as ob
from tests import plan_geometry_reference as pr
from tests.test_plan_geometry_reference import compare, random_plan, random_states

pytestmark = pytest.mark.gpu
TOL = 1e-12
INVALID, CAPACITY = -1, -6
SENTINEL = -7.0
OUTPUTS = ("optimized", "desired", "footholds", "summary")


def _itf(robot):
    from bipedal_control_amd import scenarios as sc
    return sc.interface(robot)


def _handle(robot, max_batch, N, launches=0):
    import bipedal_control_amd as bp
    plan = bp.PlanGeometry(_itf(robot), max_batch, N)
    plan.configure(launches)
    return plan


def _fill(plan, value=SENTINEL):
    out = plan.outputs()
    for k in OUTPUTS:
        out[k].torch().fill_(value)
    out["foothold_count"].torch().fill_(int(value))
    torch.cuda.synchronize()


def _read(plan):
    torch.cuda.synchronize()
    out = plan.outputs()
    got = {k: out[k].torch().cpu().numpy().copy() for k in OUTPUTS}
    got["count"] = out["foothold_count"].torch().cpu().numpy().copy()
    return got


def _same(a, b, keys=OUTPUTS + ("count",)):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


def _status(call):
    import bipedal_control_amd as bp
    with pytest.raises(bp.BpmpcError) as e:
        call()
    return e.value.status


def _arrays(robot, N, n_nodes, events, zero_forces_robot, seed):
    """the arguments of update_arrays with the handle's strides, and the plans they were cut from"""
    m = ob.model(robot)
    nx = 12 + m["nj"]
    rng = np.random.default_rng(seed)
    B = len(n_nodes)
    a = dict(n_nodes=np.array(n_nodes, np.int32), t=np.zeros((B, N + 1)), x=np.zeros((B, N + 1, nx)), mode=np.zeros((B, N), np.int32),
             kind=np.zeros((B, N), np.int32), u=np.zeros((B, N, nx)), xref=np.zeros((B, N, nx)))
    plans = []
    for b, n in enumerate(n_nodes):
        t, x, mode, kind, u = random_plan(m, n, rng, events=events[b], zero_forces=b == zero_forces_robot)
        xref = random_states(m, n, rng)
        a["t"][b, :n + 1], a["x"][b, :n + 1], a["mode"][b, :n], a["kind"][b, :n], a["u"][b, :n], a["xref"][b, :n] = t, x, mode, kind, u, xref
        plans.append((t, x, mode, kind, u, xref))
    return m, a, plans


def _check_against_restatement(m, got, plans, what, desired=True):
    worst = np.zeros(4)
    for b, (t, x, mode, kind, u, xref) in enumerate(plans):
        n = len(t) - 1
        want = pr.plan(m, t, x, mode, kind, u)
        worst = np.maximum(worst, compare((got["optimized"][b, :n + 1], got["footholds"][b], int(got["count"][b]), got["summary"][b]), want,
                                          "%s robot %d" % (what, b)))
        if desired:
            ref = pr.rows(m, t, np.r_[xref, xref[-1:]], mode, kind)[:n]
            d = np.abs(got["desired"][b, :n, :pr.TIME] - ref[:, :pr.TIME]).max()
            print("plan geometry %s robot %d: desired rows %.3e" % (what, b, d))
            assert d <= TOL and np.array_equal(got["desired"][b, :n, pr.TIME:], ref[:, pr.TIME:]) and np.all(ref[:, [15, 16, 17, 21]] == 0.0)
            worst[0] = max(worst[0], d)
    return worst


def _check_sentinels(got, n_nodes, max_batch, desired=True):
    B = len(n_nodes)
    for b, n in enumerate(n_nodes):
        assert np.all(got["optimized"][b, n + 1:] == SENTINEL) and np.all(got["desired"][b, (n if desired else 0):] == SENTINEL)
        assert np.all(got["footholds"][b, min(int(got["count"][b]), 16):] == SENTINEL)
    for k in OUTPUTS:
        assert np.all(got[k][B:max_batch] == SENTINEL), k
    assert np.all(got["count"][B:max_batch] == int(SENTINEL))


CASES = {"h1": dict(max_batch=4, n_nodes=(16, 17, 1), events=((3, 9), (4, 5, 12), ()), zero=1),
         "g1": dict(max_batch=2, n_nodes=(33, 5), events=((6, 20, 21, 30), (2,)), zero=1)}


# ---------------------------------------------------------------------------------------------------------------- stand-alone arrays
@pytest.mark.parametrize("robot,launches", [("h1", 1), ("h1", 2), ("g1", 1), ("g1", 2)])
def test_arrays_against_restatement(robot, launches):
    c, N = CASES[robot], 40
    m, a, plans = _arrays(robot, N, c["n_nodes"], c["events"], c["zero"], seed=3)
    plan = _handle(robot, c["max_batch"], N, launches)
    _fill(plan)
    plan.update_arrays(**a)
    got = _read(plan)
    worst = _check_against_restatement(m, got, plans, "%s arrays, %d launch(es)" % (robot, launches))
    _check_sentinels(got, c["n_nodes"], c["max_batch"])
    z = c["zero"]
    n = c["n_nodes"][z]
    assert np.all(got["optimized"][z, :n + 1, 15:18] == 0.0) and np.all(got["optimized"][z, :n + 1, 21] == 0.0) and got["summary"][z, pr.S_MIN_SUM_Z] == 0.0
    assert got["count"][:len(plans)].sum() >= 2 and got["summary"][0, pr.S_MIN_SUM_Z] >= 200.0
    # what the accessors hand out is what lives on the device
    assert np.array_equal(plan.nodes(), got["optimized"][:len(plans)]) and np.array_equal(plan.nodes("desired"), got["desired"][:len(plans)])
    entries, count = plan.footholds()
    assert np.array_equal(entries, got["footholds"][:len(plans)]) and np.array_equal(count, got["count"][:len(plans)])
    assert np.array_equal(plan.summary(), got["summary"][:len(plans)])
    print("plan geometry %s arrays, %d launch(es): worst rows %.3e footholds %.3e path %.3e maxima %.3e" % ((robot, launches) + tuple(worst)))


@pytest.mark.parametrize("robot", ["h1", "g1"])
def test_host_arrays_device_pointers_and_both_launches_give_the_same_bits(robot):
    c, N = CASES[robot], 40
    m, a, plans = _arrays(robot, N, c["n_nodes"], c["events"], c["zero"], seed=3)
    results = []
    for launches, on_device in ((1, False), (1, True), (2, False), (2, True)):
        plan = _handle(robot, c["max_batch"], N, launches)
        _fill(plan)
        args = {k: torch.from_numpy(v).cuda() for k, v in a.items()} if on_device else a
        torch.cuda.synchronize()
        plan.update_arrays(**args)
        results.append(_read(plan))
    assert all(_same(results[0], r) for r in results[1:])


def test_a_nan_joint_flags_its_row_and_no_other():
    c, N = CASES["h1"], 40
    m, a, plans = _arrays("h1", N, c["n_nodes"], c["events"], c["zero"], seed=3)
    plan = _handle("h1", c["max_batch"], N)
    _fill(plan)
    plan.update_arrays(**a)
    before = _read(plan)
    a["x"][0, 5, 14] = np.nan
    _fill(plan)
    plan.update_arrays(**a)
    after = _read(plan)
    flags = after["optimized"][0, :17, pr.BAD]
    assert flags.tolist() == [0.0] * 5 + [1.0] + [0.0] * 11 and after["summary"][0, pr.S_BAD] == 1.0 and before["summary"][0, pr.S_BAD] == 0.0
    others = [k for k in range(17) if k != 5]
    assert np.array_equal(after["optimized"][0, others], before["optimized"][0, others]) and np.array_equal(after["optimized"][0, 5, pr.TIME:pr.BAD], before["optimized"][0, 5, pr.TIME:pr.BAD])
    for k in OUTPUTS + ("count",):
        assert np.array_equal(after[k][1:], before[k][1:]), k
    # the flagged row takes part in nothing else: the restatement with the same state gives the robot's summary
    plans[0][1][5, 14] = np.nan
    _check_against_restatement(m, after, plans, "h1 arrays with a NaN joint")
    assert np.all(np.isfinite(after["summary"]))


# ---------------------------------------------------------------------------------------------------------------- from the solver
H, MAX_NODES = 0.6, 48
T0 = np.array([0.0, 0.1])


def _solver(bp, sc, itf, **kw):
    x0 = sc.perturbed_initial_states(itf, 2)
    sched = sc.gait_schedule(itf, "trot", 0.0, H)                             # holds t0 - H .. t0 + 2 H of both robots
    targets = [itf.cmdVelToTargetTrajectories((0.3, 0.0, 0.0, 0.0), T0[b], x0[b], H) for b in range(2)]
    mpc = bp.BatchedSqpMpc(itf, max_batch=2, max_nodes=MAX_NODES, **kw)
    mpc.setup(T0, x0, [sched, sched], targets, horizon=H)                     # one schedule per problem: the t0 differ
    mpc.enqueue()
    return mpc, sched


def _solver_plans(mpc, nx):
    """the plans of the robots as the solver holds them: fetch for x and u, read for the grid tables and the references"""
    mpc.synchronize()
    t, x, u, K, stats = mpc.fetch()
    N, MB = mpc.max_nodes, mpc.max_batch
    g_time, g_kind, g_mode = mpc.read("g_time").reshape(MB, N + 1), mpc.read("g_kind").reshape(MB, N).astype(int), mpc.read("g_mode").reshape(MB, N).astype(int)
    g_nodes, p_grid, xref = mpc.read("g_nodes").astype(int), mpc.read("p_grid").astype(int), mpc.read("xref").reshape(MB, N, nx)
    plans = []
    for b in range(mpc.batch):
        g = p_grid[b]
        n = g_nodes[g]
        plans.append((g_time[g, :n + 1], x[b, :n + 1], g_mode[g, :n], g_kind[g, :n], u[b, :n], xref[b, :n]))
    return plans, p_grid, (x, u, [bytes(s) for s in stats])


def test_from_the_solver():
    import bipedal_control_amd as bp
    from bipedal_control_amd import scenarios as sc
    itf, m = _itf("h1"), ob.model("h1")
    mpc, sched = _solver(bp, sc, itf)
    plan = _handle("h1", 2, MAX_NODES + 2)                                    # the outputs' node stride differs from the solver's
    _fill(plan)
    plan.update(mpc)
    got = _read(plan)
    plans, p_grid, solution = _solver_plans(mpc, 22)
    assert p_grid.tolist() == [0, 1] and all(len(p[0]) - 1 <= MAX_NODES for p in plans)
    _check_against_restatement(m, got, plans, "h1 from the solver")
    _check_sentinels(got, [len(p[0]) - 1 for p in plans], 2)
    # independently of the grid tables: the landings of the mode schedule strictly inside each robot's horizon
    ev, modes = np.asarray(sched.eventTimes, float), list(sched.modeSequence)
    for b in range(2):
        want = [(te, i) for e, te in enumerate(ev) if T0[b] < te < T0[b] + H
                for i in range(4) if not pr.contact_flag(modes[e], i) and pr.contact_flag(modes[e + 1], i)]
        have = [(row[0], int(row[1])) for row in got["footholds"][b, :got["count"][b]]]
        print("plan geometry from the solver robot %d: footholds" % b, have, "schedule", want)
        assert len(want) >= 2 and have == want
    # the solver's own results are those of a run without an update behind it
    alone, _ = _solver(bp, sc, itf)
    alone.synchronize()
    t, x, u, K, stats = alone.fetch()
    assert np.array_equal(x, solution[0]) and np.array_equal(u, solution[1]) and [bytes(s) for s in stats] == solution[2]


def test_from_a_policy_buffer():
    import bipedal_control_amd as bp
    from bipedal_control_amd import scenarios as sc
    itf = _itf("h1")
    mpc, _ = _solver(bp, sc, itf, feedback_policy=False)
    pol = bp.PolicyBuffer(mpc, 2)
    from_solver, from_policy = _handle("h1", 2, MAX_NODES), _handle("h1", 2, MAX_NODES)
    _fill(from_solver); _fill(from_policy)
    assert _status(lambda: from_policy.update_from_policy(pol)) == INVALID      # waiting for the initial policy
    pol.publish()
    assert _status(lambda: from_policy.update_from_policy(pol)) == INVALID      # published, not adopted
    assert pol.update() is True
    from_policy.update_from_policy(pol)
    from_solver.update(mpc)
    a, b = _read(from_policy), _read(from_solver)
    assert _same(a, b, ("optimized", "footholds", "summary", "count")) and b["count"].min() >= 2
    assert np.all(a["desired"] == SENTINEL) and not np.all(b["desired"] == SENTINEL)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    import bipedal_control_amd as bp
    from bipedal_control_amd import load_library, scenarios as sc
    lib = load_library()
    itf = _itf("h1")
    plan = _handle("h1", 4, 40)
    m, a, plans = _arrays("h1", 40, (3, 4, 5, 6, 7), ((), (), (), (), ()), -1, seed=1)
    assert _status(lambda: plan.update_arrays(**a)) == CAPACITY and b"max_batch" in lib.bpmpc_last_error()
    four = {k: v[:4].copy() for k, v in a.items()}
    four["n_nodes"][1] = 41
    assert _status(lambda: plan.update_arrays(**four)) == INVALID and b"n_nodes[1] = 41" in lib.bpmpc_last_error()
    four["n_nodes"][1] = 0
    assert _status(lambda: plan.update_arrays(**four)) == INVALID and b"n_nodes[1] = 0" in lib.bpmpc_last_error()
    assert _status(lambda: plan.nodes(batch=5)) == CAPACITY and _status(lambda: plan.summary(batch=5)) == CAPACITY
    with pytest.raises(KeyError):
        plan.nodes("measured")
    mpc = bp.BatchedSqpMpc(itf, max_batch=2, max_nodes=MAX_NODES)
    assert _status(lambda: plan.update(mpc)) == INVALID and b"no setup yet" in lib.bpmpc_last_error()
    mpc, _ = _solver(bp, sc, itf)
    mpc.synchronize()
    assert _status(lambda: plan.update(mpc)) == CAPACITY and b"max_nodes" in lib.bpmpc_last_error()      # 48 nodes into a handle of 40
    small = _handle("h1", 1, MAX_NODES)
    assert _status(lambda: small.update(mpc)) == CAPACITY and b"max_batch" in lib.bpmpc_last_error()
    other = _handle("g1", 2, MAX_NODES)
    assert _status(lambda: other.update(mpc)) == INVALID and b"different robots" in lib.bpmpc_last_error()
    dims = [C.c_int() for _ in range(5)]
    assert lib.bpmpc_plan_dims(plan._h, *[C.byref(d) for d in dims]) == 0 and [d.value for d in dims] == [4, 40, 24, 16, 16]
    assert _status(lambda: plan.configure(3)) == INVALID
