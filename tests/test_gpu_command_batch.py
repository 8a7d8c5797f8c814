"""GPU tier: device-resident target trajectories (bpmpc_command_batch, bpmpc_solver_attach_commands) against bpmpc_solver_setup_commands, the
host path bpmpc_solver_setup fed the stored trajectories, and the numpy restatement tests/command_batch_reference.py.  Every comparison is bit
for bit: both sides of each run the same contraction-free arithmetic (ref_command_target on the device, cmd_vel_to_targets / goal_to_targets
and the lower_bound window on the host), and the references are interpolated by the same kernel from the same points.
H1 at batch 5 in handles of max_batch 8, max_nodes 64, horizon 30 DT; the nx = 24 path with G1 at batch 3."""
import ctypes as C

import numpy as np
import pytest

from tests.command_batch_reference import GOAL, START, TRAJECTORY, VELOCITY, CommandBatchReference
from tests.test_gpu_gait_batch import _same_tables, _tables

pytestmark = pytest.mark.gpu

NB, MAXB, NODES = 5, 8, 64
_CTX = {}


def ctx(robot="h1"):
    if robot not in _CTX:
        import bipedal_control_amd as bp
        from bipedal_control_amd import scenarios as sc
        from tests import oracle_bridge as ob
        itf = sc.interface(robot)
        lib = [bp.loadModeSequenceTemplate(itf.gaitFile, n) for n in ("stance", "trot", "standing_trot", "flying_trot")]
        _CTX[robot] = (bp, sc, itf, ob.model(robot), lib, 30 * sc.DT, itf.mpcSettings()["timeHorizon"])
    return _CTX[robot]


def _states(robot, nb, seed, yaws=None):
    bp, sc, itf, m, lib, H, TH = ctx(robot)
    x = sc.perturbed_initial_states(itf, nb, seed=seed)
    if yaws is not None:
        x[:, 9] = yaws[:nb]
    return x


def _xref(mpc, nb):
    """[robot][valid nodes][nx]: the references of the current setup"""
    pg = mpc.read("p_grid").astype(int)[:nb]
    nodes = mpc.read("g_nodes").astype(int)[pg]
    xr = mpc.read("xref").reshape(mpc.max_batch, mpc.max_nodes, mpc.nx)
    return [xr[b, :nodes[b]].copy() for b in range(nb)]


def _same_xref(a, b, nb):
    xa, xb = _xref(a, nb), _xref(b, nb)
    for r in range(nb):
        assert xa[r].shape[0] > 20 and np.array_equal(xa[r], xb[r]), r


def _route(x, t_first, dt, n=12):
    """A waypoint route from the state x: a base pose walking along a bent line, turning; momenta and joints as a command's target has them."""
    ts = t_first + dt * np.arange(n)
    xs = np.tile(x, (n, 1))
    xs[:, :6] = 0.0
    xs[:, 6] += 0.03 * np.arange(n)
    xs[:, 7] += 0.01 * np.arange(n) ** 2
    xs[:, 9] += 0.02 * np.arange(n)
    return ts, xs


def _snapshot(cmds, robots=MAXB):
    return [cmds.targets(r) for r in range(robots)], cmds.status()


def _same_snapshot(a, b):
    for r, ((ta, xa), (tb, xb)) in enumerate(zip(a[0], b[0])):
        assert np.array_equal(ta, tb) and np.array_equal(xa, xb), r
    assert np.array_equal(a[1], b[1])


class DeviceBuf:
    """A numpy array copied into device memory of the library's own HIP runtime, seen through __cuda_array_interface__."""

    hip = None

    def __init__(self, values, dtype):
        DeviceBuf.hip = DeviceBuf.hip or C.CDLL("libamdhip64.so")
        a = np.ascontiguousarray(values, dtype)
        self.ptr = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.ptr), C.c_size_t(max(a.nbytes, 16))) == 0
        assert self.hip.hipMemcpy(self.ptr, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0   # host to device, synchronous
        self.__cuda_array_interface__ = {"shape": a.shape, "typestr": "<i4" if a.dtype == np.int32 else "<f8", "data": (self.ptr.value, False),
                                         "version": 3, "strides": None}

    def free(self):
        self.hip.hipFree(self.ptr)


# ---- 1. velocity commands at every setup are setup_commands (and the nx = 24 path)
@pytest.mark.parametrize("robot,nb,through", [("h1", NB, "setup_commands"), ("h1", NB, "setup_gaits"), ("g1", 3, "setup_commands")])
def test_velocity_command_before_every_setup_equals_setup_commands(robot, nb, through):
    bp, sc, itf, m, lib, H, TH = ctx(robot)
    ref, dev = (bp.BatchedSqpMpc(itf, max_batch=MAXB, max_nodes=NODES) for _ in range(2))
    cmds = bp.BatchedCommands(dev)
    dev.attachCommands(cmds)
    gop = np.array([0, 1, 2, 3, 1], np.int32)[:nb]
    gs = [bp.BatchedGaitSchedule(h, lib) for h in (ref, dev)] if through == "setup_gaits" else None
    if gs:
        for g in gs:
            g.insertModeSequenceTemplate(np.array([1, 1, 2, 3, 1], np.int32)[:nb], sc.GAIT_START, 0.3 + 2 * H)
    cmd = np.array([(0.2, 0.0, 0.0, 0.1), (-0.1, 0.05, 0.0, 0.0), (0.3, -0.1, 0.02, -0.2), (0.0, 0.0, 0.0, 0.3), (0.4, 0.1, 0.0, 0.05)])[:nb]
    for k, t0 in enumerate((0.3, 0.32, 0.34)):
        x0 = _states(robot, nb, seed=100 + k)
        cmds.cmdVel(cmd, t0, x0)                              # TIME_TO_TARGET = mpc.timeHorizon, computed here, once
        if gs:
            lr = ref.setup_gaits(gs[0], t0, x0, cmd, horizon=H, time_to_target=TH)
            ld = dev.setup_gaits(gs[1], t0, x0, None, horizon=H)
        else:
            lr = ref.setup_commands(t0, x0, lib, gop, sc.GAIT_START, cmd, horizon=H, time_to_target=TH)
            ld = dev.setup_commands(t0, x0, lib, gop, sc.GAIT_START, None, horizon=H)
        assert lr == ld and ld["batch"] == nb, (t0, lr, ld)
        _same_tables(_tables(ref, nb), _tables(dev, nb), range(nb))
        assert np.array_equal(ref.read("xref"), dev.read("xref")) and np.array_equal(ref.read("x"), dev.read("x")), t0
        _same_xref(ref, dev, nb)
    assert cmds.status(nb).tolist() == [[3, 0, VELOCITY, 2]] * nb


# ---- 2. a goal is given once
def test_goal_is_computed_once_from_the_observation_of_its_message():
    bp, sc, itf, m, lib, H, TH = ctx()
    yaws = np.array([3.0, 3.3, -3.0, 3.14, 0.2])              # both sides of pi
    xs = [_states("h1", NB, seed=200 + k, yaws=yaws + 0.01 * k) for k in range(3)]
    goal = np.array([(0.5, 0.1, 0.0, 3.3), (-0.2, 0.3, 0.0, 3.0), (0.1, -0.4, 0.0, 3.2), (1.5, 0.0, 0.0, 3.14), (0.0, 0.0, 0.0, -0.4)])
    dev, host, every = (bp.BatchedSqpMpc(itf, max_batch=MAXB, max_nodes=NODES) for _ in range(3))
    cmds = bp.BatchedCommands(dev)
    dev.attachCommands(cmds)
    cmds.goal(goal, 0.4, xs[0])
    given_once = [itf.goalToTargetTrajectories(goal[b], 0.4, xs[0][b]) for b in range(NB)]
    gop = np.ones(NB, np.int32)
    for k, t0 in enumerate((0.4, 0.42, 0.44)):
        dev.setup_commands(t0, xs[k], lib, gop, sc.GAIT_START, None, horizon=H)
        host.setup(t0, xs[k], sc.gait_schedule(itf, "trot", t0, H), given_once, horizon=H)
        every.setup_commands(t0, xs[k], lib, gop, sc.GAIT_START, goal, horizon=H, goal=True)
        _same_tables(_tables(dev, NB), _tables(host, NB), range(NB))
        _same_xref(dev, host, NB)
        differs = [not np.array_equal(a, b) for a, b in zip(_xref(dev, NB), _xref(every, NB))]
        assert differs == [k > 0] * NB, (t0, differs)         # re-estimated from the current state at every solve: another line, another reach time
    for b in range(NB):
        ts, st = cmds.targets(b)
        assert np.array_equal(ts, given_once[b].timeTrajectory) and np.array_equal(st, given_once[b].stateTrajectory)
    assert cmds.status(NB).tolist() == [[1, 0, GOAL, 2]] * NB


# ---- 3. a mixed batch
def _mixed(cmds, ref, x, t):
    """robot 0 started only, 1 under a velocity command, 2 under a goal, 3 on a 12-point route, 4 with a dropped message - the same calls on the
    command batch and on the restatement.
    The velocity command is (vx, 0, 0, yaw rate), the shape of every command of the benchmark's sweep, for a reason that lies in the oracle:
    its cmd_vel_to_target_trajectories rotates the command with numpy's matrix product, whose order of summation (and use of fused multiply-adds)
    is the BLAS's own and differs from machine to machine, so with a lateral or vertical component the oracle itself is defined only to the last
    place - against the product's contraction-free host function it differs in 110 of 200 perturbed states, by one ulp.  With vy = vz = 0 the
    product has a single non-zero term and every order gives the same bits (0 of 500 differ).  Commands with all four components are compared,
    bit for bit as well, in test_mixed_batch_equals_the_host_path_fed_the_host_functions below."""
    cmd, goal = np.array([0.3, 0.0, 0.0, 0.2]), np.array([0.6, -0.2, 0.0, 3.2])
    rt, rx = _route(x[3], t, 0.1)
    times, states = np.tile(rt, (NB, 1)), np.tile(rx, (NB, 1, 1))
    cmds.start(t, x)
    cmds.cmdVel(cmd, t, x, mask=[0, 1, 0, 0, 0])
    cmds.goal(goal, t, x, mask=[0, 0, 1, 0, 0])
    cmds.setTargets(times, states, mask=[0, 0, 0, 1, 0])
    cmds.cmdVel(cmd, [t, t, t, t, 0.0], x, mask=[0, 0, 0, 0, 1])
    cmds.goal(goal, 0.0, x, mask=[0, 0, 0, 0, 1])
    ref.start(t, x)
    ref.cmd_vel(cmd, t, x, mask=[0, 1, 0, 0, 0])
    ref.goal(goal, t, x, mask=[0, 0, 1, 0, 0])
    ref.set_targets(times, states, mask=[0, 0, 0, 1, 0])
    ref.cmd_vel(cmd, [t, t, t, t, 0.0], x, mask=[0, 0, 0, 0, 1])
    ref.goal(goal, 0.0, x, mask=[0, 0, 0, 0, 1])


def test_mixed_batch_equals_the_host_path_fed_the_restatement():
    bp, sc, itf, m, lib, H, TH = ctx()
    x = _states("h1", NB, seed=300, yaws=np.array([0.1, -0.3, 3.0, 0.5, 3.3]))
    dev, host = (bp.BatchedSqpMpc(itf, max_batch=MAXB, max_nodes=NODES) for _ in range(2))
    cmds, ref = bp.BatchedCommands(dev, max_points=12), CommandBatchReference(m, MAXB, 12, TH)
    dev.attachCommands(cmds)
    _mixed(cmds, ref, x, 0.3)
    assert ref.status(NB).tolist() == [[0, 0, START, 1], [1, 0, VELOCITY, 2], [1, 0, GOAL, 2], [0, 0, TRAJECTORY, 12], [0, 2, START, 1]]
    assert np.array_equal(cmds.status(NB), ref.status(NB))
    assert np.array_equal(cmds.status()[NB:], np.zeros((MAXB - NB, 4), np.int32))
    dev.setup_commands(0.3, x, lib, np.ones(NB, np.int32), sc.GAIT_START, None, horizon=H)
    host.setup(0.3, x, sc.gait_schedule(itf, "trot", 0.3, H), [bp.TargetTrajectories(*ref.targets(b)) for b in range(NB)], horizon=H)
    xd, xh = _xref(dev, NB), _xref(host, NB)
    for b in range(NB):
        print("robot", b, "stored times", cmds.targets(b)[0], "max |xref - host|", np.abs(xd[b] - xh[b]).max())
    for b in range(NB):
        assert np.array_equal(xd[b], xh[b]), b
        assert np.array_equal(cmds.targets(b)[0], ref.targets(b)[0]) and np.array_equal(cmds.targets(b)[1], ref.targets(b)[1]), b


def test_mixed_batch_equals_the_host_path_fed_the_host_functions():
    """The mixed batch again with commands of all four components, each robot under a velocity command or a goal: the stored trajectories are
    those of the product's host functions (bpmpc_cmd_vel_to_targets / bpmpc_goal_to_targets, whose sums run left to right without contraction,
    as the device's do), and so are the references of a setup."""
    bp, sc, itf, m, lib, H, TH = ctx()
    x = _states("h1", NB, seed=310, yaws=np.array([0.1, -0.3, 3.0, 0.5, 3.3]))
    rows = np.array([(0.3, -0.1, 0.05, 0.2), (0.6, -0.2, 0.0, 3.2), (-0.2, 0.15, -0.03, -0.3), (-0.4, 0.7, 0.0, 2.9), (0.1, 0.2, 0.3, 0.4)])
    is_goal = np.array([0, 1, 0, 1, 0])
    dev, host = (bp.BatchedSqpMpc(itf, max_batch=MAXB, max_nodes=NODES) for _ in range(2))
    cmds = bp.BatchedCommands(dev)
    dev.attachCommands(cmds)
    cmds.cmdVel(rows, 0.3, x, mask=1 - is_goal, time_to_target=0.8)
    cmds.goal(rows, 0.3, x, mask=is_goal)
    given = [itf.goalToTargetTrajectories(rows[b], 0.3, x[b]) if is_goal[b] else itf.cmdVelToTargetTrajectories(rows[b], 0.3, x[b], 0.8) for b in range(NB)]
    for b in range(NB):
        ts, st = cmds.targets(b)
        assert np.array_equal(ts, given[b].timeTrajectory) and np.array_equal(st, given[b].stateTrajectory), b
    dev.setup_commands(0.3, x, lib, np.ones(NB, np.int32), sc.GAIT_START, None, horizon=H)
    host.setup(0.3, x, sc.gait_schedule(itf, "trot", 0.3, H), given, horizon=H)
    _same_xref(dev, host, NB)


# ---- 4. windowing
def test_window_of_a_route_and_a_rejected_window():
    bp, sc, itf, m, lib, H, TH = ctx()
    x = _states("h1", NB, seed=400)
    dev, host = (bp.BatchedSqpMpc(itf, max_batch=MAXB, max_nodes=NODES) for _ in range(2))
    cmds = bp.BatchedCommands(dev, max_points=12)
    dev.attachCommands(cmds)
    routes = [_route(x[b], 0.3 + 0.01 * b, 0.1 + 0.01 * b) for b in range(NB)]          # 12 points each, every robot its own spacing
    cmds.setTargets(np.array([r[0] for r in routes]), np.array([r[1] for r in routes]))
    gop = np.ones(NB, np.int32)
    for t0 in (0.3, 0.62, 1.3, 2.5):                           # at the route's start, inside it, over its end, behind it
        dev.setup_commands(t0, x, lib, gop, sc.GAIT_START, None, horizon=H)
        host.setup(t0, x, sc.gait_schedule(itf, "trot", t0, H), [bp.TargetTrajectories(*r) for r in routes], horizon=H)
        _same_xref(dev, host, NB)
    # 1 + k / 16: at t0 = 1.0625 point 0 lies before the window, 1 .. 8 inside [1.0625, 1.5125], point 9 behind it - ten points
    dense = 1.0 + np.arange(12) / 16.0
    cmds.setTargets(np.tile(dense, (NB, 1)), np.tile(routes[2][1], (NB, 1, 1)), mask=[0, 0, 1, 0, 0])
    before = _snapshot(cmds)
    with pytest.raises(bp.BpmpcError, match="robot 2: target trajectory has 10 points inside the horizon, the solver holds 8") as e:
        dev.setup_commands(1.0625, x, lib, gop, sc.GAIT_START, None, horizon=H)
    assert e.value.status == -1
    _same_snapshot(before, _snapshot(cmds))
    dev.setup_commands(1.3, x, lib, gop, sc.GAIT_START, None, horizon=H)       # point 4 before 1.3, 5 .. 11 inside: eight fit
    routes[2] = (dense, routes[2][1])
    host.setup(1.3, x, sc.gait_schedule(itf, "trot", 1.3, H), [bp.TargetTrajectories(*r) for r in routes], horizon=H)
    _same_xref(dev, host, NB)
    cmds.reset()
    cmds.start(0.3, x, mask=[1, 1, 1, 0, 1])
    with pytest.raises(bp.BpmpcError, match="robot 3: target trajectories need at least one point") as e:
        dev.setup_commands(0.3, x, lib, gop, sc.GAIT_START, None, horizon=H)
    assert e.value.status == -1


# ---- 5. masks and device inputs
def test_device_inputs_equal_host_inputs_and_masks_keep_the_others():
    bp, sc, itf, m, lib, H, TH = ctx()
    mpc = bp.BatchedSqpMpc(itf, max_batch=MAXB, max_nodes=NODES)
    P = 64
    on_host, on_dev = bp.BatchedCommands(mpc, max_points=P), bp.BatchedCommands(mpc, max_points=P)
    rng = np.random.default_rng(5)
    sent_t = np.sort(rng.uniform(5.0, 9.0, (MAXB, P)), axis=1)
    sent_x, sent_n = rng.standard_normal((MAXB, P, mpc.nx)), np.array([64, 1, 33, 7, 64, 2, 50, 64], np.int32)
    x = _states("h1", NB, seed=500, yaws=np.array([3.0, 3.3, 0.0, -3.0, 0.4]))
    t = np.array([0.3, 0.0, 0.5, 0.7, 0.9])                   # robot 1: its messages are dropped
    cmd, goal = rng.uniform(-0.3, 0.3, (NB, 4)), rng.uniform(-1.0, 1.0, (NB, 4))
    rt, rx = np.sort(rng.uniform(0.0, 3.0, (NB, P)), axis=1), rng.standard_normal((NB, P, mpc.nx))
    rn = np.array([64, 5, 1, 12, 40], np.int32)
    masks = [np.array(mk, np.int32) for mk in ([1, 1, 0, 1, 0], [0, 1, 1, 0, 0], [1, 0, 0, 0, 1], [0, 0, 1, 1, 0])]
    bufs = []

    def dv(a, dtype=np.float64):
        bufs.append(DeviceBuf(a, dtype))
        return bufs[-1]

    for c in (on_host, on_dev):
        c.setTargets(sent_t, sent_x, n_points=sent_n)
    sentinel = _snapshot(on_host)
    _same_snapshot(sentinel, _snapshot(on_dev))
    steps = [("start", lambda c, d: c.start(d(t), d(x), mask=d(masks[0], np.int32))),
             ("cmdVel", lambda c, d: c.cmdVel(d(cmd), d(t), d(x), mask=d(masks[1], np.int32), time_to_target=0.7)),
             ("goal", lambda c, d: c.goal(d(goal), d(t), d(x), mask=d(masks[2], np.int32))),
             ("setTargets", lambda c, d: c.setTargets(d(rt), d(rx), n_points=d(rn, np.int32), mask=d(masks[3], np.int32)))]
    touched = np.zeros(MAXB, bool)
    for (name, call), mask in zip(steps, masks):
        call(on_host, lambda a, dtype=np.float64: np.asarray(a, dtype))
        call(on_dev, dv)
        touched[:NB] |= (mask != 0) & ~((t == 0.0) & (name in ("cmdVel", "goal")))
        now = _snapshot(on_host)
        _same_snapshot(now, _snapshot(on_dev))
        for r in np.flatnonzero(~touched):                     # outside every mask so far, or at / beyond the batch: the sentinel, every bit
            assert np.array_equal(now[0][r][0], sentinel[0][r][0]) and np.array_equal(now[0][r][1], sentinel[0][r][1]), (name, r)
            assert np.array_equal(now[1][r], sentinel[1][r]), (name, r)
    assert touched.tolist() == [True] * NB + [False] * (MAXB - NB)
    st = on_dev.status()
    assert st[:NB].tolist() == [[1, 0, GOAL, 2], [0, 1, START, 1], [1, 0, TRAJECTORY, 1], [0, 0, TRAJECTORY, 12], [1, 0, GOAL, 2]]
    assert np.array_equal(on_dev.targets(3)[0], rt[3, :12]) and np.array_equal(on_dev.targets(3)[1], rx[3, :12])
    for b in bufs:                                             # every call that read them has been waited for (the snapshots synchronise)
        b.free()


# ---- 6. x = None after a controller tick
def test_observations_of_the_last_tick_are_the_default_observation():
    from tests.test_gpu_controller_tick import _rbd
    bp, sc, itf, m, lib, H, TH = ctx()
    mpc = bp.BatchedSqpMpc(itf, max_batch=MAXB, max_nodes=NODES, return_gains=True)
    from_tick, from_host = bp.BatchedCommands(mpc), bp.BatchedCommands(mpc)
    x0 = _states("h1", NB, seed=600)
    cmd = np.array([0.25, 0.05, 0.0, -0.15])
    with pytest.raises(bp.BpmpcError, match="x_obs == NULL needs a rollout of the same batch"):
        from_tick.cmdVel(cmd, np.full(NB, 0.3))               # neither a tick nor a rollout yet
    mpc.setup_commands(0.3, x0, lib, np.ones(NB, np.int32), sc.GAIT_START, cmd, horizon=H)
    mpc.enqueue()
    ctrl = bp.BatchedController(mpc, bp.WeightedWbc(itf, max_batch=MAXB))
    rng = np.random.default_rng(6)
    rbd = np.array([_rbd(m, x0[b], rng, speed=0.05)[0] for b in range(NB)])
    out = ctrl.tick(np.full(NB, 0.3025), rbd)
    from_tick.cmdVel(cmd, 0.3025)
    from_host.cmdVel(cmd, 0.3025, x=out["x_obs"])
    _same_snapshot(_snapshot(from_tick, NB), _snapshot(from_host, NB))
    assert np.array_equal(from_tick.targets(0)[1][0, 6:10], np.array([out["x_obs"][0, 6], out["x_obs"][0, 7], m["com_height"], out["x_obs"][0, 9]]))
    with pytest.raises(bp.BpmpcError, match="x_obs == NULL needs a rollout of the same batch"):
        from_tick.cmdVel(cmd, np.full(3, 0.3025))             # another batch size than the tick's
    xe, _, _ = mpc.rollout(0.02)                               # a rollout ran last: its end states are the observations now
    from_tick.goal([0.5, 0.0, 0.0, 0.3], 0.32)
    from_host.goal([0.5, 0.0, 0.0, 0.3], 0.32, x=xe)
    _same_snapshot(_snapshot(from_tick, NB), _snapshot(from_host, NB))


# ---- 7. detach, and the DDP solver
def test_detached_solver_runs_what_it_ran_before():
    bp, sc, itf, m, lib, H, TH = ctx()
    x0 = _states("h1", NB, seed=700)
    cmd = np.tile([0.2, 0.0, 0.0, 0.1], (NB, 1))
    gop = np.ones(NB, np.int32)
    never, dev = (bp.BatchedSqpMpc(itf, max_batch=MAXB, max_nodes=NODES) for _ in range(2))
    cmds = bp.BatchedCommands(dev)
    dev.attachCommands(cmds)
    cmds.start(0.3, x0)                                        # a standing target: not what the velocity command gives
    dev.setup_commands(0.3, x0, lib, gop, sc.GAIT_START, None, horizon=H)
    never.setup_commands(0.3, x0, lib, gop, sc.GAIT_START, cmd, horizon=H)
    assert not np.array_equal(never.read("xref"), dev.read("xref"))
    dev.attachCommands(None)
    with pytest.raises(bp.BpmpcError):
        dev.setup_commands(0.32, x0, lib, gop, sc.GAIT_START, None, horizon=H)      # detached: cmd_vel is needed again
    for h in (never, dev):
        lay = h.setup_commands(0.32, x0, lib, gop, sc.GAIT_START, cmd, horizon=H)
    assert lay == never.layout()
    _same_tables(_tables(never, NB), _tables(dev, NB), range(NB))
    assert np.array_equal(never.read("xref"), dev.read("xref")) and np.array_equal(never.read("x"), dev.read("x"))
    other = bp.BatchedSqpMpc(itf, max_batch=MAXB, max_nodes=NODES)
    with pytest.raises(bp.BpmpcError, match="belongs to another solver"):
        other.attachCommands(cmds)


def test_ddp_solver_reads_the_same_tables():
    bp, sc, itf, m, lib, H, TH = ctx()
    x0 = _states("h1", NB, seed=710)
    cmd = np.tile([0.2, 0.05, 0.0, -0.1], (NB, 1))
    gop = np.ones(NB, np.int32)
    ref, dev = (bp.BatchedDdpMpc(itf, MAXB, NODES) for _ in range(2))
    cmds = bp.BatchedCommands(dev)
    dev.attachCommands(cmds)
    cmds.cmdVel(cmd, 0.3, x0)
    lr = ref.setup_commands(0.3, x0, lib, gop, sc.GAIT_START, cmd, horizon=H, time_to_target=TH)
    ld = dev.setup_commands(0.3, x0, lib, gop, sc.GAIT_START, None, horizon=H)
    assert lr == ld
    _same_tables(_tables(ref, NB), _tables(dev, NB), range(NB))
    assert np.array_equal(ref.read("xref"), dev.read("xref")) and np.array_equal(ref.read("x"), dev.read("x"))


# ---- 8. ten ticks of the loop
def test_ten_ticks_of_the_loop_with_a_goal_then_a_velocity_command():
    bp, sc, itf, m, lib, H, TH = ctx()
    tick = 0.02
    mpc = bp.BatchedSqpMpc(itf, max_batch=MAXB, max_nodes=NODES, return_gains=True)
    gs, cmds = bp.BatchedGaitSchedule(mpc, lib), bp.BatchedCommands(mpc)
    mpc.attachCommands(cmds)
    gs.insertModeSequenceTemplate(1, sc.GAIT_START, 0.3 + 2 * H)
    x0 = _states("h1", NB, seed=800, yaws=np.array([3.0, 3.3, 0.1, -0.2, 0.0]))
    goal = np.array([(0.4, 0.0, 0.0, 3.2), (0.3, 0.1, 0.0, 3.1), (0.5, -0.1, 0.0, 0.3), (0.2, 0.2, 0.0, 0.0), (0.6, 0.0, 0.0, 0.1)])
    cmds.start(0.3, x0)
    cmds.goal(goal, 0.3, x0)
    mpc.setup_gaits(gs, 0.3, x0, None, horizon=H)
    mpc.enqueue()
    stored = [_snapshot(cmds, NB)]
    for k in range(1, 10):
        t = 0.3 + k * tick
        mpc.rollout(tick, fetch=False)
        if k == 5:
            cmds.cmdVel([0.2, 0.0, 0.0, 0.1], t)              # from the end states of the rollout, on the device
        mpc.setup_gaits(gs, t, None, None, horizon=H, from_previous=True)
        mpc.enqueue()
        stored.append(_snapshot(cmds, NB))
    _, x, _, _, st = mpc.fetch()
    assert [s.status for s in st[:NB]] == [0] * NB and np.isfinite(x[:NB]).all()
    for k in range(1, 5):
        _same_snapshot(stored[0], stored[k])                   # the reach time (and everything else) is fixed by the message
    for b in range(NB):
        assert stored[4][0][b][0][1] == stored[0][0][b][0][1] > 0.3
        assert not np.array_equal(stored[5][0][b][0], stored[4][0][b][0]) and stored[5][0][b][0][0] == 0.3 + 5 * tick
    for k in range(6, 10):
        _same_snapshot(stored[5], stored[k])
    assert stored[9][1].tolist() == [[2, 0, VELOCITY, 2]] * NB + [[0, 0, 0, 0]] * (MAXB - NB)


# ---- every argument check on a live handle: its status, a message naming the robot and the entry, and nothing changed
def test_argument_checks_change_nothing():
    bp, sc, itf, m, lib, H, TH = ctx()
    mpc = bp.BatchedSqpMpc(itf, max_batch=MAXB, max_nodes=NODES)
    for bad in (1, 65, 0, -3):
        with pytest.raises(bp.BpmpcError, match="max_points") as e:
            bp.BatchedCommands(mpc, max_points=bad)
        assert e.value.status == -1
    cmds = bp.BatchedCommands(mpc, max_points=12)
    x = _states("h1", NB, seed=900)
    rt, rx = _route(x[0], 0.3, 0.1)
    times, states = np.tile(rt, (NB, 1)), np.tile(rx, (NB, 1, 1))
    cmds.start(0.3, x)
    cmds.setTargets(times, states, mask=[0, 0, 0, 1, 1])
    before = _snapshot(cmds)

    def bad(a, index, value=np.nan):
        a = np.array(a, float)
        a[index] = value
        return a

    cmd, t = np.tile([0.2, 0.0, 0.0, 0.1], (NB, 1)), np.full(NB, 0.5)
    dec = times.copy()
    dec[1, 3] = dec[1, 2] - 1e-9
    refused = [("robot 2: cmd\\[1\\] is not finite", lambda: cmds.cmdVel(bad(cmd, (2, 1)), t, x)),
               ("robot 4: t_obs is not finite", lambda: cmds.cmdVel(cmd, bad(t, 4, np.inf), x)),
               ("robot 1: x_obs\\[7\\] is not finite", lambda: cmds.cmdVel(cmd, t, bad(x, (1, 7)))),
               ("time_to_target is not finite", lambda: cmds.cmdVel(cmd, t, x, time_to_target=np.nan)),
               ("robot 0: goal\\[3\\] is not finite", lambda: cmds.goal(bad(cmd, (0, 3)), t, x)),
               ("robot 3: goal\\[0\\] is not finite", lambda: cmds.goal(bad(cmd, (3, 0), -np.inf), t, x)),
               ("robot 3: x_obs\\[0\\] is not finite", lambda: cmds.start(t, bad(x, (3, 0)))),
               ("robot 0: t_obs is not finite", lambda: cmds.start(bad(t, 0), x)),
               ("robot 2: n_points 0 is outside 1 .. 12", lambda: cmds.setTargets(times, states, n_points=[12, 12, 0, 12, 12])),
               ("robot 4: n_points 13 is outside 1 .. 12", lambda: cmds.setTargets(times, states, n_points=[12, 12, 1, 12, 13])),
               ("robot 1: times\\[3\\] is below times\\[2\\]", lambda: cmds.setTargets(dec, states)),
               ("robot 0: times\\[11\\] is not finite", lambda: cmds.setTargets(bad(times, (0, 11)), states)),
               ("robot 2: states\\[1\\]\\[5\\] is not finite", lambda: cmds.setTargets(times, bad(states, (2, 1, 5)))),
               ("batch exceeds the command batch's max_batch", lambda: cmds.start(np.full(MAXB + 1, 0.3), np.zeros((MAXB + 1, mpc.nx)))),
               ("batch exceeds the command batch's max_batch", lambda: cmds.status(MAXB + 1)),
               ("x_obs == NULL needs a rollout", lambda: cmds.goal(cmd, t)),
               ("robot out of range", lambda: cmds.targets(MAXB)),
               ("robot out of range", lambda: cmds.targets(-1))]
    for message, call in refused:
        with pytest.raises(bp.BpmpcError, match=message) as e:
            call()
        assert e.value.status == -1, message
        _same_snapshot(before, _snapshot(cmds))
    # what is not used is not read: a goal's third entry, a masked-out robot's row, the points behind n_points
    cmds.goal(bad(cmd, (0, 2)), t, x, mask=[1, 0, 0, 0, 0])
    cmds.cmdVel(bad(cmd, (1, 0)), t, x, mask=[1, 0, 0, 0, 0])
    cmds.setTargets(bad(times, (0, 5)), bad(states, (0, 7, 3)), n_points=5, mask=[1, 0, 0, 0, 0])
    assert cmds.status(1).tolist() == [[2, 0, TRAJECTORY, 5]]
    assert np.array_equal(cmds.targets(0)[0], rt[:5]) and np.array_equal(cmds.targets(0)[1], rx[:5])
