"""GPU tier: the batched rigid-body plant (include/bpmpc.h "Plant"; kernels/plant.h k_plant_step) against the numpy restatement
tests/plant_reference.py, whose rigid-body quantities come from oracle/wbc_py.py (nle from the Lagrangian by complex-step derivatives).
  one substep      H1 and G1, batch 5: a robot in the air, one on both feet, one on its left foot only (the ground under the right foot lowered),
                   one moving fast with a knee command beyond its torque limit, one pushed on uneven ground; v+, q+, contact forces, every sensor
  twenty substeps  one launch of 20 substeps against 20 restatement substeps; the same control step as 20 launches of one substep: the same bits
  masks            batch 67 (k_plant_step holds one robot per workgroup: 67 workgroups): two runs the same bits; a masked set_state and a masked
                   set_params leave the other robots' later states bit-identical; host arrays and device tensors the same bits
  estimator        the plant's device outputs through the from-topic estimator return the plant's rbd; ten Kalman updates enqueued behind ten steps
  the loop         step_controlled -> estimator update -> tick_estimated, setup_commands(x0 = NULL) + run every 10 ticks: through device pointers,
                   free-running and read at every tick, and with every array through the host - the same bits
  refusals
No contact decision of a compared case is left to rounding: the restatement's |d_i| > 1e-6 and |n_i - contact_threshold| > 1e-6 are asserted at
every substep.  Every comparison prints its maximum before it asserts (pytest -s)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (torch's own HIP runtime sees the GPU only when it is loaded before the library's runtime initialises)

from oracle import wbc_py as wp
from tests import oracle_bridge as ob
from tests import plant_reference as pr

pytestmark = pytest.mark.gpu
TOL = 1e-9                     # relative to max(1, |value|): the project's tolerance of a linear solve against the oracle (test_qp_step_matches_oracle)
TOL20 = 100 * 6.5e-15          # twenty substeps: 100 x the restatement's own floor (test_twenty_substeps_in_one_launch)
PERIOD, SUBSTEPS = 0.01, 20
H = PERIOD / SUBSTEPS          # the substep length k_plant_step forms; a launch of one substep with period = H forms H / 1, the same bits
B5 = 5
SENSORS = ("joint_pos", "joint_vel", "quat", "angular_vel_local", "linear_accel_local", "contact", "feet_heights", "odom_pos", "odom_quat", "odom_lin_vel",
           "odom_ang_vel", "rbd", "contact_force")


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())


def _limits(robot):
    from bipedal_control_amd import scenarios as sc
    return wp.load_settings(sc.ROBOTS[robot]["task"], ob.model(robot)["nj"])["torque_limits"]


def _plant(robot, B):
    import bipedal_control_amd as bp
    from bipedal_control_amd import scenarios as sc
    return bp.BatchedPlant(sc.interface(robot), max_batch=B)


def _read(plant):
    """every output as a numpy array (synchronises through get_state first: the outputs are read on torch's stream)"""
    plant.get_state()
    return {k: v.torch().cpu().numpy() for k, v in plant.outputs().items()}


@functools.lru_cache(maxsize=None)
def _cases(robot):
    """The five robots: states q, v [5, nv], the command arrays, base forces [5, 3] and ground heights [5, 4]."""
    from tests.test_plant_reference import standing_state
    m = ob.model(robot)
    nj = m["nj"]
    nv = 6 + nj
    rng = np.random.default_rng(41 + nj)
    q0, _, _ = standing_state(m, depth=0.003)
    q = np.tile(q0, (B5, 1)) + rng.standard_normal((B5, nv)) * np.r_[np.zeros(3), np.full(3, 0.002), np.full(nj, 0.004)]      # the soles stay within about a millimetre
    v = 0.05 * rng.standard_normal((B5, nv))
    ground = np.zeros((B5, 4))
    force = np.zeros((B5, 3))
    q[0, 2] += 0.5                                   # in the air
    ground[2, 2:] = -0.05                            # left foot only: the ground under the right foot's two points is 5 cm lower
    v[3] = rng.standard_normal(nv) * np.r_[0.5 * np.ones(3), 0.3 * np.ones(nv - 3)]      # fast
    v[3] *= 1.0 / np.abs(v[3]).max()
    force[4] = [30.0, -10.0, 5.0]
    ground[4] = [0.002, -0.0015, 0.001, 0.0025]
    cmd = dict(pos_des=q[:, 6:] + 0.02 * rng.standard_normal((B5, nj)), vel_des=0.1 * rng.standard_normal((B5, nj)), tau_ff=5.0 * rng.standard_normal((B5, nj)),
               kp=rng.uniform(500.0, 2000.0, (B5, nj)), kd=rng.uniform(10.0, 40.0, (B5, nj)))
    cmd["pos_des"][3, 3] += 1.0                      # a knee asked for 1 rad at kp >= 500: beyond its torque limit
    return q, v, cmd, force, ground


@functools.lru_cache(maxsize=None)
def _reference(robot, n):
    """n restatement substeps of the five robots: per robot the list of substep dicts, and the restatement's own floor - the largest difference of
    v+ between numpy.linalg.solve and a Cholesky solve of the same system, relative to max(1, |v+|), over all substeps.  Computed once per robot."""
    m = ob.model(robot)
    q, v, cmd, force, ground = _cases(robot)
    lim = _limits(robot)
    steps, floor = [], 0.0
    for b in range(B5):
        qb, vb, rows = q[b], v[b], []
        cb = {k: a[b] for k, a in cmd.items()}
        for _ in range(n):
            s = pr.substep(m, qb, vb, cb, H, ground=ground[b], w_ext=force[b], torque_limits=lim)
            assert np.abs(s["d"]).min() > 1e-6, (robot, b, s["d"])
            assert np.abs(s["n"] - pr.DEFAULT_ROW[5]).min() > 1e-6, (robot, b, s["n"])
            floor = max(floor, _rel(pr.cholesky_solve(s["A"], s["rhs"]), s["v"]))
            rows.append(s)
            qb, vb = s["q"], s["v"]
        steps.append(rows)
    return steps, floor


def _set_and_step(plant, robot, period, substeps, launches=1):
    m = ob.model(robot)
    q, v, cmd, force, ground = _cases(robot)
    plant.set_state(np.array([wp.rbd_from(m, q[b], v[b]) for b in range(B5)]))
    for _ in range(launches):
        plant.step(cmd["pos_des"], cmd["vel_des"], cmd["tau_ff"], cmd["kp"], cmd["kd"], base_force=force, feet_heights=ground, period=period, substeps=substeps)
    return _read(plant)


def _compare(robot, out, steps, tol):
    """every output of the device against the sensors of the restatement's last substep; returns the maxima by key"""
    m = ob.model(robot)
    _, _, _, _, ground = _cases(robot)
    worst = {}
    for b in range(B5):
        ref = pr.sensors(m, steps[b][-1], ground=ground[b])
        assert np.array_equal(out["contact"][b], ref["contact"]), (robot, b, out["contact"][b], ref["contact"])
        qd, vd = wp.measured_state(m, out["rbd"][b])
        worst["q+"] = max(worst.get("q+", 0.0), _rel(qd, steps[b][-1]["q"]))
        worst["v+"] = max(worst.get("v+", 0.0), _rel(vd, steps[b][-1]["v"]))
        for k in SENSORS:
            if k != "contact":
                worst[k] = max(worst.get(k, 0.0), _rel(out[k][b], ref[k]))
    print("plant", robot, len(steps[0]), "substeps", {k: "%.2e" % x for k, x in worst.items()})
    assert max(worst.values()) < tol, worst
    return worst


@pytest.mark.parametrize("robot", ["h1", "g1"])
def test_one_substep_matches_restatement(robot):
    """1e-9 relative to max(1, |value|) holds with room: the device's largest figures were 2.8e-14 (H1) and 5.0e-14 (G1), both for
    linear_accel_local, which divides by h.  The restatement's own floor (numpy.linalg.solve against a Cholesky solve of the same system: 2.2e-15 for
    H1, 5.6e-15 for G1) is printed beside them; it is not needed as a bound."""
    steps, floor = _reference(robot, 1)
    closed = np.array([steps[b][0]["closed"] for b in range(B5)])
    assert not closed[0].any() and closed[1].all() and closed[2].tolist() == [True, True, False, False] and closed[3].any() and closed[4].any()
    print("restatement floor", robot, floor)
    out = _set_and_step(_plant(robot, B5), robot, H, 1)
    _compare(robot, out, steps, TOL)


def test_twenty_substeps_in_one_launch():
    """Tolerance: 100 x the restatement's own floor over the twenty substeps.  The floor - the largest difference of v+ between numpy.linalg.solve
    and a Cholesky solve of the same system, relative to max(1, |v+|) - measured 6.5e-15 (on two machines, the same figure), so the tolerance is
    6.5e-13; the floor is measured again and printed at every run.  The device's largest figure at this tolerance was 3.1e-13 (contact forces of
    some hundred newtons), 2.4e-14 for v+.  The same control step as twenty launches of one substep gives the same bits."""
    robot = "h1"
    steps, floor = _reference(robot, SUBSTEPS)
    tol = TOL20
    print("restatement floor over", SUBSTEPS, "substeps", floor, "tolerance", tol)
    one = _set_and_step(_plant(robot, B5), robot, PERIOD, SUBSTEPS)
    _compare(robot, one, steps, tol)
    many = _set_and_step(_plant(robot, B5), robot, H, 1, launches=SUBSTEPS)
    for k in SENSORS:
        assert np.array_equal(one[k], many[k]), k


# ---------------------------------------------------------------------------------------------------------------- masks and determinism
B67 = 67


@functools.lru_cache(maxsize=None)
def _fleet67():
    from tests.test_plant_reference import standing_state
    m = ob.model("h1")
    nj = m["nj"]
    nv = 6 + nj
    rng = np.random.default_rng(67)
    q0, _, _ = standing_state(m, depth=0.0025)
    q = np.tile(q0, (B67, 1)) + rng.standard_normal((B67, nv)) * np.r_[np.zeros(3), np.full(3, 0.002), np.full(nj, 0.004)]
    v = 0.05 * rng.standard_normal((B67, nv))
    rbd = np.array([wp.rbd_from(m, q[b], v[b]) for b in range(B67)])
    cmd = [q[:, 6:] + 0.01 * rng.standard_normal((B67, nj)), np.zeros((B67, nj)), 2.0 * rng.standard_normal((B67, nj)), rng.uniform(500.0, 2000.0, (B67, nj)),
           rng.uniform(10.0, 40.0, (B67, nj))]
    force = 10.0 * rng.standard_normal((B67, 3))
    ground = 0.001 * rng.standard_normal((B67, 4))
    other = np.array([wp.rbd_from(m, q[b] + 0.005 * rng.standard_normal(nv) * np.r_[np.zeros(3), np.ones(nv - 3)], 0.1 * rng.standard_normal(nv)) for b in range(B67)])
    return rbd, cmd, force, ground, other


def _run67(device=False, set_state_at=None, params_mask=None, steps=10):
    """states after every control step [steps, 67, 2 nv] and the outputs after the last"""
    rbd, cmd, force, ground, other = _fleet67()
    plant = _plant("h1", B67)
    dev = (lambda a, dt=torch.float64: torch.tensor(a, dtype=dt, device="cuda")) if device else (lambda a, dt=None: a)
    arrays = [dev(a) for a in cmd] + [dev(force), dev(ground)]
    mask = (np.arange(B67) % 3 == 0).astype(np.int32)
    if device:
        torch.cuda.synchronize()
    if params_mask is not None:
        plant.setParams(dev(pr.DEFAULT_ROW * np.r_[1.6, 1.0, 1.0, 0.5, 1.0, 1.0, 1.0, 1.0]), mask=dev(params_mask, torch.int32) if device else params_mask)
    plant.set_state(dev(rbd))
    states = []
    for k in range(steps):
        if set_state_at == k:
            plant.set_state(dev(other), mask=dev(mask, torch.int32) if device else mask)
        plant.step(*arrays[:5], base_force=arrays[5], feet_heights=arrays[6], period=0.002, substeps=4)
        states.append(plant.get_state())
    return np.array(states), _read(plant), mask


def test_masks_and_determinism():
    a, out_a, mask = _run67()
    assert np.all(np.isfinite(a))
    b, out_b, _ = _run67()
    assert np.array_equal(a, b) and all(np.array_equal(out_a[k], out_b[k]) for k in SENSORS)
    d, out_d, _ = _run67(device=True)
    assert np.array_equal(a, d) and all(np.array_equal(out_a[k], out_d[k]) for k in SENSORS)
    keep = mask == 0
    for device in (False, True):
        c, _, _ = _run67(device=device, set_state_at=5)
        assert np.array_equal(c[:, keep], a[:, keep]) and np.array_equal(c[:5], a[:5])
        assert all(not np.array_equal(c[5:, i], a[5:, i]) for i in np.nonzero(mask)[0])
        p, _, _ = _run67(device=device, params_mask=mask)
        assert np.array_equal(p[:, keep], a[:, keep])
        assert all(not np.array_equal(p[:, i], a[:, i]) for i in np.nonzero(mask)[0])
    plant = _plant("h1", B67)
    plant.setParams(pr.DEFAULT_ROW * 2.0, mask=mask)
    assert np.array_equal(plant.getParams(3), pr.DEFAULT_ROW * 2.0) and np.array_equal(plant.getParams(4), pr.DEFAULT_ROW) and np.array_equal(plant.getParams(), pr.DEFAULT_ROW)
    plant.resetParams()
    assert np.array_equal(plant.getParams(3), pr.DEFAULT_ROW)


# ---------------------------------------------------------------------------------------------------------------- estimator round trip
def test_estimator_round_trip():
    import bipedal_control_amd as bp
    from bipedal_control_amd import scenarios as sc
    rbd, cmd, force, ground, _ = _fleet67()
    B = B5
    itf = sc.interface("h1")
    plant = bp.BatchedPlant(itf, max_batch=B)
    topic = bp.BatchedStateEstimate(itf, kind="from_topic", max_batch=B)
    dev = [torch.tensor(a[:B], device="cuda") for a in cmd + [force, ground]]
    torch.cuda.synchronize()
    plant.set_state(rbd[:B])
    plant.step(*dev[:5], base_force=dev[5], feet_heights=dev[6], period=0.002, substeps=4)      # only enqueued
    est_rbd = topic.update_from_plant(plant, period=0.002)                                   # waits for the step on the device
    truth = plant.get_state()
    print("from-topic estimate against the plant's rbd", np.abs(est_rbd - truth).max())
    assert np.abs(est_rbd - truth).max() < 1e-12
    # the same through bpmpc_estimator_update itself, the output tensors as its arguments
    o = {k: v.torch() for k, v in plant.outputs().items()}
    again = topic.update(o["joint_pos"], o["joint_vel"], odom=(o["odom_pos"], o["odom_quat"], o["odom_lin_vel"], o["odom_ang_vel"]), period=0.002)
    assert np.array_equal(again, est_rbd)
    # Kalman: ten steps and ten updates, nothing synchronised in between
    kalman = bp.BatchedStateEstimate(itf, kind="kalman", max_batch=B)
    for _ in range(10):
        plant.step(*dev[:5], base_force=dev[5], feet_heights=dev[6], period=0.002, substeps=4)
        assert kalman.update_from_plant(plant, period=0.002, fetch=False) is None
    x_hat, P = kalman.getState()                                                             # synchronises the estimator's stream
    outs = kalman.device_outputs()
    xy = outs["xy_reset"].torch().cpu().numpy()
    nv = 6 + itf.actuatedDofNum
    lin = outs["rbd"].torch().cpu().numpy()[:, nv + 3:nv + 6]
    assert xy.shape == (B,) and np.all(np.isfinite(lin)) and np.all(np.isfinite(x_hat)) and np.all(np.isfinite(P))
    assert set(np.unique(_read(plant)["contact"]).tolist()) <= {0, 1}


# ---------------------------------------------------------------------------------------------------------------- the loop
NB, NI, TICKS, REARM = 3, 20, 50, 10
TICK_KEYS = ("x_obs", "x_opt", "u_opt", "joint_cmd", "wbc_solution", "planned_mode", "wbc_status", "safe", "joint_torque")


class _Loop:
    def __init__(self):
        import bipedal_control_amd as bp
        from bipedal_control_amd import scenarios as sc
        from tests.test_plant_reference import standing_state
        self.itf = itf = sc.interface("h1")
        self.H = NI * sc.DT
        self.mpc = bp.BatchedSqpMpc(itf, max_batch=NB, max_nodes=sc.max_nodes_for(NI, self.H), return_gains=True)
        self.wbc = bp.WeightedWbc(itf, max_batch=NB)
        self.ctrl = bp.BatchedController(self.mpc, self.wbc)
        self.est = bp.BatchedStateEstimate(itf, kind="from_topic", max_batch=NB)
        self.plant = bp.BatchedPlant(itf, max_batch=NB)
        self.gaits = [bp.loadModeSequenceTemplate(sc.ROBOTS["h1"]["gait"], "stance")]
        m = ob.model("h1")
        q, v, _ = standing_state(m, depth=0.0025)
        rng = np.random.default_rng(5)
        self.rbd0 = np.array([wp.rbd_from(m, q + 0.002 * rng.standard_normal(len(q)) * np.r_[np.zeros(6), np.ones(len(q) - 6)], v) for _ in range(NB)])
        self.x0 = np.tile(itf.getInitialState(), (NB, 1))
        self.x0[:, 6:] = np.c_[self.rbd0[:, 3:6], self.rbd0[:, 0:3], self.rbd0[:, 6:6 + m["nj"]]]
        self.ctrl.setJointGains(np.full(m["nj"], bp.WbcParams.RECONFIGURE_MOTOR_KP), np.full(m["nj"], bp.WbcParams.RECONFIGURE_MOTOR_KD))

    def arm(self, t, first):
        self.mpc.setup_commands(t, self.x0 if first else None, self.gaits, -1, 0.0, np.zeros(4), horizon=self.H, from_previous=not first)
        self.mpc.enqueue()

    def snapshot(self):
        """plant outputs and tick outputs as numpy (the caller has synchronised)"""
        s = {k: v.torch().cpu().numpy() for k, v in self.plant.outputs().items()}
        s.update({k: v.torch().cpu().numpy() for k, v in self.ctrl.device_outputs().items() if k in TICK_KEYS})
        return s


def _loop_on_device(read_every_tick):
    lp = _Loop()
    lp.plant.set_state(lp.rbd0)
    lp.arm(0.0, True)
    t = torch.zeros(NB, dtype=torch.float64, device="cuda")
    times = [torch.full((NB,), 0.002 * (k + 1), dtype=torch.float64, device="cuda") for k in range(TICKS)]
    torch.cuda.synchronize()                      # the tensors are filled on torch's stream, which the handles' streams do not wait for
    lp.ctrl.tick(t, lp.plant.outputs()["rbd"].torch(), period=0.002, fetch=False)
    shots = {}
    for k in range(TICKS):
        lp.plant.step_controlled(lp.ctrl, period=0.002, substeps=4)
        lp.est.update_from_plant(lp.plant, period=0.002, fetch=False)
        lp.ctrl.tick_estimated(times[k], lp.est, period=0.002, fetch=False)
        if k % REARM == REARM - 1:
            lp.arm(0.002 * (k + 1), False)
        if read_every_tick or k % REARM == REARM - 1:      # the free-running loop is read at the re-arm points only
            torch.cuda.synchronize()
            shots[k] = lp.snapshot()
    return shots


def _loop_through_host():
    lp = _Loop()
    lp.plant.set_state(lp.rbd0)
    lp.arm(0.0, True)
    out = lp.ctrl.tick(np.zeros(NB), lp.plant.get_state(), period=0.002)
    shots = {}
    for k in range(TICKS):
        cmd = out["joint_cmd"]
        lp.plant.step(cmd[:, 0], cmd[:, 1], cmd[:, 2], out["joint_kp"], out["joint_kd"], period=0.002, substeps=4)
        s = _read(lp.plant)
        rbd = lp.est.update(s["joint_pos"], s["joint_vel"], odom=(s["odom_pos"], s["odom_quat"], s["odom_lin_vel"], s["odom_ang_vel"]), period=0.002)
        out = lp.ctrl.tick(np.full(NB, 0.002 * (k + 1)), rbd, period=0.002)
        if k % REARM == REARM - 1:
            lp.arm(0.002 * (k + 1), False)
        s.update({key: out[key] for key in TICK_KEYS})
        shots[k] = s
    return shots


def test_the_loop_closes_on_the_device():
    host = _loop_through_host()
    for k, s in host.items():
        assert all(np.all(np.isfinite(np.asarray(a, float))) for a in s.values()), k
        assert np.all(s["safe"] == 1), (k, s["safe"])
    print("loop: base height after", TICKS, "ticks", host[TICKS - 1]["odom_pos"][:, 2], "wbc status", host[TICKS - 1]["wbc_status"])
    read = _loop_on_device(True)
    free = _loop_on_device(False)
    assert sorted(read) == list(range(TICKS)) and sorted(free) == list(range(REARM - 1, TICKS, REARM))
    for shots in (read, free):
        for k, s in shots.items():
            for key in SENSORS + TICK_KEYS:
                assert np.array_equal(s[key], host[k][key]), (k, key)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    import bipedal_control_amd as bp
    INVALID, CAPACITY = -1, -6
    rbd, cmd, force, ground, _ = _fleet67()
    plant = _plant("h1", 4)
    args = [a[:4] for a in cmd]

    def status(call):
        with pytest.raises(bp.BpmpcError) as e:
            call()
        return e.value.status

    plant.batch = 4
    assert status(lambda: plant.step(*args)) == INVALID                           # before any set_state
    plant.set_state(rbd[:4])
    before = plant.get_state()
    assert status(lambda: plant.step(*args, substeps=0)) == INVALID
    assert status(lambda: plant.step(*args, period=0.0)) == INVALID
    assert status(lambda: plant.step(*args, period=-0.002)) == INVALID
    assert status(lambda: plant.step(*args, period=float("nan"))) == INVALID
    plant.batch = 3
    assert status(lambda: plant.step(*[a[:3] for a in cmd])) == INVALID and "set_state" in bp.load_library().bpmpc_last_error().decode()
    plant.batch = 5
    assert status(lambda: plant.step(*[a[:5] for a in cmd])) == CAPACITY
    assert status(lambda: plant.set_state(rbd[:5])) == CAPACITY
    plant.batch = 4
    bad = rbd[:4].copy()
    bad[2, 7] = np.nan
    assert status(lambda: plant.set_state(bad)) == INVALID
    assert status(lambda: plant.setParams(pr.DEFAULT_ROW * np.r_[0.0, np.ones(7)])) == INVALID
    lib = bp.load_library()
    from bipedal_control_amd.api import _JointCommand, _d
    partial = _JointCommand(pos_des=_d(np.ascontiguousarray(args[0])))
    assert lib.bpmpc_plant_step(plant._h, 4, C.byref(partial), 0, 0.002, 4) == INVALID and b"null" in lib.bpmpc_last_error()
    assert np.array_equal(plant.get_state(), before)                             # no refusal touched the state
    # step_controlled before any tick
    lp = _Loop()
    lp.plant.set_state(lp.rbd0)
    assert status(lambda: lp.plant.step_controlled(lp.ctrl)) == INVALID and "not ticked" in lib.bpmpc_last_error().decode()
    lp.arm(0.0, True)
    lp.ctrl.tick(np.zeros(NB), lp.rbd0)
    lp.plant.step_controlled(lp.ctrl)
    lp.plant.set_state(lp.rbd0[:2])
    assert status(lambda: lp.plant.step_controlled(lp.ctrl)) == INVALID

